"""pandasim — MI355X-native batched Panda manipulation envs (PandaReach/Push/Slide/PickAndPlace/Stack/Flip-v3).

Host layer over libpandasim.so (HIP, gfx950).  See DESIGN.md.
"""
from . import panda_cartesian, skills
from ._lib import PandasimError, lib
from .cloudnet import (CloudLabels, CloudMlp, CloudSegNet, DecodedWaypoints, PolicyEvaluation, PolicyLoss,
                       demonstration_records, fold_batchnorm, round_bfloat16)
from .core import PyBulletRobot, RobotTaskEnv, Task, TimeLimit
from .envs import REGISTRY, PandaVecEnv, make
from .panda_tasks import (PandaFlipEnv, PandaPickAndPlaceEnv, PandaPushEnv, PandaReachEnv, PandaSlideEnv,
                          PandaStackEnv)
from .replay import HerReplay, ReplaySample
from .robots import Panda
from .sim import GRASP_VIEWS, PandaSim, keypoint_features_args, patch_size, project_to_pixels
from .tasks import Flip, PickAndPlace, Push, Reach, Slide, Stack

__all__ = ["make", "PandaVecEnv", "PandaSim", "GRASP_VIEWS", "keypoint_features_args", "patch_size", "project_to_pixels", "CloudMlp", "fold_batchnorm", "round_bfloat16", "CloudSegNet", "DecodedWaypoints", "REGISTRY", "PandasimError", "lib", "PyBulletRobot",
           "Task", "RobotTaskEnv", "TimeLimit", "Panda", "Reach", "Push", "PickAndPlace", "PandaReachEnv",
           "PandaPushEnv", "PandaPickAndPlaceEnv", "Slide", "Stack", "Flip", "PandaSlideEnv", "PandaStackEnv", "PandaFlipEnv", "panda_cartesian",
           "skills", "HerReplay", "ReplaySample", "CloudLabels", "PolicyLoss", "PolicyEvaluation",
           "demonstration_records"]
__version__ = "0.1.0"
