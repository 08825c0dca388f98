"""GPU tests of the oriented env step (ps_step_oriented; PandaVecEnv.step's
euler_xyz / orientation; Panda.set_action(action, euler_xyz) of
panda_ori.py:52-99) and of the Euler/quaternion conversion kernels.

The yardstick is tests/test_ori_cpu.py's oracle_oriented_step, the fp64
oracle's step composed with a target orientation, which reproduces
oracle.step bit for bit at the standard orientation
(test_composed_step_reproduces_oracle_step).  Bounds and classes are those of
the un-oriented tests: parity_judge.judge / TOL / LOOSE / not_tight_cap.
"""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as R

import oracle as O
from helpers import oracle_config_for, oracle_env_from, quat_err, snapshot
from parity_judge import FREE_GRIPPER, LOOSE, TOL, done_flags_ok, judge, not_tight_cap
from parity_judge import groups_for as _groups
from test_ori_cpu import DELTA_DEG, SCHEDULE_B, SCHEDULE_SEED, SCHEDULE_STEPS, oracle_oriented_step, quat_of, schedule

pytestmark = pytest.mark.gpu

ALL_TASKS = ["reach", "push", "pick_and_place", "slide", "stack", "flip"]
ENV_IDS = {"push": "PandaPush", "pick_and_place": "PandaPickAndPlace"}


@pytest.fixture(scope="module")
def ps():
    import pandasim

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return pandasim


def make_env(task, control, n, reward="sparse", lanes=0, autoreset=False):
    from pandasim.envs import PandaVecEnv

    return PandaVecEnv(task, reward, control, n, "cuda", autoreset=autoreset, lanes_per_env=lanes)


def _group_errors(task, a, b):
    """max |a - b| per observation group of two [B, obs_dim] tensors."""
    groups = _groups(task, 7 if task in FREE_GRIPPER else 6)
    return {k: float((a[:, idx] - b[:, idx]).abs().max()) for k, idx in groups.items()}


# ------------------------------------------- teacher-forced against the oracle
@pytest.mark.parametrize("task,lanes", [(t, 1) for t in ALL_TASKS] +
                         [(t, l) for l in (16, 8) for t in ("reach", "push", "pick_and_place")])
def test_oriented_step_parity_teacher_forced(ps, monkeypatch, task, lanes):
    """Each fused oriented GPU step vs one composed oracle step from the same
    state, the target angles (-180, 0, 0) + U(-15, 15) degrees per axis redrawn
    per env and step (test_ori_cpu.schedule), classified by
    parity_judge.judge, whose oracle.step is this env's composed step for the
    duration of the call.  Assertions as test_env_step_parity_teacher_forced:
    no sample beyond the tight bounds, bifurcated samples within LOOSE, counts
    within not_tight_cap, the done-flag rule, `truncated` equal."""
    B, steps = SCHEDULE_B, SCHEDULE_STEPS
    env = make_env(task, "ee", B, lanes=lanes)
    assert env.lanes_per_env == lanes
    env.reset(seed=SCHEDULE_SEED)
    cfg = oracle_config_for(env.sim.cfg)
    groups = _groups(task, 7 if task in FREE_GRIPPER else 6)
    assert max(max(v) for v in groups.values()) == env.obs_dim - 1
    worst = {k: 0.0 for k in groups}
    worst_bif = {k: 0.0 for k in groups}
    counts = {"tight": 0, "conditioned": 0, "bif": 0, "beyond": 0}
    beyond, flag_bad = [], []
    flag_mismatch = 0
    G = env.goal_dim
    for s, (a, eul) in enumerate(schedule(env.action_dim, DELTA_DEG, B, steps)):
        snap = snapshot(env.sim)
        obs, r, te, tr, _ = env.step(torch.from_numpy(a).cuda(), euler_xyz=torch.from_numpy(eul).cuda())
        og, te, tr = obs["observation"].cpu().numpy(), te.cpu().numpy(), tr.cpu().numpy()
        agg = obs["achieved_goal"].cpu().numpy()
        quats = quat_of(eul)
        for i in range(B):
            q_i = quats[i]
            with monkeypatch.context() as m:
                m.setattr(O, "step", lambda c, e, act, autoreset=False, stats=None, q_i=q_i:
                          oracle_oriented_step(c, e, act, q_i))
                o, ag, dg, rr, t_e, t_r = O.step(cfg, oracle_env_from(cfg, snap, i), a[i])
                cls, errs = judge(cfg, snap, i, a[i], o, og[i], groups, task)
            counts[cls] += 1
            for k, err in errs.items():
                if cls == "bif":
                    worst_bif[k] = max(worst_bif[k], err)
                else:
                    worst[k] = max(worst[k], err)
            if cls == "beyond":
                beyond.append((s, i, {k: f"{v:.2e}" for k, v in errs.items()}))
            assert t_r == bool(tr[i])
            ok, mismatch = done_flags_ok(task, te[i], agg[i], t_e, ag, snap["goal"][:G, i])
            flag_mismatch += mismatch
            if not ok:
                flag_bad.append((s, i, bool(te[i]), t_e))
    print(task, f"lanes {lanes}", counts, "worst", {k: f"{v:.2e}" for k, v in worst.items()},
          "ill-conditioned worst", {k: f"{v:.2e}" for k, v in worst_bif.items()}, "beyond", beyond[:8],
          f"terminated mismatches (straddling the threshold) {flag_mismatch}")
    assert not beyond
    assert not flag_bad, flag_bad
    for k, v in worst_bif.items():
        assert v <= LOOSE[k], (k, v)
    if task in FREE_GRIPPER:
        assert counts["bif"] <= not_tight_cap(task) * B * steps
        assert counts["conditioned"] <= 0.02 * B * steps
    else:
        assert counts["bif"] + counts["conditioned"] <= not_tight_cap(task) * B * steps


# ------------------------------------- the standard orientation is ps_step's
def _pair(task, B=100, seed=31, **kw):
    envs = [make_env(task, "ee", B, lanes=1, **kw) for _ in range(2)]
    for e in envs:
        e.reset(seed=seed)
    return envs


@pytest.mark.parametrize("task", ["reach", "push"])
def test_standard_orientation_reproduces_ps_step(ps, task):
    """Two envs from one seed, B = 100 (a ragged last wave), lanes 1, 5 steps
    of the same actions: one through ps_step, one with orientation
    (1, 0, 0, 0).  The kernels may contract differently, so the observations
    agree within parity_judge.TOL per group, not bit for bit."""
    B = 100
    plain, ori = _pair(task, B)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    worst = {}
    for s in range(5):
        a = torch.rand(B, plain.action_dim, device="cuda", generator=g) * 2 - 1
        o_p, r_p, te_p, tr_p, _ = plain.step(a)
        o_o, r_o, te_o, tr_o, _ = ori.step(a, orientation=[1.0, 0.0, 0.0, 0.0])
        for k, v in _group_errors(task, o_o["observation"], o_p["observation"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert torch.equal(o_o["desired_goal"], o_p["desired_goal"])
        assert torch.equal(tr_o, tr_p)
    print(task, "oriented (standard) vs ps_step, max per group", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= TOL[task][k], (k, v)


# ------------------------------------------- the orientation takes effect
def test_target_orientation_is_reached(ps):
    """Reach, 16 envs, 25 free-running steps of zero displacement towards
    (-180, 0, 45) degrees: the end effector's rotation angle to the target
    (ps_link_state(11)) ends within the composed oracle's angle + 2e-3 rad
    (test_ik_parity's IK bound) and at most half of what it was at step 0."""
    B = 16
    env = make_env("reach", "ee", B)
    env.reset(seed=3)
    cfg = oracle_config_for(env.sim.cfg)
    snap = snapshot(env.sim)
    euler = [-180.0, 0.0, 45.0]
    q_t = quat_of(euler)

    def angles(quats):
        return (R.from_quat(q_t) * R.from_quat(np.asarray(quats, np.float64)).inv()).magnitude()

    first = angles(env.sim.get_link_orientation("panda", 11).cpu().numpy())
    zeros = torch.zeros(B, 3, device="cuda")
    for _ in range(25):
        env.step(zeros, euler_xyz=euler)
    last = angles(env.sim.get_link_orientation("panda", 11).cpu().numpy())
    ref = []
    for i in range(B):
        e = oracle_env_from(cfg, snap, i)
        for _ in range(25):
            oracle_oriented_step(cfg, e, np.zeros(3, np.float32), q_t)
        ref.append(O.link_state(cfg, e, 11)[1])
    ref = angles(np.array(ref))
    print(f"angle to the target: step 0 {first.max():.4f}, GPU {last.max():.2e}, oracle {ref.max():.2e} rad")
    assert (first > 0.7).all()
    assert (last <= ref + 2e-3).all(), (last, ref)
    assert (last <= 0.5 * first).all()


# ------------------------------------------------ plugin path = fused path
@pytest.mark.parametrize("task", ["push", "pick_and_place"])
def test_plugin_path_matches_fused_oriented_step(ps, task):
    """As test_plugin_path_matches_fused_kernel, with a target orientation per
    env: RobotTaskEnv.step(a, euler_xyz=e) against PandaVecEnv.step(a,
    euler_xyz=e) at lanes 1 from the fused env's state, 8 steps, B = 128."""
    from pandasim.envs import PandaVecEnv

    B = 128
    fused = PandaVecEnv(task, "dense", "ee", B, "cuda", autoreset=False, lanes_per_env=1)
    fused.reset(seed=777)
    env = ps.make(f"{ENV_IDS[task]}Dense-v3", num_envs=B, fused=False)
    env.reset(seed=777)
    assert torch.equal(env.task.get_goal(), fused.sim.goal[:fused.goal_dim, :B].t())
    groups = _groups(task, 7 if task in FREE_GRIPPER else 6)
    worst = {k: 0.0 for k in groups}
    for a, eul in schedule(fused.action_dim, DELTA_DEG, B, 8, seed=17):
        env.sim.state.copy_(fused.sim.state)
        a, eul = torch.from_numpy(a).cuda(), torch.from_numpy(eul).cuda()
        o_f, r_f, te_f, _, _ = fused.step(a, euler_xyz=eul)
        o_p, r_p, te_p, tr_p, info = env.step(a, euler_xyz=eul)
        assert o_p["observation"].shape == o_f["observation"].shape
        assert torch.equal(o_p["desired_goal"], o_f["desired_goal"])
        for k, idx in groups.items():
            worst[k] = max(worst[k], float((o_p["observation"][:, idx] - o_f["observation"][:, idx]).abs().max()))
        assert float((r_p - r_f).abs().max()) <= 4 * TOL[task]["obj_pos"]
        assert int((te_p != te_f.bool()).sum()) <= 2
        assert torch.equal(info["is_success"], te_p)
        assert not tr_p.any()
    print(task, {k: f"{v:.2e}" for k, v in worst.items()})
    tol = LOOSE if task in FREE_GRIPPER else TOL[task]
    for k, v in worst.items():
        assert v <= tol[k], (k, v)


# --------------------------------------------------------- the conversions
def test_conversions_match_scipy(ps):
    """4096 random angle triples (|pitch| <= 80 degrees), rounded to f32: the
    quaternions are within 2e-7 of scipy's on the same f32 input up to sign
    (half an f32 ulp at 1 plus fp64 slack), and the angles back from those f32
    quaternions within 2e-5 degrees of scipy's on the same quaternions (half an
    f32 ulp at 180)."""
    from pandasim.sim import PandaSim

    sim = PandaSim("reach", num_envs=4)
    rng = np.random.default_rng(8)
    e = np.stack([rng.uniform(-180, 180, 4096), rng.uniform(-80, 80, 4096), rng.uniform(-180, 180, 4096)],
                 -1).astype(np.float32)
    q = sim.euler_xyz_to_quat(torch.from_numpy(e))
    assert q.shape == (4096, 4) and q.dtype == torch.float32
    q = q.cpu().numpy()
    err_q = quat_err(q, R.from_euler("xyz", e.astype(np.float64), degrees=True).as_quat())
    back = sim.quat_to_euler_xyz(torch.from_numpy(q)).cpu().numpy()
    err_e = np.abs(back.astype(np.float64) - R.from_quat(q.astype(np.float64)).as_euler("xyz", degrees=True))
    print(f"euler -> quat max error {err_q.max():.2e}; quat -> euler max error {err_e.max():.2e} degrees")
    assert err_q.max() <= 2e-7
    assert err_e.max() <= 2e-5
    # shapes: one triple, leading dims
    assert sim.euler_xyz_to_quat([-180.0, 0.0, 0.0]).shape == (4,)
    assert sim.quat_to_euler_xyz(torch.from_numpy(q).reshape(64, 64, 4)).shape == (64, 64, 3)


def test_get_ee_orientation(ps):
    env = ps.make("PandaReach-v3", num_envs=32, fused=False)
    env.reset(seed=2)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for _ in range(3):
        env.step(torch.rand(32, 3, device="cuda", generator=g) * 2 - 1, euler_xyz=[-170.0, 10.0, 30.0])
    robot = env.robot
    got = robot.get_ee_orientation()
    assert got.shape == (32, 3)
    assert torch.equal(got, env.sim.quat_to_euler_xyz(robot.get_link_orientation(robot.ee_link)))
    want = R.from_quat(robot.get_link_orientation(11).double().cpu().numpy()).as_euler("xyz", degrees=True)
    assert np.abs(got.double().cpu().numpy() - want).max() <= 2e-5


# ------------------------------------------------- flags and side paths
@pytest.mark.parametrize("task", ["reach", "push"])
def test_side_paths_under_the_oriented_step(ps, task):
    """Auto-reset, final_obs, the episode statistics and the non-finite guard
    give the rows the un-oriented step gives (two envs from one seed, B = 100,
    lanes 1, standard orientation): flags and counts exactly, floats within
    parity_judge.TOL."""
    B = 100
    plain, ori = _pair(task, B, reward="dense", autoreset=True)
    stats = [e.record_episode_statistics() for e in (plain, ori)]
    for e in (plain, ori):
        e.set_nonfinite_guard(True, reset=True)
        e.sim.elapsed[:B // 2] = e.max_episode_steps - 2  # the TimeLimit ends these episodes at step 2
    g = torch.Generator(device="cuda")
    g.manual_seed(6)
    tol = max(TOL[task].values())
    resets = 0
    for s in range(4):
        if s == 2:
            for e in (plain, ori):
                e.sim.f[0, 70] = float("nan")  # joint 0 of env 70
        a = torch.rand(B, plain.action_dim, device="cuda", generator=g) * 2 - 1
        o_p, r_p, te_p, tr_p, i_p = plain.step(a)
        o_o, r_o, te_o, tr_o, i_o = ori.step(a, orientation=[1.0, 0.0, 0.0, 0.0])
        assert torch.equal(tr_o, tr_p) and torch.equal(te_o, te_p)
        assert torch.equal(i_o["nonfinite"], i_p["nonfinite"])
        assert bool(i_o["nonfinite"][70]) == (s == 2) and int(i_o["nonfinite"].sum()) == (s == 2)
        assert torch.equal(ori.sim.elapsed[:B], plain.sim.elapsed[:B])
        resets += int((te_o | tr_o).sum())
        finite = torch.isfinite(i_p["final_observation"]).all(-1)
        assert torch.equal(finite, torch.isfinite(i_o["final_observation"]).all(-1))
        for k, v in _group_errors(task, o_o["observation"], o_p["observation"]).items():
            assert v <= TOL[task][k], (s, k, v)
        for k, v in _group_errors(task, i_o["final_observation"][finite], i_p["final_observation"][finite]).items():
            assert v <= TOL[task][k], (s, "final", k, v)
        assert float((i_o["final_achieved_goal"][finite] - i_p["final_achieved_goal"][finite]).abs().max()) <= tol
        assert torch.equal(o_o["desired_goal"], o_p["desired_goal"])  # the resets drew the same goals
        assert float((r_o - r_p)[finite].abs().max()) <= tol
        assert torch.equal(stats[1][2:], stats[0][2:])  # successes and finished episodes
        keep = torch.isfinite(stats[0][:2]).all(0)
        assert torch.equal(keep, torch.isfinite(stats[1][:2]).all(0))
        assert float((stats[1][:2, keep] - stats[0][:2, keep]).abs().max()) <= 4 * tol  # returns: up to 4 rewards
    assert resets >= B // 2 + 1 and int(stats[1][3].sum()) == resets


def test_oriented_step_argument_errors(ps):
    """ps_step_oriented: orn == NULL is PS_ERR_ARG; a joints-control context is
    PS_ERR_UNSUPPORTED (PandaVecEnv.step falls back to ps_step there)."""
    from pandasim.sim import _ptr

    def call(env, orn):
        a = torch.zeros(env.num_envs, env.action_dim, device="cuda")
        s = env.sim
        return s._lib.ps_step_oriented(s._ctx, _ptr(s.state), _ptr(a), _ptr(orn), _ptr(env._obs), _ptr(env._ag),
                                       _ptr(env._dg), _ptr(env._reward), _ptr(env._term), _ptr(env._trunc), 0,
                                       None, None, s._stream())

    orn = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 8, device="cuda")
    ee = make_env("reach", "ee", 8)
    ee.reset(seed=1)
    assert call(ee, None) == -1  # PS_ERR_ARG
    assert call(ee, orn) == 0
    joints = make_env("reach", "joints", 8)
    joints.reset(seed=1)
    before = joints.sim.state.clone()
    assert call(joints, orn) == -3  # PS_ERR_UNSUPPORTED
    assert call(joints, None) == -1
    assert torch.equal(joints.sim.state, before)
    # the Python layer ignores the orientation with joints control: ps_step
    ref = make_env("reach", "joints", 8)
    ref.reset(seed=1)
    a = torch.full((8, 7), 0.3, device="cuda")
    o_j, *_ = joints.step(a, euler_xyz=[-180.0, 0.0, 45.0])
    o_r, *_ = ref.step(a)
    assert torch.equal(o_j["observation"], o_r["observation"])
