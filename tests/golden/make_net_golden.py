"""Generate the golden vector of the whole point-cloud policy network from the
reference's own envs/inference/models/model_cls_off_rot.py on torch CPU.

Run where the reference is present (the GPU machine does not have it):
    python tests/golden/make_net_golden.py

The yardstick is get_model(14, 6, 4) loaded with tests/net_helpers.py's
seeded_state(STATE_SEED), in .eval() and .double(): every parameter is a float32
value, so the f64 run is the exact-arithmetic result of f32 data.  The cloud is
one make_group_golden.make_cloud cloud of N = 600 (normalised, f32) with random
colours in 0..1.  farthest_point_sample and query_ball_point of the model's
module are wrapped while it runs and what they return is stored, exactly as
make_mlp_golden.py does (the sampler is fed the f32 cloud: it keeps its
distances in f32), so a test feeds the same indices and no ball-query
ambiguity enters.  conv2's output x (the head before log_softmax and the
split into cls / off / rot) is taken by a forward hook.

Stored: xyz [1, 600, 3] f32, colors [1, 600, 3] f32, fps1 [1, 512] and fps2
[1, 128] i16, group1_0..2 and group2_0..1 i16, head [1, 600, 18] f64, and the
state's seed.

Output: tests/golden/net_golden.npz (data only).
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "panda-lang-manip_amd"))
from make_group_golden import REF, make_cloud  # noqa: E402
from net_helpers import NUM_CLASSES, NUM_INPUT, NUM_OUTPUT, STATE_SEED, seeded_state  # noqa: E402

OUT = os.path.join(HERE, "net_golden.npz")
CLOUD_SEED, N = 20261021, 600


def main():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(REF)))  # envs/inference: `models.pointnet2_utils`
    model_mod = importlib.import_module("models.model_cls_off_rot")
    ref = importlib.import_module("models.pointnet2_utils")
    rng = np.random.default_rng(CLOUD_SEED)
    torch.manual_seed(CLOUD_SEED)
    xyz = make_cloud(rng, N, None)[None]
    colors = rng.random((1, N, NUM_INPUT - 3)).astype(np.float32)
    model = model_mod.get_model(NUM_OUTPUT, NUM_INPUT, NUM_CLASSES)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in seeded_state(STATE_SEED).items()})
    model = model.double().eval()
    seen = {"fps": [], "ball": [], "x": []}
    fps0, ball0 = ref.farthest_point_sample, ref.query_ball_point

    def fps(*a, **k):
        seen["fps"].append(fps0(a[0].float(), *a[1:], **k))
        return seen["fps"][-1]

    def ball(*a, **k):
        seen["ball"].append(ball0(*a, **k))
        return seen["ball"][-1]

    hook = model.conv2.register_forward_hook(lambda m, i, o: seen["x"].append(o.detach()))
    ref.farthest_point_sample, ref.query_ball_point = fps, ball
    try:
        with torch.no_grad():
            inp = torch.from_numpy(np.concatenate([xyz, colors], -1).astype(np.float64)).permute(0, 2, 1)
            cls, off, rot = model(inp)
    finally:
        ref.farthest_point_sample, ref.query_ball_point = fps0, ball0
        hook.remove()
    assert len(seen["fps"]) == 2 and len(seen["ball"]) == 5 and len(seen["x"]) == 1
    head = seen["x"][0].permute(0, 2, 1).contiguous().numpy()
    assert head.shape == (1, N, NUM_CLASSES + NUM_OUTPUT) and head.dtype == np.float64
    # the hook's x is what forward splits: its columns behind the logits are off and rot
    assert np.array_equal(head[..., NUM_CLASSES:NUM_CLASSES + 6], off.numpy())
    assert np.array_equal(head[..., NUM_CLASSES + 6:], rot.numpy())
    assert np.abs(torch.log_softmax(torch.from_numpy(head[..., :NUM_CLASSES]), -1).numpy() - cls.numpy()).max() < 1e-12
    out = dict(xyz=xyz, colors=colors, head=head, seed=np.int64(STATE_SEED),
               fps1=seen["fps"][0].numpy().astype(np.int16), fps2=seen["fps"][1].numpy().astype(np.int16))
    for i in range(3):
        out[f"group1_{i}"] = seen["ball"][i].numpy().astype(np.int16)
    for i in range(2):
        out[f"group2_{i}"] = seen["ball"][3 + i].numpy().astype(np.int16)
    assert out["fps1"].shape == (1, 512) and out["fps2"].shape == (1, 128)
    assert out["group1_2"].shape == (1, 512, 128) and out["group2_1"].shape == (1, 128, 128)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
