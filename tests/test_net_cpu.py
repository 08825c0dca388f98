"""CPU tests of the point-cloud policy (ps_cloud_decode_waypoints,
PandaSim.decode_waypoints / segment_cloud / predict_waypoints, CloudSegNet):
the new ABI symbol, the numpy restatement of the network's wiring
(tests/net_helpers.py: segnet_np) held to the golden recorded from the
reference's own get_model in float64 (tests/golden/make_net_golden.py), the
folded layer lists CloudSegNet uploads, Inference.predict's decoding restated
(decode_np) on a hand-worked case, and every refusal of the state-dict checker
and the argument functions.
"""
import os

import numpy as np
import pytest

from cloud_helpers import assert_abi_topic
from pandasim.cloudnet import decode_waypoints_args, segment_cloud_args, segnet_layers
from net_helpers import (END_MASK, NUM_CLASSES, START_MASK, STATE_SEED, chain_np, decode_np, euler_xyz_deg, fold_np,
                         seeded_state, segnet_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_SYMBOLS = ("ps_cloud_decode_waypoints",)

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "net_golden.npz")))
    return _golden


def golden_idx():
    g = golden()
    return dict(fps1=g["fps1"].astype(np.int64), fps2=g["fps2"].astype(np.int64),
                group1=[g[f"group1_{i}"].astype(np.int64) for i in range(3)],
                group2=[g[f"group2_{i}"].astype(np.int64) for i in range(2)])


def test_header_and_signatures_carry_the_new_symbol():
    from pandasim import _lib as L

    src = assert_abi_topic(DECODE_SYMBOLS, "decode", ("PS_CLOUD_DECODE_MAX_CLASSES", "PS_CLOUD_DECODE_MAX_LD"))
    assert (L.CLOUD_DECODE_MAX_CLASSES, L.CLOUD_DECODE_MAX_LD) == (16, 4096)
    # the rules of the decode are stated where the symbol is declared
    for word in ("Label.", "Waypoint.", "Quaternion.", "Euler.", "Empty set.", "deviation"):
        assert word in src, word


def test_python_surface_exists():
    import pandasim

    for name in ("decode_waypoints", "segment_cloud", "predict_waypoints"):
        assert hasattr(pandasim.PandaSim, name) and hasattr(pandasim.PandaVecEnv, name)
    assert isinstance(pandasim.CloudSegNet, type) and isinstance(pandasim.DecodedWaypoints, type)
    net = pandasim.CloudSegNet
    assert (net.SA1_NPOINT, net.SA1_RADII, net.SA1_NSAMPLES) == (512, (0.1, 0.2, 0.4), (32, 64, 128))
    assert (net.SA2_NPOINT, net.SA2_RADII, net.SA2_NSAMPLES) == (128, (0.4, 0.8), (64, 128))
    assert pandasim.DecodedWaypoints.__slots__ == ("waypoints", "quats", "euler_deg", "counts", "first_idx", "labels")


def test_golden_is_what_the_generator_says():
    g = golden()
    assert g["xyz"].shape == (1, 600, 3) and g["xyz"].dtype == np.float32 and g["colors"].shape == (1, 600, 3)
    assert g["head"].shape == (1, 600, 18) and g["head"].dtype == np.float64 and int(g["seed"]) == STATE_SEED
    assert g["fps1"].shape == (1, 512) and g["fps2"].shape == (1, 128)
    assert [g[f"group1_{i}"].shape[2] for i in range(3)] == [32, 64, 128]
    assert [g[f"group2_{i}"].shape[2] for i in range(2)] == [64, 128]
    assert 0 <= g["fps2"].min() and g["fps2"].max() < 512 and g["group1_2"].max() < 600 and g["group2_1"].max() < 512
    # both point sets are populated and differ (net_helpers.STATE_SEED)
    counts = decode_np(g["head"], g["xyz"], NUM_CLASSES)["counts"][0]
    assert 0 < counts[0] < counts[1] <= 600


def test_wiring_restated_in_f64_meets_the_reference():
    """segnet_np in f64 on the golden's indices against get_model.forward in
    f64: the wiring (which tensor in front of which, xyz first at sa3, the nine
    channels of fp1's points1, the repeat at fp3) is the reference's."""
    g = golden()
    got = segnet_np(seeded_state(STATE_SEED), g["xyz"], g["colors"], golden_idx(), np.float64)
    err = np.abs(got - g["head"]).max()
    print(f"max |segnet_np(f64) - golden| = {err:.3e}, max |golden| = {np.abs(g['head']).max():.3f}")
    assert err <= 1e-9 * np.abs(g["head"]).max()


def test_class_margins_of_the_seeded_state_are_wide():
    """What tests/test_gpu_net.py relies on, checked for segnet_np alone: with
    the seeded state no point's class margin is under four times the distance
    of the f32 restatement from the f64 one."""
    g = golden()
    state, idx = seeded_state(STATE_SEED), golden_idx()
    h64 = segnet_np(state, g["xyz"], g["colors"], idx, np.float64)
    h32 = segnet_np(state, g["xyz"], g["colors"], idx, np.float32)
    tol = 4 * np.abs(h32 - h64).max()
    logits = np.sort(h64[..., :NUM_CLASSES], -1)
    margin = logits[..., -1] - logits[..., -2]
    print(f"tol = {tol:.3e}, smallest margin = {margin.min():.3e}, under tol: {(margin <= tol).mean():.4f}")
    assert 0 < tol < 1e-4 * np.abs(h64).max()
    assert (margin <= tol).mean() <= 0.02


def test_segnet_layers_are_the_fold_of_the_seeded_state():
    from pandasim import fold_batchnorm
    from pandasim.cloudnet import cloud_mlp_layers

    state = seeded_state(STATE_SEED)
    layers, nc, c = segnet_layers(state)
    assert (nc, c) == (4, 6)
    shapes = {"sa1": [[9, 32, 32, 64], [9, 64, 64, 128], [9, 64, 96, 128]],
              "sa2": [[323, 128, 128, 256], [323, 128, 196, 256]], "sa3": [515, 256, 512, 1024],
              "fp3": [1536, 256, 256], "fp2": [576, 256, 128], "fp1": [137, 128, 128], "head": [128, 128, 18]}

    def check(mlp, convs, bns, widths):
        cloud_mlp_layers(mlp)  # within the library's limits
        assert [mlp[0][0].shape[1]] + [w.shape[0] for w, _, _ in mlp] == widths
        for j, (w, b, relu) in enumerate(mlp):
            p = [state[f"{convs}.{j}.weight"], state[f"{convs}.{j}.bias"]] + \
                [state[f"{bns}.{j}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")]
            wf, bf = fold_batchnorm(*p, 1e-5)
            assert relu is True and np.array_equal(w, wf) and np.array_equal(b, bf)
            w32, b32 = fold_np(state, f"{convs}.{j}", f"{bns}.{j}", np.float32)  # the tests' own f32 fold
            assert np.array_equal(w, w32) and np.array_equal(b, b32)

    for name in ("sa1", "sa2"):
        assert len(layers[name]) == len(shapes[name])
        for i, mlp in enumerate(layers[name]):
            check(mlp, f"{name}.conv_blocks.{i}", f"{name}.bn_blocks.{i}", shapes[name][i])
    for name in ("sa3", "fp3", "fp2", "fp1"):
        check(layers[name], f"{name}.mlp_convs", f"{name}.mlp_bns", shapes[name])
    (w1, b1, r1), (w2, b2, r2) = layers["head"]
    wf, bf = fold_batchnorm(state["conv1.weight"], state["conv1.bias"], state["bn1.weight"], state["bn1.bias"],
                            state["bn1.running_mean"], state["bn1.running_var"], 1e-5)
    assert r1 is True and r2 is False and np.array_equal(w1, wf) and np.array_equal(b1, bf)
    assert np.array_equal(w2, state["conv2.weight"][:, :, 0]) and np.array_equal(b2, state["conv2.bias"])
    assert [w1.shape[1], w1.shape[0], w2.shape[0]] == shapes["head"]
    # tensors are taken as arrays are, num_batches_tracked is not read, eps is the caller's
    import torch

    as_t = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items() if "num_batches" not in k}
    again, _, _ = segnet_layers(as_t)
    assert np.array_equal(again["fp2"][1][0], layers["fp2"][1][0])
    other, _, _ = segnet_layers(state, eps=1e-3)
    assert not np.array_equal(other["fp2"][1][0], layers["fp2"][1][0])
    assert len(chain_np(state, "sa3.mlp_convs", "sa3.mlp_bns", np.float64)) == 3


def test_segnet_layers_refusals_name_the_key():
    state = seeded_state(STATE_SEED)
    f = np.float32

    def refused(key, change):
        bad = dict(state)
        change(bad)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            segnet_layers(bad)

    for key in ("sa1.conv_blocks.0.0.weight", "sa1.bn_blocks.2.1.running_var", "sa2.conv_blocks.1.2.bias",
                "sa3.mlp_convs.0.weight", "sa3.mlp_bns.1.bias", "fp3.mlp_bns.0.running_mean", "fp2.mlp_bns.0.weight",
                "fp1.mlp_convs.1.bias", "fp3.mlp_convs.1.weight", "conv1.weight", "bn1.running_mean", "conv2.weight", "conv2.bias"):
        refused(key, lambda s, k=key: s.pop(k))                                      # missing
    refused("sa1.conv_blocks.1.0.weight", lambda s: s.update({"sa1.conv_blocks.1.0.weight": np.zeros((64, 10, 1, 1), f)}))
    refused("sa1.conv_blocks.0.0.weight", lambda s: s.update({"sa1.conv_blocks.0.0.weight": np.zeros((32, 5, 1, 1), f)}))
    refused("sa1.conv_blocks.0.1.weight", lambda s: s.update({"sa1.conv_blocks.0.1.weight": np.zeros((32, 32, 2, 1), f)}))
    refused("sa1.conv_blocks.0.1.weight", lambda s: s.update({"sa1.conv_blocks.0.1.weight": np.zeros(32, f)}))
    refused("sa2.conv_blocks.0.0.weight", lambda s: s.update({"sa2.conv_blocks.0.0.weight": np.zeros((128, 320, 1, 1), f)}))
    refused("sa3.mlp_convs.0.weight", lambda s: s.update({"sa3.mlp_convs.0.weight": np.zeros((256, 512, 1, 1), f)}))
    refused("fp3.mlp_convs.0.weight", lambda s: s.update({"fp3.mlp_convs.0.weight": np.zeros((256, 1024, 1), f)}))
    refused("fp2.mlp_convs.0.weight", lambda s: s.update({"fp2.mlp_convs.0.weight": np.zeros((256, 577, 1), f)}))
    refused("fp1.mlp_convs.0.weight", lambda s: s.update({"fp1.mlp_convs.0.weight": np.zeros((128, 134, 1), f)}))
    refused("conv1.weight", lambda s: s.update({"conv1.weight": np.zeros((128, 64, 1), f)}))
    refused("conv2.weight", lambda s: s.update({"conv2.weight": np.zeros((18, 64, 1), f)}))
    refused("conv2.weight", lambda s: s.update({"conv2.weight": np.zeros((15, 128, 1), f),      # one class
                                                "conv2.bias": np.zeros(15, f)}))
    refused("conv2.weight", lambda s: s.update({"conv2.weight": np.zeros((31, 128, 1), f),      # seventeen
                                                "conv2.bias": np.zeros(31, f)}))
    refused("conv2.bias", lambda s: s.update({"conv2.bias": np.zeros(17, f)}))
    refused("fp2.mlp_bns.1.running_var", lambda s: s.update({"fp2.mlp_bns.1.running_var": np.ones(127, f)}))
    refused("fp2.mlp_bns.1", lambda s: s.update({"fp2.mlp_bns.1.running_var": -np.ones(128, f)}))  # var + eps <= 0
    refused("sa1.conv_blocks.3.0.weight", lambda s: s.update({"sa1.conv_blocks.3.0.weight": np.zeros((8, 9, 1, 1), f)}))
    refused("sa2.conv_blocks.2.0.weight", lambda s: s.update({"sa2.conv_blocks.2.0.weight": np.zeros((8, 323, 1, 1), f)}))


def test_decode_waypoints_argument_checks():
    import torch

    ok = dict(num_envs=3, head=torch.zeros(3, 50, 18), xyz=torch.zeros(3, 50, 3), num_classes=4, centroid=None,
              scale=None, start_classes=(1, 3), end_classes=(2, 3))
    assert decode_waypoints_args(**ok) == (50, 18, 4, (0b1010, 0b1100))
    assert decode_waypoints_args(**dict(ok, head=torch.zeros(3, 50, 23), centroid=torch.zeros(3, 3),
                                        scale=torch.ones(3), start_classes=[0], end_classes=np.array([3, 3, 1]))) == \
        (50, 23, 4, (0b0001, 0b1010))
    assert decode_waypoints_args(**dict(ok, head=torch.zeros(3, 50, 30), num_classes=16, end_classes=(15,)))[3] == \
        (0b1010, 1 << 15)
    for bad in (dict(head=torch.zeros(2, 50, 18)), dict(head=torch.zeros(3, 50)), dict(head=torch.zeros(3, 50, 18).double()),
                dict(head=torch.zeros(3, 50, 17)), dict(head=torch.zeros(3, 0, 18), xyz=torch.zeros(3, 0, 3)),
                dict(head=torch.zeros(3, 2, 4097), xyz=torch.zeros(3, 2, 3)),
                dict(xyz=torch.zeros(3, 49, 3)), dict(xyz=torch.zeros(3, 50, 4)), dict(xyz=torch.zeros(3, 50, 3).double()),
                dict(num_classes=1), dict(num_classes=17, head=torch.zeros(3, 50, 40)), dict(num_classes=4.0),
                dict(num_classes=True), dict(num_classes=5),                      # ld = 18 < 5 + 14
                dict(centroid=torch.zeros(3, 3)), dict(scale=torch.ones(3)),      # one without the other
                dict(centroid=torch.zeros(3, 4), scale=torch.ones(3)), dict(centroid=torch.zeros(3, 3), scale=torch.ones(2)),
                dict(centroid=torch.zeros(3, 3).double(), scale=torch.ones(3)),
                dict(centroid=torch.zeros(3, 3), scale=torch.ones(3, 1)),
                dict(start_classes=()), dict(end_classes=[]), dict(start_classes=(4,)), dict(end_classes=(-1,)),
                dict(start_classes=(1.0,)), dict(start_classes=(True,)), dict(end_classes=3), dict(end_classes=None)):
        with pytest.raises(ValueError):
            decode_waypoints_args(**dict(ok, **bad))


def test_segment_cloud_argument_checks():
    import torch
    from types import SimpleNamespace

    from pandasim import CloudSegNet
    net = SimpleNamespace(sa1=1, sa2=1, sa3=1, fp3=1, fp2=1, fp1=1, head=1, num_input_channels=6,
                          SA1_NPOINT=CloudSegNet.SA1_NPOINT)
    ok = dict(num_envs=2, net=net, points=torch.zeros(2, 600, 3), colors=torch.zeros(2, 600, 3))
    assert segment_cloud_args(**ok) == 600
    assert segment_cloud_args(**dict(ok, points=torch.zeros(2, 512, 3), colors=torch.zeros(2, 512, 3))) == 512
    for bad in (dict(net="x"), dict(net=None), dict(points=torch.zeros(3, 600, 3)), dict(points=torch.zeros(2, 600, 4)),
                dict(points=torch.zeros(2, 600, 3).double()), dict(points=torch.zeros(2, 511, 3), colors=torch.zeros(2, 511, 3)),
                dict(points=torch.zeros(2, 8193, 3), colors=torch.zeros(2, 8193, 3)), dict(colors=torch.zeros(2, 600, 4)),
                dict(colors=torch.zeros(2, 599, 3)), dict(colors=torch.zeros(2, 600, 3, dtype=torch.uint8)),
                dict(colors=torch.zeros(2, 600))):
        with pytest.raises(ValueError):
            segment_cloud_args(**dict(ok, **bad))


def test_decode_np_on_a_hand_worked_case():
    """Six points, four classes.  Labels by the largest logit: 0 1 3 2 1 0
    (point 5 ties classes 0 and 2 at 0.5: the lowest wins).  Start set
    (classes 1, 3) = points 1 2 4, end set (classes 2, 3) = points 2 3."""
    head = np.zeros((1, 6, 18))
    logits = [[2, 0, 1, 0], [0, 3, 1, 2], [0, 1, 2, 5], [1, 0, 4, 0], [-1, -0.5, -2, -3], [0.5, 0, 0.5, 0.25]]
    head[0, :, :4] = logits
    xyz = np.array([[[9, 9, 9], [1, 0, 0], [0, 2, 0], [0, 0, 4], [3, 2, 1], [7, 7, 7]]], float)
    head[0, :, 4:7] = [[5, 5, 5], [0.5, 0, 0], [0, 0.5, 0], [8, 8, 8], [0, 0, -2], [6, 6, 6]]    # start offsets
    head[0, :, 7:10] = [[5, 5, 5], [4, 4, 4], [1, 1, 1], [-1, -1, -1], [3, 3, 3], [6, 6, 6]]      # end offsets
    head[0, 1, 10:14] = [0, 0, 2, 2]      # the start set's first point: 90 degrees about z, unnormalised
    head[0, 2, 10:14] = [1, 0, 0, 0]      # not the first of the start set: unused
    head[0, 2, 14:18] = [3, 0, 0, 3]      # the end set's first point: 90 degrees about x
    head[0, 3, 14:18] = [0, 1, 0, 0]
    d = decode_np(head, xyz, 4)
    assert d["labels"].tolist() == [[0, 1, 3, 2, 1, 0]]
    assert d["counts"].tolist() == [[3, 2]] and d["first_idx"].tolist() == [[1, 2]]
    # start: mean of (0.5 0 0), (0 1.5 0), (3 2 3) ; end: mean of (-1 1 -1), (1 1 5)
    assert np.allclose(d["waypoints"][0], [[3.5 / 3, 3.5 / 3, 1.0], [0.0, 1.0, 2.0]], rtol=0, atol=1e-15)
    r = np.sqrt(0.5)
    assert np.allclose(d["quats"][0], [[0, 0, r, r], [r, 0, 0, r]], rtol=0, atol=1e-15)
    assert np.allclose(d["euler_deg"][0], [[0, 0, 90], [90, 0, 0]], rtol=0, atol=1e-12)
    # un-normalised: times the scale, plus the centroid
    d2 = decode_np(head, xyz, 4, centroid=np.array([[10.0, 20.0, 30.0]]), scale=np.array([2.0]))
    assert np.allclose(d2["waypoints"][0], [[10 + 7 / 3, 20 + 7 / 3, 32.0], [10.0, 22.0, 34.0]], rtol=0, atol=1e-14)
    # other sets: class 0 alone, and a class nobody has -> empty: NaN, 0, -1
    d3 = decode_np(head[..., :18], xyz, 4, masks=(0b0001, 0b0100))
    assert d3["counts"].tolist() == [[2, 1]] and d3["first_idx"].tolist() == [[0, 3]]
    assert np.allclose(d3["waypoints"][0, 0], [(4 + 1) / 2] * 3)
    assert np.isnan(d3["quats"][0, 0]).all()   # point 0's start quaternion is zero: NaN, as the reference
    d4 = decode_np(head[:, :2], xyz[:, :2], 4, masks=(START_MASK, END_MASK))
    assert d4["counts"].tolist() == [[1, 0]] and d4["first_idx"].tolist() == [[1, -1]]
    assert np.isnan(d4["waypoints"][0, 1]).all() and np.isnan(d4["quats"][0, 1]).all() and \
        np.isnan(d4["euler_deg"][0, 1]).all()
    # the closed form is scipy's 'xyz' (extrinsic): a rotation composed about x, then y, then z
    a, b, c = np.radians([20.0, -35.0, 50.0]) / 2
    qx, qy, qz = [np.sin(a), 0, 0, np.cos(a)], [0, np.sin(b), 0, np.cos(b)], [0, 0, np.sin(c), np.cos(c)]

    def mul(p, q):
        return [p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1], p[3] * q[1] - p[0] * q[2] + p[1] * q[3] + p[2] * q[0],
                p[3] * q[2] + p[0] * q[1] - p[1] * q[0] + p[2] * q[3], p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2]]

    assert np.allclose(euler_xyz_deg(mul(qz, mul(qy, qx))), [20.0, -35.0, 50.0], rtol=0, atol=1e-12)
