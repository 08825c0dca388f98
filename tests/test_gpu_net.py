"""GPU tests of the point-cloud policy's network and its batched predict
(PandaSim.segment_cloud / predict_waypoints, CloudSegNet), at B = 2, N = 600
with tests/net_helpers.py's seeded state.

The units are pinned by their own modules; here the composition is: it is the
sequence of public calls DESIGN.md §11.6 states, bit for bit; it repeats; an
env's result does not depend on the batch around it; and it computes
get_model.forward -- against tests/net_helpers.py's segnet_np in f64 (itself
held to the reference's f64 golden in tests/test_net_cpu.py) run on the GPU's
own sampling and grouping indices, which tests/test_gpu_group.py pins, so no
ball-query ambiguity enters.  The bound is computed on the CPU:
    tol = 4 max|segnet_np(f32) - segnet_np(f64)| + 1e-6 max|head|,
the factor 4 covering the different summation orders of numpy's f32 matmul and
the kernels' k-ordered chain.

Farthest point sampling starts from fps_start(seed, env, N), so a cloud run
alone (env 0 of B = 1) starts elsewhere than as env 1 of B = 2; the batch
independence test therefore runs the cloud alone through the written-out
sequence with env 1's two start indices given to group_cloud.
"""
import numpy as np
import pytest
import torch

from cloud_helpers import DEV, dev, make_sims, same_bits
from net_helpers import END_MASK, NUM_CLASSES, START_MASK, STATE_SEED, decode_np, seeded_state, segnet_np
from test_net_cpu import golden

pytestmark = pytest.mark.gpu

SEED, N = 3, 600


def forward_by_public_calls(sim, net, points, colors, seed, starts=(None, None)):
    """DESIGN.md §11.6's wiring, one public call per line -> head, g1, g2."""
    g1 = sim.group_cloud(points, None, 512, (0.1, 0.2, 0.4), (32, 64, 128), seed, True, starts[0])
    l0 = torch.cat([g1.xyz, colors], dim=2)
    l1 = sim.abstract_features(g1, l0, mlps=net.sa1)
    g2 = sim.group_cloud(g1.new_xyz, None, 128, (0.4, 0.8), (64, 128), seed + 1, False, starts[1])
    l2 = sim.abstract_features(g2, l1, mlps=net.sa2)
    l3 = sim.shared_mlp(torch.cat([g2.new_xyz, l2], dim=2), net.sa3, pool=128)
    l2 = sim.shared_mlp(sim.propagate_features(g2.new_xyz, torch.zeros(points.shape[0], 1, 3, device=DEV), l3, l2), net.fp3)
    l1 = sim.shared_mlp(sim.propagate_features(g1.new_xyz, g2.new_xyz, l2, l1), net.fp2)
    l0 = sim.shared_mlp(sim.propagate_features(g1.xyz, g1.new_xyz, l1, torch.cat([g1.xyz, l0], dim=2)), net.fp1)
    return sim.shared_mlp(l0, net.head), g1, g2


@pytest.fixture(scope="module")
def run():
    """Everything the tests share, computed once: the two clouds (the golden's
    and a second one, un-normalised), the network, segment_cloud's result, the
    written-out sequence's, and segnet_np in f64 and f32 on the GPU's indices."""
    from types import SimpleNamespace

    from pandasim import CloudSegNet

    sims = make_sims((2, 1))
    g, rng = golden(), np.random.default_rng(77)
    second = rng.uniform(-1, 1, (N, 3)) * [0.35, 0.35, 0.05]
    box = rng.random(N) < 0.4
    second[box] = rng.uniform(-1, 1, (int(box.sum()), 3)) * 0.07 + [0.05, -0.1, 0.1]
    xyz = np.stack([g["xyz"][0], second]).astype(np.float32) * np.float32(0.4) + np.array([0.1, -0.2, 0.5], np.float32)
    colors = np.stack([g["colors"][0], rng.random((N, 3)).astype(np.float32)])
    net = CloudSegNet(seeded_state(STATE_SEED), DEV)
    points, cols = dev(xyz), dev(colors)
    head, g1 = sims[2].segment_cloud(net, points, cols, SEED)
    written, w1, w2 = forward_by_public_calls(sims[2], net, points, cols, SEED)
    torch.cuda.synchronize()
    idx = dict(fps1=w1.fps_idx.cpu().numpy(), group1=[t.cpu().numpy() for t in w1.group_idx],
               fps2=w2.fps_idx.cpu().numpy(), group2=[t.cpu().numpy() for t in w2.group_idx])
    state, nx = seeded_state(STATE_SEED), w1.xyz.cpu().numpy()
    h64 = segnet_np(state, nx, colors, idx, np.float64)
    h32 = segnet_np(state, nx, colors, idx, np.float32)
    tol = 4 * np.abs(h32 - h64).max() + 1e-6 * np.abs(h64).max()
    for a in (h64, h32):
        a.setflags(write=False)
    return SimpleNamespace(sims=sims, net=net, points=points, colors=cols, head=head, g1=g1, written=written, w1=w1,
                           w2=w2, h64=h64, h32=h32, tol=tol)


def test_network_shapes_come_from_the_state(run):
    net = run.net
    assert (net.num_classes, net.num_input_channels) == (4, 6)
    assert net.widths == {"sa1": [[32, 32, 64], [64, 64, 128], [64, 96, 128]], "sa2": [[128, 128, 256], [128, 196, 256]],
                          "sa3": [256, 512, 1024], "fp3": [256, 256], "fp2": [256, 128], "fp1": [128, 128],
                          "head": [128, 18]}
    assert [m.c_in for m in net.sa1] == [9] * 3 and [m.c_in for m in net.sa2] == [323] * 2
    assert (net.sa3.c_in, net.fp3.c_in, net.fp2.c_in, net.fp1.c_in, net.head.c_in) == (515, 1536, 576, 137, 128)
    assert net.head.relu == [True, False]
    assert run.head.shape == (2, N, 18) and run.head.dtype == torch.float32 and bool(torch.isfinite(run.head).all())


def test_segment_cloud_is_the_written_out_sequence_of_public_calls(run):
    assert same_bits(run.head, run.written)
    for k in ("xyz", "centroid", "scale", "fps_idx", "new_xyz"):
        assert same_bits(getattr(run.g1, k), getattr(run.w1, k)), k
    # the cloud is normalised once: level 2 samples the 512 centres as they are
    assert run.w2.centroid is None and same_bits(run.w2.xyz, run.w1.new_xyz)


def test_a_repeated_call_gives_the_same_bits(run):
    again, g1 = run.sims[2].segment_cloud(run.net, run.points, run.colors, SEED)
    assert same_bits(again, run.head) and same_bits(g1.fps_idx, run.g1.fps_idx)
    other, _ = run.sims[2].segment_cloud(run.net, run.points, run.colors, SEED + 5)
    assert not same_bits(other, run.head)  # the seed moves the sampling


def test_an_env_does_not_depend_on_its_batch(run):
    from pandasim.cloudnet import fps_start

    starts = (torch.tensor([fps_start(SEED, 1, N)], dtype=torch.int32), torch.tensor([fps_start(SEED + 1, 1, 512)],
                                                                                       dtype=torch.int32))
    assert int(run.g1.fps_idx[1, 0]) == int(starts[0][0]) and int(run.w2.fps_idx[1, 0]) == int(starts[1][0])
    alone, g1, _ = forward_by_public_calls(run.sims[1], run.net, run.points[1:2].contiguous(),
                                           run.colors[1:2].contiguous(), SEED, starts)
    assert same_bits(g1.fps_idx[0], run.g1.fps_idx[1])
    assert same_bits(alone[0], run.head[1])


def test_head_against_the_f64_restatement_on_the_gpus_own_indices(run):
    got = run.head.cpu().numpy().astype(np.float64)
    err = np.abs(got - run.h64).max()
    print(f"max |gpu - f64| = {err:.3e}, tol = {run.tol:.3e}, ratio = {err / run.tol:.3f}, "
          f"max |f32 - f64| = {np.abs(run.h32 - run.h64).max():.3e}, max |head| = {np.abs(run.h64).max():.3f}")
    assert 0 < run.tol < 1e-4 * np.abs(run.h64).max()
    assert err <= run.tol


def test_predict_waypoints_is_segment_then_decode(run):
    sim, net = run.sims[2], run.net
    pred = sim.predict_waypoints(net, run.points, run.colors, SEED)
    dec = sim.decode_waypoints(run.head, run.g1.xyz, net.num_classes, run.g1.centroid, run.g1.scale, return_labels=True)
    for k in ("waypoints", "quats", "euler_deg", "counts", "first_idx"):
        assert same_bits(getattr(pred, k), getattr(dec, k)), k
    assert pred.labels is None
    # on the GPU's own head the decode is decode_np's
    head, xyz = run.head.cpu().numpy(), run.g1.xyz.cpu().numpy()
    want = decode_np(head, xyz, NUM_CLASSES, run.g1.centroid.cpu().numpy(), run.g1.scale.cpu().numpy(),
                     (START_MASK, END_MASK))
    srt = np.sort(head[..., :NUM_CLASSES].astype(np.float64), -1)
    margin = srt[..., -1] - srt[..., -2]
    print(f"points under the margin tol = {run.tol:.3e}: {(margin <= run.tol).mean():.4f}; counts {want['counts'].tolist()}")
    assert (margin <= run.tol).mean() <= 0.02
    sure = margin > run.tol
    assert np.array_equal(dec.labels.cpu().numpy()[sure], want["labels"][sure])
    if sure.all():
        assert np.array_equal(pred.counts.cpu().numpy(), want["counts"])
        assert np.array_equal(pred.first_idx.cpu().numpy(), want["first_idx"])
    # ... and the labels are the f64 network's wherever its margin is wider than the bound
    lab64 = run.h64[..., :NUM_CLASSES].argmax(-1)
    s64 = np.sort(run.h64[..., :NUM_CLASSES], -1)
    wide = (s64[..., -1] - s64[..., -2]) > run.tol
    assert np.array_equal(dec.labels.cpu().numpy()[wide], lab64[wide])
    # a populated set has a finite waypoint, an empty one NaN
    wp = pred.waypoints.cpu().numpy()
    ok = want["counts"] > 0
    assert np.isfinite(wp[ok]).all() and np.isnan(wp[~ok]).all()
