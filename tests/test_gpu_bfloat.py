"""GPU tests of the bfloat16 shared MLP (ps_cloud_mlp_bfloat,
ps_cloud_group_mlp_bfloat, CloudMlp / CloudSegNet precision="bfloat16").

The yardstick is tests/bfloat_reference.py's float64 restatement of
include/pandasim.h's specification.  On dyadic data (small integers times
powers of two, every partial sum exactly representable in f32, asserted here
from |Wh| |xh| + |b|) the kernels equal it on every element, whatever the order
of the matrix core's additions; on random data they stay within the bound the
restatement carries beside its values.

The kernel as built has row tiles of 64, k steps of 16, k chunks of 512 in the
first layer and output chunks of 32 per wave, 1, 2, 4 or 8 waves: the shapes
below sit on both sides of each.
"""
import numpy as np
import pytest
import torch

from bfloat_reference import (dyadic_net, dyadic_rows, exact_in_f32, mlp_bfloat_np, mlp_bfloat_with_bound,
                              segnet_bfloat_np)
import cloud_helpers
from cloud_helpers import DEV, SENTINEL, dev, make_sims, net, random_groups, raw_call, raw_group, same_bits
from cloud_reference import group_rows_np
from test_mlp_cpu import CASES, case_of, folded, golden

pytestmark = pytest.mark.gpu


# the shared helpers at this module's precision and entry points
def upload(layers, precision="bfloat16"):
    return cloud_helpers.upload(layers, precision)


def raw_mlp(*args, **kwargs):
    return cloud_helpers.raw_mlp(*args, suffix="_bfloat", **kwargs)


def raw_group_mlp(*args, **kwargs):
    return cloud_helpers.raw_group_mlp(*args, suffix="_bfloat", **kwargs)


@pytest.fixture(scope="module")
def sims():
    return make_sims((2, 1, 7))


def equals(got, want):
    """Every element of the f32 tensor equals the f64 restatement, by value."""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return got.shape == want.shape and got.dtype == np.float32 and bool((got.astype(np.float64) == want).all())


def dyadic_groups(seed, nb, n, s, k, d):
    """random_groups with coordinates and features that are small dyadic
    numbers, so that the centred differences are exact bf16 values."""
    xyz, feats, centre, gidx = random_groups(seed, nb, n, s, k, d)
    rng = np.random.default_rng(seed + 1000)
    xyz = (rng.integers(-8, 9, size=xyz.shape) * 0.25).astype(np.float32)
    feats = None if feats is None else dyadic_rows(seed + 2000, feats.shape)
    return xyz, feats, centre, gidx


# ------------------------------------------------- exact on dyadic data
SHAPES = {  # name: (B, R, C0, widths, relus or None, pools)
    "trivial":        (1, 1, 1, [1], None, (1,)),
    "k7-last33":      (2, 33, 7, [33], None, (1, 3)),
    "k8-last1":       (2, 31, 8, [1], [False], (1, 31)),
    "k9-hidden1":     (2, 65, 9, [1, 33], None, (1, 5, 65)),
    "k15-hidden31":   (1, 130, 15, [31, 1000], None, (1, 2, 130)),
    "k16-hidden32":   (2, 64, 16, [32, 33], None, (1, 32, 64)),
    "k17-hidden33":   (2, 65, 17, [33, 1], None, (1, 65)),
    "k31-hidden96":   (2, 63, 31, [96, 33], None, (1, 3)),
    "k33-four":       (1, 130, 33, [32, 96, 196, 1000], None, (1, 130)),
    "k45-hidden196":  (2, 65, 45, [196, 1], None, (1, 5)),
    "k511":           (1, 33, 511, [33], None, (1,)),
    "k512":           (1, 33, 512, [64, 33], None, (1,)),
    "k513":           (1, 33, 513, [33], None, (1, 33)),
    "k515-hidden96":  (2, 31, 515, [96, 33], None, (1, 31)),
    "k1025":          (1, 5, 1025, [31, 33], None, (1,)),
    "groups":         (2, 384, 9, [64, 64], [True, False], (128, 32, 64, 192)),
    "group-of-all":   (2, 130, 45, [64, 128], None, (130, 65)),
    "largest-widths": (1, 40, 2051, [512, 512, 1024], None, (1, 40)),
    "four-largest":   (1, 5, 9, [512, 512, 512, 1024], None, (1, 5)),
}


@pytest.mark.parametrize("name", SHAPES)
def test_kernel_equals_the_restatement_on_dyadic_data(sims, name):
    nb, r, c0, widths, relus, pools = SHAPES[name]
    seed = sum(map(ord, name))
    rows, layers = dyadic_rows(seed, (nb, r, c0)), dyadic_net(seed + 1, c0, widths, relus)
    assert exact_in_f32(rows, layers)
    want = mlp_bfloat_np(rows, layers, 1)  # unpooled once; a pool is a max over it
    assert np.abs(want).max() > 0
    mlp, x = upload(layers), dev(rows)
    for pool in pools:
        out = raw_mlp(sims[nb], x, mlp, pool)
        assert equals(out, want.reshape(nb, r // pool, pool, -1).max(axis=2)), (name, pool)


@pytest.mark.parametrize("d,k", ((0, 12), (6, 12), (16, 33), (320, 5), (13, 65), (509, 2), (510, 3)))
def test_gathered_rows_equal_the_restatement_on_dyadic_data(sims, d, k):
    xyz, feats, centre, gidx = dyadic_groups(20 + d, 2, 60, 7, k, d)
    layers = dyadic_net(d, d + 3, [32, 96, 40])
    rows = group_rows_np(xyz, feats, centre, gidx).reshape(2, -1, d + 3)
    assert exact_in_f32(rows, layers)
    fused = raw_group_mlp(sims[2], dev(xyz), dev(feats), dev(centre), dev(gidx), upload(layers))
    assert equals(fused, mlp_bfloat_np(rows, layers, k))  # duplicate rows included


# --------------------------------------------------------- random data
@pytest.mark.parametrize("c0,c_out,r", ((1, 33, 65), (9, 64, 130), (45, 33, 65), (323, 128, 70), (515, 96, 33),
                                        (2051, 512, 40), (2051, 1024, 3)))
def test_one_layer_within_the_accumulation_bound(sims, c0, c_out, r):
    """|gpu - exact sum| <= (c_in + 1) 2^-23 (|Wh| |xh| + |b|) on every element."""
    rng = np.random.default_rng(c0 + c_out)
    rows = rng.normal(size=(2, r, c0)).astype(np.float32)
    layers = net(c0, c0, [c_out], [False])
    want, bound = mlp_bfloat_with_bound(rows, layers)
    got = raw_mlp(sims[2], dev(rows), upload(layers)).cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print(f"c_in = {c0}: worst |gpu - f64| = {err.max():.3e}, worst error / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("widths", ([96, 40], [64, 196, 33], [32, 96, 196, 100]))
def test_layers_within_the_carried_bound(sims, widths):
    rng = np.random.default_rng(len(widths))
    rows = rng.normal(size=(2, 130, 45)).astype(np.float32)
    layers = net(7 + len(widths), 45, widths)
    mlp = upload(layers)
    for pool in (1, 65):
        want, bound = mlp_bfloat_with_bound(rows, layers, pool)
        got = sims[2].shared_mlp(dev(rows), mlp, pool=pool).cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        print(f"{len(widths)} layers, pool {pool}: worst error / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all()


@pytest.mark.parametrize("name", CASES)
def test_python_entry_points_on_the_golden_cases(sims, name):
    g, sim = golden(), sims[2]
    parts, golden64 = case_of(name)
    mlps = [upload(folded(prefix)) for _, prefix, _, _, _ in parts]
    want, bound = np.zeros(golden64.shape), np.zeros(golden64.shape)
    for rows, prefix, pool, off, _ in parts:
        y, e = mlp_bfloat_with_bound(rows, folded(prefix), pool)
        want[..., off:off + y.shape[-1]], bound[..., off:off + y.shape[-1]] = y, e
    if name == "msg":
        args = (dev(g["msg_xyz"]), dev(g["msg_feats"]), dev(g["msg_centre_idx"]),
                [dev(g["msg_group_idx0"]), dev(g["msg_group_idx1"])], mlps)
        got = sim.abstract_features(*args)
        assert same_bits(got, sim.abstract_features(*args, fused=True))
        assert same_bits(got, sim.abstract_features(*args, fused=False))
    else:
        rows, _, pool, _, _ = parts[0]
        got = sim.shared_mlp(dev(rows), mlps[0], pool=pool)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"{name}: worst error / bound = {(err / bound).max():.4f}; against the f64 golden "
          f"{np.abs(got.cpu().numpy() - golden64).max():.3e} of max {np.abs(golden64).max():.3f}")
    assert (err <= bound).all()


# ------------------------------------------- what the f32 file pins, restated
def test_pooled_maximum_of_negative_values_is_negative(sims):
    rng = np.random.default_rng(3)
    rows = rng.integers(1, 4, size=(2, 192, 9)).astype(np.float32)
    w = -rng.integers(1, 3, size=(40, 9)).astype(np.float32)
    layers = [(w, -np.ones(40, np.float32), False)]
    mlp, x = upload(layers), dev(rows)
    for pool in (4, 64, 96, 192):  # groups inside a tile, a whole tile, over two tiles, over three
        out = raw_mlp(sims[2], x, mlp, pool)
        assert (out < 0).all()
        assert equals(out, mlp_bfloat_np(rows, layers, pool)), pool


def test_a_layer_that_relu_kills_gives_zeros(sims):
    rng = np.random.default_rng(4)
    rows = rng.uniform(0.5, 2.0, size=(2, 40, 12)).astype(np.float32)
    dead = (-np.ones((70, 12), np.float32), -np.ones(70, np.float32), True)
    assert (raw_mlp(sims[2], dev(rows), upload([dead]), 1) == 0).all()
    assert (raw_mlp(sims[2], dev(rows), upload([dead]), 8) == 0).all()
    after = net(9, 70, [33], [False])  # behind a dead layer only the bias is left
    out = raw_mlp(sims[2], dev(rows), upload([dead] + after), 1)
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to(after[0][1], (2, 40, 33)))


@pytest.mark.parametrize("d", (0, 6, 16))
def test_fused_equals_group_then_mlp_bit_for_bit(sims, d):
    xyz, feats, centre, gidx = random_groups(20 + d, 2, 200, 21, 12, d)  # duplicate rows included
    layers = net(d, d + 3, [32, 96, 40])
    mlp = upload(layers)
    x, f, c, g = dev(xyz), dev(feats), dev(centre), dev(gidx)
    grouped = raw_group(sims[2], x, f, c, g)
    composed = raw_mlp(sims[2], grouped.view(2, -1, d + 3), mlp, 12)
    fused = raw_group_mlp(sims[2], x, f, c, g, mlp)
    assert same_bits(fused, composed)
    for flag in (None, True, False):
        assert same_bits(sims[2].abstract_features(x, f, c, [g], [mlp], fused=flag), fused)
    want, bound = mlp_bfloat_with_bound(group_rows_np(xyz, feats, centre, gidx).reshape(2, -1, d + 3), layers, 12)
    assert (np.abs(fused.cpu().numpy().astype(np.float64) - want) <= bound).all()


def test_a_wild_index_is_the_clamped_one(sims):
    xyz, feats, centre, gidx = random_groups(42, 2, 77, 9, 8, 4)
    mlp = upload(net(6, 7, [32, 20]))
    wild_g, wild_c = gidx.copy(), centre.copy()
    wild_g[0, 0, 0], wild_g[0, 3, 2], wild_g[1, 8, 7], wild_g[1, 2, 1] = -5, 77, 2 ** 31 - 1, -2 ** 31
    wild_c[0, 1], wild_c[1, 8] = -1, 1000
    x, f = dev(xyz), dev(feats)
    got = raw_group_mlp(sims[2], x, f, dev(wild_c), dev(wild_g), mlp)
    want = raw_group_mlp(sims[2], x, f, dev(np.clip(wild_c, 0, 76)), dev(np.clip(wild_g, 0, 76)), mlp)
    assert same_bits(got, want)
    assert not same_bits(got, raw_group_mlp(sims[2], x, f, dev(centre), dev(gidx), mlp))


def test_scales_land_side_by_side_and_nothing_else_is_written(sims):
    nb, n, s, d = 2, 150, 19, 6
    ks, widths = (8, 16, 33), ([32, 32, 64], [64, 64, 128], [64, 96, 128])
    cases = [dyadic_groups(50 + i, nb, n, s, k, d) for i, k in enumerate(ks)]
    xyz, feats, centre = cases[0][:3]
    nets = [dyadic_net(60 + i, d + 3, w) for i, w in enumerate(widths)]
    mlps = [upload(layers) for layers in nets]
    x, f, c = dev(xyz), dev(feats), dev(centre)
    rows = [group_rows_np(xyz, feats, centre, case[3]).reshape(nb, -1, d + 3) for case in cases]
    assert all(exact_in_f32(r, layers) for r, layers in zip(rows, nets))
    want = np.concatenate([mlp_bfloat_np(r, layers, k) for r, layers, k in zip(rows, nets, ks)], -1)
    for width in (320, 333):
        out = torch.full((nb, s, width), SENTINEL, device=DEV)
        for case, mlp, off in zip(cases, mlps, (0, 64, 192)):
            before = out.clone()
            raw_group_mlp(sims[2], x, f, c, dev(case[3]), mlp, out=out, offset=off)
            changed = (out != before).any(0).any(0).cpu().numpy()
            assert not changed[:off].any() and not changed[off + mlp.widths[-1]:].any()
        assert equals(out[:, :, :320].contiguous(), want), width
        assert (out[:, :, 320:] == SENTINEL).all()
    for fused in (None, True, False):
        assert equals(sims[2].abstract_features(x, f, c, [dev(case[3]) for case in cases], mlps, fused=fused), want)
    out = torch.full((nb, 6, 100), SENTINEL, device=DEV)
    r24 = dyadic_rows(1, (nb, 24, d + 3))
    assert sims[2].shared_mlp(dev(r24), mlps[0], pool=4, out=out, out_offset=30) is out
    assert equals(out[:, :, 30:94].contiguous(), mlp_bfloat_np(r24, nets[0], 4))
    assert (out[:, :, :30] == SENTINEL).all() and (out[:, :, 94:] == SENTINEL).all()


def test_a_cloud_gives_the_same_bits_in_any_batch_and_on_a_repeated_call(sims):
    xyz, feats, centre, gidx = random_groups(70, 1, 120, 11, 9, 5)
    mlp = upload(net(71, 8, [64, 96, 50]))
    rows = group_rows_np(xyz, feats, centre, gidx).reshape(1, -1, 8)
    alone = raw_group_mlp(sims[1], dev(xyz), dev(feats), dev(centre), dev(gidx), mlp)
    alone_rows = raw_mlp(sims[1], dev(rows), mlp, 3)
    assert same_bits(alone, raw_group_mlp(sims[1], dev(xyz), dev(feats), dev(centre), dev(gidx), mlp))
    assert same_bits(alone_rows, raw_mlp(sims[1], dev(rows), mlp, 3))
    big = [np.array(a) for a in random_groups(72, 7, 120, 11, 9, 5)]
    for env in (0, 3, 6):
        for a, one in zip(big, (xyz, feats, centre, gidx)):
            a[env] = one[0]
    got = raw_group_mlp(sims[7], *(dev(a) for a in big), mlp)
    got_rows = raw_mlp(sims[7], dev(group_rows_np(*big).reshape(7, -1, 8)), mlp, 3)
    for env in (0, 3, 6):
        assert same_bits(got[env], alone[0]) and same_bits(got_rows[env], alone_rows[0]), env
    assert not same_bits(got[1], alone[0])


def test_every_refusal_leaves_the_outputs_untouched(sims):
    from pandasim import _lib as L
    from pandasim.sim import _ptr

    sim = sims[2]
    xyz, feats, centre, gidx = (dev(a) for a in random_groups(90, 2, 40, 4, 4, 6))
    rows = torch.zeros(2, 16, 9, device=DEV)
    out = torch.full((2, 16, 64), SENTINEL, device=DEV)
    w = torch.zeros(1024 * 2056, dtype=torch.int16, device=DEV)
    b = torch.zeros(1024, device=DEV)
    assert w.data_ptr() % 16 == 0

    def array(*c_outs, W=w.data_ptr(), bias=b.data_ptr()):
        a = (L.CloudMlpBfloatLayer * max(len(c_outs), 1))()
        for item, c_out in zip(a, c_outs):
            item.W, item.b, item.c_out, item.relu = W, bias, c_out, 1
        return a

    def mlp(*, ctx=sim._ctx, rows=rows, R=16, C0=9, layers=array(32, 64), n=2, G=1, out=out, stride=64, offset=0):
        return raw_call(sim, "ps_cloud_mlp_bfloat", ctx, _ptr(rows), R, C0, layers, n, G, _ptr(out), stride, offset,
                        sim._stream())

    def gmlp(*, xyz=xyz, feats=feats, N=40, D=6, centre=centre, S=4, gidx=gidx, K=4, layers=array(32, 64), n=2,
             out=out, stride=64, offset=0):
        return raw_call(sim, "ps_cloud_group_mlp_bfloat", sim._ctx, _ptr(xyz), _ptr(feats), N, D, _ptr(centre), S,
                        _ptr(gidx), K, layers, n, _ptr(out), stride, offset, sim._stream())

    misaligned = [array(32, 64, W=w.data_ptr() + off) for off in (2, 4, 8)]
    bad_mlp = [dict(ctx=None), dict(rows=None), dict(layers=None), dict(out=None), dict(n=0),
               dict(n=5, layers=array(8, 8, 8, 8, 8)), dict(C0=0), dict(C0=2052), dict(layers=array(0, 64)),
               dict(layers=array(513, 64)), dict(layers=array(32, 1025), stride=2000), dict(layers=array(32, 0)),
               dict(layers=array(32, 64, W=None)), dict(layers=array(32, 64, bias=None)),
               dict(R=0), dict(G=0), dict(G=-1), dict(R=16, G=3), dict(offset=-1), dict(offset=1), dict(stride=63),
               dict(stride=0)] + [dict(layers=a) for a in misaligned]
    for bad in bad_mlp:
        assert mlp(**bad) == -1, bad
    bad_gmlp = [dict(xyz=None), dict(centre=None), dict(gidx=None), dict(layers=None), dict(out=None),
                dict(feats=None), dict(D=0), dict(D=2049), dict(D=-1), dict(N=0), dict(N=8193), dict(S=0), dict(S=41),
                dict(K=0), dict(K=2 ** 30), dict(n=0), dict(n=5), dict(layers=array(600, 64)), dict(layers=array(32, 2000)),
                dict(offset=-1), dict(offset=1), dict(stride=10)] + [dict(layers=a) for a in misaligned]
    for bad in bad_gmlp:
        assert gmlp(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # the limits themselves pass: the largest network, D = 2048
    assert mlp(C0=9, layers=array(512, 512, 512, 1024), n=4, out=torch.empty(2, 16, 1024, device=DEV), stride=1024) == 0
    assert gmlp(feats=torch.zeros(2, 40, 2048, device=DEV), D=2048, layers=array(512, 1024), n=2,
                out=torch.empty(2, 4, 1024, device=DEV), stride=1024) == 0
    torch.cuda.synchronize()
    # and the Python layer raises before the library is called
    with pytest.raises(ValueError):
        sim.shared_mlp(rows, upload(net(1, 8, [4])))
    with pytest.raises(ValueError):
        sim.abstract_features(xyz, feats, centre, [gidx, gidx], [upload(net(1, 9, [4])),
                                                                 upload(net(1, 9, [4]), "float32")])


# ------------------------------------------------------------ the network
SEED, N = 3, 600


@pytest.fixture(scope="module")
def run():
    from types import SimpleNamespace

    from net_helpers import STATE_SEED, seeded_state
    from pandasim import CloudSegNet
    from test_gpu_net import forward_by_public_calls
    from test_net_cpu import golden as net_golden

    sims = make_sims((2,))
    g, rng = net_golden(), np.random.default_rng(77)
    second = rng.uniform(-1, 1, (N, 3)) * [0.35, 0.35, 0.05]
    xyz = np.stack([g["xyz"][0], second]).astype(np.float32) * np.float32(0.4) + np.array([0.1, -0.2, 0.5], np.float32)
    colors = np.stack([g["colors"][0], rng.random((N, 3)).astype(np.float32)])
    state = seeded_state(STATE_SEED)
    net16, net32 = CloudSegNet(state, DEV, precision="bfloat16"), CloudSegNet(state, DEV)
    points, cols = dev(xyz), dev(colors)
    head32_before, _ = sims[2].segment_cloud(net32, points, cols, SEED)
    head, g1 = sims[2].segment_cloud(net16, points, cols, SEED)
    written, w1, w2 = forward_by_public_calls(sims[2], net16, points, cols, SEED)
    head32_after, _ = sims[2].segment_cloud(net32, points, cols, SEED)
    torch.cuda.synchronize()
    return SimpleNamespace(sim=sims[2], net16=net16, net32=net32, points=points, colors=cols, colors_np=colors,
                           state=state, head=head, g1=g1, written=written, w1=w1, w2=w2, head32=head32_before,
                           head32_after=head32_after)


def test_bfloat_net_is_the_written_out_sequence_of_public_calls(run):
    assert run.head.shape == (2, N, 18) and bool(torch.isfinite(run.head).all())
    assert same_bits(run.head, run.written)
    for k in ("xyz", "centroid", "scale", "fps_idx", "new_xyz"):
        assert same_bits(getattr(run.g1, k), getattr(run.w1, k)), k
    again, _ = run.sim.segment_cloud(run.net16, run.points, run.colors, SEED)
    assert same_bits(again, run.head)


def test_float_net_keeps_its_bits_beside_the_bfloat_one(run):
    assert same_bits(run.head32, run.head32_after)
    assert not same_bits(run.head32, run.head)
    diff = (run.head32 - run.head).abs().max().item()
    print(f"max |bf16 head - f32 head| = {diff:.3e} of max |head| {run.head32.abs().max().item():.3f}")


def test_bfloat_head_within_the_carried_bound_of_the_restatement(run):
    idx = dict(fps1=run.w1.fps_idx.cpu().numpy(), group1=[t.cpu().numpy() for t in run.w1.group_idx],
               fps2=run.w2.fps_idx.cpu().numpy(), group2=[t.cpu().numpy() for t in run.w2.group_idx])
    want, bound = segnet_bfloat_np(run.state, run.w1.xyz.cpu().numpy(), run.colors_np, idx)
    err = np.abs(run.head.cpu().numpy().astype(np.float64) - want)
    print(f"max |gpu - restatement| = {err.max():.3e}, bound at most {bound.max():.3e}, worst error / bound = "
          f"{(err / bound).max():.4f}, max |head| = {np.abs(want).max():.3f}")
    assert np.isfinite(bound).all() and (err <= bound).all()


def test_predict_waypoints_is_segment_then_decode(run):
    pred = run.sim.predict_waypoints(run.net16, run.points, run.colors, SEED)
    dec = run.sim.decode_waypoints(run.head, run.g1.xyz, run.net16.num_classes, run.g1.centroid, run.g1.scale)
    for k in ("waypoints", "quats", "euler_deg", "counts", "first_idx"):
        assert same_bits(getattr(pred, k), getattr(dec, k)), k
