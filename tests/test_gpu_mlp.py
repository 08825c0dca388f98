"""GPU tests of the shared MLP with max-pool (ps_cloud_mlp, ps_cloud_group_mlp,
PandaSim.shared_mlp / abstract_features).

The yardstick is tests/cloud_reference.py's numpy restatement (an exact fmaf chain
from the bias, k ascending) run on the same inputs; the kernels equal it on
every element, by value (-0 equals +0).  That restatement is held to the f64
golden recorded from the reference within a bound derived there; the golden
cases are asserted here once more on the kernels' own output through the
Python entry points.
"""
import numpy as np
import pytest
import torch

from cloud_helpers import (DEV, SENTINEL, dev, make_sims, net, random_groups, raw_call, raw_group, raw_group_mlp, raw_mlp,
                           upload)
from cloud_reference import group_rows_np, mlp_np
from test_mlp_cpu import CASES, case_of, folded, golden, restated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sims():
    """Contexts of 2 clouds (the golden's batch), of 1 and of 7."""
    return make_sims((2, 1, 7))


def same_values(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return got.shape == want.shape and got.dtype == want.dtype and bool((got == want).all())


# ----------------------------------------------------- shapes against the restatement
SHAPES = {  # name: (B, R, C0, widths, relus or None, pools)
    "trivial":        (1, 1, 1, [1], None, (1,)),
    "k9-last33":      (2, 33, 9, [33], None, (1,)),
    "k515-hidden96":  (2, 31, 515, [96, 33], None, (1, 31)),
    "k45-hidden196":  (2, 65, 45, [196, 1], None, (1, 5)),
    "four-layers":    (1, 130, 9, [32, 96, 196, 1000], None, (1, 130)),
    "one-layer":      (2, 130, 45, [64], [False], (1, 2)),
    "groups-of-3":    (2, 66, 9, [32, 33], None, (3,)),
    "group-of-128":   (2, 256, 9, [64, 64], [True, False], (128, 32, 64)),
    "group-of-all":   (2, 130, 45, [64, 128], None, (130, 65)),
    "largest-widths": (1, 40, 2051, [512, 512, 1024], None, (1, 40)),
}


@pytest.mark.parametrize("name", SHAPES)
def test_kernel_equals_the_restatement_on_every_element(sims, name):
    nb, r, c0, widths, relus, pools = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    rows = rng.normal(size=(nb, r, c0)).astype(np.float32)
    layers = net(11 + r + c0, c0, widths, relus)
    want = mlp_np(rows, layers, 1)  # unpooled once; a pool is a max over it
    mlp, x = upload(layers), dev(rows)
    for pool in pools:
        out = raw_mlp(sims[nb], x, mlp, pool)
        assert same_values(out, want.reshape(nb, r // pool, pool, -1).max(axis=2)), (name, pool)


def test_pooled_maximum_of_negative_values_is_negative(sims):
    """The last layer has no ReLU and every pre-activation is negative: a
    running maximum started at 0 would return 0."""
    rng = np.random.default_rng(3)
    rows = rng.uniform(0.5, 2.0, size=(2, 192, 9)).astype(np.float32)
    w = -rng.uniform(0.1, 1.0, size=(40, 9)).astype(np.float32)
    layers = [(w, -np.ones(40, np.float32), False)]
    mlp, x = upload(layers), dev(rows)
    for pool in (4, 64, 192):  # groups inside a tile, a group over two tiles, over six
        out = raw_mlp(sims[2], x, mlp, pool)
        assert (out < 0).all()
        assert same_values(out, mlp_np(rows, layers, pool)), pool


def test_a_layer_that_relu_kills_gives_zeros(sims):
    rng = np.random.default_rng(4)
    rows = rng.uniform(0.5, 2.0, size=(2, 40, 12)).astype(np.float32)
    dead = (-np.ones((70, 12), np.float32), -np.ones(70, np.float32), True)
    out = raw_mlp(sims[2], dev(rows), upload([dead]), 1)
    assert (out == 0).all()
    out = raw_mlp(sims[2], dev(rows), upload([dead]), 8)
    assert (out == 0).all()
    # behind a dead layer only the bias is left
    after = net(9, 70, [33], [False])
    out = raw_mlp(sims[2], dev(rows), upload([dead] + after), 1)
    assert same_values(out, np.broadcast_to(after[0][1], (2, 40, 33)).copy())


# ------------------------------------------------------- gathered rows
@pytest.mark.parametrize("d", (0, 6, 16))
def test_fused_equals_group_then_mlp_bit_for_bit(sims, d):
    xyz, feats, centre, gidx = random_groups(20 + d, 2, 200, 21, 12, d)
    layers = net(d, d + 3, [32, 96, 40])
    mlp = upload(layers)
    x, f, c, g = dev(xyz), dev(feats), dev(centre), dev(gidx)
    grouped = raw_group(sims[2], x, f, c, g)
    assert same_values(grouped, group_rows_np(xyz, feats, centre, gidx))
    composed = raw_mlp(sims[2], grouped.view(2, -1, d + 3), mlp, 12)
    fused = raw_group_mlp(sims[2], x, f, c, g, mlp)
    assert torch.equal(fused.view(torch.int32), composed.view(torch.int32))
    want = mlp_np(group_rows_np(xyz, feats, centre, gidx).reshape(2, -1, d + 3), layers, 12)
    assert same_values(fused, want)  # duplicate rows included


@pytest.mark.parametrize("k", (1, 40, 64))
def test_group_sizes_of_the_fused_call(sims, k):
    xyz, feats, centre, gidx = random_groups(30 + k, 2, 90, 5, k, 3)
    layers = net(k, 6, [64, 33])
    fused = raw_group_mlp(sims[2], dev(xyz), dev(feats), dev(centre), dev(gidx), upload(layers))
    assert same_values(fused, mlp_np(group_rows_np(xyz, feats, centre, gidx).reshape(2, -1, 6), layers, k))


def test_more_features_than_the_group_call_takes(sims):
    """D = 320 (sa2): above ps_cloud_group's 16, so against the restatement."""
    xyz, feats, centre, gidx = random_groups(41, 2, 60, 6, 5, 320)
    layers = net(5, 323, [128, 196, 40])
    fused = raw_group_mlp(sims[2], dev(xyz), dev(feats), dev(centre), dev(gidx), upload(layers))
    assert same_values(fused, mlp_np(group_rows_np(xyz, feats, centre, gidx).reshape(2, -1, 323), layers, 5))


def test_a_wild_index_is_the_clamped_one(sims):
    xyz, feats, centre, gidx = random_groups(42, 2, 77, 9, 8, 4)
    mlp = upload(net(6, 7, [32, 20]))
    wild_g, wild_c = gidx.copy(), centre.copy()
    wild_g[0, 0, 0], wild_g[0, 3, 2], wild_g[1, 8, 7], wild_g[1, 2, 1] = -5, 77, 2 ** 31 - 1, -2 ** 31
    wild_c[0, 1], wild_c[1, 8] = -1, 1000
    x, f = dev(xyz), dev(feats)
    got = raw_group_mlp(sims[2], x, f, dev(wild_c), dev(wild_g), mlp)
    want = raw_group_mlp(sims[2], x, f, dev(np.clip(wild_c, 0, 76)), dev(np.clip(wild_g, 0, 76)), mlp)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, raw_group_mlp(sims[2], x, f, dev(centre), dev(gidx), mlp))


def test_scales_land_side_by_side_and_nothing_else_is_written(sims):
    """Three scales at columns 0, 64 and 192 of one [B, S, 320] tensor: every
    column written once; in a wider tensor the rest keeps the sentinel."""
    nb, n, s, d = 2, 150, 19, 6
    ks, widths = (8, 16, 33), ([32, 32, 64], [64, 64, 128], [64, 96, 128])
    cases = [random_groups(50 + i, nb, n, s, k, d) for i, k in enumerate(ks)]
    xyz, feats, centre = cases[0][:3]
    nets = [net(60 + i, d + 3, w) for i, w in enumerate(widths)]
    mlps = [upload(layers) for layers in nets]
    x, f, c = dev(xyz), dev(feats), dev(centre)
    want = np.concatenate([mlp_np(group_rows_np(xyz, feats, centre, case[3]).reshape(nb, -1, d + 3), layers, k)
                           for case, layers, k in zip(cases, nets, ks)], -1)
    for width in (320, 333):
        out = torch.full((nb, s, width), SENTINEL, device=DEV)
        for case, mlp, off in zip(cases, mlps, (0, 64, 192)):
            before = out.clone()
            raw_group_mlp(sims[2], x, f, c, dev(case[3]), mlp, out=out, offset=off)
            changed = (out != before).any(0).any(0).cpu().numpy()
            assert not changed[:off].any() and not changed[off + mlp.widths[-1]:].any()
        assert same_values(out[:, :, :320].contiguous(), want), width
        assert (out[:, :, 320:] == SENTINEL).all()
    # the Python entry point builds the same tensor, fused and composed
    for fused in (None, True, False):
        assert same_values(sims[2].abstract_features(x, f, c, [dev(case[3]) for case in cases], mlps, fused=fused), want)
    # and ps_cloud_mlp writes at an offset as well
    rows = np.random.default_rng(1).normal(size=(nb, 24, d + 3)).astype(np.float32)
    out = torch.full((nb, 6, 100), SENTINEL, device=DEV)
    assert sims[2].shared_mlp(dev(rows), mlps[0], pool=4, out=out, out_offset=30) is out
    assert same_values(out[:, :, 30:94].contiguous(), mlp_np(rows, nets[0], 4))
    assert (out[:, :, :30] == SENTINEL).all() and (out[:, :, 94:] == SENTINEL).all()


def test_a_cloud_gives_the_same_values_in_any_batch(sims):
    xyz, feats, centre, gidx = random_groups(70, 1, 120, 11, 9, 5)
    layers = net(71, 8, [64, 96, 50])
    mlp = upload(layers)
    rows = group_rows_np(xyz, feats, centre, gidx).reshape(1, -1, 8)
    alone = raw_group_mlp(sims[1], dev(xyz), dev(feats), dev(centre), dev(gidx), mlp)
    alone_rows = raw_mlp(sims[1], dev(rows), mlp, 3)
    assert same_values(alone, mlp_np(rows, layers, 9))
    others = random_groups(72, 7, 120, 11, 9, 5)
    big = [np.array(a) for a in others]
    for env in (0, 3, 6):
        for a, one in zip(big, (xyz, feats, centre, gidx)):
            a[env] = one[0]
    got = raw_group_mlp(sims[7], *(dev(a) for a in big), mlp)
    big_rows = group_rows_np(*big).reshape(7, -1, 8)
    got_rows = raw_mlp(sims[7], dev(big_rows), mlp, 3)
    for env in (0, 3, 6):
        assert torch.equal(got[env].view(torch.int32), alone[0].view(torch.int32)), env
        assert torch.equal(got_rows[env].view(torch.int32), alone_rows[0].view(torch.int32)), env
    assert not torch.equal(got[1], alone[0])


def test_output_offsets_beyond_two_to_the_31(sims):
    """2 clouds x (2^20 + 64) rows x 1 024 channels are 2^31 + 131 072 floats:
    the second cloud's last rows lie past a 32-bit offset.  One layer, C0 = 1,
    no pooling; the rows repeat with period 64, so every block of 64 output
    rows is the first one, which is the restatement's."""
    nb, r, c = 2, 2 ** 20 + 64, 1024
    assert nb * r * c > 2 ** 31
    rng = np.random.default_rng(8)
    first = rng.normal(size=(nb, 64, 1)).astype(np.float32)
    layers = net(80, 1, [c], [False])
    rows = dev(first).repeat(1, r // 64, 1)
    out = sims[2].shared_mlp(rows, upload(layers))
    assert out.shape == (nb, r, c)
    assert same_values(out[:, :64].contiguous(), mlp_np(first, layers))
    blocks = out.view(nb, r // 64, 64, c)
    assert all(bool((blocks[b] == blocks[b, 0]).all()) for b in range(nb))


# ------------------------------------------------------------- refusals
def test_every_refusal_leaves_the_outputs_untouched(sims):
    from pandasim import _lib as L
    from pandasim.sim import _ptr

    sim = sims[2]
    xyz, feats, centre, gidx = (dev(a) for a in random_groups(90, 2, 40, 4, 4, 6))
    rows = torch.zeros(2, 16, 9, device=DEV)
    out = torch.full((2, 16, 64), SENTINEL, device=DEV)
    w = torch.zeros(1024 * 2051, device=DEV)

    def array(*c_outs, W=w, b=w):
        a = (L.CloudMlpLayer * max(len(c_outs), 1))()
        for item, c_out in zip(a, c_outs):
            item.W, item.b, item.c_out, item.relu = (None if W is None else W.data_ptr(),
                                                     None if b is None else b.data_ptr(), c_out, 1)
        return a

    def mlp(*, ctx=sim._ctx, rows=rows, R=16, C0=9, layers=array(32, 64), n=2, G=1, out=out, stride=64, offset=0):
        return raw_call(sim, "ps_cloud_mlp", ctx, _ptr(rows), R, C0, layers, n, G, _ptr(out), stride, offset, sim._stream())

    def gmlp(*, xyz=xyz, feats=feats, N=40, D=6, centre=centre, S=4, gidx=gidx, K=4, layers=array(32, 64), n=2,
             out=out, stride=64, offset=0):
        return raw_call(sim, "ps_cloud_group_mlp", sim._ctx, _ptr(xyz), _ptr(feats), N, D, _ptr(centre), S, _ptr(gidx), K,
                   layers, n, _ptr(out), stride, offset, sim._stream())

    bad_mlp = [dict(ctx=None), dict(rows=None), dict(layers=None), dict(out=None), dict(n=0), dict(n=5, layers=array(8, 8, 8, 8, 8)),
               dict(C0=0), dict(C0=2052), dict(layers=array(0, 64)), dict(layers=array(513, 64)),
               dict(layers=array(32, 1025), stride=2000), dict(layers=array(32, 0)),
               dict(layers=array(32, 64, W=None)), dict(layers=array(32, 64, b=None)),
               dict(R=0), dict(G=0), dict(G=-1), dict(R=16, G=3), dict(offset=-1), dict(offset=1), dict(stride=63),
               dict(stride=0)]
    for bad in bad_mlp:
        assert mlp(**bad) == -1, bad
    bad_gmlp = [dict(xyz=None), dict(centre=None), dict(gidx=None), dict(layers=None), dict(out=None),
                dict(feats=None), dict(D=0), dict(D=2049), dict(D=-1), dict(N=0), dict(N=8193), dict(S=0), dict(S=41),
                dict(K=0), dict(K=2 ** 30), dict(n=0), dict(n=5), dict(layers=array(600, 64)), dict(layers=array(32, 2000)),
                dict(offset=-1), dict(offset=1), dict(stride=10)]
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
        sim.abstract_features(xyz, feats, centre, [gidx], [upload(net(1, 8, [4]))])


# ------------------------------------------------------ the golden's cases
@pytest.mark.parametrize("name", CASES)
def test_python_entry_points_meet_the_golden_within_the_derived_bound(sims, name):
    g, sim = golden(), sims[2]
    parts, want = case_of(name)
    want_np, bound = restated(name)
    mlps = [upload(folded(prefix)) for _, prefix, _, _, _ in parts]
    if name == "msg":
        args = (dev(g["msg_xyz"]), dev(g["msg_feats"]), dev(g["msg_centre_idx"]),
                [dev(g["msg_group_idx0"]), dev(g["msg_group_idx1"])], mlps)
        got = sim.abstract_features(*args)
        assert torch.equal(got, sim.abstract_features(*args, fused=True))
    else:
        rows, _, pool, _, _ = parts[0]
        got = sim.shared_mlp(dev(rows), mlps[0], pool=pool)
    assert same_values(got, want_np)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"{name}: worst |kernel - golden| = {err.max():.3e}, worst error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
