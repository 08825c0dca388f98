"""GPU tests of the PointNet++ front end (ps_cloud_normalize / _fps /
_ball_query / _group / _set_abstraction, PandaSim.group_cloud).

Two yardsticks, both exact: the golden recorded from the reference's
pointnet2_utils.py (tests/golden/group_golden.npz; ball-query rows marked
ambiguous there are skipped, and only those) and tests/cloud_reference.py's
numpy restatement run on the same inputs, which uses the kernels' own
comparison and excuses no row.  Only the normalisation has a tolerance:
2 * eps_f32 * max|value| against an f64 pc_normalize of the same f32 input (one
f32 rounding of the centroid, one subtraction, one division).
"""
import numpy as np
import pytest
import torch

from cloud_helpers import DEV, dev, make_sims, raw_call, raw_group, same_bits
from cloud_reference import ball_query_np, fps_np, group_rows_np, normalize_np
from test_group_cpu import CASES, QUERY_CASES, assert_matches_golden, case_of, restated

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def sims():
    """Contexts of 3 clouds (the golden's batch) and of 1."""
    return make_sims((3, 1))


# ------------------------------------------------ the raw calls (ctypes)
def raw_normalize(sim, pts, check=True):
    from pandasim.sim import _ptr

    nb, n = pts.shape[:2]
    out = (torch.empty(nb, n, 3, device=DEV), torch.empty(nb, 3, device=DEV), torch.empty(nb, device=DEV))
    rc = raw_call(sim, "ps_cloud_normalize", sim._ctx, _ptr(pts), n, *(_ptr(t) for t in out), sim._stream())
    assert not check or rc == 0
    return out


def raw_fps(sim, xyz, start, s):
    from pandasim.sim import _ptr

    idx = torch.empty(xyz.shape[0], s, dtype=torch.int32, device=DEV)
    assert raw_call(sim, "ps_cloud_fps", sim._ctx, _ptr(xyz), xyz.shape[1], _ptr(start), s, _ptr(idx), sim._stream()) == 0
    return idx


def raw_query(sim, xyz, centre_idx, radius, nsample):
    from pandasim.sim import _ptr

    nb, s = centre_idx.shape
    gidx = torch.empty(nb, s, nsample, dtype=torch.int32, device=DEV)
    assert raw_call(sim, "ps_cloud_ball_query", sim._ctx, _ptr(xyz), xyz.shape[1], _ptr(centre_idx), s, float(radius),
               nsample, _ptr(gidx), sim._stream()) == 0
    return gidx


# -------------------------------------------------------------------- FPS
@pytest.mark.parametrize("name", CASES)
def test_fps_equals_the_golden(sims, name):
    c = case_of(name)
    idx = raw_fps(sims[3], dev(c["xyz"]), dev(c["start"]), c["fps_idx"].shape[1])
    assert np.array_equal(idx.cpu().numpy(), c["fps_idx"])


def test_largest_cloud_the_entry_points_take(sims):
    """N = 8 192: every lane of the FPS block owns 8 points, 96 KiB of LDS."""
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-0.5, 0.5, size=(3, 8192, 3)).astype(np.float32)
    xyz[:, 8000:] = xyz[:, :192]  # duplicates across lanes
    start = np.array([0, 8191, 4096], np.int32)
    idx = raw_fps(sims[3], dev(xyz), dev(start), 8)
    want = np.stack([fps_np(xyz[b], start[b], 8) for b in range(3)])
    assert np.array_equal(idx.cpu().numpy(), want)
    gidx = raw_query(sims[3], dev(xyz), idx, 0.1, 8).cpu().numpy()
    assert np.array_equal(gidx, np.stack([ball_query_np(xyz[b], want[b], 0.1, 8) for b in range(3)]))


# --------------------------------------------------- ball query and group
@pytest.mark.parametrize("name", QUERY_CASES)
def test_ball_query_and_group_equal_the_golden_and_the_restatement(sims, name):
    c, r = case_of(name), restated(name)
    xyz, feats, cidx = dev(c["xyz"]), dev(c["feats"]), dev(c["fps_idx"])
    for k, (radius, nsample) in enumerate(c["scales"]):
        gidx = raw_query(sims[3], xyz, cidx, radius, nsample)
        grouped, new_xyz = raw_group(sims[3], xyz, feats, cidx, gidx, new_xyz=True)
        g, gr = gidx.cpu().numpy(), grouped.cpu().numpy()
        assert_matches_golden(name, k, g, gr, "kernels")
        # every row, against the restatement (the golden's centres are its own: test_group_cpu)
        assert np.array_equal(g, r[f"group_idx_{k}"]), (name, k)
        assert np.array_equal(gr.view(np.uint32), r[f"grouped_{k}"].view(np.uint32)), (name, k)
        want_new = np.stack([c["xyz"][b][c["fps_idx"][b]] for b in range(3)])
        assert np.array_equal(new_xyz.cpu().numpy(), want_new)
        # without features: the centred coordinates alone
        bare, _ = raw_group(sims[3], xyz, None, cidx, gidx, new_xyz=True)
        assert np.array_equal(bare.cpu().numpy().view(np.uint32), r[f"grouped_{k}"][..., 4:].view(np.uint32))


def test_nsample_beyond_the_cloud_pads_with_the_first(sims):
    c = case_of("A")
    cidx = dev(c["fps_idx"])
    gidx = raw_query(sims[3], dev(c["xyz"]), cidx, 0.4, 300).cpu().numpy()  # N = 257 < 300
    want = np.stack([ball_query_np(c["xyz"][b], c["fps_idx"][b], 0.4, 300) for b in range(3)])
    assert np.array_equal(gidx, want)


# -------------------------------------------------------------- normalise
def test_normalize_within_two_eps_of_f64(sims):
    rng = np.random.default_rng(11)
    worst = {}
    for name in ("A", "E"):
        raw = (case_of(name)["xyz"] * np.float32(0.37) + np.array([0.21, -0.13, 0.33], np.float32)).astype(np.float32)
        raw += rng.normal(0, 1e-3, raw.shape).astype(np.float32)
        xyz, cen, sc = (t.cpu().numpy() for t in raw_normalize(sims[3], dev(raw)))
        for b in range(3):
            wx, wc, ws = normalize_np(raw[b])
            for what, got, want in (("xyz", xyz[b], wx), ("centroid", cen[b], wc), ("scale", sc[b], ws)):
                err = float(np.abs(got.astype(np.float64) - want).max())
                bound = 2 * EPS * float(np.abs(want).max())
                worst[what] = max(worst.get(what, 0.0), err / bound)
                print(f"case {name} cloud {b} {what}: worst error {err:.3e}, bound {bound:.3e}")
                assert err <= bound, (name, b, what, err, bound)
    print("worst error / bound:", {k: round(v, 3) for k, v in worst.items()})


def test_normalize_of_a_zero_scale_cloud_is_zero(sims):
    pts = torch.zeros(3, 64, 3, device=DEV)  # env 0: the empty cloud's zeros
    pts[1] = torch.tensor([0.25, -1.5, 3.0], device=DEV)  # all points equal
    pts[2] = torch.rand(64, 3, device=DEV)
    xyz, cen, sc = raw_normalize(sims[3], pts)
    assert bool(torch.isfinite(xyz).all()) and bool(torch.isfinite(sc).all())
    assert not xyz[:2].any() and not sc[:2].any() and float(sc[2]) > 0
    assert torch.equal(cen[1], pts[1, 0]) and not cen[0].any()
    assert abs(float(xyz[2].norm(dim=-1).max()) - 1.0) <= 2 * EPS


# ----------------------------------------------------- fused and composed
@pytest.mark.parametrize("normalize", (False, True), ids=("as-is", "normalize"))
@pytest.mark.parametrize("with_feats", (False, True), ids=("xyz", "feats"))
@pytest.mark.parametrize("name", QUERY_CASES)
def test_fused_equals_the_four_calls_composed(sims, name, with_feats, normalize):
    c, sim = case_of(name), sims[3]
    pts, start = dev(c["xyz"] * np.float32(0.8) if normalize else c["xyz"]), dev(c["start"])
    feats = dev(c["feats"]) if with_feats else None
    s = c["fps_idx"].shape[1]
    radii, nsamples = [r for r, _ in c["scales"]], [k for _, k in c["scales"]]
    got = sim.group_cloud(pts, feats, npoint=s, radii=radii, nsamples=nsamples, normalize=normalize, start=start)
    xyz = pts
    if normalize:
        xyz, cen, sc = raw_normalize(sim, pts)
        assert same_bits(got.xyz, xyz) and same_bits(got.centroid, cen) and same_bits(got.scale, sc)
    else:
        assert got.centroid is None and got.scale is None and got.xyz.data_ptr() == pts.data_ptr()
    idx = raw_fps(sim, xyz, start, s)
    assert same_bits(got.fps_idx, idx)
    if not normalize:
        assert np.array_equal(idx.cpu().numpy(), c["fps_idx"])
    for k, (radius, nsample) in enumerate(c["scales"]):
        gidx = raw_query(sim, xyz, idx, radius, nsample)
        grouped, new_xyz = raw_group(sim, xyz, feats, idx, gidx, new_xyz=True)
        assert same_bits(got.group_idx[k], gidx), (name, k)
        assert same_bits(got.grouped[k], grouped), (name, k)
        assert same_bits(got.new_xyz, new_xyz)
        assert got.grouped[k].shape == (3, s, nsample, (4 if with_feats else 0) + 3)


def _fields(g):
    return [g.xyz, g.centroid, g.scale, g.fps_idx, g.new_xyz, *g.group_idx, *g.grouped]


def test_a_clouds_result_does_not_depend_on_the_batch(sims):
    c = case_of("B")
    kw = dict(npoint=128, radii=(0.1, 0.2, 0.4), nsamples=(32, 64, 128))
    pts, feats = c["xyz"] * np.float32(0.8), c["feats"]
    full = _fields(sims[3].group_cloud(dev(pts), dev(feats), start=dev(c["start"]), **kw))
    perm = [2, 0, 1]
    mixed = _fields(sims[3].group_cloud(dev(pts[perm]), dev(feats[perm]), start=dev(c["start"][perm]), **kw))
    for b in range(3):
        alone = _fields(sims[1].group_cloud(dev(pts[b:b + 1]), dev(feats[b:b + 1]), start=dev(c["start"][b:b + 1]),
                                            **kw))
        for f, (x, y, z) in enumerate(zip(full, alone, mixed)):
            assert same_bits(x[b], y[0]), (b, f)
            assert same_bits(x[b], z[perm.index(b)]), (b, f)


def test_same_seed_repeats_and_the_start_is_the_counter_draw(sims):
    from pandasim.cloudnet import fps_start
    from test_cloud_cpu import rank

    c = case_of("B")
    pts = dev(c["xyz"])
    kw = dict(npoint=16, radii=(0.2,), nsamples=(8,), normalize=False)
    a, b = sims[3].group_cloud(pts, seed=9, **kw), sims[3].group_cloud(pts, seed=9, **kw)
    other = sims[3].group_cloud(pts, seed=10, **kw)
    for x, y in zip(_fields(a)[3:], _fields(b)[3:]):
        assert same_bits(x, y)
    assert not torch.equal(a.fps_idx, other.fps_idx)
    for seed, g in ((9, a), (10, other)):
        want = [rank(seed, env, 1000) for env in range(3)]  # the cloud's draw of counter env, in a cloud of N
        assert g.fps_idx[:, 0].tolist() == want == [fps_start(seed, env, 1000) for env in range(3)]


# ------------------------------------------------------------- end to end
def test_point_cloud_into_group_cloud():
    import pandasim
    from pandasim.envs import PandaVecEnv

    env = PandaVecEnv("push", "sparse", "ee", 1, DEV, autoreset=False)
    env.reset(seed=31)
    env.step(torch.zeros(1, env.action_dim, device=DEV))
    K = 257
    cloud = env.point_cloud(list(pandasim.GRASP_VIEWS[:2]), n_points=K, width=64, height=48, seed=3)
    assert int(cloud["count"][0]) > 0
    g = env.group_cloud(cloud["points"], cloud["colors"].float(), npoint=32, radii=(0.2,), nsamples=(16,), seed=4)
    assert g.grouped[0].shape == (1, 32, 16, 6)
    xyz = g.xyz[0].cpu().numpy()
    wx, wc, ws = normalize_np(cloud["points"][0].cpu().numpy())
    assert np.abs(xyz - wx).max() <= 2 * EPS * np.abs(wx).max()
    from pandasim.cloudnet import fps_start

    idx = fps_np(xyz, fps_start(4, 0, K), 32)
    gidx = ball_query_np(xyz, idx, 0.2, 16)
    assert np.array_equal(g.fps_idx[0].cpu().numpy(), idx)
    assert np.array_equal(g.group_idx[0][0].cpu().numpy(), gidx)
    want = group_rows_np(xyz[None], cloud["colors"].float().cpu().numpy(), idx[None], gidx[None])[0]
    assert np.array_equal(g.grouped[0][0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(g.new_xyz[0].cpu().numpy(), xyz[idx])
    got = g.group_idx[0][0].cpu().numpy()
    assert got.min() >= 0 and got.max() < K
    d = xyz[got[:, 0]] - xyz[idx]
    assert bool((np.sqrt((d.astype(np.float64) ** 2).sum(-1)) <= 0.2 + 1e-6).all())


# -------------------------------------------------------- argument errors
def test_argument_errors_leave_the_outputs_untouched(sims):
    from pandasim import _lib as L
    from pandasim.sim import _ptr

    sim, c = sims[3], case_of("A")
    n, s = 257, 64
    xyz, feats, start, cidx = dev(c["xyz"]), dev(c["feats"]), dev(c["start"]), dev(c["fps_idx"])
    st, ctx, p = sim._stream(), sim._ctx, _ptr
    idx = torch.full((3, s), -7, dtype=torch.int32, device=DEV)
    gidx = torch.full((3, s, 16), -7, dtype=torch.int32, device=DEV)
    out = torch.full((3, s, 16, 7), -7.0, device=DEV)
    nx = torch.full((3, s, 3), -7.0, device=DEV)
    o3, cen, sc = torch.full((3, n, 3), -7.0, device=DEV), torch.full((3, 3), -7.0, device=DEV), \
        torch.full((3,), -7.0, device=DEV)
    inf, nan = float("inf"), float("nan")
    scale = (L.CloudScale * 1)()
    scale[0].radius, scale[0].nsample, scale[0].group_idx, scale[0].grouped = 0.2, 16, gidx.data_ptr(), out.data_ptr()

    def fused(points=xyz, f=feats, n_=n, d=4, s_=s, scales=scale, n_scales=1, normalize=1, x=o3, fidx=idx,
              start_=start, context=ctx):
        return raw_call(sim, "ps_cloud_set_abstraction", context, p(points), p(f), n_, d, p(start_), s_, scales, n_scales,
                   normalize, p(x), p(cen), p(sc), p(fidx), p(nx), st)

    def with_scale(radius, nsample, group_idx=gidx):
        bad = (L.CloudScale * 1)()
        bad[0].radius, bad[0].nsample, bad[0].grouped = radius, nsample, out.data_ptr()
        bad[0].group_idx = None if group_idx is None else group_idx.data_ptr()
        return bad

    codes = [
        raw_call(sim, "ps_cloud_normalize", None, p(xyz), n, p(o3), p(cen), p(sc), st),
        raw_call(sim, "ps_cloud_normalize", ctx, None, n, p(o3), p(cen), p(sc), st),
        raw_call(sim, "ps_cloud_normalize", ctx, p(xyz), n, None, p(cen), p(sc), st),
        raw_call(sim, "ps_cloud_normalize", ctx, p(xyz), 0, p(o3), p(cen), p(sc), st),
        raw_call(sim, "ps_cloud_normalize", ctx, p(xyz), 8193, p(o3), p(cen), p(sc), st),
        raw_call(sim, "ps_cloud_fps", ctx, p(xyz), n, p(start), 0, p(idx), st),  # S < 1
        raw_call(sim, "ps_cloud_fps", ctx, p(xyz), n, p(start), n + 1, p(idx), st),  # S > N
        raw_call(sim, "ps_cloud_fps", ctx, p(xyz), 8193, p(start), s, p(idx), st),
        raw_call(sim, "ps_cloud_fps", ctx, p(xyz), 0, p(start), 0, p(idx), st),
        raw_call(sim, "ps_cloud_fps", ctx, p(xyz), n, None, s, p(idx), st),
        raw_call(sim, "ps_cloud_fps", ctx, p(xyz), n, p(start), s, None, st),
    ]
    for radius, nsample in ((0.0, 16), (-0.2, 16), (inf, 16), (nan, 16), (0.2, 0), (0.2, -3)):
        codes.append(raw_call(sim, "ps_cloud_ball_query", ctx, p(xyz), n, p(cidx), s, radius, nsample, p(gidx), st))
        codes.append(fused(scales=with_scale(radius, nsample)))
    codes += [
        raw_call(sim, "ps_cloud_ball_query", ctx, p(xyz), n, p(cidx), n + 1, 0.2, 16, p(gidx), st),
        raw_call(sim, "ps_cloud_ball_query", ctx, p(xyz), n, None, s, 0.2, 16, p(gidx), st),
        raw_call(sim, "ps_cloud_group", ctx, p(xyz), p(feats), n, 17, p(cidx), s, p(gidx), 16, p(out), p(nx), st),
        raw_call(sim, "ps_cloud_group", ctx, p(xyz), p(feats), n, -1, p(cidx), s, p(gidx), 16, p(out), p(nx), st),
        raw_call(sim, "ps_cloud_group", ctx, p(xyz), None, n, 4, p(cidx), s, p(gidx), 16, p(out), p(nx), st),
        raw_call(sim, "ps_cloud_group", ctx, p(xyz), p(feats), n, 0, p(cidx), s, p(gidx), 16, p(out), p(nx), st),
        raw_call(sim, "ps_cloud_group", ctx, p(xyz), p(feats), n, 4, p(cidx), s, p(gidx), 0, p(out), p(nx), st),
        raw_call(sim, "ps_cloud_group", ctx, p(xyz), p(feats), n, 4, p(cidx), s, p(gidx), 16, None, p(nx), st),
        fused(context=None), fused(points=None), fused(start_=None), fused(fidx=None), fused(scales=None),
        fused(x=None), fused(n_=0), fused(n_=8193), fused(s_=0), fused(s_=n + 1), fused(d=17), fused(f=None),
        fused(d=0), fused(n_scales=0), fused(n_scales=5), fused(scales=with_scale(0.2, 16, None)),
    ]
    assert [L.ERRORS.get(rc, rc) for rc in codes] == ["PS_ERR_ARG"] * len(codes)
    assert b"" != L.lib().ps_last_error(ctx)  # a message was left
    torch.cuda.synchronize()
    for t in (idx, gidx, out, nx, o3, cen, sc):
        assert bool((t == -7).all())
    # a start or a centre outside the cloud is clamped into it, not read out of bounds
    wild = dev(np.array([-5, 10 ** 6, 3], np.int32))
    got = raw_fps(sim, xyz, wild, s).cpu().numpy()
    assert np.array_equal(got, np.stack([fps_np(c["xyz"][b], k, s) for b, k in enumerate((0, n - 1, 3))]))
    with pytest.raises(ValueError):
        sim.group_cloud(xyz, npoint=n + 1)
    with pytest.raises(ValueError):
        sim.group_cloud(xyz, npoint=8, start=[0, n, 1])
    # nothing faulted: the valid call still computes the golden
    assert fused(normalize=0, x=None) == 0
    assert np.array_equal(idx.cpu().numpy(), c["fps_idx"])
    assert_matches_golden("A", 0, gidx.cpu().numpy(), out.cpu().numpy(), "after the refused calls")
