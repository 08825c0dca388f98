"""GPU tests of the PointNet++ feature propagation (ps_cloud_three_nn /
_interpolate / _feature_propagation, PandaSim.propagate_features).

The yardstick is tests/cloud_reference.py's numpy restatement run on the
same inputs, which the kernels equal bit for bit on every row: idx index for
index, weight and out bit for bit.  That restatement is held to the f64 golden
recorded from the reference within 12 eps_f32 max|points2| there, so the
kernels meet the golden within that bound by construction; it is asserted
here once more on the kernels' own output.
"""
import numpy as np
import pytest
import torch

from cloud_helpers import DEV, dev, make_sims, raw_call, same_bits
from cloud_reference import propagate_np
from test_propagate_cpu import CASES, EPS, K_BOUND, SHAPES, case_of, restated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sims():
    """Contexts of 2 clouds (the golden's batch), of 1 and of 7."""
    return make_sims((2, 1, 7))


# ------------------------------------------------ the raw calls (ctypes)
def raw_three_nn(sim, xyz1, xyz2):
    from pandasim.sim import _ptr

    nb, n = xyz1.shape[:2]
    idx = torch.empty(nb, n, 3, dtype=torch.int32, device=DEV)
    weight = torch.empty(nb, n, 3, device=DEV)
    assert raw_call(sim, "ps_cloud_three_nn", sim._ctx, _ptr(xyz1), n, _ptr(xyz2), xyz2.shape[1], _ptr(idx), _ptr(weight),
               sim._stream()) == 0
    return idx, weight


def raw_interpolate(sim, points1, points2, idx, weight):
    from pandasim.sim import _ptr

    nb, n = idx.shape[:2]
    d1, (s, d2) = 0 if points1 is None else points1.shape[2], points2.shape[1:]
    out = torch.empty(nb, n, d1 + d2, device=DEV)
    assert raw_call(sim, "ps_cloud_interpolate", sim._ctx, _ptr(points1), d1, _ptr(points2), d2, n, s, _ptr(idx),
               _ptr(weight), _ptr(out), sim._stream()) == 0
    return out


def raw_fused(sim, xyz1, xyz2, points2, points1=None, nn=True):
    from pandasim.sim import _ptr

    nb, n = xyz1.shape[:2]
    d1, (s, d2) = 0 if points1 is None else points1.shape[2], points2.shape[1:]
    out = torch.empty(nb, n, d1 + d2, device=DEV)
    idx = torch.empty(nb, n, 3, dtype=torch.int32, device=DEV) if nn else None
    weight = torch.empty(nb, n, 3, device=DEV) if nn else None
    assert raw_call(sim, "ps_cloud_feature_propagation", sim._ctx, _ptr(xyz1), n, _ptr(xyz2), s, _ptr(points1), d1,
               _ptr(points2), d2, _ptr(out), _ptr(idx), _ptr(weight), sim._stream()) == 0
    return out, idx, weight


def assert_equals_restatement(sim, xyz1, xyz2, points2, points1, what):
    """The three entry points on numpy inputs against propagate_np: every row,
    every bit.  Returns the fused out."""
    want_out, want_idx, want_w = propagate_np(xyz1, xyz2, points2, points1)
    x1, x2, p2, p1 = dev(xyz1), dev(xyz2), dev(points2), dev(points1)
    idx, weight = raw_three_nn(sim, x1, x2)
    assert np.array_equal(idx.cpu().numpy(), want_idx), (what, "idx")
    assert same_bits(weight, want_w), (what, "weight")
    assert same_bits(raw_interpolate(sim, p1, p2, idx, weight), want_out), (what, "interpolate")
    out, fidx, fw = raw_fused(sim, x1, x2, p2, p1)
    assert same_bits(out, want_out), (what, "fused out")
    assert same_bits(fidx, want_idx) and same_bits(fw, want_w), (what, "fused idx, weight")
    return out


def random_case(seed, nb, n, s, d1, d2):
    rng = np.random.default_rng(seed)
    xyz1 = rng.uniform(-1, 1, size=(nb, n, 3)).astype(np.float32)
    xyz2 = rng.uniform(-1, 1, size=(nb, s, 3)).astype(np.float32)
    k = min(n, s) // 2  # some coarse points are dense points: distances of exactly 0
    xyz2[:, :k] = xyz1[:, :k]
    points2 = rng.normal(size=(nb, s, d2)).astype(np.float32)
    points1 = rng.normal(size=(nb, n, d1)).astype(np.float32) if d1 else None
    return xyz1, xyz2, points2, points1


# ---------------------------------------------------- the golden's cases
@pytest.mark.parametrize("name", CASES)
def test_kernels_equal_the_restatement_on_every_row(sims, name):
    c = case_of(name)
    want_out, want_idx, want_w = restated(name)
    x1, x2, p2, p1 = dev(c["xyz1"]), dev(c["xyz2"]), dev(c["points2"]), dev(c["points1"])
    idx, weight = raw_three_nn(sims[2], x1, x2)
    assert np.array_equal(idx.cpu().numpy(), want_idx)  # ambiguous rows included
    assert same_bits(weight, want_w)
    assert same_bits(raw_interpolate(sims[2], p1, p2, idx, weight), want_out)
    out, fidx, fw = raw_fused(sims[2], x1, x2, p2, p1)
    assert same_bits(out, want_out) and same_bits(fidx, want_idx) and same_bits(fw, want_w)
    # and so the f64 golden within the CPU test's bound
    keep, got = ~c["ambiguous"], out.cpu().numpy().astype(np.float64)
    for b in range(2):
        err = float(np.abs(got[b] - c["out"][b])[keep[b]].max())
        scale = EPS * float(np.abs(c["points2"][b]).max())
        print(f"case {name} cloud {b}: worst error {err / scale:.2f} eps_f32 max|points2| (bound {K_BOUND})")
        assert err <= K_BOUND * scale


def test_ties_zero_distances_and_the_lowest_index(sims):
    """Exact duplicates among the coarse points, dense points that coincide
    with coarse ones (with a duplicated one too), dense duplicates."""
    rng = np.random.default_rng(3)
    xyz2 = rng.uniform(-1, 1, size=(2, 96, 3)).astype(np.float32)
    xyz2[:, 40:80] = xyz2[:, :40]  # every one of the first 40 twice, the copy 40 later
    xyz2[:, 90:] = xyz2[:, 5:6]  # and one of them eight times
    xyz1 = rng.uniform(-1, 1, size=(2, 333, 3)).astype(np.float32)
    xyz1[:, :96] = xyz2
    xyz1[:, 200:260] = xyz1[:, 100:160]
    points2 = rng.normal(size=(2, 96, 6)).astype(np.float32)
    assert_equals_restatement(sims[2], xyz1, xyz2, points2, None, "ties")
    _, idx, w = propagate_np(xyz1, xyz2, points2)
    assert idx[0, 5].tolist() == [5, 45, 90] and idx[0, 45].tolist() == [5, 45, 90]  # d2 = 0 three times
    assert np.isfinite(w).all() and np.abs(w[0, 5] - 1 / 3).max() <= 2 * EPS


# ------------------------------------------------------------ shape edges
@pytest.mark.parametrize("n,s,d1,d2", [
    (1, 3, 0, 1), (63, 1, 2, 1), (65, 63, 0, 3), (300, 64, 1, 2), (257, 65, 0, 300), (130, 5, 700, 257),
    (70, 8192, 0, 1), (1, 1, 0, 1), (64, 4, 0, 2048)])
def test_shape_edges(sims, n, s, d1, d2):
    xyz1, xyz2, points2, points1 = random_case(n * 31 + s, 2, n, s, d1, d2)
    assert_equals_restatement(sims[2], xyz1, xyz2, points2, points1, (n, s, d1, d2))


def test_both_walks_one_lane_and_four_lanes_per_point(sims):
    """2 clouds of 262 400 points are 2 050 blocks of 256, past the 2 048 below
    which the walk is split: one lane per dense point.  The same cloud alone
    is 1 025 blocks: four lanes per point, merged.  Both equal the restatement,
    hence each other.  (Every other test here runs the split walk, bar the
    one beyond 2^31.)"""
    n, s = 262400, 9
    xyz1, xyz2, points2, _ = random_case(77, 2, n, s, 0, 1)
    xyz1[:, 300:400] = xyz1[:, 100:200]
    xyz2[:, 5:9] = xyz2[:, 1:5]  # ties for both walks
    want_out, want_idx, want_w = propagate_np(xyz1, xyz2, points2)
    for sim, rows in ((sims[2], slice(0, 2)), (sims[1], slice(1, 2))):
        x1, x2, p2 = dev(xyz1[rows]), dev(xyz2[rows]), dev(points2[rows])
        idx, weight = raw_three_nn(sim, x1, x2)
        out, fidx, fw = raw_fused(sim, x1, x2, p2)
        assert np.array_equal(idx.cpu().numpy(), want_idx[rows]) and same_bits(weight, want_w[rows])
        assert same_bits(fidx, want_idx[rows]) and same_bits(fw, want_w[rows]) and same_bits(out, want_out[rows])


def test_output_offsets_beyond_two_to_the_31():
    """64 clouds x 16 400 points x 2 048 channels are 2^31 + 2.1e6 floats: the
    last cloud's rows lie past a 32-bit offset.  Every cloud is the same, so
    every cloud's result is the first one's, which is the restatement's."""
    from pandasim.sim import PandaSim

    nb, n, s, d2 = 64, 16400, 3, 2048
    assert nb * n * d2 > 2 ** 31
    xyz1, xyz2, points2, _ = random_case(5, 1, n, s, 0, d2)
    want = propagate_np(xyz1, xyz2, points2)[0]
    sim = PandaSim("reach", num_envs=nb, device=DEV)
    out = sim.propagate_features(dev(xyz1).expand(nb, -1, -1), dev(xyz2).expand(nb, -1, -1),
                                 dev(points2).expand(nb, -1, -1))
    assert out.shape == (nb, n, d2)
    assert same_bits(out[0], want[0])
    assert all(torch.equal(out[b], out[0]) for b in range(1, nb))


# ----------------------------------------------------- fused and composed
@pytest.mark.parametrize("nn", (False, True), ids=("out-only", "with-nn"))
@pytest.mark.parametrize("with_points1", (False, True), ids=("bare", "points1"))
@pytest.mark.parametrize("name", ("A", "B", "C", "E"))
def test_fused_equals_the_two_calls_composed(sims, name, with_points1, nn):
    c, sim = case_of(name), sims[2]
    x1, x2, p2 = dev(c["xyz1"]), dev(c["xyz2"]), dev(c["points2"])
    p1 = None
    if with_points1:
        p1 = dev(c["points1"]) if c["points1"] is not None else torch.rand(2, SHAPES[name][0], 9, device=DEV)
    idx, weight = raw_three_nn(sim, x1, x2)
    composed = raw_interpolate(sim, p1, p2, idx, weight)
    out, fidx, fw = raw_fused(sim, x1, x2, p2, p1, nn=nn)
    assert same_bits(out, composed)
    assert out.shape == (2, SHAPES[name][0], (0 if p1 is None else p1.shape[2]) + SHAPES[name][3])
    if nn:
        assert same_bits(fidx, idx) and same_bits(fw, weight)
    # one of the two outputs alone
    from pandasim.sim import _ptr

    only = torch.full_like(idx, -7)
    o2 = torch.empty_like(out)
    assert raw_call(sim, "ps_cloud_feature_propagation", sim._ctx, _ptr(x1), x1.shape[1], _ptr(x2), x2.shape[1], _ptr(p1),
               0 if p1 is None else p1.shape[2], _ptr(p2), p2.shape[2], _ptr(o2), _ptr(only), None,
               sim._stream()) == 0
    assert same_bits(only, idx) and same_bits(o2, composed)


def test_a_clouds_result_does_not_depend_on_the_batch(sims):
    c = case_of("B")
    rng = np.random.default_rng(8)
    xyz1, xyz2, points2, points1 = random_case(9, 7, 1000, 128, 5, 8)
    for b in (0, 3, 6):
        xyz1[b], xyz2[b], points2[b], points1[b] = c["xyz1"][0], c["xyz2"][0], c["points2"][0], c["points1"][0]
    xyz1[1] = c["xyz1"][1][rng.permutation(1000)]
    alone = raw_fused(sims[1], dev(xyz1[:1]), dev(xyz2[:1]), dev(points2[:1]), dev(points1[:1]))
    full = raw_fused(sims[7], dev(xyz1), dev(xyz2), dev(points2), dev(points1))
    want = restated("B")
    for b in (0, 3, 6):
        for f, (x, y, z) in enumerate(zip(full, alone, want)):
            assert same_bits(x[b], y[0]), (b, f)
            assert same_bits(x[b], z[0]), (b, f)


# ------------------------------------------------------------ the Python layer
def test_python_layer_equals_the_abi_call(sims):
    from pandasim.envs import PandaVecEnv

    c = case_of("B")
    x1, x2, p2, p1 = dev(c["xyz1"]), dev(c["xyz2"]), dev(c["points2"]), dev(c["points1"])
    want = raw_fused(sims[2], x1, x2, p2, p1)
    got = sims[2].propagate_features(x1, x2, p2, p1, return_nn=True)
    assert all(same_bits(a, b) for a, b in zip(got, want))
    out = sims[2].propagate_features(c["xyz1"], c["xyz2"], c["points2"])  # numpy in, no points1, out only
    assert torch.is_tensor(out) and same_bits(out, want[0][..., 5:])
    env = PandaVecEnv("reach", "sparse", "ee", 2, DEV, autoreset=False)
    got = env.propagate_features(x1, x2, p2, points1=p1, return_nn=True)
    assert all(same_bits(a, b) for a, b in zip(got, want))
    assert same_bits(env.propagate_features(x1.transpose(1, 2).contiguous().transpose(1, 2), x2, p2, p1), want[0])
    for bad in (dict(xyz2=x2[:, :2], points2=p2[:, :2]), dict(xyz1=x1[:1]), dict(points2=p2.double()),
                dict(points1=p1[:, :5]), dict(points2=torch.zeros(2, 128, 2049, device=DEV))):
        with pytest.raises(ValueError):
            sims[2].propagate_features(**{**dict(xyz1=x1, xyz2=x2, points2=p2, points1=p1), **bad})


# -------------------------------------------------------- argument errors
def test_argument_errors_leave_the_outputs_untouched(sims):
    from pandasim import _lib as L
    from pandasim.sim import _ptr as p

    sim, c = sims[2], case_of("B")
    n, s, d1, d2 = SHAPES["B"]
    x1, x2, p2, p1 = dev(c["xyz1"]), dev(c["xyz2"]), dev(c["points2"]), dev(c["points1"])
    ctx, st = sim._ctx, sim._stream()
    good_idx, good_w = raw_three_nn(sim, x1, x2)
    idx = torch.full((2, n, 3), -7, dtype=torch.int32, device=DEV)
    w = torch.full((2, n, 3), -7.0, device=DEV)
    out = torch.full((2, n, d1 + d2), -7.0, device=DEV)

    def nn(context=ctx, a=x1, n_=n, b=x2, s_=s, i=idx, w_=w):
        return raw_call(sim, "ps_cloud_three_nn", context, p(a), n_, p(b), s_, p(i), p(w_), st)

    def interp(context=ctx, f1=p1, d1_=d1, f2=p2, d2_=d2, n_=n, s_=s, i=good_idx, w_=good_w, o=out):
        return raw_call(sim, "ps_cloud_interpolate", context, p(f1), d1_, p(f2), d2_, n_, s_, p(i), p(w_), p(o), st)

    def fused(context=ctx, a=x1, n_=n, b=x2, s_=s, f1=p1, d1_=d1, f2=p2, d2_=d2, o=out, i=idx, w_=w):
        return raw_call(sim, "ps_cloud_feature_propagation", context, p(a), n_, p(b), s_, p(f1), d1_, p(f2), d2_, p(o),
                   p(i), p(w_), st)

    big = (1 << 20) + 1
    codes = [
        nn(context=None), nn(a=None), nn(b=None), nn(i=None), nn(w_=None),
        nn(n_=0), nn(n_=-1), nn(n_=big), nn(s_=0), nn(s_=-3), nn(s_=2), nn(s_=8193),
        interp(context=None), interp(f2=None), interp(i=None), interp(w_=None), interp(o=None),
        interp(n_=0), interp(n_=big), interp(s_=0), interp(s_=2), interp(s_=8193),
        interp(d2_=0), interp(d2_=-1), interp(d2_=2049), interp(d1_=-1), interp(d1_=2049),
        interp(f1=None), interp(d1_=0),
        fused(context=None), fused(a=None), fused(b=None), fused(f2=None), fused(o=None),
        fused(n_=0), fused(n_=big), fused(s_=0), fused(s_=2), fused(s_=8193),
        fused(d2_=0), fused(d2_=2049), fused(d1_=-1), fused(d1_=2049), fused(f1=None), fused(d1_=0),
    ]
    assert [L.ERRORS.get(rc, rc) for rc in codes] == ["PS_ERR_ARG"] * len(codes)
    assert b"" != L.lib().ps_last_error(ctx)  # a message was left
    torch.cuda.synchronize()
    for t in (idx, w, out):
        assert bool((t == -7).all())
    # nothing faulted: the valid calls still compute the restatement
    want_out, want_idx, want_w = restated("B")
    assert fused() == 0
    assert same_bits(out, want_out) and same_bits(idx, want_idx) and same_bits(w, want_w)


def test_an_index_outside_the_coarse_cloud_is_clamped(sims):
    c = case_of("A")
    n, s, _, d2 = SHAPES["A"]
    p2 = dev(c["points2"])
    rng = np.random.default_rng(4)
    idx = rng.integers(0, s, size=(2, n, 3)).astype(np.int32)
    wild = idx.copy()
    wild[:, ::3, 0], wild[:, 1::3, 1], wild[:, 2::3, 2] = -1, s, 2 ** 31 - 1
    wild[0, 0], wild[1, -1] = (-2 ** 31, s + 10 ** 6, -5), (10 ** 9, -10 ** 9, s)
    weight = dev(rng.uniform(0, 1, size=(2, n, 3)).astype(np.float32))
    got = raw_interpolate(sims[2], None, p2, dev(wild), weight)
    want = raw_interpolate(sims[2], None, p2, dev(np.clip(wild, 0, s - 1)), weight)
    assert same_bits(got, want) and bool(torch.isfinite(got).all())
    assert not same_bits(got, raw_interpolate(sims[2], None, p2, dev(idx), weight))
