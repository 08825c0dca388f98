"""GPU tests of the policy's waypoint decoding (ps_cloud_decode_waypoints,
PandaSim.decode_waypoints).

The yardstick is tests/net_helpers.py's decode_np: Inference.predict's lines
68-107 in f64 numpy, held to a hand-worked case in tests/test_net_cpu.py.  The
heads are synthetic: logits are multiples of 1/64 with the best at least 0.5
above the second, so no comparison rests on a tie (the ties of their own test
are exact).  Bounds: counts, labels and first_idx are equal; a waypoint is an
f64 sum rounded once, so it lies within 1 f32 ulp of float32(decode_np) (double
rounding); a quaternion component is a correctly rounded norm and one f32
division, within 4 ulp; the Euler angles are the closed form evaluated in f64
on the kernel's own quaternion, to 1e-3 degrees, with |pitch| < 80 degrees.
"""
import numpy as np
import pytest
import torch

from cloud_helpers import DEV, dev, make_sims, raw_call, same_bits
from net_helpers import END_MASK, START_MASK, decode_np, euler_xyz_deg

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
ISENTINEL = -777
CLASS_SETS = {2: ((1,), (0, 1)), 4: ((1, 3), (2, 3)), 16: ((1, 3, 15), (2, 3, 9))}


@pytest.fixture(scope="module")
def sims():
    return make_sims((1, 3, 7))


def mask_of(classes):
    return sum(1 << c for c in set(classes))


def quats_of(rng, shape):
    """Unnormalised xyzw quaternions of either sign with |pitch| <= 75 degrees."""
    roll, yaw = (np.radians(rng.uniform(-180, 180, shape)) / 2 for _ in range(2))
    pitch = np.radians(rng.uniform(-75, 75, shape)) / 2
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                  cr * cp * cy + sr * sp * sy], -1)
    return q * (rng.uniform(0.3, 3.0, shape) * rng.choice([-1.0, 1.0], shape))[..., None]


def make_case(seed, nb, n, nc, extra=0, labels=None, share=0.3):
    """-> head [B, N, nc + 14 + extra] f32 (the extra columns NaN: reading one
    would show), xyz [B, N, 3], centroid [B, 3], scale [B], labels [B, N].
    About `share` of the points get a class other than 0 unless labels is given."""
    rng = np.random.default_rng(seed)
    if labels is None:
        labels = np.where(rng.random((nb, n)) < share, rng.integers(1, nc, (nb, n)), 0)
    labels = np.broadcast_to(np.asarray(labels), (nb, n))
    head = np.full((nb, n, nc + 14 + extra), np.nan, np.float32)
    logits = rng.integers(-64, 65, (nb, n, nc)) / 64.0
    best = 1.5 + rng.integers(0, 65, (nb, n)) / 64.0  # at least 0.5 above every other
    np.put_along_axis(logits, labels[..., None], best[..., None], axis=-1)
    head[..., :nc] = logits
    head[..., nc:nc + 6] = rng.normal(size=(nb, n, 6)) * 0.1
    head[..., nc + 6:nc + 10] = quats_of(rng, (nb, n))
    head[..., nc + 10:nc + 14] = quats_of(rng, (nb, n))
    xyz = (rng.uniform(-1, 1, (nb, n, 3)) + 0.3).astype(np.float32)
    centroid = rng.normal(size=(nb, 3)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, nb).astype(np.float32)
    srt = np.sort(head[..., :nc].astype(np.float64), -1)
    assert (srt[..., -1] - srt[..., -2] >= 0.5).all() and np.array_equal(head[..., :nc].argmax(-1), labels)
    return head, xyz, centroid, scale, labels.astype(np.int32)


def within_ulps(got, want64, ulps):
    """got f32 against float32(want64), NaN matching NaN."""
    want = np.asarray(want64, np.float64).astype(np.float32)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))[~nan]
    return bool((err <= ulps * np.spacing(np.abs(want[~nan])).astype(np.float64)).all())


def check_against_decode_np(res, head, xyz, nc, centroid, scale, masks, tag):
    want = decode_np(head, xyz, nc, centroid, scale, masks)
    got = {k: getattr(res, k).cpu().numpy() for k in ("waypoints", "quats", "euler_deg", "counts", "first_idx")}
    assert np.array_equal(got["counts"], want["counts"]) and got["counts"].dtype == np.int32, tag
    assert np.array_equal(got["first_idx"], want["first_idx"]) and got["first_idx"].dtype == np.int32, tag
    if res.labels is not None:
        assert np.array_equal(res.labels.cpu().numpy(), want["labels"]), tag
    assert got["waypoints"].shape == want["waypoints"].shape and within_ulps(got["waypoints"], want["waypoints"], 1), tag
    assert got["quats"].shape == want["quats"].shape and within_ulps(got["quats"], want["quats"], 4), tag
    # the angles of the kernel's own quaternion, in f64
    angles = euler_xyz_deg(got["quats"])
    empty = want["counts"] == 0
    assert np.array_equal(np.isnan(got["euler_deg"]), np.broadcast_to(empty[..., None], got["euler_deg"].shape)), tag
    if (~empty).any():
        assert np.abs(angles[~empty, 1]).max() < 80.0, tag
        diff = np.abs(got["euler_deg"][~empty].astype(np.float64) - angles[~empty])
        assert np.minimum(diff, 360.0 - diff).max() <= 1e-3, tag
    return want


# ------------------------------------------------------------------- values
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257, 1000, 5000))
def test_values_against_decode_np_over_the_shapes(sims, n):
    for nb in (1, 3, 7):
        for nc in (2, 4, 16):
            for extra in (0, 5):
                head, xyz, centroid, scale, labels = make_case(1000 * n + 10 * nb + nc + extra, nb, n, nc, extra)
                start, end = CLASS_SETS[nc]
                res = sims[nb].decode_waypoints(dev(head), dev(xyz), nc, dev(centroid), dev(scale), start, end,
                                                return_labels=True)
                want = check_against_decode_np(res, head, xyz, nc, centroid, scale, (mask_of(start), mask_of(end)),
                                               (n, nb, nc, extra))
                assert np.array_equal(want["labels"], labels)
                assert res.waypoints.shape == (nb, 2, 3) and res.quats.shape == (nb, 2, 4)
                assert res.euler_deg.shape == (nb, 2, 3) and res.labels.shape == (nb, n)


def test_reference_sets_are_the_defaults(sims):
    head, xyz, centroid, scale, _ = make_case(5, 3, 300, 4)
    res = sims[3].decode_waypoints(dev(head), dev(xyz), 4, dev(centroid), dev(scale))
    assert res.labels is None
    want = check_against_decode_np(res, head, xyz, 4, centroid, scale, (START_MASK, END_MASK), "defaults")
    assert (want["counts"] > 0).all()


# -------------------------------------------------------------------- cases
def test_a_set_of_one_point_and_one_whose_only_member_is_the_last(sims):
    n = 1500  # past one walk of the workgroup's 1024 threads
    labels = np.zeros((3, n), np.int64)
    labels[0, 700], labels[0, n - 1] = 1, 2     # start {700}, end {N - 1}
    labels[1, n - 1] = 3                        # both sets {N - 1}
    labels[2, 0], labels[2, 1023], labels[2, 1024] = 2, 1, 1   # end {0}, start {1023, 1024}
    head, xyz, centroid, scale, _ = make_case(6, 3, n, 4, labels=labels)
    res = sims[3].decode_waypoints(dev(head), dev(xyz), 4, dev(centroid), dev(scale), return_labels=True)
    want = check_against_decode_np(res, head, xyz, 4, centroid, scale, (START_MASK, END_MASK), "single")
    assert want["counts"].tolist() == [[1, 1], [1, 1], [2, 1]]
    assert want["first_idx"].tolist() == [[700, n - 1], [n - 1, n - 1], [1023, 0]]


def test_class_three_only_makes_both_sets_the_same_points(sims):
    labels = np.zeros((1, 400), np.int64)
    labels[0, 17::7] = 3
    head, xyz, centroid, scale, _ = make_case(7, 1, 400, 4, labels=labels)
    res = sims[1].decode_waypoints(dev(head), dev(xyz), 4, dev(centroid), dev(scale))
    want = check_against_decode_np(res, head, xyz, 4, centroid, scale, (START_MASK, END_MASK), "class 3")
    assert want["counts"][0, 0] == want["counts"][0, 1] == len(range(17, 400, 7))
    assert want["first_idx"].tolist() == [[17, 17]]
    # the same points, each set with its own offsets and quaternion
    assert not np.array_equal(res.waypoints[0, 0].cpu().numpy(), res.waypoints[0, 1].cpu().numpy())


def raw_decode(sim, head, xyz, nc, centroid=None, scale=None, masks=(START_MASK, END_MASK), labels=True, first=True,
               expect=0, override=()):
    """ps_cloud_decode_waypoints on device tensors, the outputs sentinel-filled
    before the call -> (waypoints, quats, euler_deg, counts, labels, first_idx)."""
    from pandasim.sim import _ptr

    nb, n, ld = head.shape
    outs = [torch.full((nb, 2, 3), SENTINEL, device=DEV), torch.full((nb, 2, 4), SENTINEL, device=DEV),
            torch.full((nb, 2, 3), SENTINEL, device=DEV), torch.full((nb, 2), ISENTINEL, dtype=torch.int32, device=DEV),
            torch.full((nb, n), ISENTINEL, dtype=torch.int32, device=DEV) if labels else None,
            torch.full((nb, 2), ISENTINEL, dtype=torch.int32, device=DEV) if first else None]
    a = dict(ctx=sim._ctx, head=_ptr(head), n=n, ld=ld, nc=nc, xyz=_ptr(xyz), centroid=_ptr(centroid),
             scale=_ptr(scale), m0=masks[0], m1=masks[1], waypoints=_ptr(outs[0]), quats=_ptr(outs[1]),
             euler=_ptr(outs[2]), counts=_ptr(outs[3]), labels=_ptr(outs[4]), first=_ptr(outs[5]))
    a.update(dict(override))
    rc = raw_call(sim, "ps_cloud_decode_waypoints", *a.values(), sim._stream())
    assert (rc == 0) == (expect == 0), (rc, override)
    torch.cuda.synchronize()
    return outs


def untouched(outs):
    return all(o is None or bool((o == (SENTINEL if o.is_floating_point() else ISENTINEL)).all()) for o in outs)


def test_empty_sets_are_nan_zero_minus_one_and_everything_is_written(sims):
    head, xyz, centroid, scale, _ = make_case(8, 3, 200, 4, labels=np.zeros((3, 200), np.int64))
    wp, q, e, counts, labels, first = raw_decode(sims[3], dev(head), dev(xyz), 4, dev(centroid), dev(scale))
    assert bool(torch.isnan(wp).all()) and bool(torch.isnan(q).all()) and bool(torch.isnan(e).all())
    assert bool((counts == 0).all()) and bool((first == -1).all()) and bool((labels == 0).all())
    # one empty, one not: the other set is unaffected
    lab = np.zeros((3, 200), np.int64)
    lab[:, 5] = 2
    head, xyz, centroid, scale, _ = make_case(9, 3, 200, 4, labels=lab)
    wp, q, e, counts, labels, first = raw_decode(sims[3], dev(head), dev(xyz), 4, dev(centroid), dev(scale))
    assert bool(torch.isnan(wp[:, 0]).all()) and bool(torch.isnan(q[:, 0]).all()) and bool(torch.isnan(e[:, 0]).all())
    assert bool(torch.isfinite(wp[:, 1]).all()) and bool(torch.isfinite(q[:, 1]).all())
    assert counts.tolist() == [[0, 1]] * 3 and first.tolist() == [[-1, 5]] * 3
    # the optional outputs may be left out
    again = raw_decode(sims[3], dev(head), dev(xyz), 4, dev(centroid), dev(scale), labels=False, first=False)
    assert same_bits(again[0], wp) and same_bits(again[3], counts) and again[4] is None and again[5] is None


def test_ties_in_the_logits_resolve_to_the_lowest_class(sims):
    head, xyz, centroid, scale, _ = make_case(10, 1, 6, 4)
    head[0, :, :4] = [[1, 1, 0, 0], [0, 2, 2, 2], [0, 0, 3, 3], [5, 5, 5, 5], [-1, -2, -1, -1], [0, 0.5, 0.25, 0.5]]
    res = sims[1].decode_waypoints(dev(head), dev(xyz), 4, dev(centroid), dev(scale), return_labels=True)
    assert res.labels.tolist() == [[0, 1, 2, 0, 0, 1]]
    check_against_decode_np(res, head, xyz, 4, centroid, scale, (START_MASK, END_MASK), "ties")
    assert res.counts.tolist() == [[2, 1]] and res.first_idx.tolist() == [[1, 2]]


def test_custom_class_sets(sims):
    head, xyz, centroid, scale, _ = make_case(11, 3, 333, 4, share=0.6)
    for start, end in (((0,), (0, 1, 2, 3)), ((2,), (1,)), ((3, 3), [1, 2])):
        res = sims[3].decode_waypoints(dev(head), dev(xyz), 4, dev(centroid), dev(scale), start, end, return_labels=True)
        want = check_against_decode_np(res, head, xyz, 4, centroid, scale, (mask_of(start), mask_of(end)), (start, end))
        assert (want["counts"] > 0).all()
    assert want["counts"].sum() < 3 * 333  # the last pair leaves some points out


def test_no_centroid_and_scale_is_centroid_zero_and_scale_one(sims):
    head, xyz, _, _, _ = make_case(12, 3, 700, 4)
    none = sims[3].decode_waypoints(dev(head), dev(xyz), 4)
    unit = sims[3].decode_waypoints(dev(head), dev(xyz), 4, torch.zeros(3, 3, device=DEV), torch.ones(3, device=DEV))
    for k in ("waypoints", "quats", "euler_deg", "counts", "first_idx"):
        assert same_bits(getattr(none, k), getattr(unit, k)), k
    check_against_decode_np(none, head, xyz, 4, None, None, (START_MASK, END_MASK), "no centroid")


# -------------------------------------------------------------- determinism
def test_a_cloud_decodes_to_the_same_bits_alone_in_a_batch_and_again(sims):
    head, xyz, centroid, scale, _ = make_case(13, 7, 5000, 4)
    for env in (0, 2, 6):  # these envs of the batch hold the cloud decoded alone
        head[env], xyz[env], centroid[env], scale[env] = head[4], xyz[4], centroid[4], scale[4]
    alone = sims[1].decode_waypoints(dev(head[4:5]), dev(xyz[4:5]), 4, dev(centroid[4:5]), dev(scale[4:5]),
                                     return_labels=True)
    batch = sims[7].decode_waypoints(dev(head), dev(xyz), 4, dev(centroid), dev(scale), return_labels=True)
    again = sims[7].decode_waypoints(dev(head), dev(xyz), 4, dev(centroid), dev(scale), return_labels=True)
    assert int(alone.counts.min()) > 100
    for k in ("waypoints", "quats", "euler_deg", "counts", "first_idx", "labels"):
        assert same_bits(getattr(batch, k), getattr(again, k)), k
        for env in (0, 2, 4, 6):
            assert same_bits(getattr(batch, k)[env], getattr(alone, k)[0]), (k, env)
    assert not same_bits(batch.waypoints[1], batch.waypoints[0])


# ---------------------------------------------------------------- refusals
def test_every_refusal_returns_an_error_and_writes_nothing(sims):
    sim = sims[3]
    head, xyz, centroid, scale, _ = make_case(14, 3, 100, 4, extra=2)
    h, x, c, s = dev(head), dev(xyz), dev(centroid), dev(scale)
    assert not untouched(raw_decode(sim, h, x, 4, c, s))  # the call itself is a good one
    bad = [dict(ctx=None), dict(head=None), dict(xyz=None), dict(waypoints=None), dict(quats=None), dict(euler=None),
           dict(counts=None),
           dict(n=0), dict(n=-1), dict(n=(1 << 20) + 1),
           dict(nc=1), dict(nc=0), dict(nc=17), dict(nc=7),          # nc = 7: ld = 20 < 7 + 14
           dict(ld=17), dict(ld=4097), dict(ld=-1),
           dict(m0=0), dict(m1=0), dict(m0=1 << 4), dict(m1=0b11100), dict(m0=1 << 31),
           dict(centroid=None), dict(scale=None)]
    for override in bad:
        outs = raw_decode(sim, h, x, 4, c, s, expect=-1, override=override)
        assert untouched(outs), override
    # ... and through the Python entry point the same are ValueErrors before any launch
    with pytest.raises(ValueError):
        sim.decode_waypoints(h, x, 7)
    with pytest.raises(ValueError):
        sim.decode_waypoints(h, x, 4, c, None)
    with pytest.raises(ValueError):
        sim.decode_waypoints(h, x, 4, start_classes=(4,))
