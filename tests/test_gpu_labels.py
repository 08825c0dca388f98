"""GPU tests of the policy's demonstration labels and losses
(ps_cloud_waypoint_labels, ps_cloud_policy_loss; PandaSim.label_cloud /
policy_loss / evaluate_policy).

The yardstick is tests/labels_reference.py, the numpy restatement of both
specifications, held to sklearn and torch in tests/test_labels_cpu.py.  Bounds:
the labels are f32 operations in a fixed order, so cls and the 14 target
columns are equal bit for bit; the L1 sums are exact terms in a fixed order,
bit for bit; counts and confusion are whole numbers, equal; the NLL sum goes
through the device's exp and log, which differ from numpy's by ulps, within
labels_reference.nll_bound (16 * 2^-53 * sum (|m| + |x_cls| + log nc)).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cloud_helpers import DEV, dev, make_sims, raw_call, same_bits
from labels_reference import END_MASK, START_MASK, U32, d2_f32, labels_np, loss_np, nll_bound, radius2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.5
ISENTINEL = -777
RADIUS = 0.125


@pytest.fixture(scope="module")
def sims():
    return make_sims((1, 3, 7))


def make_cloud(seed, nb, n):
    """A table top's worth of points off the origin and two waypoints inside
    it, about 0.1 m apart: -> points [B, N, 3], waypoints [B, 2, 3], quats
    [B, 2, 4] f32."""
    rng = np.random.default_rng(seed)
    origin = rng.uniform(-0.5, 0.5, (nb, 1, 3))
    points = (origin + rng.uniform([-0.3, -0.3, 0.0], [0.3, 0.3, 0.2], (nb, n, 3))).astype(np.float32)
    waypoints = (origin + rng.uniform([-0.1, -0.1, 0.02], [0.1, 0.1, 0.15], (nb, 2, 3))).astype(np.float32)
    return points, waypoints, rng.normal(size=(nb, 2, 4)).astype(np.float32)


def host(t):
    return None if t is None else t.cpu().numpy()


def raw_labels(sim, points, xyz, centroid, scale, waypoints, quats, radius=RADIUS, count=None, ld=14, offset=0,
               expect=0, override=()):
    """ps_cloud_waypoint_labels on device tensors, the outputs sentinel-filled
    before the call -> cls [B, N], target [B, N, ld]."""
    from pandasim.sim import _ptr

    nb, n = points.shape[:2]
    cls = torch.full((nb, n), ISENTINEL, dtype=torch.int32, device=DEV)
    target = torch.full((nb, n, ld), SENTINEL, device=DEV)
    a = dict(ctx=sim._ctx, points=_ptr(points), xyz=_ptr(xyz), centroid=_ptr(centroid), scale=_ptr(scale),
             waypoints=_ptr(waypoints), quats=_ptr(quats), radius=radius, count=_ptr(count), n=n, cls=_ptr(cls),
             target=_ptr(target), ld=ld, offset=offset)
    a.update(dict(override))
    rc = raw_call(sim, "ps_cloud_waypoint_labels", *a.values(), sim._stream())
    assert (rc == 0) == (expect == 0), (rc, override)
    torch.cuda.synchronize()
    return cls, target


def raw_loss(sim, head, cls, target, nc, masks=(START_MASK, END_MASK), offset=0, confusion=True, expect=0,
             override=()):
    """ps_cloud_policy_loss on device tensors, the outputs sentinel-filled
    before the call -> sums [B, 5] f64, counts [B, 4], confusion [B, nc, nc]."""
    from pandasim.sim import _ptr

    nb, n, ld = head.shape
    sums = torch.full((nb, 5), SENTINEL, dtype=torch.float64, device=DEV)
    counts = torch.full((nb, 4), ISENTINEL, dtype=torch.int32, device=DEV)
    conf = torch.full((nb, nc, nc), ISENTINEL, dtype=torch.int32, device=DEV) if confusion else None
    a = dict(ctx=sim._ctx, head=_ptr(head), n=n, ld=ld, nc=nc, cls=_ptr(cls), target=_ptr(target),
             ld_t=target.shape[2], t_off=offset, m0=masks[0], m1=masks[1], sums=_ptr(sums), counts=_ptr(counts),
             confusion=_ptr(conf))
    a.update(dict(override))
    rc = raw_call(sim, "ps_cloud_policy_loss", *a.values(), sim._stream())
    assert (rc == 0) == (expect == 0), (rc, override)
    torch.cuda.synchronize()
    return sums, counts, conf


def untouched(outs):
    return all(o is None or bool((o == (SENTINEL if o.is_floating_point() else ISENTINEL)).all()) for o in outs)


# ------------------------------------------------------------------- labels
@pytest.mark.parametrize("n", (1, 63, 1025, 2500))
def test_labels_bit_for_bit_over_the_shapes(sims, n):
    """Below one block of 256 points, several blocks with a remainder; the
    three store widths: the [B, N, 14] target (64-bit stores), ld = 23 with
    out_offset = 5 (dword stores), ld = 24 with out_offset = 4 (128-bit)."""
    for nb in (1, 3, 7):
        points, wp, q = make_cloud(100 * n + nb, nb, n)
        res = sims[nb].label_cloud(dev(points), dev(wp), dev(q))
        xyz, centroid, scale = host(res.xyz), host(res.centroid), host(res.scale)
        cls, target = labels_np(points, xyz, centroid, scale, wp, q, RADIUS)
        assert res.cls.dtype == torch.int32 and res.target.shape == (nb, n, 14)
        assert np.array_equal(host(res.cls), cls) and same_bits(res.target, target), (n, nb)
        if n >= 1025:
            assert all((cls == c).any() for c in range(4)), "every class occurs"
        for ld, off in ((23, 5), (24, 4), (14, 0)):
            c2, t2 = raw_labels(sims[nb], dev(points), res.xyz, res.centroid, res.scale, dev(wp), dev(q), ld=ld,
                                offset=off)
            assert np.array_equal(host(c2), cls) and same_bits(t2[..., off:off + 14].contiguous(), target), (n, nb, ld)
            rest = torch.cat([t2[..., :off], t2[..., off + 14:]], -1)
            assert bool((rest == SENTINEL).all()), (n, nb, ld)  # the other columns keep the sentinel


def test_points_on_the_boundary(sims):
    """d2 equal to r2 and one f32 ulp either side of it, from exactly
    representable coordinates (the waypoint at the origin): d2 == r2 is inside,
    the ulp above it is not."""
    f = np.float32
    cases = [  # radius, point, d2 - r2 in ulps of r2's binade
        (0.375, [0, 0, 0.375], 0), (0.375, [2.0 ** -13, 0, 0.375], 1), (0.375, [0.25, 0.125 - 2.0 ** -24, 0.25], -1),
        (0.125, [0, 0, 0.125], 0), (0.125, [2.0 ** -15, 2.0 ** -15, 0.125], 1)]
    for radius, point, ulps in cases:
        r2 = radius2(radius)
        p = np.array(point, f)
        assert np.array_equal(p.astype(np.float64), np.array(point)), "representable"
        d2 = d2_f32(p, np.zeros(3, f))
        step = np.spacing(r2) if ulps >= 0 else r2 - np.nextafter(r2, f(0))
        assert d2.dtype == f and d2 == f(r2 + ulps * step) and (ulps == 0) == (d2 == r2), (radius, point)
        points = np.zeros((1, 4, 3), f)
        points[0, 1] = p
        points[0, 3] = 10.0  # far away: the cloud's scale
        wp = np.zeros((1, 2, 3), f)
        wp[0, 1] = 5.0
        q = np.ones((1, 2, 4), f)
        res = sims[1].label_cloud(dev(points), dev(wp), dev(q), radius=radius)
        want, target = labels_np(points, host(res.xyz), host(res.centroid), host(res.scale), wp, q, radius)
        assert want[0, 1] == (1 if ulps <= 0 else 0), (radius, point)
        assert host(res.cls).tolist() == want.tolist() == [[1, want[0, 1], 1, 0]], (radius, point)
        assert same_bits(res.target, target)


def test_label_edge_cases(sims):
    sim = sims[3]
    points, wp, q = make_cloud(5, 3, 700)
    # a waypoint equal to a cloud point: a zero offset there, bit for bit
    wp[0, 0], wp[2, 1] = points[0, 123], points[2, 699]
    # cloud 1 has scale 0: every point the same, its start waypoint on it
    points[1] = points[1, 0]
    wp[1, 0] = points[1, 0]
    res = sim.label_cloud(dev(points), dev(wp), dev(q))
    cls, target = labels_np(points, host(res.xyz), host(res.centroid), host(res.scale), wp, q, RADIUS)
    got_c, got_t = host(res.cls), host(res.target)
    assert np.array_equal(got_c, cls) and same_bits(got_t, target)
    assert got_c[0, 123] & 1 and got_t[0, 123, 0:3].view(np.uint32).tolist() == [0, 0, 0]
    assert got_c[2, 699] & 2 and got_t[2, 699, 3:6].view(np.uint32).tolist() == [0, 0, 0]
    assert float(res.scale[1]) == 0.0 and (got_c[1] & 1).all() and not got_t[1, :, :6].any()
    assert np.isfinite(got_t).all() and np.array_equal(got_t[1, :, 6:10], np.broadcast_to(q[1, 0], (700, 4)))
    # count: an empty cloud among full ones gets -1 and zeros, the others are unchanged
    count = torch.tensor([700, 0, 12], dtype=torch.int32, device=DEV)
    part = sim.label_cloud(dev(points), dev(wp), dev(q), count=count)
    assert bool((part.cls[1] == -1).all()) and not bool(part.target[1].any())
    assert same_bits(part.cls[[0, 2]], res.cls[[0, 2]]) and same_bits(part.target[[0, 2]], res.target[[0, 2]])
    # the same normalisation handed over as a group gives the same bits
    class Group:
        xyz, centroid, scale = res.xyz, res.centroid, res.scale

    again = sim.label_cloud(dev(points), dev(wp), dev(q), group=Group, count=count)
    assert same_bits(again.cls, part.cls) and same_bits(again.target, part.target) and again.xyz is res.xyz
    # a NaN point is in no set: class 0, zero targets; the others are unchanged
    bad = points.copy()
    bad[0, 123, 1] = np.nan
    c2, t2 = raw_labels(sim, dev(bad), res.xyz, res.centroid, res.scale, dev(wp), dev(q))
    want_c, want_t = labels_np(bad, host(res.xyz), host(res.centroid), host(res.scale), wp, q, RADIUS)
    assert int(c2[0, 123]) == 0 and not bool(t2[0, 123].any())
    assert np.array_equal(host(c2), want_c) and same_bits(t2, want_t)
    keep = np.ones(700, bool)
    keep[123] = False
    assert same_bits(t2[0][dev(keep)], res.target[0][dev(keep)])


def test_golden_clouds_get_the_golden_classes(sims):
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "demo_labels.npz")))
    res = sims[3].label_cloud(dev(g["points"]), dev(g["waypoints"]), dev(g["quats"]), radius=float(g["radius"]))
    assert np.array_equal(host(res.cls), g["cls"])
    # and the offsets are the golden's, world frame over the loader's m, within the f32 bound of the CPU test
    want = g["offsets"] / g["m"][:, None, None]
    mag = (np.abs(g["points"]).max() + np.abs(g["waypoints"]).max() + np.abs(g["centroid"]).max()) / g["m"].min()
    assert np.abs(host(res.target)[..., :6] - want).max() <= 4 * U32 * mag


# --------------------------------------------------------------------- loss
def loss_case(seed, nb, n, nc, ld):
    rng = np.random.default_rng(seed)
    head = rng.normal(size=(nb, n, ld)).astype(np.float32)
    head[..., :nc] *= 3
    cls = rng.integers(0, nc, (nb, n)).astype(np.int32)
    cls[rng.random((nb, n)) < 0.1] = -1      # ignored points
    cls[1][(cls[1] == 1) | (cls[1] == nc - 1)] = 0  # cloud 1: an empty start set
    target = rng.normal(size=(nb, n, 14)).astype(np.float32)
    return head, cls, target


def check_loss(got, head, cls, target, nc, masks, tag):
    sums, counts, conf = (host(t) for t in got)
    want_s, want_c, want_f, _ = loss_np(head, cls, target, nc, masks)
    bound = nll_bound(head, cls, nc)
    err = np.abs(sums[:, 0] - want_s[:, 0])
    print(f"{tag}: nll {sums[:, 0]} |diff| / bound {err / bound}")
    assert (err <= bound).all(), tag
    assert same_bits(sums[:, 1:].copy(), want_s[:, 1:].copy()), tag  # the L1 sums bit for bit
    assert np.array_equal(counts, want_c) and counts.dtype == np.int32, tag
    if conf is not None:
        assert np.array_equal(conf, want_f), tag
    return want_s, want_c


@pytest.mark.parametrize("nc", (3, 4))
def test_loss_against_the_restatement(sims, nc):
    masks = (0b1010, 0b1100) if nc == 4 else (0b110, 0b100)  # the start set holds classes 1 and nc - 1
    classes = ((1, 3), (2, 3)) if nc == 4 else ((1, 2), (2,))
    for ld in (nc + 14, 30):
        head, cls, target = loss_case(10 * nc + ld, 3, 2500, nc, ld)
        got = raw_loss(sims[3], dev(head), dev(cls), dev(target), nc, masks)
        want_s, want_c = check_loss(got, head, cls, target, nc, masks, (nc, ld))
        assert want_c[1, 1] == 0 and want_s[1, 1] == 0 and want_s[1, 3] == 0 and (want_c[[0, 2], 1] > 0).all()
        assert (want_c[:, 0] < 2500).all() and (want_c[:, 0] > 2000).all()
        # the confusion matrix is optional, and the Python entry point returns the same with the means
        none = raw_loss(sims[3], dev(head), dev(cls), dev(target), nc, masks, confusion=False)
        assert same_bits(none[0], got[0]) and same_bits(none[1], got[1])
        res = sims[3].policy_loss(dev(head), dev(cls), dev(target), nc, *classes, return_confusion=True)
        assert same_bits(res.sums, got[0]) and same_bits(res.counts, got[1]) and same_bits(res.confusion, got[2])
        s, c = host(got[0]).sum(0), host(got[1]).sum(0).astype(np.float64)
        want = [s[0] / c[0], (s[1] + s[2]) / (3 * (c[1] + c[2])), (s[3] + s[4]) / (4 * (c[1] + c[2])), c[3] / c[0]]
        have = [float(getattr(res, k)) for k in ("cls_loss", "offset_loss", "rot_loss", "accuracy")]
        assert np.allclose(have, want, rtol=1e-14, atol=0) and res.cls_loss.dtype == torch.float64
        assert res.cls_loss.device.type == "cuda" and sims[3].policy_loss(dev(head), dev(cls), dev(target), nc,
                                                                          *classes).confusion is None
    # a target inside wider rows
    wide = np.full((3, 2500, 20), np.nan, np.float32)
    wide[..., 3:17] = target
    off = raw_loss(sims[3], dev(head), dev(cls), dev(wide), nc, masks, offset=3)
    assert all(same_bits(a, b) for a, b in zip(off, got))


def test_a_nan_logit_stays_in_its_cloud_and_its_nll(sims):
    head, cls, target = loss_case(77, 3, 1500, 4, 18)
    base = raw_loss(sims[3], dev(head), dev(cls), dev(target), 4)
    i = int(np.nonzero(cls[2] >= 0)[0][5])
    head[2, i, 1] = np.nan
    got = raw_loss(sims[3], dev(head), dev(cls), dev(target), 4)
    assert bool(torch.isnan(got[0][2, 0])) and same_bits(got[0][2, 1:], base[0][2, 1:])
    assert same_bits(got[0][:2], base[0][:2]) and same_bits(got[1][:2], base[1][:2]) and same_bits(got[2][:2], base[2][:2])
    want = loss_np(head, cls, target, 4)
    assert np.array_equal(host(got[1]), want[1]) and np.array_equal(host(got[2]), want[2])  # a NaN logit never wins


# --------------------------------------------------------------- end to end
def perfect_head(cls, target, nc):
    head = torch.zeros(*cls.shape, nc + 14, device=DEV)
    head.scatter_(2, cls.long().unsqueeze(-1), 10.0)
    head[..., nc:] = target
    return head


def test_labels_as_a_perfect_head_decode_to_their_waypoints(sims):
    """The inverse: decode_waypoints of the labels returns each non-empty set's
    waypoint.  Per component the decoded value is the mean of xyz - (xyz - wn),
    times scale, plus centroid: f32 roundings of values no larger than
    scale * (max|xyz| + |wn|) + |centroid|, eight of them at most
    ((w - c) / s, xyz - wn, the final rounding, and the waypoint's own), so the
    bound is 8 * 2^-24 of that."""
    sim = sims[7]
    points, wp, q = make_cloud(31, 7, 2500)
    wp[6, 1] = points[6].max(0) + 1.0  # cloud 6: an empty end set
    lab = sim.label_cloud(dev(points), dev(wp), dev(q))
    head = perfect_head(lab.cls, lab.target, 4)
    dec = sim.decode_waypoints(head, lab.xyz, 4, lab.centroid, lab.scale)
    counts = host(dec.counts)
    cls = host(lab.cls)
    assert np.array_equal(counts[:, 0], ((cls & 1) == 1).sum(1)) and np.array_equal(counts[:, 1], ((cls & 2) == 2).sum(1))
    assert counts[6, 1] == 0 and (counts[:6] > 0).all() and counts[6, 0] > 0
    xyz, centroid, scale = (host(t).astype(np.float64) for t in (lab.xyz, lab.centroid, lab.scale))
    wn = (wp.astype(np.float64) - centroid[:, None, :]) / scale[:, None, None]
    bound = 8 * U32 * (scale[:, None, None] * (np.abs(xyz).max(1)[:, None, :] + np.abs(wn)) + np.abs(centroid)[:, None, :])
    err = np.abs(host(dec.waypoints).astype(np.float64) - wp.astype(np.float64))
    full = counts > 0
    print(f"largest round-trip error / bound = {(err / bound)[full].max():.3f}")
    assert (err[full] <= bound[full]).all() and np.isnan(host(dec.waypoints)[6, 1]).all()
    # its quaternion is the input's, normalised: a correctly rounded norm and one f32 division, within 4 ulp
    want_q = q.astype(np.float64) / np.sqrt((q.astype(np.float64) ** 2).sum(-1, keepdims=True))
    got_q = host(dec.quats)
    ulp = np.spacing(np.abs(want_q.astype(np.float32))).astype(np.float64)
    assert (np.abs(got_q.astype(np.float64) - want_q.astype(np.float32))[full] <= 4 * ulp[full]).all()
    # the losses of that head: no L1 error, every point right, the restatement's NLL
    loss = sim.policy_loss(head, lab.cls, lab.target, 4, return_confusion=True)
    assert not bool(loss.sums[:, 1:].any()) and float(loss.accuracy) == 1.0
    assert float(loss.offset_loss) == 0.0 and float(loss.rot_loss) == 0.0
    check_loss((loss.sums, loss.counts, loss.confusion), host(head), cls, host(lab.target), 4, (START_MASK, END_MASK),
               "perfect head")
    assert bool((loss.counts[:, 0] == 2500).all()) and bool((loss.counts[:, 3] == 2500).all())


def test_through_the_env_the_cube_is_labelled(sims):
    import pandasim
    from test_gpu_cloud import stepped_env

    env = stepped_env("push", 4)
    cloud = env.point_cloud(list(pandasim.GRASP_VIEWS[:3]), 300, 64, 48, 11)
    # the demonstration of a push: from the object to its target
    wp = torch.stack([env.sim.get_base_position("object").float(), env.sim.goals().float()[:, :3]], 1).contiguous()
    q = torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV).expand(4, 2, 4).contiguous()
    lab = env.label_cloud(cloud["points"], wp, q, count=cloud["count"])
    cls = host(lab.cls)
    print("classes per env:", [np.bincount(c, minlength=4).tolist() for c in cls])
    assert int(cloud["count"].min()) > 0 and (cls >= 0).all()
    assert ((cls == 1).sum(1) >= 1).all()  # the cube is in view of every env
    want, target = labels_np(host(cloud["points"]), host(lab.xyz), host(lab.centroid), host(lab.scale), host(wp),
                             host(q), RADIUS)
    assert np.array_equal(cls, want) and same_bits(lab.target, target)
    for name in ("policy_loss", "evaluate_policy"):
        assert callable(getattr(env, name))


def test_side_stream_sees_the_work_queued_before():
    """label_cloud, policy_loss and decode_waypoints on a side stream are
    ordered behind the copies queued before them there: the same bits as on
    the default stream.  In a fresh process (tests/labels_stream_run.py), as
    tests/test_gpu_replay.py does and for its reason."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "labels_stream_run.py")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "side stream == default stream" in r.stdout, r.stdout[-2000:]


def test_a_cloud_gives_the_same_bits_alone_in_a_batch_and_again(sims):
    points, wp, q = make_cloud(41, 7, 2500)
    for env in (0, 2, 6):  # these envs of the batch hold the cloud labelled alone
        points[env], wp[env], q[env] = points[4], wp[4], q[4]

    def run(sim, sl):
        lab = sim.label_cloud(dev(points[sl]), dev(wp[sl]), dev(q[sl]))
        head = perfect_head(lab.cls, lab.target, 4)
        head[..., :4] += dev(8 * np.random.default_rng(1).normal(size=(2500, 4)).astype(np.float32))  # some points wrong
        head[..., 4:] *= 1.25
        loss = sim.policy_loss(head, lab.cls, lab.target, 4, return_confusion=True)
        return [lab.cls, lab.target, loss.sums, loss.counts, loss.confusion]

    alone, batch, again = run(sims[1], slice(4, 5)), run(sims[7], slice(0, 7)), run(sims[7], slice(0, 7))
    assert int(alone[3][0, 1]) > 10 and int(alone[3][0, 3]) < 2500 and float(alone[2][0, 1]) > 0
    for k, (a, b, c) in enumerate(zip(alone, batch, again)):
        assert same_bits(b, c), k
        for env in (0, 2, 4, 6):
            assert same_bits(b[env], a[0]), (k, env)
    assert not same_bits(batch[2][1], batch[2][0])


def test_evaluate_policy_composes_the_calls(sims):
    from net_helpers import STATE_SEED, seeded_state
    from pandasim import CloudSegNet

    sim = sims[1]
    net = CloudSegNet(seeded_state(STATE_SEED), DEV)
    points, wp, q = make_cloud(51, 1, 600)
    colors = dev(np.random.default_rng(2).integers(0, 256, (1, 600, 3)).astype(np.float32))
    ev = sim.evaluate_policy(net, dev(points), colors, dev(wp), dev(q), seed=3)
    head, g1 = sim.segment_cloud(net, dev(points), colors, 3)
    lab = sim.label_cloud(dev(points), dev(wp), dev(q), group=g1)
    loss = sim.policy_loss(head, lab.cls, lab.target, 4)
    dec = sim.decode_waypoints(head, g1.xyz, 4, g1.centroid, g1.scale)
    assert same_bits(ev.head, head) and same_bits(ev.labels.cls, lab.cls) and same_bits(ev.labels.target, lab.target)
    assert same_bits(ev.loss.sums, loss.sums) and same_bits(ev.loss.counts, loss.counts)
    assert same_bits(ev.decoded.waypoints, dec.waypoints) and ev.waypoint_error.shape == (1, 2)
    want = np.linalg.norm(host(dec.waypoints).astype(np.float64) - wp, axis=-1)
    got = host(ev.waypoint_error)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got, want, rtol=1e-5, equal_nan=True)
    assert int(ev.loss.counts[0, 0]) == 600 and np.isfinite(float(ev.loss.cls_loss))
    check_loss((loss.sums, loss.counts, None), host(head), host(lab.cls), host(lab.target), 4, (START_MASK, END_MASK),
               "the network's head")


# ---------------------------------------------------------------- refusals
def test_every_refusal_of_the_labels_writes_nothing(sims):
    sim = sims[3]
    points, wp, q = make_cloud(61, 3, 100)
    res = sim.label_cloud(dev(points), dev(wp), dev(q))
    args = (dev(points), res.xyz, res.centroid, res.scale, dev(wp), dev(q))
    assert not untouched(raw_labels(sim, *args, ld=20, offset=2))  # the call itself is a good one
    bad = [dict(ctx=None), dict(points=None), dict(xyz=None), dict(centroid=None), dict(scale=None),
           dict(waypoints=None), dict(quats=None), dict(cls=None), dict(target=None),
           dict(n=0), dict(n=-1), dict(n=(1 << 20) + 1),
           dict(radius=0.0), dict(radius=-0.125), dict(radius=float("inf")), dict(radius=float("nan")),
           dict(offset=-1), dict(offset=7), dict(ld=15), dict(ld=13), dict(ld=4097), dict(ld=-1)]
    for override in bad:
        assert untouched(raw_labels(sim, *args, ld=20, offset=2, expect=-1, override=override)), override
    # ... and through the Python entry point the same are ValueErrors before any launch
    with pytest.raises(ValueError):
        sim.label_cloud(dev(points), dev(wp), dev(q), radius=0.0)
    with pytest.raises(ValueError):
        sim.label_cloud(dev(points), dev(wp[:, :1]), dev(q))


def test_every_refusal_of_the_loss_writes_nothing(sims):
    sim = sims[3]
    head, cls, target = loss_case(62, 3, 100, 4, 20)
    h, c, t = dev(head), dev(cls), dev(np.concatenate([target, target[..., :2]], -1))  # ld_t = 16
    assert not untouched(raw_loss(sim, h, c, t, 4, offset=1))  # the call itself is a good one
    bad = [dict(ctx=None), dict(head=None), dict(cls=None), dict(target=None), dict(sums=None), dict(counts=None),
           dict(n=0), dict(n=-1), dict(n=(1 << 20) + 1),
           dict(nc=1), dict(nc=0), dict(nc=17), dict(nc=7),   # nc = 7: ld = 20 < 7 + 14
           dict(ld=17), dict(ld=4097), dict(ld=-1),
           dict(t_off=-1), dict(t_off=3), dict(ld_t=14), dict(ld_t=4097),
           dict(m0=0), dict(m1=0), dict(m0=1 << 4), dict(m1=0b11100), dict(m0=1 << 31)]
    for override in bad:
        assert untouched(raw_loss(sim, h, c, t, 4, offset=1, expect=-1, override=override)), override
    with pytest.raises(ValueError):
        sim.policy_loss(h, c, dev(target), 7)
    with pytest.raises(ValueError):
        sim.policy_loss(h, c, dev(target), 4, start_classes=(4,))
