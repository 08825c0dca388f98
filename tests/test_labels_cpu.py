"""CPU tests of the policy's demonstration labels and losses
(ps_cloud_waypoint_labels, ps_cloud_policy_loss; PandaSim.label_cloud /
policy_loss / evaluate_policy, pandasim.demonstration_records): the new ABI
symbols, the argument checks, and the numpy restatement of both specifications
(tests/labels_reference.py) held to what it restates -- sklearn's
radius_neighbors through tests/golden/demo_labels.npz, torch's nll_loss and
L1Loss in f64, the reference loader's normalisation.
"""
import os
import re

import numpy as np
import pytest
import torch

from cloud_helpers import assert_abi_topic
from labels_reference import (END_MASK, START_MASK, U32, U64, labels_np, loss_np, nll_bound, normalize_f32,
                              normalized_waypoints, ordered_sum, pour_dataset_item, radius2)
from pandasim.cloudnet import demonstration_records, policy_loss_args, waypoint_labels_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS_SYMBOLS = ("ps_cloud_waypoint_labels", "ps_cloud_policy_loss")

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "demo_labels.npz")))
    return _golden


def golden_normalised():
    """The golden's clouds through the f32 normalisation -> xyz, centroid, scale."""
    parts = [normalize_f32(p) for p in golden()["points"]]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]),
            np.array([p[2] for p in parts], np.float32))


# ------------------------------------------------------------------ the ABI
def test_header_signatures_and_group_agree():
    from pandasim import _lib as L
    from pandasim import build as B

    src = assert_abi_topic(LABELS_SYMBOLS, "labels", ("PS_CLOUD_LABEL_MAX_LD", "PS_CLOUD_LABEL_COLUMNS"))
    assert (L.CLOUD_LABEL_MAX_LD, L.CLOUD_LABEL_COLUMNS) == (4096, 14)
    assert ("label_kernels", "label_kernels.hip", []) in B.UNITS
    # the rules are stated where the symbols are declared
    for word in ("Distance.", "Class.", "Waypoint.", "Targets.", "Zero scale.", "Empty.", "deviation", "Skipped.",
                 "NLL.", "L1.", "Prediction.", "Sums."):
        assert word in src, word
    # one definition of the arg-max rule, used by the decode and by the loss
    csrc = os.path.join(ROOT, "panda-lang-manip_amd", "csrc")
    for unit in ("decode_kernels.hip", "label_kernels.hip"):
        assert re.search(r"\bcloud_argmax\(", open(os.path.join(csrc, unit)).read()), unit
    resources = open(os.path.join(ROOT, "scripts", "kernel_resources.py")).read()
    assert "label_kernels.o" in resources


def test_python_surface_exists():
    import pandasim

    for name in ("label_cloud", "policy_loss", "evaluate_policy"):
        assert hasattr(pandasim.PandaSim, name) and hasattr(pandasim.PandaVecEnv, name), name
    assert pandasim.CloudLabels.__slots__ == ("cls", "target", "xyz", "centroid", "scale")
    assert pandasim.PolicyLoss.__slots__ == ("sums", "counts", "confusion", "cls_loss", "offset_loss", "rot_loss",
                                             "accuracy")
    assert callable(pandasim.demonstration_records)


# ------------------------------------------------------------ the arguments
class _Group:
    def __init__(self, nb, n, centroid=True):
        self.xyz, self.scale = torch.zeros(nb, n, 3), torch.ones(nb)
        self.centroid = torch.zeros(nb, 3) if centroid else None


def test_waypoint_labels_args_good_and_bad():
    pts, wp, q = torch.zeros(3, 100, 3), torch.zeros(3, 2, 3), torch.zeros(3, 2, 4)
    cnt = torch.ones(3, dtype=torch.int32)
    assert waypoint_labels_args(3, pts, wp, q, 0.125, None, None) == (100, 0.125)
    assert waypoint_labels_args(3, pts, wp, q, 1, _Group(3, 100), cnt) == (100, 1.0)
    big = torch.zeros(1, 8193, 3)
    assert waypoint_labels_args(1, big, wp[:1], q[:1], 0.125, _Group(1, 8193), None)[0] == 8193
    bad = [dict(points=torch.zeros(2, 100, 3)), dict(points=torch.zeros(3, 100, 2)), dict(points=pts.double()),
           dict(points=torch.zeros(3, 0, 3)), dict(waypoints=torch.zeros(3, 3, 3)), dict(waypoints=torch.zeros(3, 2, 4)),
           dict(quats=torch.zeros(3, 2, 3)), dict(quats=torch.zeros(2, 2, 4)),
           dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")),
           dict(radius=True), dict(radius="0.125"),
           dict(group=_Group(3, 99)), dict(group=_Group(2, 100)), dict(group=_Group(3, 100, centroid=False)),
           dict(group=object()), dict(count=torch.ones(3)), dict(count=torch.ones(2, dtype=torch.int32))]
    for override in bad:
        a = dict(points=pts, waypoints=wp, quats=q, radius=0.125, group=None, count=None)
        a.update(override)
        with pytest.raises(ValueError):
            waypoint_labels_args(3, *a.values())
    with pytest.raises(ValueError):  # without a group the cloud is normalised here: ps_cloud_normalize's limit
        waypoint_labels_args(1, big, wp[:1], q[:1], 0.125, None, None)


def test_policy_loss_args_good_and_bad():
    head, cls, tgt = torch.zeros(3, 50, 18), torch.zeros(3, 50, dtype=torch.int32), torch.zeros(3, 50, 14)
    assert policy_loss_args(3, head, cls, tgt, 4, (1, 3), (2, 3)) == (50, 18, 4, 14, (START_MASK, END_MASK))
    assert policy_loss_args(3, torch.zeros(3, 50, 30), cls, tgt, 3, (1,), [2])[:3] == (50, 30, 3)
    bad = [dict(head=torch.zeros(3, 50, 17)), dict(head=torch.zeros(3, 50, 4097)), dict(head=torch.zeros(2, 50, 18)),
           dict(head=head.double()), dict(cls=cls.long()), dict(cls=torch.zeros(3, 49, dtype=torch.int32)),
           dict(target=torch.zeros(3, 50, 13)), dict(target=torch.zeros(3, 50, 15)), dict(target=tgt.double()),
           dict(num_classes=1), dict(num_classes=17), dict(num_classes=4.0), dict(num_classes=True),
           dict(num_classes=5),  # 5 + 14 > 18
           dict(start_classes=()), dict(start_classes=(4,)), dict(end_classes=(-1,)), dict(end_classes=3)]
    for override in bad:
        a = dict(head=head, cls=cls, target=tgt, num_classes=4, start_classes=(1, 3), end_classes=(2, 3))
        a.update(override)
        with pytest.raises(ValueError, match="policy_loss"):
            policy_loss_args(3, *a.values())


# ---------------------------------------------------- the labels' restatement
def test_golden_is_what_the_generator_says():
    g = golden()
    assert g["points"].shape == (3, 300, 3) and g["points"].dtype == np.float32
    assert g["waypoints"].dtype == np.float32 and float(g["radius"]) == 0.125
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "demo_labels.npz")) < 100_000
    for b in range(3):
        assert all((g["cls"][b] == c).sum() >= 5 for c in range(4)), b  # every class in every cloud
        p, w = g["points"][b].astype(np.float64), g["waypoints"][b].astype(np.float64)
        assert np.linalg.norm(w[0] - w[1]) < 0.25
        for k in range(2):  # no point within 1e-5 of a sphere: zero points are set aside below
            assert (np.abs(np.sqrt(((p - w[k]) ** 2).sum(1)) - 0.125) >= 1e-5).all(), (b, k)


def test_restated_labels_reproduce_sklearn():
    """cls exactly; the offsets against the golden's world-frame offsets divided
    by the loader's m in f64.  The restated offset is three rounded f32
    operations deep ((a - c) / s twice, then the difference) on values of
    magnitude at most (|p| + |w| + |c|) / s per component, each rounding within
    2^-24 of its result: the bound is 4 * 2^-24 times that magnitude."""
    g = golden()
    xyz, centroid, scale = golden_normalised()
    cls, target = labels_np(g["points"], xyz, centroid, scale, g["waypoints"], g["quats"], float(g["radius"]))
    assert np.array_equal(cls, g["cls"])
    want = g["offsets"] / g["m"][:, None, None]
    p = np.abs(g["points"].astype(np.float64))
    w = np.abs(g["waypoints"].astype(np.float64))
    c = np.abs(centroid.astype(np.float64))[:, None, :]
    worst = 0.0
    for k in range(2):
        mag = (p + w[:, k:k + 1, :] + c) / scale.astype(np.float64)[:, None, None]
        err = np.abs(target[..., 3 * k:3 * k + 3].astype(np.float64) - want[..., 3 * k:3 * k + 3])
        worst = max(worst, float((err / (4 * U32 * mag)).max()))
        assert (err <= 4 * U32 * mag).all(), k
    print(f"largest offset error / bound = {worst:.3f}")
    # where a point is in a set the golden's offset is not zero, elsewhere both are
    in0, in1 = (g["cls"] & 1) == 1, (g["cls"] & 2) == 2
    assert (np.abs(target[..., 0:3]).sum(-1) > 0)[in0].all() and not target[..., 0:3][~in0].any()
    assert (np.abs(target[..., 3:6]).sum(-1) > 0)[in1].all() and not target[..., 3:6][~in1].any()
    # the quaternions go through unchanged
    for b in range(3):
        assert np.array_equal(target[b, in0[b], 6:10], np.broadcast_to(g["quats"][b, 0], (in0[b].sum(), 4)))
        assert np.array_equal(target[b, in1[b], 10:14], np.broadcast_to(g["quats"][b, 1], (in1[b].sum(), 4)))
        assert not target[b, ~in0[b], 6:10].any() and not target[b, ~in1[b], 10:14].any()


def test_restated_labels_edge_rules():
    r2 = radius2(0.125)
    assert r2 == np.float32(0.015625) and radius2(0.1) == np.float32(np.float32(0.1) * np.float32(0.1))
    pts = np.array([[[0.125, 0, 0], [0.12500001, 0, 0], [np.nan, 0, 0], [0, 0, 0]]], np.float32)
    wp, q = np.zeros((1, 2, 3), np.float32), np.ones((1, 2, 4), np.float32)
    wp[0, 1] = [5, 5, 5]
    xyz, cen, sc = pts.copy(), np.zeros((1, 3), np.float32), np.ones(1, np.float32)
    cls, target = labels_np(pts, xyz, cen, sc, wp, q, 0.125)
    assert cls.tolist() == [[1, 0, 0, 1]]  # d2 == r2 is inside, the next f32 is not, NaN is in no set
    assert target[0, 3, 0:3].tolist() == [0, 0, 0] and target[0, 0, 0] == np.float32(0.125)
    cls, target = labels_np(pts, xyz, cen, np.zeros(1, np.float32), wp, q, 0.125)
    assert cls.tolist() == [[1, 0, 0, 1]] and not target[..., :6].any() and target[0, 0, 6:10].tolist() == [1, 1, 1, 1]
    cls, target = labels_np(pts, xyz, cen, sc, wp, q, 0.125, count=np.array([0]))
    assert (cls == -1).all() and not target.any()


# ----------------------------------------------------- the losses' restatement
def loss_case(seed, nb, n, nc, ld, ignore=0.1):
    rng = np.random.default_rng(seed)
    head = rng.normal(size=(nb, n, ld)).astype(np.float32)
    head[..., :nc] *= 3
    cls = rng.integers(0, nc, (nb, n)).astype(np.int32)
    cls[rng.random((nb, n)) < ignore] = -1
    target = rng.normal(size=(nb, n, 14)).astype(np.float32)
    return head, cls, target


def test_ordered_sum_is_the_specified_order():
    rng = np.random.default_rng(0)
    terms, include = rng.normal(size=(2500, 3)), rng.random(2500) < 0.7
    part = np.zeros(1024)
    for i in range(2500):  # the walk, one addition at a time
        if include[i]:
            for k in range(3):
                part[i % 1024] += terms[i, k]
    h = 512
    while h:
        for t in range(h):
            part[t] += part[t + h]
        h //= 2
    assert ordered_sum(terms, include) == part[0]


@pytest.mark.parametrize("nc,ld", ((4, 18), (3, 30)))
def test_restated_nll_is_torch_nll_loss(nc, ld):
    """Against F.nll_loss(log_softmax(x.double()), reduction='sum') per cloud,
    ignore_index = -1.  The bound, from the arithmetic: each term is m +
    log(sum exp(x - m)) - x_cls, a few ulp for exp, log and the additions times
    the terms' magnitude |m| + |x_cls| + log nc, and the two sides add the terms
    in different orders: 16 * 2^-53 * sum_i (|m_i| + |x_cls,i| + log nc)."""
    head, cls, target = loss_case(nc, 3, 2500, nc, ld)
    sums, counts, _, _ = loss_np(head, cls, target, nc, (0b010, 0b100) if nc == 3 else (START_MASK, END_MASK))
    x = torch.from_numpy(head[..., :nc]).double()
    bound = nll_bound(head, cls, nc)
    for b in range(3):
        want = torch.nn.functional.nll_loss(torch.log_softmax(x[b], -1), torch.from_numpy(cls[b]).long(),
                                            ignore_index=-1, reduction="sum").item()
        print(f"nll {sums[b, 0]:.17g} torch {want:.17g} |diff| / bound = {abs(sums[b, 0] - want) / bound[b]:.4f}")
        assert abs(sums[b, 0] - want) <= bound[b]
        assert counts[b, 0] == (cls[b] >= 0).sum()
    # the mean of the batch is F.nll_loss' own mean over the labelled points
    mean = torch.nn.functional.nll_loss(torch.log_softmax(x.reshape(-1, nc), -1),
                                        torch.from_numpy(cls.reshape(-1)).long(), ignore_index=-1).item()
    assert abs(sums[:, 0].sum() / counts[:, 0].sum() - mean) <= bound.sum() / counts[:, 0].sum() + 4 * U64 * abs(mean)


@pytest.mark.parametrize("nc,ld", ((4, 18), (3, 30)))
def test_restated_l1_is_torch_l1loss(nc, ld):
    """Against nn.L1Loss(reduction='sum') in f64 on the rows of each set: the
    terms are exact, only the order of the N' terms differs, so the bound is
    N' * 2^-53 * sum |d|."""
    head, cls, target = loss_case(10 + nc, 3, 2500, nc, ld)
    masks = (0b010, 0b100) if nc == 3 else (START_MASK, END_MASK)
    sums, counts, _, _ = loss_np(head, cls, target, nc, masks)
    l1 = torch.nn.L1Loss(reduction="sum")
    cols = ((nc, nc + 3, 0, 3), (nc + 3, nc + 6, 3, 6), (nc + 6, nc + 10, 6, 10), (nc + 10, nc + 14, 10, 14))
    for b in range(3):
        valid = cls[b] >= 0
        rows = [valid & (((m >> np.where(valid, cls[b], 0)) & 1) == 1) for m in masks]
        assert counts[b, 1:3].tolist() == [rows[0].sum(), rows[1].sum()]
        for j, (h0, h1, t0, t1) in enumerate(cols):
            r = rows[j % 2]
            want = l1(torch.from_numpy(head[b, r, h0:h1]).double(), torch.from_numpy(target[b, r, t0:t1]).double()).item()
            terms = int(r.sum()) * (h1 - h0)
            assert abs(sums[b, 1 + j] - want) <= terms * U64 * want, (b, j)


def test_restated_counts_confusion_and_nan():
    head, cls, target = loss_case(3, 2, 700, 4, 18)
    sums, counts, conf, _ = loss_np(head, cls, target, 4)
    pred = head[..., :4].argmax(-1)
    for b in range(2):
        valid = cls[b] >= 0
        assert counts[b, 3] == (pred[b] == cls[b])[valid].sum() == np.trace(conf[b])
        assert conf[b].sum() == counts[b, 0] and conf[b].sum(1).tolist() == np.bincount(cls[b][valid], minlength=4).tolist()
    # a class outside 0..nc-1 is ignored like -1
    cls2 = cls.copy()
    cls2[cls2 == -1] = 4
    again = loss_np(head, cls2, target, 4)
    assert all(np.array_equal(a, b) for a, b in zip(again, (sums, counts, conf)))
    # a NaN logit makes that cloud's NLL NaN and nothing else
    i = int(np.nonzero(cls[1] >= 0)[0][0])
    head[1, i, 2] = np.nan
    s2, c2, f2, _ = loss_np(head, cls, target, 4)
    assert np.isnan(s2[1, 0]) and np.array_equal(s2[0], sums[0]) and np.array_equal(s2[1, 1:], sums[1, 1:])
    assert np.array_equal(c2[0], counts[0]) and np.array_equal(f2[0], conf[0])


# ---------------------------------------------------------------- the records
def test_records_round_trip_through_the_loader(tmp_path):
    """demonstration_records -> np.save -> np.load(allow_pickle=True).item() ->
    PourDataset.__getitem__ restated: the loader's normalised waypoints equal the
    kernel specification's wn within 4 * 2^-24 times their magnitude (three f32
    roundings: the centroid, the difference, the quotient; the scale's own)."""
    g = golden()
    xyz, centroid, scale = golden_normalised()
    wn = normalized_waypoints(g["waypoints"], centroid, scale)
    rng = np.random.default_rng(1)
    colors = rng.integers(0, 256, (3, 300, 3)).astype(np.uint8)
    kpt = (rng.random((3, 300)) < 0.1).astype(np.float32)
    records = demonstration_records(torch.from_numpy(g["points"]), torch.from_numpy(colors), kpt, g["waypoints"],
                                    g["quats"], g["cls"], label=["pour", "pick", "push"])
    assert len(records) == 3
    keys = {"xyz", "xyz_color", "xyz_kpt", "start_waypoint", "end_waypoint", "cls", "start_ori", "end_ori", "label"}
    for b, rec in enumerate(records):
        assert set(rec) == keys and rec["label"] == ["pour", "pick", "push"][b]
        path = os.path.join(tmp_path, f"{b:05d}.npy")
        np.save(path, rec)
        data = np.load(path, allow_pickle=True).item()
        assert set(data) == keys and data["xyz"].shape == (300, 3) and data["xyz"].dtype == np.float64
        assert data["xyz_color"].shape == (300, 3) and data["xyz_kpt"].shape == (300,)
        assert data["cls"].shape == (300,) and np.array_equal(data["cls"], g["cls"][b])
        assert data["cls"].reshape(-1, 1).shape == (300, 1)  # what the loader does with it
        assert np.array_equal(data["start_ori"], g["quats"][b, 0].astype(np.float64))
        pts, start, end, c, m = pour_dataset_item(data)
        assert np.abs(np.stack([start, end]) - g["wn"][b]).max() <= 1e-12  # the golden's own loader values
        for k, got in enumerate((start, end)):
            mag = (np.abs(g["waypoints"][b, k].astype(np.float64)) + np.abs(c)) / m
            assert (np.abs(wn[b, k].astype(np.float64) - got) <= 4 * U32 * mag).all(), (b, k)
        assert np.abs(pts - xyz[b].astype(np.float64)).max() <= 4 * U32 * (np.abs(data["xyz"]).max() + np.abs(c).max()) / m
    # an empty cloud has no points, and the shapes are checked
    empty = demonstration_records(g["points"], colors, None, g["waypoints"], g["quats"], g["cls"], count=[5, 0, 9])
    assert empty[1]["xyz"].shape == (0, 3) and empty[1]["cls"].shape == (0,) and empty[0]["xyz"].shape == (300, 3)
    assert not empty[0]["xyz_kpt"].any()
    for bad in (dict(colors=colors[:, :10]), dict(waypoints=g["waypoints"][:, :1]), dict(cls=g["cls"][:2]),
                dict(label=["a", "b"]), dict(keypoint=kpt[:, :5]), dict(count=[1, 2])):
        a = dict(points=g["points"], colors=colors, keypoint=kpt, waypoints=g["waypoints"], quats=g["quats"],
                 cls=g["cls"], label="pour", count=None)
        a.update(bad)
        with pytest.raises(ValueError):
            demonstration_records(**a)
