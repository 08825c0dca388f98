"""ps_cloud_waypoint_labels and ps_cloud_policy_loss restated in numpy
(include/pandasim.h), for tests/test_labels_cpu.py, which holds the restatement
to sklearn's radius_neighbors and to torch's losses, and tests/test_gpu_labels.py,
which holds the kernels to the restatement.

f32 operations are done on np.float32 arrays, so every rounding is the
specified one (numpy has no fused multiply-add); the f64 sums are taken in the
specified order (ordered_sum).
"""
import numpy as np

LOSS_THREADS = 1024
START_MASK, END_MASK = 0b1010, 0b1100  # classes 1 and 3, classes 2 and 3
U32, U64 = 2.0 ** -24, 2.0 ** -53     # the unit roundoffs of f32 and f64


# ------------------------------------------------------------------ labels
def d2_f32(p, w):
    """The header's squared distance: [..., 3] f32, [3] f32 -> [...] f32."""
    d = p - w
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def radius2(radius):
    """r2 = fl32(fl32(radius) * fl32(radius))."""
    r = np.float32(radius)
    return np.float32(r * r)


def normalize_f32(points):
    """ps_cloud_normalize of one cloud [N, 3] f32 but for the order of the
    centroid's f64 sum: -> xyz [N, 3], centroid [3], scale (all f32)."""
    p = np.asarray(points, np.float32)
    c = (p.astype(np.float64).sum(0) / p.shape[0]).astype(np.float32)
    s = np.sqrt(d2_f32(p, c).max())
    assert s.dtype == np.float32
    return ((p - c) / s if s > 0 else np.zeros_like(p)), c, s


def normalized_waypoints(waypoints, centroid, scale):
    """wn = (w - centroid) / scale in f32: [B, 2, 3], [B, 3], [B] -> [B, 2, 3]."""
    w, c, s = (np.asarray(a, np.float32) for a in (waypoints, centroid, scale))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (w - c[:, None, :]) / s[:, None, None]


def labels_np(points, xyz, centroid, scale, waypoints, quats, radius, count=None):
    """-> cls [B, N] i32 and target [B, N, 14] f32, every operation in f32."""
    p, x, c, s, w, q = (np.asarray(a, np.float32) for a in (points, xyz, centroid, scale, waypoints, quats))
    nb, n = p.shape[:2]
    r2 = radius2(radius)
    wn = normalized_waypoints(w, c, s)
    cls = np.zeros((nb, n), np.int32)
    target = np.zeros((nb, n, 14), np.float32)
    for b in range(nb):
        if count is not None and int(count[b]) == 0:
            cls[b] = -1
            continue
        for k in range(2):
            with np.errstate(invalid="ignore", over="ignore"):
                inside = d2_f32(p[b], w[b, k]) <= r2  # a NaN compares false
            cls[b] += (1 + k) * inside.astype(np.int32)
            if s[b] > 0:
                with np.errstate(invalid="ignore", over="ignore"):
                    off = x[b] - wn[b, k]
                assert off.dtype == np.float32
                target[b, :, 3 * k:3 * k + 3] = np.where(inside[:, None], off, np.float32(0))
            target[b, :, 6 + 4 * k:10 + 4 * k] = np.where(inside[:, None], q[b, k], np.float32(0))
    return cls, target


# -------------------------------------------------------------------- loss
def ordered_sum(terms, include):
    """The kernels' f64 sum of one cloud: terms [N, K] f64 (a point's K columns
    are added one after the other), include [N] bool.  Thread t of 1024 takes
    points t, t + 1024, ... ascending into a partial sum that starts at +0.0;
    the partials are added by halving.  A point left out adds +0.0 here, which
    changes no partial sum: none can be -0.0."""
    terms = np.where(include[:, None], np.asarray(terms, np.float64), 0.0)
    n, k = terms.shape
    rounds = -(-n // LOSS_THREADS)
    padded = np.zeros((rounds * LOSS_THREADS, k))
    padded[:n] = terms
    red = np.zeros(LOSS_THREADS)
    with np.errstate(invalid="ignore"):
        for r in range(rounds):
            for col in range(k):
                red = red + padded[r * LOSS_THREADS:(r + 1) * LOSS_THREADS, col]
        h = LOSS_THREADS // 2
        while h > 0:
            red[:h] = red[:h] + red[h:2 * h]
            h //= 2
    return red[0]


def argmax_np(logits):
    """The Label rule: the largest logit, the lowest index among equal ones; a
    NaN never wins.  [..., nc] f32 -> [...] i32."""
    best, label = logits[..., 0].copy(), np.zeros(logits.shape[:-1], np.int32)
    for c in range(1, logits.shape[-1]):
        with np.errstate(invalid="ignore"):
            win = logits[..., c] > best
        best, label = np.where(win, logits[..., c], best), np.where(win, c, label).astype(np.int32)
    return label


def nll_np(logits, cls):
    """Per point (m + log(sum_c exp(x_c - m))) - x_cls in f64, c ascending, m
    the maximum taken ascending with >.  logits [N, nc] f32, cls [N] in
    0..nc-1 -> [N] f64."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    m = x[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for c in range(1, x.shape[1]):
            m = np.where(x[:, c] > m, x[:, c], m)
        s = np.zeros(len(x))
        for c in range(x.shape[1]):
            s = s + np.exp(x[:, c] - m)
        return (m + np.log(s)) - x[np.arange(len(x)), cls]


def loss_np(head, cls, target, nc, masks=(START_MASK, END_MASK), target_offset=0):
    """-> sums [B, 5] f64, counts [B, 4] i32, confusion [B, nc, nc] i32 and the
    per-point NLL terms [B, N] f64 (0 at a skipped point: what the bound of a
    comparison is worked out from)."""
    head, target, cls = np.asarray(head, np.float32), np.asarray(target, np.float32), np.asarray(cls)
    nb, n = cls.shape
    sums, counts = np.zeros((nb, 5)), np.zeros((nb, 4), np.int32)
    confusion, nll = np.zeros((nb, nc, nc), np.int32), np.zeros((nb, n))
    h64 = head.astype(np.float64)
    t64 = target[..., target_offset:target_offset + 14].astype(np.float64)
    for b in range(nb):
        valid = (cls[b] >= 0) & (cls[b] < nc)
        true = np.where(valid, cls[b], 0)
        nll[b] = np.where(valid, nll_np(head[b, :, :nc], true), 0.0)
        sums[b, 0] = ordered_sum(nll[b][:, None], valid)
        pred = argmax_np(head[b, :, :nc])
        in0, in1 = (valid & (((mask >> true) & 1) == 1) for mask in masks)
        counts[b] = [valid.sum(), in0.sum(), in1.sum(), (valid & (pred == true)).sum()]
        np.add.at(confusion[b], (true[valid], pred[valid]), 1)
        diff = np.abs(h64[b, :, nc:nc + 14] - t64[b])  # exact: f32 operands, f64 difference
        sums[b, 1] = ordered_sum(diff[:, 0:3], in0)
        sums[b, 2] = ordered_sum(diff[:, 3:6], in1)
        sums[b, 3] = ordered_sum(diff[:, 6:10], in0)
        sums[b, 4] = ordered_sum(diff[:, 10:14], in1)
    return sums, counts, confusion, nll


def nll_bound(head, cls, nc):
    """16 * 2^-53 * sum_i (|m_i| + |x_cls,i| + log nc) over a cloud's labelled
    points, per cloud: a few ulp per term for exp, log and the additions, times
    the terms' magnitude.  head [B, N, >= nc] f32, cls [B, N] -> [B]."""
    x = np.asarray(head, np.float32)[..., :nc].astype(np.float64)
    cls = np.asarray(cls)
    valid = (cls >= 0) & (cls < nc)
    xc = np.take_along_axis(x, np.where(valid, cls, 0)[..., None].astype(np.int64), -1)[..., 0]
    mag = np.abs(x.max(-1)) + np.abs(xc) + np.log(nc)
    return 16 * U64 * np.where(valid, mag, 0.0).sum(-1)


# --------------------------------------------------------------- the loader
def pour_dataset_item(data):
    """PourDataset.__getitem__ (PourDataLoader_cls_off.py:33-45) up to its
    random choice, restated: the record's cloud normalised with its own
    centroid and largest radius, and the two waypoints with the same.
    -> xyz [M, 3], start [3], end [3], centroid [3], m (f64)."""
    pts = np.asarray(data["xyz"], np.float64)[:, 0:3]
    centroid = np.mean(pts, axis=0)
    pc = pts - centroid
    m = np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
    return pc / m, (data["start_waypoint"] - centroid) / m, (data["end_waypoint"] - centroid) / m, centroid, m
