"""The PointNet++ kernels' arithmetic restated in numpy, in one place.  The
tests/test_{group,propagate,mlp}_cpu.py modules hold these functions to the
goldens recorded from the reference and derive their bounds; the
tests/test_gpu_{group,propagate,mlp}.py modules hold the kernels to them.
"""
import numpy as np

U = 2.0 ** -24  # the unit roundoff of f32


# ------------------------------------------------------------ the front end
def d2_direct(xyz, centre):
    """[N, 3] f32, [3] f32 -> [N] f32: no fused multiply-add (numpy has none)."""
    d = xyz - centre
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def fps_np(xyz, start, s):
    """farthest_point_sample of one cloud [N, 3] f32 from index `start`."""
    dist = np.full(xyz.shape[0], 1e10, np.float32)
    far, idx = int(start), np.empty(s, np.int32)
    for it in range(s):
        idx[it] = far
        dist = np.minimum(dist, d2_direct(xyz, xyz[far]))
        far = int(np.argmax(dist))  # the lowest index among equal values
    return idx


def ball_query_np(xyz, centre_idx, radius, nsample):
    """query_ball_point of one cloud with the kernel's own comparison:
    not d2 > f32(r * r), r * r in f64 -> [S, nsample] i32."""
    r2 = np.float32(float(radius) * float(radius))
    out = np.empty((len(centre_idx), nsample), np.int32)
    for row, c in enumerate(centre_idx):
        hit = np.nonzero(~(d2_direct(xyz, xyz[c]) > r2))[0][:nsample]
        out[row, :len(hit)] = hit
        out[row, len(hit):] = hit[0]
    return out


def group_rows_np(xyz, feats, centre_idx, group_idx, dtype=np.float32):
    """ps_cloud_group's rows: [B, S, K, D + 3] = feats[group_idx], then
    xyz[group_idx] - xyz[centre_idx] in f32 (in xyz's own precision with
    another dtype)."""
    out = []
    for b in range(xyz.shape[0]):
        rel = xyz[b][group_idx[b]] - xyz[b][centre_idx[b]][:, None, :]
        out.append(rel if feats is None else np.concatenate([feats[b][group_idx[b]], rel], -1))
    return np.stack(out).astype(dtype)


def normalize_np(points):
    """pc_normalize of one cloud in f64 -> xyz, centroid, scale (f64)."""
    p = points.astype(np.float64)
    c = p.mean(0)
    d = p - c
    m = np.sqrt((d ** 2).sum(1)).max()
    return (d / m if m > 0 else np.zeros_like(d)), c, m


# ------------------------------------------------------ feature propagation
def d2_matrix(xyz1, xyz2):
    """[N, 3], [S, 3] f32 -> [N, S] f32: d = a - b, (d.x*d.x + d.y*d.y) + d.z*d.z,
    every product and sum rounded (numpy has no fused multiply-add)."""
    d = xyz1[:, None, :] - xyz2[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def three_nn_np(xyz1, xyz2):
    """One cloud -> idx [N, 3] i32, weight [N, 3] f32.  A stable sort: ascending
    distance, the lowest index first among equal values."""
    n, s = xyz1.shape[0], xyz2.shape[0]
    if s == 1:
        return np.zeros((n, 3), np.int32), np.tile(np.array([1, 0, 0], np.float32), (n, 1))
    idx = np.empty((n, 3), np.int32)
    d3 = np.empty((n, 3), np.float32)
    for lo in range(0, n, 4096):  # in slabs, to bound the matrix
        d2 = d2_matrix(xyz1[lo:lo + 4096], xyz2)
        order = np.argsort(d2, axis=1, kind="stable")[:, :3]
        idx[lo:lo + 4096] = order
        d3[lo:lo + 4096] = np.take_along_axis(d2, order, axis=1)
    w = np.float32(1.0) / (d3 + np.float32(1e-8))
    norm = (w[:, 0] + w[:, 1]) + w[:, 2]
    return idx, (w / norm[:, None]).astype(np.float32)


def interpolate_np(points1, points2, idx, weight):
    """One cloud -> [N, D1 + D2] f32: points1, then (p0*w0 + p1*w1) + p2*w2."""
    if points2.shape[0] == 1:
        interp = np.repeat(points2, idx.shape[0], axis=0)
    else:
        t = points2[idx] * weight[:, :, None]  # [N, 3, D2], each product rounded
        interp = (t[:, 0] + t[:, 1]) + t[:, 2]
    interp = interp.astype(np.float32)
    return interp if points1 is None else np.concatenate([points1, interp], -1)


def propagate_np(xyz1, xyz2, points2, points1=None):
    """Batched: -> out [B, N, D1 + D2], idx [B, N, 3], weight [B, N, 3]."""
    outs, idxs, ws = [], [], []
    for b in range(xyz1.shape[0]):
        idx, w = three_nn_np(xyz1[b], xyz2[b])
        outs.append(interpolate_np(None if points1 is None else points1[b], points2[b], idx, w))
        idxs.append(idx)
        ws.append(w)
    return np.stack(outs), np.stack(idxs), np.stack(ws)


# ----------------------------------------------------------- the shared MLP
def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays (broadcast), exactly rounded."""
    p = a.astype(np.float64) * b.astype(np.float64)  # exact
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)  # TwoSum: p + c = s + err exactly
    bits = s.view(np.int64) if s.flags.writeable else s.copy().view(np.int64)
    fix = (err != 0.0) & ((bits & 1) == 0)
    # round to odd: the neighbour of s on err's side; |s| grows iff err has s's sign
    step = np.where((err > 0.0) == (s > 0.0), 1, -1)
    odd = np.where(fix, bits + step, bits).view(np.float64)
    return odd.astype(np.float32)


def layer_np(x, w, b, relu):
    """[rows, C_in] f32 -> [rows, C_out] f32: the fmaf chain from the bias."""
    y = np.broadcast_to(b[None, :], (x.shape[0], w.shape[0])).astype(np.float32)
    wt = np.ascontiguousarray(w.T)
    for k in range(w.shape[1]):
        y = fma32(x[:, k:k + 1], wt[k][None, :], y)
    return np.where(y > 0, y, np.float32(0)) if relu else y


def mlp_np(rows, layers, pool=1):
    """rows [..., R, C0] f32 -> [..., R / pool, C_n] f32."""
    lead, r, c0 = rows.shape[:-2], rows.shape[-2], rows.shape[-1]
    x = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, c0)
    for w, b, relu in layers:
        x = layer_np(x, w, b, relu)
    x = x.reshape(*lead, r // pool, pool, x.shape[-1]).max(axis=-2)
    return x


def mlp_with_bound(rows, layers, pool=1, centred=0):
    """mlp_np and, beside it, the bound on its distance from the exact
    arithmetic of the unfolded f64 layers (tests/test_mlp_cpu.py's docstring).
    The last `centred` input columns are f32 differences (ps_cloud_group's
    centring), each one rounding away from the reference's f64 difference:
    u |x| there."""
    lead, r, c0 = rows.shape[:-2], rows.shape[-2], rows.shape[-1]
    x = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, c0)
    e = np.zeros(x.shape)
    if centred:
        e[:, c0 - centred:] = U * np.abs(x[:, c0 - centred:].astype(np.float64))
    for w, b, relu in layers:
        aw, ab, ax = np.abs(w.astype(np.float64)), np.abs(b.astype(np.float64)), np.abs(x.astype(np.float64))
        mag = ax @ aw.T + ab[None, :]
        e = 1.01 * ((w.shape[1] + 1) * U * mag + e @ aw.T + U * (mag + e @ aw.T))
        x = layer_np(x, w, b, relu)
    shape = (*lead, r // pool, pool, x.shape[-1])
    return x.reshape(shape).max(axis=-2), e.reshape(shape).max(axis=-2)
