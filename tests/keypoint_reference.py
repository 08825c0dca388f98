"""The keypoint conditioning of take_rgbd (run_policy.py:202-285) restated in
numpy f64, as include/pandasim.h states ps_cloud_keypoint_features: the patch
of a keypoint and the labelling of points by their nearest patch target.
"""
import math

import numpy as np


def patch_offsets_np(radius):
    """The integer offsets (dx, dy) with dx^2 + dy^2 <= radius^2, dx ascending
    then dy ascending: [P, 2]."""
    r = int(radius)
    return np.array([(dx, dy) for dx in range(-r, r + 1)
                     for dy in range(-math.isqrt(r * r - dx * dx), math.isqrt(r * r - dx * dx) + 1)], np.int64)


def patch_pixels_np(kp, radius, w, h):
    """Keypoint kp (column, row) -> its patch's pixels [P, 2] (column, row) in
    slot order and inside [P] bool: the slots whose pixel lies in the w x h
    image (pix2pix_neighborhood keeps exactly those); none for a keypoint with
    a negative coordinate, the caller's "absent"."""
    kp = np.asarray(kp, np.int64)
    pix = kp[None, :] + patch_offsets_np(radius)
    inside = (pix[:, 0] >= 0) & (pix[:, 0] < w) & (pix[:, 1] >= 0) & (pix[:, 1] < h) & bool((kp >= 0).all())
    return pix, inside


def keypoint_min_dist_np(points, targets):
    """points [K, 3] (f32 values widened, or f64) and targets [n_kp, P, 3] f64
    (NaN rows: slots outside the image) -> sqrt(m_k) [K, n_kp] f64, +inf for a
    keypoint without a slot.  d2 = (dx*dx + dy*dy) + dz*dz, each rounded."""
    p = np.asarray(points, np.float64)[:, None, None, :]
    t = np.asarray(targets, np.float64)[None]
    with np.errstate(invalid="ignore"):
        d = p - t
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        d2 = np.where(np.isnan(d2), np.inf, d2)  # a NaN never lowers the minimum
        return np.sqrt(d2.min(axis=-1, initial=np.inf))


def keypoint_cond_np(points, targets, threshold, values):
    """The channel [K] f32: values[k] of the highest-index keypoint whose
    nearest target lies strictly closer than threshold (f64), else 0."""
    dist = keypoint_min_dist_np(points, targets)
    out = np.zeros(dist.shape[0], np.float32)
    for k, v in enumerate(values):
        out[dist[:, k] < np.float64(threshold)] = np.float32(v)
    return out
