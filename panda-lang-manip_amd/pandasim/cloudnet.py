"""The batched PointNet++ layer over a point-cloud observation:
sampling and grouping, feature propagation, the shared MLP with max-pool.

``CloudNet`` is a mixin of ``PandaSim``; the checkers, ``GroupedCloud``,
``CloudMlp`` and ``fold_batchnorm`` beside it need no simulator at all.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from ._lib import _ptr


class CloudNet:
    """group_cloud, propagate_features, shared_mlp and abstract_features for B
    clouds.  They read no simulator state.  The host class provides exactly
    ``self.num_envs`` (B), ``self.device`` (a torch.device), ``self._ctx`` (a
    library context of B envs on that device), ``self._call(name, *args)``
    (the library call, raising on its error code) and ``self._stream()`` (the
    current stream as a void pointer); the methods use nothing else of it."""

    def group_cloud(self, points, feats=None, npoint: int = 512, radii=(0.1, 0.2, 0.4), nsamples=(32, 64, 128),
                    seed: int = 0, normalize: bool = True, start=None) -> "GroupedCloud":
        """What the reference's policies do to every cloud before the first
        learned weight (pointnet2_utils.py: pc_normalize, farthest_point_sample,
        query_ball_point, index_points and the centring of
        PointNetSetAbstractionMsg.forward) -- fused (ps_cloud_set_abstraction),
        for every env, without the distance matrix and the sort.  The defaults
        are model_cls_off_rot.py's first layer.

        points [B, N, 3] f32 (point_cloud()'s "points"), feats None or
        [B, N, D] f32 with D <= 16 (its "colors" as .float()).  The first
        sampled point of env b is start[b] (i32 [B], each in [0, N)) or, with
        start None, fps_start(seed, b, N): the point cloud's splitmix64 draw of
        counter b, so a seed repeats.  Returns a GroupedCloud."""
        B = self.num_envs
        pts = torch.as_tensor(points, device=self.device)
        if feats is not None:
            feats = torch.as_tensor(feats, device=self.device)
        N, S, D, radii, nsamples, first = group_cloud_args(B, pts, feats, npoint, radii, nsamples, seed, start)
        feats = None if feats is None else feats.contiguous()
        first = first.to(self.device)
        pts = pts.contiguous()
        dev = self.device
        out = GroupedCloud()
        if normalize:
            out.xyz = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
            out.centroid = torch.empty(B, 3, dtype=torch.float32, device=dev)
            out.scale = torch.empty(B, dtype=torch.float32, device=dev)
        else:
            out.xyz, out.centroid, out.scale = pts, None, None
        out.fps_idx = torch.empty(B, S, dtype=torch.int32, device=dev)
        out.new_xyz = torch.empty(B, S, 3, dtype=torch.float32, device=dev)
        out.group_idx = [torch.empty(B, S, k, dtype=torch.int32, device=dev) for k in nsamples]
        out.grouped = [torch.empty(B, S, k, D + 3, dtype=torch.float32, device=dev) for k in nsamples]
        scales = (L.CloudScale * len(radii))()
        for sc, r, k, gi, g in zip(scales, radii, nsamples, out.group_idx, out.grouped):
            sc.radius, sc.nsample, sc.group_idx, sc.grouped = r, k, gi.data_ptr(), g.data_ptr()
        self._call("ps_cloud_set_abstraction", self._ctx, _ptr(pts), _ptr(feats), N, D, _ptr(first), S, scales,
                   len(radii), int(bool(normalize)), _ptr(out.xyz) if normalize else None, _ptr(out.centroid),
                   _ptr(out.scale), _ptr(out.fps_idx), _ptr(out.new_xyz), self._stream())
        return out

    def propagate_features(self, xyz1, xyz2, points2, points1=None, return_nn: bool = False):
        """The interpolation of PointNetFeaturePropagation.forward
        (pointnet2_utils.py:276-310) -- fused (ps_cloud_feature_propagation),
        for every env, without the distance matrix and the sort: each dense
        point's three nearest coarse points, inverse-distance weights, the
        weighted sum of their features behind the dense point's own.

        xyz1 [B, N, 3] f32 the dense points, xyz2 [B, S, 3] f32 the coarse
        points (S = 1 or S >= 3), points2 [B, S, D2] f32 their features,
        points1 None or [B, N, D1] f32; D1, D2 <= 2048.  Returns out
        [B, N, D1 + D2] f32 (points1, then the interpolation: forward's tensor
        before its final permute), with return_nn also idx [B, N, 3] i32 and
        weight [B, N, 3] f32."""
        B, dev = self.num_envs, self.device
        xyz1, xyz2, points2 = (torch.as_tensor(t, device=dev) for t in (xyz1, xyz2, points2))
        if points1 is not None:
            points1 = torch.as_tensor(points1, device=dev)
        N, S, D1, D2 = propagate_features_args(B, xyz1, xyz2, points2, points1)
        xyz1, xyz2, points2 = xyz1.contiguous(), xyz2.contiguous(), points2.contiguous()
        points1 = None if points1 is None else points1.contiguous()
        out = torch.empty(B, N, D1 + D2, dtype=torch.float32, device=dev)
        idx = torch.empty(B, N, 3, dtype=torch.int32, device=dev) if return_nn else None
        weight = torch.empty(B, N, 3, dtype=torch.float32, device=dev) if return_nn else None
        self._call("ps_cloud_feature_propagation", self._ctx, _ptr(xyz1), N, _ptr(xyz2), S, _ptr(points1), D1,
                   _ptr(points2), D2, _ptr(out), _ptr(idx), _ptr(weight), self._stream())
        return (out, idx, weight) if return_nn else out

    def shared_mlp(self, rows, layers: "CloudMlp", pool: int = 1, out=None, out_offset: int = 0):
        """The learned layers between the point-cloud steps, at inference
        (ps_cloud_mlp, f32 MFMA): per row the chain of `layers` (pointwise
        linear layers with the batch norm folded in, ReLU where a layer says
        so), then the maximum over every `pool` consecutive rows -- the loop
        F.relu(bn(conv(x))) and torch.max(x, 2)[0] of pointnet2_utils.py:196-200
        and :253-257, the loop alone (:312-314, pool = 1), the head's conv1 and
        conv2 (pool = 1), sa3's group_all (pool = R).

        rows [B, R, C0] f32 (or [B, S, K, C0], read as R = S * K), R a multiple
        of pool.  Returns [B, R / pool, C_n] f32; with `out` [B, R / pool, W]
        f32 (contiguous) the columns out_offset .. out_offset + C_n - 1 of it
        are written, the others left, and `out` is returned."""
        B, dev = self.num_envs, self.device
        rows = torch.as_tensor(rows, device=dev)
        if out is not None:
            out = torch.as_tensor(out, device=dev)
        R, C0, width = shared_mlp_args(B, rows, layers, pool, out, out_offset)
        rows = rows.contiguous()
        if out is None:
            out = torch.empty(B, R // pool, width, dtype=torch.float32, device=dev)
        self._call("ps_cloud_mlp", self._ctx, _ptr(rows), R, C0, layers.array, len(layers), int(pool), _ptr(out),
                   int(out.shape[2]), int(out_offset), self._stream())
        return out

    def abstract_features(self, xyz, feats=None, centre_idx=None, group_idx=None, mlps=None, fused=None):
        """PointNetSetAbstractionMsg.forward after its sampling
        (pointnet2_utils.py:239-261): per scale the rows of `group_idx[k]`
        (feats[group_idx], then xyz[group_idx] - xyz[centre_idx]) through
        `mlps[k]` and the maximum over each neighbourhood, the scales side by
        side in one [B, S, sum C_n] f32 tensor (the reference's torch.cat,
        before its permute).  fused=True is ps_cloud_group_mlp: the rows are
        gathered inside the kernel, the grouped tensor never exists.
        fused=False is ps_cloud_group then ps_cloud_mlp per scale, the same
        values bit for bit through a grouped tensor of one scale at a time
        (D <= 16).  The default (None) is the composed path where it exists,
        which measured 1.4 to 2.3 % faster at sa1's shape,
        and the fused one above D = 16.

        xyz [B, N, 3] f32, feats None or [B, N, D] f32 (D <= 2048), centre_idx
        [B, S] i32, group_idx a list of [B, S, K_k] i32, mlps a list of
        CloudMlp whose first layer takes D + 3 channels; or a GroupedCloud in
        place of the first four: abstract_features(grouped, feats, mlps=mlps)."""
        B, dev = self.num_envs, self.device
        if isinstance(xyz, GroupedCloud):
            xyz, centre_idx, group_idx = xyz.xyz, xyz.fps_idx, xyz.group_idx
        xyz, centre_idx = torch.as_tensor(xyz, device=dev), torch.as_tensor(centre_idx, device=dev)
        group_idx = [torch.as_tensor(g, device=dev) for g in group_idx]
        if feats is not None:
            feats = torch.as_tensor(feats, device=dev)
        N, S, D, offsets, width = abstract_features_args(B, xyz, feats, centre_idx, group_idx, mlps)
        xyz, centre_idx = xyz.contiguous(), centre_idx.contiguous()
        feats = None if feats is None else feats.contiguous()
        out = torch.empty(B, S, width, dtype=torch.float32, device=dev)
        if fused is None:
            fused = D > L.CLOUD_MAX_FEATURES
        for gi, mlp, off in zip(group_idx, mlps, offsets):
            gi, K = gi.contiguous(), int(gi.shape[2])
            if fused:
                self._call("ps_cloud_group_mlp", self._ctx, _ptr(xyz), _ptr(feats), N, D, _ptr(centre_idx), S, _ptr(gi),
                           K, mlp.array, len(mlp), _ptr(out), width, off, self._stream())
            else:
                grouped = torch.empty(B, S, K, D + 3, dtype=torch.float32, device=dev)
                self._call("ps_cloud_group", self._ctx, _ptr(xyz), _ptr(feats), N, D, _ptr(centre_idx), S, _ptr(gi), K,
                           _ptr(grouped), None, self._stream())
                self._call("ps_cloud_mlp", self._ctx, _ptr(grouped), S * K, D + 3, mlp.array, len(mlp), K, _ptr(out),
                           width, off, self._stream())
        return out


class GroupedCloud:
    """PandaSim.group_cloud's result: xyz [B, N, 3] (normalised; the input
    itself with normalize=False), centroid [B, 3] and scale [B] (None with
    normalize=False), fps_idx [B, S] i32, new_xyz [B, S, 3], and per scale
    group_idx[k] [B, S, nsample_k] i32 and grouped[k] [B, S, nsample_k, D + 3]
    (the features, then the centred coordinates)."""

    __slots__ = ("xyz", "centroid", "scale", "fps_idx", "new_xyz", "group_idx", "grouped")


def fps_start(seed: int, env: int, n: int) -> int:
    """The point farthest point sampling starts from in env `env`'s cloud of n
    points under `seed`: (z * n) >> 64, z the splitmix64 output of counter
    `env` (include/pandasim.h, ps_point_cloud's draw)."""
    m = (1 << 64) - 1
    z = ((int(seed) & m) + 0x9E3779B97F4A7C15 * (env + 1)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return ((z ^ (z >> 31)) * int(n)) >> 64


def _want(fn: str, name: str, t, shape, dtype=torch.float32) -> None:
    """ValueError unless tensor `t` of `fn`'s argument `name` has `dtype` and
    one dimension per entry of `shape`: a number is the size it must have, a
    string names a dimension that is free."""
    got = t.shape
    bad = len(got) != len(shape) or t.dtype != dtype
    for want, have in zip(shape, got):  # a plain loop: every call of the four methods passes here
        if want != have and not isinstance(want, str):
            bad = True
    if bad:
        raise ValueError(f"{fn}: {name} must be [{', '.join(map(str, shape))}] {str(dtype)[6:]}, got "
                         f"{tuple(t.shape)} {t.dtype}")


def group_cloud_args(num_envs: int, points, feats, npoint, radii, nsamples, seed, start):
    """group_cloud's argument checks (ValueError), on tensors of any device:
    -> N, S, D, radii, nsamples and the start indices (i32 [B], on the CPU)."""
    B = int(num_envs)
    _want("group_cloud", "points", points, (B, "N", 3))
    N, S = int(points.shape[1]), int(npoint)
    if not 1 <= N <= L.CLOUD_MAX_POINTS:
        raise ValueError(f"group_cloud: N = {N} points (1 to {L.CLOUD_MAX_POINTS})")
    if not 1 <= S <= N:
        raise ValueError(f"group_cloud: npoint = {S} (1 to N = {N})")
    radii, nsamples = [float(r) for r in radii], [int(k) for k in nsamples]
    if len(radii) != len(nsamples) or not 1 <= len(radii) <= L.CLOUD_MAX_SCALES:
        raise ValueError(f"group_cloud: {len(radii)} radii and {len(nsamples)} nsamples (equal, 1 to "
                         f"{L.CLOUD_MAX_SCALES})")
    if any(not (0.0 < r < math.inf) for r in radii) or any(k < 1 for k in nsamples):
        raise ValueError("group_cloud: a radius must be positive and finite, an nsample at least 1")
    D = 0
    if feats is not None:
        _want("group_cloud", "feats", feats, (B, N, "D"))
        D = int(feats.shape[2])
        if not 1 <= D <= L.CLOUD_MAX_FEATURES:
            raise ValueError(f"group_cloud: D = {D} feature channels (1 to {L.CLOUD_MAX_FEATURES})")
    if start is None:
        first = torch.tensor([fps_start(seed, b, N) for b in range(B)], dtype=torch.int32)
    else:
        first = torch.as_tensor(start).detach().cpu().reshape(-1)
        if first.numel() != B or first.is_floating_point() or first.dtype == torch.bool:
            raise ValueError(f"group_cloud: start must be {B} integers")
        if int(first.min()) < 0 or int(first.max()) >= N:
            raise ValueError(f"group_cloud: start outside [0, {N})")
        first = first.to(torch.int32)
    return N, S, D, radii, nsamples, first


def propagate_features_args(num_envs: int, xyz1, xyz2, points2, points1):
    """propagate_features' argument checks (ValueError), on tensors of any
    device: -> N, S, D1, D2."""
    B = int(num_envs)
    _want("propagate_features", "xyz1", xyz1, (B, "N", 3))
    _want("propagate_features", "xyz2", xyz2, (B, "S", 3))
    N, S = int(xyz1.shape[1]), int(xyz2.shape[1])
    if not 1 <= N <= L.CLOUD_MAX_DENSE_POINTS:
        raise ValueError(f"propagate_features: N = {N} dense points (1 to {L.CLOUD_MAX_DENSE_POINTS})")
    if not 1 <= S <= L.CLOUD_MAX_POINTS or S == 2:
        raise ValueError(f"propagate_features: S = {S} coarse points (1, or 3 to {L.CLOUD_MAX_POINTS}: the "
                         f"reference's interpolation takes three neighbours and raises on two)")
    _want("propagate_features", "points2", points2, (B, S, "D2"))
    D1, D2 = 0, int(points2.shape[2])
    if points1 is not None:
        _want("propagate_features", "points1", points1, (B, N, "D1"))
        D1 = int(points1.shape[2])
    if not 1 <= D2 <= L.CLOUD_MAX_PROP_FEATURES or (points1 is not None and not 1 <= D1 <= L.CLOUD_MAX_PROP_FEATURES):
        raise ValueError(f"propagate_features: D1 = {D1}, D2 = {D2} feature channels (1 to "
                         f"{L.CLOUD_MAX_PROP_FEATURES} each; no points1 for none)")
    return N, S, D1, D2


def fold_batchnorm(conv_w, conv_b, gamma, beta, mean, var, eps: float = 1e-5):
    """A 1x1 convolution followed by a batch norm at inference, as one layer
    of a CloudMlp: -> (W' [C_out, C_in] f32, b' [C_out] f32) with
        s = gamma / sqrt(var + eps),  W' = W * s[:, None],  b' = (b - mean) * s + beta,
    computed in float64 and rounded once to f32.  conv_w is [C_out, C_in] or a
    conv weight [C_out, C_in, 1(, 1)]; conv_b may be None (no bias).  Host
    numpy; tensors of any device are accepted."""
    def f64(a):
        return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)

    w = f64(conv_w)
    if w.ndim > 2 and all(d == 1 for d in w.shape[2:]):
        w = w.reshape(w.shape[:2])
    if w.ndim != 2:
        raise ValueError(f"fold_batchnorm: conv_w must be [C_out, C_in] or [C_out, C_in, 1(, 1)], got {w.shape}")
    c_out = w.shape[0]
    b = np.zeros(c_out) if conv_b is None else f64(conv_b)
    gamma, beta, mean, var = f64(gamma), f64(beta), f64(mean), f64(var)
    for name, a in (("conv_b", b), ("gamma", gamma), ("beta", beta), ("mean", mean), ("var", var)):
        if a.shape != (c_out,):
            raise ValueError(f"fold_batchnorm: {name} must be [{c_out}], got {a.shape}")
    if not float(eps) >= 0.0 or (var + float(eps) <= 0.0).any():
        raise ValueError("fold_batchnorm: var + eps must be positive")
    s = gamma / np.sqrt(var + float(eps))
    return (w * s[:, None]).astype(np.float32), ((b - mean) * s + beta).astype(np.float32)


def cloud_mlp_layers(layers):
    """CloudMlp's argument checks (ValueError), on the CPU: a sequence of
    (W [c_out, c_in], b [c_out], relu) -> [(W f32, b f32, relu bool)] as
    contiguous numpy arrays, the widths chained and within the limits of
    include/pandasim.h."""
    layers = list(layers)
    if not 1 <= len(layers) <= L.CLOUD_MLP_MAX_LAYERS:
        raise ValueError(f"CloudMlp: {len(layers)} layers (1 to {L.CLOUD_MLP_MAX_LAYERS})")
    out, c_in = [], None
    for k, layer in enumerate(layers):
        if len(layer) != 3:
            raise ValueError(f"CloudMlp: layer {k} must be (W, b, relu)")
        w, b, relu = layer
        w = np.asarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w)
        b = np.asarray(b.detach().cpu().numpy() if torch.is_tensor(b) else b)
        if w.ndim != 2 or b.shape != (w.shape[0],) or w.dtype != np.float32 or b.dtype != np.float32:
            raise ValueError(f"CloudMlp: layer {k} must be W [c_out, c_in] and b [c_out] float32, got {w.shape} "
                             f"{w.dtype} and {b.shape} {b.dtype}")
        if not (np.isfinite(w).all() and np.isfinite(b).all()):
            raise ValueError(f"CloudMlp: layer {k} has a weight or bias that is not finite")
        c_out, most = int(w.shape[0]), L.CLOUD_MLP_MAX_LAST if k == len(layers) - 1 else L.CLOUD_MLP_MAX_HIDDEN
        if not 1 <= c_out <= most:
            raise ValueError(f"CloudMlp: layer {k} has {c_out} outputs (1 to {most}; the last layer 1 to "
                             f"{L.CLOUD_MLP_MAX_LAST})")
        if c_in is None:
            if not 1 <= w.shape[1] <= L.CLOUD_MAX_PROP_FEATURES + 3:
                raise ValueError(f"CloudMlp: the first layer takes {w.shape[1]} channels (1 to "
                                 f"{L.CLOUD_MAX_PROP_FEATURES + 3})")
        elif w.shape[1] != c_in:
            raise ValueError(f"CloudMlp: layer {k} takes {w.shape[1]} channels, the layer before it gives {c_in}")
        c_in = c_out
        out.append((np.ascontiguousarray(w), np.ascontiguousarray(b), bool(relu)))
    return out


class CloudMlp:
    """The layers of one shared MLP (PandaSim.shared_mlp, abstract_features):
    a sequence of (W [c_out, c_in] f32, b [c_out] f32, relu), uploaded once to
    `device` and kept alive here.  c_in is the first layer's input width,
    widths the layers' outputs; array / len() are what the library takes."""

    def __init__(self, layers, device="cuda"):
        host = cloud_mlp_layers(layers)
        self.c_in = int(host[0][0].shape[1])
        self.widths = [int(w.shape[0]) for w, _, _ in host]
        self.relu = [r for _, _, r in host]
        self.device = torch.device(device)
        self.W = [torch.from_numpy(w).to(self.device) for w, _, _ in host]
        self.b = [torch.from_numpy(b).to(self.device) for _, b, _ in host]
        self.array = (L.CloudMlpLayer * len(host))()
        for a, w, b, r in zip(self.array, self.W, self.b, self.relu):
            a.W, a.b, a.c_out, a.relu = w.data_ptr(), b.data_ptr(), int(w.shape[0]), int(r)

    def __len__(self):
        return len(self.widths)


def _mlp_of(what: str, layers):
    if not (hasattr(layers, "widths") and hasattr(layers, "c_in") and hasattr(layers, "array")):
        raise ValueError(f"{what}: layers must be a CloudMlp, got {type(layers).__name__}")
    return layers


def shared_mlp_args(num_envs: int, rows, layers, pool, out, out_offset):
    """shared_mlp's argument checks (ValueError), on tensors of any device:
    -> R, C0 and the width of the result."""
    B = int(num_envs)
    layers = _mlp_of("shared_mlp", layers)
    _want("shared_mlp", "rows", rows, (B, "S", "K", "C0") if rows.dim() == 4 else (B, "R (or S, K)", "C0"))
    C0 = int(rows.shape[-1])
    R = int(rows.shape[1]) if rows.dim() == 3 else int(rows.shape[1]) * int(rows.shape[2])
    if C0 != layers.c_in:
        raise ValueError(f"shared_mlp: rows have {C0} channels, the first layer takes {layers.c_in}")
    if isinstance(pool, bool) or int(pool) != pool or pool < 1 or R < 1 or R % int(pool) != 0 or R >= 1 << 31:
        raise ValueError(f"shared_mlp: pool = {pool} must be a whole number from 1 that divides R = {R}")
    width = layers.widths[-1]
    if isinstance(out_offset, bool) or int(out_offset) != out_offset or out_offset < 0:
        raise ValueError(f"shared_mlp: out_offset = {out_offset} (a whole number from 0)")
    if out is None:
        if out_offset != 0:
            raise ValueError("shared_mlp: out_offset without out")
    else:
        _want("shared_mlp", "out", out, (B, R // int(pool), "W"))
        if not out.is_contiguous():
            raise ValueError(f"shared_mlp: out must be contiguous, got strides {out.stride()}")
        if int(out_offset) + width > out.shape[2]:
            raise ValueError(f"shared_mlp: columns {out_offset} .. {int(out_offset) + width - 1} do not fit out's "
                             f"{out.shape[2]}")
    return R, C0, width


def abstract_features_args(num_envs: int, xyz, feats, centre_idx, group_idx, mlps):
    """abstract_features' argument checks (ValueError), on tensors of any
    device: -> N, S, D, the column offset of each scale and the total width."""
    B = int(num_envs)
    _want("abstract_features", "xyz", xyz, (B, "N", 3))
    N = int(xyz.shape[1])
    if not 1 <= N <= L.CLOUD_MAX_POINTS:
        raise ValueError(f"abstract_features: N = {N} points (1 to {L.CLOUD_MAX_POINTS})")
    _want("abstract_features", "centre_idx", centre_idx, (B, "S"), torch.int32)
    S = int(centre_idx.shape[1])
    if not 1 <= S <= N:
        raise ValueError(f"abstract_features: S = {S} centres (1 to N = {N})")
    D = 0
    if feats is not None:
        _want("abstract_features", "feats", feats, (B, N, "D"))
        D = int(feats.shape[2])
        if not 1 <= D <= L.CLOUD_MAX_PROP_FEATURES:
            raise ValueError(f"abstract_features: D = {D} feature channels (1 to {L.CLOUD_MAX_PROP_FEATURES})")
    if mlps is None or len(group_idx) != len(mlps) or len(mlps) < 1:
        raise ValueError(f"abstract_features: {len(group_idx)} group_idx and {0 if mlps is None else len(mlps)} mlps "
                         f"(equal, at least 1)")
    offsets, width = [], 0
    for k, (gi, mlp) in enumerate(zip(group_idx, mlps)):
        mlp = _mlp_of("abstract_features", mlp)
        _want("abstract_features", f"group_idx[{k}]", gi, (B, S, "K"), torch.int32)
        if gi.shape[2] < 1:
            raise ValueError(f"abstract_features: group_idx[{k}] has K = 0 neighbours (at least 1)")
        if mlp.c_in != D + 3:
            raise ValueError(f"abstract_features: mlps[{k}] takes {mlp.c_in} channels, the rows have D + 3 = {D + 3}")
        offsets.append(width)
        width += mlp.widths[-1]
    return N, S, D, offsets, width
