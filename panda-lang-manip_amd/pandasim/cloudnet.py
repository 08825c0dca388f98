"""The batched PointNet++ layer over a point-cloud observation:
sampling and grouping, feature propagation, the shared MLP with max-pool, and
the policy they compose: the network's forward and the waypoint decoding; and
(§11.10) the policy's ground-truth side, forward only: a demonstration's
per-point labels and the value of the losses against them.

``CloudNet`` is a mixin of ``PandaSim``; the checkers, ``GroupedCloud``,
``CloudMlp``, ``fold_batchnorm``, ``CloudSegNet``, ``DecodedWaypoints``,
``CloudLabels``, ``PolicyLoss`` and ``demonstration_records`` beside it need
no simulator at all.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from ._lib import _ptr


class CloudNet:
    """group_cloud, propagate_features, shared_mlp, abstract_features and, on top
    of them, segment_cloud, decode_waypoints and predict_waypoints for B
    clouds; label_cloud, policy_loss and evaluate_policy hold a network
    against a demonstration.  They read no simulator state.  The host class provides exactly
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
        (ps_cloud_mlp, f32 MFMA; with a CloudMlp of precision "bfloat16"
        ps_cloud_mlp_bfloat, bf16 MFMA): per row the chain of `layers` (pointwise
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
        self._call("ps_cloud_mlp" + _SUFFIX[_precision_of(layers)], self._ctx, _ptr(rows), R, C0, layers.array,
                   len(layers), int(pool), _ptr(out), int(out.shape[2]), int(out_offset), self._stream())
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
        and the fused one above D = 16.  With mlps of precision "bfloat16"
        (all of them: a mix raises ValueError) the entry points are
        ps_cloud_group_mlp_bfloat / ps_cloud_mlp_bfloat, the default is the
        fused one, and the two paths give the same bits as well.

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
        suffix = _SUFFIX[_precision_of(mlps[0])]
        if fused is None:
            fused = D > L.CLOUD_MAX_FEATURES or suffix != ""
        for gi, mlp, off in zip(group_idx, mlps, offsets):
            gi, K = gi.contiguous(), int(gi.shape[2])
            if fused:
                self._call("ps_cloud_group_mlp" + suffix, self._ctx, _ptr(xyz), _ptr(feats), N, D, _ptr(centre_idx), S, _ptr(gi),
                           K, mlp.array, len(mlp), _ptr(out), width, off, self._stream())
            else:
                grouped = torch.empty(B, S, K, D + 3, dtype=torch.float32, device=dev)
                self._call("ps_cloud_group", self._ctx, _ptr(xyz), _ptr(feats), N, D, _ptr(centre_idx), S, _ptr(gi), K,
                           _ptr(grouped), None, self._stream())
                self._call("ps_cloud_mlp" + suffix, self._ctx, _ptr(grouped), S * K, D + 3, mlp.array, len(mlp), K,
                           _ptr(out), width, off, self._stream())
        return out

    def decode_waypoints(self, head, xyz, num_classes: int, centroid=None, scale=None, start_classes=(1, 3),
                         end_classes=(2, 3), return_labels: bool = False) -> "DecodedWaypoints":
        """What Inference.predict does after the classifier
        (inference_cls_off_rot.py:68-107) -- fused (ps_cloud_decode_waypoints),
        for every env, on the device: per point the arg-max class (the lowest
        index among equal logits), the start and the end point set (the points
        labelled with one of start_classes / end_classes), per set the mean of
        point - offset times scale plus centroid (f64 sums in a fixed order),
        and the quaternion predicted at the set's first point, normalised and
        as scipy's 'xyz' Euler degrees.  An empty set gives count 0, first_idx
        -1 and NaN, where the reference raises.

        head [B, N, ld] f32 with ld >= num_classes + 14: the logits, then start
        offset (3), end offset (3), start quaternion xyzw (4), end quaternion
        (4); xyz [B, N, 3] f32 the normalised points; centroid [B, 3] and scale
        [B] f32 (a GroupedCloud's), or both None for no un-normalisation.
        Returns a DecodedWaypoints."""
        B, dev = self.num_envs, self.device
        head, xyz = torch.as_tensor(head, device=dev), torch.as_tensor(xyz, device=dev)
        if centroid is not None:
            centroid = torch.as_tensor(centroid, device=dev)
        if scale is not None:
            scale = torch.as_tensor(scale, device=dev)
        N, ld, nc, masks = decode_waypoints_args(B, head, xyz, num_classes, centroid, scale, start_classes, end_classes)
        head, xyz = head.contiguous(), xyz.contiguous()
        centroid = None if centroid is None else centroid.contiguous()
        scale = None if scale is None else scale.contiguous()
        out = DecodedWaypoints()
        out.waypoints = torch.empty(B, 2, 3, dtype=torch.float32, device=dev)
        out.quats = torch.empty(B, 2, 4, dtype=torch.float32, device=dev)
        out.euler_deg = torch.empty(B, 2, 3, dtype=torch.float32, device=dev)
        out.counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
        out.first_idx = torch.empty(B, 2, dtype=torch.int32, device=dev)
        out.labels = torch.empty(B, N, dtype=torch.int32, device=dev) if return_labels else None
        self._call("ps_cloud_decode_waypoints", self._ctx, _ptr(head), N, ld, nc, _ptr(xyz), _ptr(centroid), _ptr(scale),
                   masks[0], masks[1], _ptr(out.waypoints), _ptr(out.quats), _ptr(out.euler_deg), _ptr(out.counts),
                   _ptr(out.labels), _ptr(out.first_idx), self._stream())
        return out

    def segment_cloud(self, net: "CloudSegNet", points, colors, seed: int = 0, normalize: bool = True):
        """model_cls_off_rot.py: get_model.forward at inference, for every env
        (DESIGN.md §11.6 restates the wiring): sa1, sa2, sa3, fp3, fp2, fp1,
        conv1 / bn1, conv2, composed of group_cloud, abstract_features,
        propagate_features and shared_mlp.  Farthest point sampling starts from
        fps_start(seed, b, N) at sa1 and fps_start(seed + 1, b, 512) at sa2.

        points [B, N, 3] f32 with 512 <= N <= CLOUD_MAX_POINTS, colors
        [B, N, C - 3] f32 (C net.num_input_channels).  Returns head
        [B, N, num_classes + 14] f32 (the reference's x before its
        log_softmax, one row per point) and level 1's GroupedCloud, whose xyz,
        centroid and scale decode_waypoints takes."""
        B, dev = self.num_envs, self.device
        points, colors = torch.as_tensor(points, device=dev), torch.as_tensor(colors, device=dev)
        segment_cloud_args(B, net, points, colors)
        g1 = self.group_cloud(points, None, net.SA1_NPOINT, net.SA1_RADII, net.SA1_NSAMPLES, seed, normalize)
        l0 = torch.cat([g1.xyz, colors], dim=2)
        l1 = self.abstract_features(g1, l0, mlps=net.sa1)
        g2 = self.group_cloud(g1.new_xyz, None, net.SA2_NPOINT, net.SA2_RADII, net.SA2_NSAMPLES, seed + 1,
                              normalize=False)
        l2 = self.abstract_features(g2, l1, mlps=net.sa2)
        l3 = self.shared_mlp(torch.cat([g2.new_xyz, l2], dim=2), net.sa3, pool=net.SA2_NPOINT)
        origin = torch.zeros(B, 1, 3, dtype=torch.float32, device=dev)
        l2 = self.shared_mlp(self.propagate_features(g2.new_xyz, origin, l3, l2), net.fp3)
        l1 = self.shared_mlp(self.propagate_features(g1.new_xyz, g2.new_xyz, l2, l1), net.fp2)
        l0 = self.shared_mlp(self.propagate_features(g1.xyz, g1.new_xyz, l1, torch.cat([g1.xyz, l0], dim=2)), net.fp1)
        return self.shared_mlp(l0, net.head), g1

    def predict_waypoints(self, net: "CloudSegNet", points, colors, seed: int = 0) -> "DecodedWaypoints":
        """The batched Inference.predict: segment_cloud, then decode_waypoints
        with that cloud's centroid and scale."""
        head, g1 = self.segment_cloud(net, points, colors, seed)
        return self.decode_waypoints(head, g1.xyz, net.num_classes, g1.centroid, g1.scale)

    def label_cloud(self, points, waypoints, quats, radius: float = 0.125, group=None, count=None) -> "CloudLabels":
        """The training targets a demonstration gives every env's cloud
        (generate_combined_dset.py:422-484, record, with the loader's
        normalisation of the waypoints, PourDataLoader_cls_off.py:43-45) --
        fused (ps_cloud_waypoint_labels), on the device: per point the class
        (0 neither, 1 within `radius` of the start waypoint, 2 of the end
        waypoint, 3 of both; the distance is not strict) and the 14 columns
        the head carries behind its logits: start offset (3) and end offset
        (3), normalised point - normalised waypoint where the point is in that
        set, else 0; start and end quaternion (4 + 4), `quats` where the point
        is in that set, else 0.  A point of class 3 carries both.

        points [B, N, 3] f32 in the world, waypoints [B, 2, 3] f32 in the world
        (start, end), quats [B, 2, 4] f32 xyzw, count None or [B] i32
        (point_cloud()'s "count": a cloud whose count is 0 gets class -1, which
        policy_loss ignores, and zero targets).  group None normalises the
        cloud here (ps_cloud_normalize, N <= CLOUD_MAX_POINTS); or the
        GroupedCloud segment_cloud returned for these points, whose xyz,
        centroid and scale are then used.  Returns a CloudLabels."""
        B, dev = self.num_envs, self.device
        points, waypoints, quats = (torch.as_tensor(t, device=dev) for t in (points, waypoints, quats))
        if count is not None:
            count = torch.as_tensor(count, device=dev)
        N, radius = waypoint_labels_args(B, points, waypoints, quats, radius, group, count)
        points, waypoints, quats = points.contiguous(), waypoints.contiguous(), quats.contiguous()
        count = None if count is None else count.contiguous()
        out = CloudLabels()
        if group is None:
            out.xyz = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
            out.centroid = torch.empty(B, 3, dtype=torch.float32, device=dev)
            out.scale = torch.empty(B, dtype=torch.float32, device=dev)
            self._call("ps_cloud_normalize", self._ctx, _ptr(points), N, _ptr(out.xyz), _ptr(out.centroid),
                       _ptr(out.scale), self._stream())
        else:
            out.xyz, out.centroid, out.scale = group.xyz.contiguous(), group.centroid.contiguous(), group.scale.contiguous()
        out.cls = torch.empty(B, N, dtype=torch.int32, device=dev)
        out.target = torch.empty(B, N, L.CLOUD_LABEL_COLUMNS, dtype=torch.float32, device=dev)
        self._call("ps_cloud_waypoint_labels", self._ctx, _ptr(points), _ptr(out.xyz), _ptr(out.centroid),
                   _ptr(out.scale), _ptr(waypoints), _ptr(quats), radius, _ptr(count), N, _ptr(out.cls),
                   _ptr(out.target), L.CLOUD_LABEL_COLUMNS, 0, self._stream())
        return out

    def policy_loss(self, head, cls, target, num_classes: int, start_classes=(1, 3), end_classes=(2, 3),
                    return_confusion: bool = False) -> "PolicyLoss":
        """The forward value of the reference's losses
        (model_cls_off_rot.py:63-79: F.nll_loss on the class log-softmax,
        nn.L1Loss on the offsets and the quaternions) of a head against
        label_cloud's targets -- fused (ps_cloud_policy_loss), with the
        accuracy; no backward pass.  A point whose cls is not a class (-1) is
        ignored everywhere.  The L1 terms run over the points whose TRUE class
        is in the start (end) set.

        head [B, N, ld] f32 with ld >= num_classes + 14, cls [B, N] i32,
        target [B, N, 14] f32.  Returns a PolicyLoss of device tensors; nothing
        here waits for the device."""
        B, dev = self.num_envs, self.device
        head, cls, target = (torch.as_tensor(t, device=dev) for t in (head, cls, target))
        N, ld, nc, ld_t, masks = policy_loss_args(B, head, cls, target, num_classes, start_classes, end_classes)
        head, cls, target = head.contiguous(), cls.contiguous(), target.contiguous()
        out = PolicyLoss()
        out.sums = torch.empty(B, 5, dtype=torch.float64, device=dev)
        out.counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
        out.confusion = torch.empty(B, nc, nc, dtype=torch.int32, device=dev) if return_confusion else None
        self._call("ps_cloud_policy_loss", self._ctx, _ptr(head), N, ld, nc, _ptr(cls), _ptr(target), ld_t, 0, masks[0],
                   masks[1], _ptr(out.sums), _ptr(out.counts), _ptr(out.confusion), self._stream())
        s, c = out.sums.sum(0), out.counts.sum(0).to(torch.float64)
        rows = c[1] + c[2]
        out.cls_loss = s[0] / c[0]
        out.offset_loss = (s[1] + s[2]) / (3.0 * rows)
        out.rot_loss = (s[3] + s[4]) / (4.0 * rows)
        out.accuracy = c[3] / c[0]
        return out

    def evaluate_policy(self, net: "CloudSegNet", points, colors, waypoints, quats, radius: float = 0.125,
                        seed: int = 0, count=None) -> "PolicyEvaluation":
        """A network against a demonstration, for every env: segment_cloud,
        label_cloud on that cloud's normalisation, policy_loss, and
        decode_waypoints with the distance of each decoded waypoint from the
        true one.  colors is what segment_cloud takes ([B, N, C - 3] f32:
        the colours, or keypoint_features' rows).  Returns a PolicyEvaluation."""
        head, g1 = self.segment_cloud(net, points, colors, seed)
        out = PolicyEvaluation()
        out.head = head
        out.labels = self.label_cloud(points, waypoints, quats, radius, g1, count)
        out.loss = self.policy_loss(head, out.labels.cls, out.labels.target, net.num_classes)
        out.decoded = self.decode_waypoints(head, g1.xyz, net.num_classes, g1.centroid, g1.scale)
        truth = torch.as_tensor(waypoints, device=self.device).to(torch.float32)
        out.waypoint_error = torch.linalg.vector_norm(out.decoded.waypoints - truth, dim=-1)
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


PRECISIONS = ("float32", "bfloat16")
_SUFFIX = {"float32": "", "bfloat16": "_bfloat"}  # of the library's entry points


def _check_precision(what: str, precision) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"{what}: precision must be one of {PRECISIONS}, got {precision!r}")
    return precision


def round_bfloat16(a):
    """f32 -> bfloat16, round to nearest even on the f32 bit pattern (host
    numpy): -> (the bf16 bit patterns as uint16, their values as float32), in
    a's shape.  A value beyond the largest finite bf16 by half a step or more
    rounds to infinity; NaN stays NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(a)
    if nan.any():  # the carry must not turn a NaN into an infinity or a number
        r = np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)
    return r, (r.astype(np.uint32) << 16).view(np.float32)


def pack_bfloat16(w):
    """W [c_out, c_in] f32 -> [c_out, ldw] uint16: its bf16 bit patterns with
    ldw = c_in rounded up to a multiple of 8 and zeros behind c_in (the layout
    of ps_cloud_mlp_bfloat_layer.W)."""
    c_out, c_in = w.shape
    out = np.zeros((c_out, (c_in + 7) & ~7), np.uint16)
    out[:, :c_in] = round_bfloat16(w)[0]
    return out


class CloudMlp:
    """The layers of one shared MLP (PandaSim.shared_mlp, abstract_features):
    a sequence of (W [c_out, c_in] f32, b [c_out] f32, relu), uploaded once to
    `device` and kept alive here.  c_in is the first layer's input width,
    widths the layers' outputs; array / len() are what the library takes.
    precision "float32" (the default) uploads W as it is; "bfloat16" rounds W
    to bfloat16 once here (pack_bfloat16; a weight that rounds to infinity
    raises ValueError) and keeps b f32: W is then the uint16 tensor, array the
    bfloat layer struct, and the calls go to the bf16 matrix cores."""

    def __init__(self, layers, device="cuda", precision="float32"):
        self.precision = _check_precision("CloudMlp", precision)
        host = cloud_mlp_layers(layers)
        self.c_in = int(host[0][0].shape[1])
        self.widths = [int(w.shape[0]) for w, _, _ in host]
        self.relu = [r for _, _, r in host]
        self.device = torch.device(device)
        self.b = [torch.from_numpy(b).to(self.device) for _, b, _ in host]
        if precision == "bfloat16":
            packed = [pack_bfloat16(w) for w, _, _ in host]
            for k, p in enumerate(packed):
                if ((p & 0x7FFF) == 0x7F80).any():
                    raise ValueError(f"CloudMlp: layer {k} has a weight that rounds to infinity in bfloat16")
            # int16 storage of the same bits: torch has no uint16 arithmetic, and needs none here
            self.W = [torch.from_numpy(p.view(np.int16)).to(self.device) for p in packed]
            if any(w.data_ptr() % 16 for w in self.W):
                raise ValueError("CloudMlp: the device allocator returned a W that is not 16-byte aligned")
            self.array = (L.CloudMlpBfloatLayer * len(host))()
            for a, w, b, r in zip(self.array, self.W, self.b, self.relu):
                a.W, a.b, a.c_out, a.relu = w.data_ptr(), b.data_ptr(), int(w.shape[0]), int(r)
            return
        self.W = [torch.from_numpy(w).to(self.device) for w, _, _ in host]
        self.array = (L.CloudMlpLayer * len(host))()
        for a, w, b, r in zip(self.array, self.W, self.b, self.relu):
            a.W, a.b, a.c_out, a.relu = w.data_ptr(), b.data_ptr(), int(w.shape[0]), int(r)

    def __len__(self):
        return len(self.widths)


def _mlp_of(what: str, layers):
    if not (hasattr(layers, "widths") and hasattr(layers, "c_in") and hasattr(layers, "array")):
        raise ValueError(f"{what}: layers must be a CloudMlp, got {type(layers).__name__}")
    return layers


def _precision_of(layers) -> str:
    """A CloudMlp's precision; an object without one is a float32 one."""
    return getattr(layers, "precision", "float32")


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
        if _precision_of(mlp) != _precision_of(mlps[0]):
            raise ValueError(f"abstract_features: mlps[{k}] is {_precision_of(mlp)}, mlps[0] {_precision_of(mlps[0])} "
                             f"(one precision for all scales)")
        offsets.append(width)
        width += mlp.widths[-1]
    return N, S, D, offsets, width


# ------------------------------------------------------------ the policy
class DecodedWaypoints:
    """PandaSim.decode_waypoints' result; index 0 of the second dimension is the
    start set, 1 the end set: waypoints [B, 2, 3] f32, quats [B, 2, 4] f32
    (normalised xyzw), euler_deg [B, 2, 3] f32 (scipy's 'xyz', what
    step(..., euler_xyz=...) takes), counts [B, 2] i32 (the sets' sizes),
    first_idx [B, 2] i32 (the lowest point index of each set, -1 for an empty
    one, whose waypoint, quaternion and angles are NaN) and labels [B, N] i32
    (None unless asked for)."""

    __slots__ = ("waypoints", "quats", "euler_deg", "counts", "first_idx", "labels")


def _class_mask(name: str, classes, nc: int) -> int:
    try:
        classes = list(classes)
    except TypeError:
        raise ValueError(f"decode_waypoints: {name} must be a sequence of class indices") from None
    mask = 0
    for c in classes:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < nc:
            raise ValueError(f"decode_waypoints: {name} holds {c!r} (whole numbers from 0 to num_classes - 1 = {nc - 1})")
        mask |= 1 << int(c)
    if mask == 0:
        raise ValueError(f"decode_waypoints: {name} is empty")
    return mask


def decode_waypoints_args(num_envs: int, head, xyz, num_classes, centroid, scale, start_classes, end_classes):
    """decode_waypoints' argument checks (ValueError), on tensors of any
    device: -> N, ld, num_classes and the two class masks."""
    B = int(num_envs)
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or \
            not 2 <= num_classes <= L.CLOUD_DECODE_MAX_CLASSES:
        raise ValueError(f"decode_waypoints: num_classes = {num_classes!r} (a whole number from 2 to "
                         f"{L.CLOUD_DECODE_MAX_CLASSES})")
    nc = int(num_classes)
    _want("decode_waypoints", "head", head, (B, "N", "ld"))
    N, ld = int(head.shape[1]), int(head.shape[2])
    if not 1 <= N <= L.CLOUD_MAX_DENSE_POINTS:
        raise ValueError(f"decode_waypoints: N = {N} points (1 to {L.CLOUD_MAX_DENSE_POINTS})")
    if not nc + 14 <= ld <= L.CLOUD_DECODE_MAX_LD:
        raise ValueError(f"decode_waypoints: head rows of {ld} columns (num_classes + 14 = {nc + 14} to "
                         f"{L.CLOUD_DECODE_MAX_LD}: logits, two offsets, two quaternions)")
    _want("decode_waypoints", "xyz", xyz, (B, N, 3))
    if (centroid is None) != (scale is None):
        raise ValueError("decode_waypoints: centroid and scale go together (both, or neither for no un-normalisation)")
    if centroid is not None:
        _want("decode_waypoints", "centroid", centroid, (B, 3))
        _want("decode_waypoints", "scale", scale, (B,))
    return N, ld, nc, (_class_mask("start_classes", start_classes, nc), _class_mask("end_classes", end_classes, nc))


# ------------------------------------------------- the labels and the losses
class CloudLabels:
    """PandaSim.label_cloud's result: cls [B, N] i32 (0 neither set, 1 start, 2
    end, 3 both; -1 at every point of an empty cloud), target [B, N, 14] f32
    (start offset 3, end offset 3, start quaternion 4, end quaternion 4: the
    head's columns behind its logits), and the normalisation the offsets are
    in: xyz [B, N, 3], centroid [B, 3], scale [B] f32."""

    __slots__ = ("cls", "target", "xyz", "centroid", "scale")


class PolicyLoss:
    """PandaSim.policy_loss' result, device tensors.  Per cloud: sums [B, 5]
    f64 (the NLL; |head - target| of the start offsets, the end offsets, the
    start quaternions, the end quaternions), counts [B, 4] i32 (the labelled
    points, those whose true class is in the start set, in the end set, those
    predicted right) and confusion [B, nc, nc] i32 (true x predicted; None
    unless asked for).  Over the batch, f64 scalars:
        cls_loss    = sum of the NLL / labelled points (F.nll_loss' mean),
        offset_loss = the two offset sums / (3 * (start rows + end rows)),
        rot_loss    = the two quaternion sums / (4 * (start rows + end rows)),
        accuracy    = points predicted right / labelled points.
    The reference ships the loss modules but no script that calls them: these
    means, L1Loss' mean over the elements of the sets' rows, are this
    package's definition.  A batch without a labelled point (a row of either
    set) gives NaN there."""

    __slots__ = ("sums", "counts", "confusion", "cls_loss", "offset_loss", "rot_loss", "accuracy")


class PolicyEvaluation:
    """PandaSim.evaluate_policy's result: head [B, N, nc + 14], labels (a
    CloudLabels), loss (a PolicyLoss), decoded (a DecodedWaypoints) and
    waypoint_error [B, 2] f32, the distance of each decoded waypoint from the
    true one (NaN where the predicted set is empty)."""

    __slots__ = ("head", "labels", "loss", "decoded", "waypoint_error")


def waypoint_labels_args(num_envs: int, points, waypoints, quats, radius, group, count):
    """label_cloud's argument checks (ValueError), on tensors of any device:
    -> N and the radius as a float."""
    B, fn = int(num_envs), "label_cloud"
    _want(fn, "points", points, (B, "N", 3))
    N = int(points.shape[1])
    most = L.CLOUD_MAX_DENSE_POINTS if group is not None else L.CLOUD_MAX_POINTS
    if not 1 <= N <= most:
        raise ValueError(f"{fn}: N = {N} points (1 to {L.CLOUD_MAX_POINTS}; to {L.CLOUD_MAX_DENSE_POINTS} with a "
                         f"group that holds the normalisation)")
    _want(fn, "waypoints", waypoints, (B, 2, 3))
    _want(fn, "quats", quats, (B, 2, 4))
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or \
            not 0.0 < float(radius) < math.inf:
        raise ValueError(f"{fn}: radius = {radius!r} must be positive and finite")
    if group is not None:
        if not all(hasattr(group, a) for a in ("xyz", "centroid", "scale")) or group.centroid is None:
            raise ValueError(f"{fn}: group must hold xyz, centroid and scale (a GroupedCloud of normalize=True)")
        _want(fn, "group.xyz", group.xyz, (B, N, 3))
        _want(fn, "group.centroid", group.centroid, (B, 3))
        _want(fn, "group.scale", group.scale, (B,))
    if count is not None:
        _want(fn, "count", count, (B,), torch.int32)
    return N, float(radius)


def policy_loss_args(num_envs: int, head, cls, target, num_classes, start_classes, end_classes):
    """policy_loss' argument checks (ValueError), on tensors of any device:
    -> N, ld, num_classes, the target's row length and the two class masks."""
    B, fn = int(num_envs), "policy_loss"
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or \
            not 2 <= num_classes <= L.CLOUD_DECODE_MAX_CLASSES:
        raise ValueError(f"{fn}: num_classes = {num_classes!r} (a whole number from 2 to "
                         f"{L.CLOUD_DECODE_MAX_CLASSES})")
    nc = int(num_classes)
    _want(fn, "head", head, (B, "N", "ld"))
    N, ld = int(head.shape[1]), int(head.shape[2])
    if not 1 <= N <= L.CLOUD_MAX_DENSE_POINTS:
        raise ValueError(f"{fn}: N = {N} points (1 to {L.CLOUD_MAX_DENSE_POINTS})")
    if not nc + L.CLOUD_LABEL_COLUMNS <= ld <= L.CLOUD_DECODE_MAX_LD:
        raise ValueError(f"{fn}: head rows of {ld} columns (num_classes + 14 = {nc + 14} to {L.CLOUD_DECODE_MAX_LD})")
    _want(fn, "cls", cls, (B, N), torch.int32)
    _want(fn, "target", target, (B, N, L.CLOUD_LABEL_COLUMNS))
    try:
        masks = (_class_mask("start_classes", start_classes, nc), _class_mask("end_classes", end_classes, nc))
    except ValueError as e:
        raise ValueError(str(e).replace("decode_waypoints", fn, 1)) from None
    return N, ld, nc, int(target.shape[2]), masks


def demonstration_records(points, colors, keypoint, waypoints, quats, cls, label="pour", count=None):
    """The B dicts record() saves (generate_combined_dset.py:483), from
    point_cloud()'s and label_cloud()'s tensors -- host side, off the hot path:
    np.save(path, records[b]) writes a file the reference's PourDataset reads.

    points [B, N, 3], colors [B, N, 3], keypoint [B, N] (the conditioning
    channel) or None, waypoints [B, 2, 3], quats [B, 2, 4], cls [B, N]; tensors
    of any device or arrays.  label one string or B of them.  count None or
    [B]: a cloud whose count is 0 has no points.  Each dict holds xyz [M, 3]
    f64, xyz_color [M, 3] f64 (the values given, 0..255 for point_cloud()'s),
    xyz_kpt [M] f64 (zeros without keypoint), start_waypoint and end_waypoint
    [3] f64, cls [M] f64, start_ori and end_ori [4] f64 xyzw, label."""
    def host(a, dtype=np.float64):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return a.astype(dtype)

    pts, col, wp, q, cl = host(points), host(colors), host(waypoints), host(quats), host(cls)
    B = pts.shape[0]
    if pts.ndim != 3 or pts.shape[2] != 3 or col.shape != pts.shape or wp.shape != (B, 2, 3) or \
            q.shape != (B, 2, 4) or cl.shape != pts.shape[:2]:
        raise ValueError(f"demonstration_records: points [B, N, 3], colors [B, N, 3], waypoints [B, 2, 3], quats "
                         f"[B, 2, 4], cls [B, N]; got {pts.shape}, {col.shape}, {wp.shape}, {q.shape}, {cl.shape}")
    kp = np.zeros(pts.shape[:2]) if keypoint is None else host(keypoint)
    if kp.shape != pts.shape[:2]:
        raise ValueError(f"demonstration_records: keypoint must be [B, N], got {kp.shape}")
    labels = [label] * B if isinstance(label, str) else list(label)
    if len(labels) != B:
        raise ValueError(f"demonstration_records: {len(labels)} labels for {B} clouds")
    cnt = None if count is None else host(count, np.int64).reshape(-1)
    if cnt is not None and cnt.shape != (B,):
        raise ValueError(f"demonstration_records: count must be [B], got {cnt.shape}")
    out = []
    for b in range(B):
        m = pts.shape[1] if cnt is None or cnt[b] > 0 else 0
        out.append({"xyz": pts[b, :m].copy(), "xyz_color": col[b, :m].copy(), "xyz_kpt": kp[b, :m].copy(),
                    "start_waypoint": wp[b, 0].copy(), "end_waypoint": wp[b, 1].copy(), "cls": cl[b, :m].copy(),
                    "start_ori": q[b, 0].copy(), "end_ori": q[b, 1].copy(), "label": labels[b]})
    return out


_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def _state_array(state, key: str):
    if key not in state:
        raise ValueError(f"CloudSegNet: the state has no {key}")
    a = state[key]
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)


def _state_layer(state, conv: str, bn, c_in: int, relu: bool, eps: float):
    """One layer of a CloudMlp from the state: `conv` (+ `bn` folded in)."""
    w = _state_array(state, conv + ".weight")
    if not 2 <= w.ndim <= 4 or any(d != 1 for d in w.shape[2:]) or w.shape[0] < 1 or w.shape[1] != c_in:
        raise ValueError(f"CloudSegNet: {conv}.weight must be [c_out, {c_in}, 1(, 1)] (the layer before it gives "
                         f"{c_in} channels), got {w.shape}")
    c_out, vec = int(w.shape[0]), []
    for key in [conv + ".bias"] + [f"{bn}.{n}" for n in (_BN_KEYS if bn else ())]:
        a = _state_array(state, key)
        if a.shape != (c_out,):
            raise ValueError(f"CloudSegNet: {key} must be [{c_out}], got {a.shape}")
        vec.append(a)
    if bn is None:
        return w.reshape(c_out, c_in).astype(np.float32), vec[0].astype(np.float32), relu
    try:
        return (*fold_batchnorm(w, *vec, eps), relu)
    except ValueError as e:
        raise ValueError(f"CloudSegNet: {bn}: {e}") from None


def _state_chain(state, convs: str, bns: str, c_in: int, eps: float):
    """The layers `convs`.0, .1, ... with their batch norms -> a CloudMlp's list."""
    layers, j = [], 0
    while j == 0 or f"{convs}.{j}.weight" in state:
        layers.append(_state_layer(state, f"{convs}.{j}", f"{bns}.{j}", c_in, True, eps))
        c_in, j = int(layers[-1][0].shape[0]), j + 1
    if any(k.startswith((f"{convs}.{j}.", f"{bns}.{j}.")) for k in state):  # a later layer's other keys
        raise ValueError(f"CloudSegNet: the state has no {convs}.{j}.weight")
    return layers


def segnet_layers(state, eps: float = 1e-5):
    """CloudSegNet's host half (ValueError naming the key that is missing or
    mis-shaped): the state_dict of a model_cls_off_rot.get_model, key ->
    array or tensor, as the folded layer lists of its seven shared MLPs:
    -> ({"sa1": [3 lists], "sa2": [2 lists], "sa3", "fp3", "fp2", "fp1",
    "head": lists of (W f32, b f32, relu)}, num_classes, num_input_channels).
    `eps` is the batch norms' (not part of a state_dict; torch's default)."""
    w0 = _state_array(state, "sa1.conv_blocks.0.0.weight")
    C = (int(w0.shape[1]) if w0.ndim >= 2 else 0) - 3
    if C < 3:
        raise ValueError(f"CloudSegNet: sa1.conv_blocks.0.0.weight must take num_input_channels + 3 >= 6 channels, "
                         f"got {w0.shape}")
    out = {}
    c_in = C
    for name, scales in (("sa1", len(CloudSegNet.SA1_RADII)), ("sa2", len(CloudSegNet.SA2_RADII))):
        if f"{name}.conv_blocks.{scales}.0.weight" in state:
            raise ValueError(f"CloudSegNet: {name}.conv_blocks.{scales}.0.weight: {name} has {scales} scales")
        out[name] = [_state_chain(state, f"{name}.conv_blocks.{i}", f"{name}.bn_blocks.{i}", c_in + 3, eps)
                     for i in range(scales)]
        c_in = sum(int(mlp[-1][0].shape[0]) for mlp in out[name])
    w1, w2 = (sum(int(mlp[-1][0].shape[0]) for mlp in out[n]) for n in ("sa1", "sa2"))
    out["sa3"] = _state_chain(state, "sa3.mlp_convs", "sa3.mlp_bns", w2 + 3, eps)
    out["fp3"] = _state_chain(state, "fp3.mlp_convs", "fp3.mlp_bns", w2 + int(out["sa3"][-1][0].shape[0]), eps)
    out["fp2"] = _state_chain(state, "fp2.mlp_convs", "fp2.mlp_bns", w1 + int(out["fp3"][-1][0].shape[0]), eps)
    out["fp1"] = _state_chain(state, "fp1.mlp_convs", "fp1.mlp_bns", 3 + C + int(out["fp2"][-1][0].shape[0]), eps)
    conv1 = _state_layer(state, "conv1", "bn1", int(out["fp1"][-1][0].shape[0]), True, eps)
    conv2 = _state_layer(state, "conv2", None, int(conv1[0].shape[0]), False, eps)
    nc = int(conv2[0].shape[0]) - CloudSegNet.NUM_OUTPUT_CHANNELS
    if not 2 <= nc <= L.CLOUD_DECODE_MAX_CLASSES:
        raise ValueError(f"CloudSegNet: conv2.weight must give num_classes + {CloudSegNet.NUM_OUTPUT_CHANNELS} "
                         f"channels with 2 to {L.CLOUD_DECODE_MAX_CLASSES} classes, got {conv2[0].shape[0]}")
    out["head"] = [conv1, conv2]
    return out, nc, C


class CloudSegNet:
    """The weights of one model_cls_off_rot.get_model at inference, for
    PandaSim.segment_cloud / predict_waypoints: built from a mapping with the
    reference's state_dict key names (sa1.conv_blocks.0.0.weight,
    sa1.bn_blocks.0.0.running_var, sa3.mlp_convs.1.bias, fp2.mlp_bns.0.weight,
    conv1.weight, bn1.running_mean, conv2.bias, ...; num_batches_tracked is not
    read) to arrays or tensors.  Every conv + bn pair is folded
    (fold_batchnorm) into a CloudMlp on `device`: sa1 and sa2 are lists of one
    per scale, sa3, fp3, fp2, fp1 one each, head is conv1 + bn1 with ReLU then
    conv2 without (dropout is the identity at inference).  num_classes,
    num_input_channels and every width come from the shapes; a missing or
    mis-shaped key raises ValueError naming it.  The sampling constants are the
    reference's (model_cls_off_rot.py:12-14).  `precision` ("float32" or
    "bfloat16") is that of every CloudMlp of the net; sampling, grouping,
    propagation and decoding are f32 either way."""

    SA1_NPOINT, SA1_RADII, SA1_NSAMPLES = 512, (0.1, 0.2, 0.4), (32, 64, 128)
    SA2_NPOINT, SA2_RADII, SA2_NSAMPLES = 128, (0.4, 0.8), (64, 128)
    NUM_OUTPUT_CHANNELS = 14  # two offsets and two quaternions behind the logits

    def __init__(self, state, device="cuda", eps: float = 1e-5, precision="float32"):
        self.precision = _check_precision("CloudSegNet", precision)
        layers, self.num_classes, self.num_input_channels = segnet_layers(state, eps)
        self.device = torch.device(device)
        self.sa1 = [CloudMlp(mlp, self.device, precision) for mlp in layers["sa1"]]
        self.sa2 = [CloudMlp(mlp, self.device, precision) for mlp in layers["sa2"]]
        self.sa3, self.fp3, self.fp2, self.fp1, self.head = (CloudMlp(layers[n], self.device, precision)
                                                             for n in ("sa3", "fp3", "fp2", "fp1", "head"))
        self.widths = {n: [m.widths for m in v] if isinstance(v, list) else v.widths
                       for n, v in (("sa1", self.sa1), ("sa2", self.sa2), ("sa3", self.sa3), ("fp3", self.fp3),
                                    ("fp2", self.fp2), ("fp1", self.fp1), ("head", self.head))}


def segment_cloud_args(num_envs: int, net, points, colors) -> int:
    """segment_cloud's argument checks (ValueError), on tensors of any device:
    -> N."""
    B = int(num_envs)
    if not all(hasattr(net, a) for a in ("sa1", "sa2", "sa3", "fp3", "fp2", "fp1", "head", "num_input_channels")):
        raise ValueError(f"segment_cloud: net must be a CloudSegNet, got {type(net).__name__}")
    _want("segment_cloud", "points", points, (B, "N", 3))
    N = int(points.shape[1])
    if not net.SA1_NPOINT <= N <= L.CLOUD_MAX_POINTS:
        raise ValueError(f"segment_cloud: N = {N} points ({net.SA1_NPOINT}, the centres of sa1, to "
                         f"{L.CLOUD_MAX_POINTS})")
    _want("segment_cloud", "colors", colors, (B, N, net.num_input_channels - 3))
    return N
