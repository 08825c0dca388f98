"""GPU tests of the keypoint conditioning (ps_cloud_keypoint_features,
PandaSim.keypoint_features / keypoint_cloud / project_to_pixels).

Two yardsticks, no tolerance in either:
  - the patches' world points must be PandaSim.deproject of render()'s depth
    at the patch pixels, of the same library, bit for bit;
  - the channel must be tests/keypoint_reference.py's keypoint_cond_np fed the
    kernel's own targets and the f32 points, on every element: the arithmetic
    is specified operation by operation (include/pandasim.h), so it is exact.
Against render()'s f64 points (the reference's cloud before any rounding) the
labels may differ only where a distance lies within 1e-6 m of the threshold.

Shapes: Push at B = 3 in 64 x 48 images and Stack at B = 1 in 96 x 96, after
three random steps; K = 300 (two blocks, the second partial), 63 and 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from cloud_helpers import DEV, raw_call, same_bits
from keypoint_reference import keypoint_cond_np, keypoint_min_dist_np, patch_pixels_np

pytestmark = pytest.mark.gpu

CASES = {"push": (3, 64, 48, "object"), "stack": (1, 96, 96, "object1")}  # B, width, height, the keyed object
K, SEED, THRESHOLD = 300, 11, 0.1


def views3():
    import pandasim

    return list(pandasim.GRASP_VIEWS[:3])


class Scene:
    """One case, computed once: the stepped env, its cloud of K samples, the
    keypoint view's depth, and the object's pixel in that view."""

    def __init__(self, task):
        from test_gpu_cloud import stepped_env

        self.B, self.w, self.h, body = CASES[task]
        self.sim = stepped_env(task, self.B).sim
        self.view = views3()[0]
        self.cloud = self.sim.point_cloud(views3(), K, self.w, self.h, SEED)
        self.tran = self.sim.get_cam2world_transforms(self.w, self.h, **self.view)[2]
        self.depth = self.sim.render(self.w, self.h, **self.view)["depth"]
        self.object_px = self.sim.project_to_pixels(self.sim.get_base_position(body).reshape(self.B, 1, 3), self.w,
                                                    self.h, **self.view)

    def features(self, keypoints, **kw):
        kw.setdefault("colors", self.cloud["colors"])
        return self.sim.keypoint_features(self.cloud["points"], keypoints, self.view, width=self.w, height=self.h,
                                          return_targets=True, **kw)

    def expected_targets(self, keypoints, radius):
        """deproject(render()["depth"], patch pixels, tran) [B, n_kp, P, 3] f64,
        NaN where a patch pixel lies outside the image."""
        kps = np.broadcast_to(np.asarray(keypoints), (self.B,) + np.asarray(keypoints).shape[-2:])
        pix = np.stack([[patch_pixels_np(kp, radius, self.w, self.h)[0] for kp in row] for row in kps])
        inside = np.stack([[patch_pixels_np(kp, radius, self.w, self.h)[1] for kp in row] for row in kps])
        safe = np.where(inside[..., None], pix, 0).reshape(self.B, -1, 2)
        got = self.sim.deproject(self.depth, torch.from_numpy(safe), self.tran, self.w, self.h).cpu().numpy()
        got = got.reshape(pix.shape[:3] + (3,))
        got[~inside] = np.nan
        return got, inside

    def expected_cond(self, targets, threshold, values, points=None):
        pts = (self.cloud["points"] if points is None else points).cpu().numpy()
        tg = targets.cpu().numpy()
        return np.stack([keypoint_cond_np(pts[b], tg[b], threshold, values) for b in range(self.B)])


@pytest.fixture(scope="module")
def scenes():
    return {task: Scene(task) for task in CASES}


def same_f64(a, b):
    """Equal bit for bit, a NaN equal to a NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


# ------------------------------------------------------------------ targets
@pytest.mark.parametrize("radius", (0, 3, 8))
@pytest.mark.parametrize("task", tuple(CASES))
def test_targets_are_deproject_of_the_rendered_depth(scenes, task, radius):
    s = scenes[task]
    w, h = s.w, s.h
    # per env the pixel of the largest depth: background, the far plane
    flat = s.depth.reshape(s.B, -1).argmax(1).cpu().numpy()
    assert bool((s.depth.reshape(s.B, -1).max(1).values == 1.0).all()), "the view shows no background"
    back = np.stack([flat % w, flat // w], -1)
    groups = [[(w // 2 + 3, h // 2 - 5), (0, 0), (w - 1, 0), (0, h - 1)],  # interior and three corners
              [(w - 1, h - 1), (w // 3, 0), (w - 1, h // 3), (w + 1, h // 2)],  # a corner, two edges, clipped from outside
              [(w + 9, 5), (5, h + 9), (-1, -1), (-1000, 7)]]  # wholly outside (radius <= 8), negative
    for kps in groups:
        _, targets = s.features(np.array(kps, np.int32), radius=radius)
        want, inside = s.expected_targets(kps, radius)
        got = targets.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == want.shape == (s.B, 4, len(inside[0, 0]), 3)
        assert np.array_equal(np.isnan(got).any(-1), ~inside) and np.isfinite(got[inside]).all()
        assert same_f64(got, want), kps
    assert np.isnan(got).all()  # the last group: discs wholly outside, and negative keypoints (absent)
    # a keypoint on the background, one per env: the far plane's point, finite and far away
    _, targets = s.features(back[:, None, :].astype(np.int32), radius=radius)
    want, inside = s.expected_targets(back[:, None, :], radius)
    assert same_f64(targets.cpu().numpy(), want)
    centre = len(inside[0, 0]) // 2  # the offset (0, 0)
    assert (np.linalg.norm(targets.cpu().numpy()[:, 0, centre], axis=-1) > 10.0).all()


# ------------------------------------------------------------- feature rows
@pytest.mark.parametrize("task", tuple(CASES))
def test_feature_rows_are_the_restatement_on_every_element(scenes, task):
    s = scenes[task]
    feats, targets = s.features(s.object_px, threshold=THRESHOLD)
    assert feats.shape == (s.B, K, 4) and feats.dtype == torch.float32
    want = s.expected_cond(targets, THRESHOLD, (1.0,))
    marked = (want != 0).mean()
    print(f"{task}: {marked:.3f} of the samples marked")
    if task == "push":  # the main case exercises both branches
        assert 0.05 <= marked <= 0.95
    assert same_bits(feats[..., 3], want)
    assert same_bits(feats[..., :3], s.cloud["colors"].float())
    # without colours the channel stands alone
    alone, _ = s.features(s.object_px, threshold=THRESHOLD, colors=None)
    assert alone.shape == (s.B, K, 1) and same_bits(alone[..., 0], want)
    # the same keypoint for every env, given once
    kp = s.object_px[0].cpu().numpy()
    once, t1 = s.features(kp, threshold=THRESHOLD)
    every, t2 = s.features(np.broadcast_to(kp, (s.B, 1, 2)).copy(), threshold=THRESHOLD)
    assert same_bits(once, every) and same_f64(t1.cpu().numpy(), t2.cpu().numpy())


@pytest.mark.parametrize("k", (1, 63))
def test_point_counts_below_a_wave_and_a_block(scenes, k):
    s = scenes["push"]
    pts, cols = s.cloud["points"][:, :k].contiguous(), s.cloud["colors"][:, :k].contiguous()
    feats, targets = s.sim.keypoint_features(pts, s.object_px, s.view, cols, width=s.w, height=s.h,
                                             return_targets=True)
    whole, _ = s.features(s.object_px)
    assert feats.shape == (s.B, k, 4) and same_bits(feats, whole[:, :k])
    assert same_bits(feats[..., 3], s.expected_cond(targets, 0.1, (1.0,), pts))


# ------------------------------------------------- overwrite order and values
def test_later_keypoints_overwrite_and_values_are_the_callers(scenes):
    s = scenes["push"]
    px = s.object_px.cpu().numpy()
    two = np.concatenate([px, px + [2, 0]], 1).astype(np.int32)  # overlapping patches
    values = (0.25, 7.5)
    feats, targets = s.features(two, values=values)
    dist = np.stack([keypoint_min_dist_np(s.cloud["points"][b].cpu().numpy(), targets[b].cpu().numpy())
                     for b in range(s.B)])
    both = (dist < 0.1).all(-1)
    only0 = (dist[..., 0] < 0.1) & ~(dist[..., 1] < 0.1)
    got = feats[..., 3].cpu().numpy()
    assert both.any() and (got[both] == np.float32(7.5)).all() and (got[only0] == np.float32(0.25)).all()
    assert same_bits(feats[..., 3], s.expected_cond(targets, 0.1, values))
    default, _ = s.features(two)
    assert set(np.unique(default[..., 3].cpu().numpy()).tolist()) <= {0.0, 1.0, 2.0}
    assert same_bits(default[..., 3], s.expected_cond(targets, 0.1, (1.0, 2.0)))
    # four keypoints, the last one absent: it overwrites nothing
    four = np.concatenate([px, px + [2, 0], px + [-6, 4], np.full_like(px, -1)], 1).astype(np.int32)
    f4, t4 = s.features(four, radius=0, threshold=0.05)
    want = s.expected_cond(t4, 0.05, (1.0, 2.0, 3.0, 4.0))
    assert same_bits(f4[..., 3], want) and not (want == 4.0).any() and np.isnan(t4[:, 3].cpu().numpy()).all()
    # a threshold above every distance marks everything with the last present keypoint's value ...
    everything, _ = s.features(four, threshold=1e3)
    assert bool((everything[..., 3] == 3.0).all())
    # ... and one below every distance marks nothing
    nothing, _ = s.features(four, threshold=1e-300)  # only a distance of exactly 0 would pass
    assert bool((nothing[..., 3] == 0.0).all())
    assert same_bits(nothing[..., :3], s.cloud["colors"].float())


# ------------------------------------------- against the reference's f64 cloud
@pytest.mark.parametrize("task", tuple(CASES))
def test_labels_of_the_f64_cloud_differ_only_at_the_threshold(scenes, task):
    s = scenes[task]
    n = s.w * s.h
    full = torch.cat([s.sim.render(s.w, s.h, **kw)["points"] for kw in views3()], 1)  # [B, V * n, 3] f64
    src = s.cloud["source"].long()
    assert bool((src >= 0).all()) and full.shape[1] == 3 * n
    exact = torch.gather(full, 1, src[..., None].expand(-1, -1, 3))
    assert same_bits(exact.float(), s.cloud["points"])  # the same samples, before rounding
    two = torch.cat([s.object_px, s.object_px + torch.tensor([5, -2], dtype=torch.int32, device=DEV)], 1)
    feats, targets = s.features(two, threshold=THRESHOLD)
    got, tg, ex = feats[..., 3].cpu().numpy(), targets.cpu().numpy(), exact.cpu().numpy()
    dist = np.stack([keypoint_min_dist_np(ex[b], tg[b]) for b in range(s.B)])
    want = np.stack([keypoint_cond_np(ex[b], tg[b], THRESHOLD, (1.0, 2.0)) for b in range(s.B)])
    near = (np.abs(dist - THRESHOLD) < 1e-6).any(-1)
    print(f"{task}: {near.mean():.4f} of the samples within 1e-6 m of the threshold; marked {(want != 0).mean():.3f}")
    assert near.mean() <= 0.01
    assert np.array_equal(got[~near], want[~near])


# --------------------------------------------------------------- keypoint_cloud
def test_keypoint_cloud_is_point_cloud_then_keypoint_features(scenes):
    s = scenes["push"]
    kps = torch.cat([s.object_px, s.object_px + torch.tensor([3, 3], dtype=torch.int32, device=DEV)], 1)
    crop = ((-10.0, -10.0, 0.002), (10.0, 10.0, 10.0))
    out = s.sim.keypoint_cloud(kps, views3(), n_points=K, width=s.w, height=s.h, seed=SEED, crop=crop)
    cloud = s.sim.point_cloud(views3(), K, s.w, s.h, SEED, crop)
    feats = s.sim.keypoint_features(cloud["points"], kps, views3()[0], cloud["colors"], cloud["count"], width=s.w,
                                    height=s.h)
    for name in ("points", "colors", "source", "count"):
        assert same_bits(out[name], cloud[name]), name
    assert same_bits(out["feats"], feats) and same_bits(out["cond"], feats[..., 3])
    assert int(out["count"].min()) > 0 and bool((out["cond"] != 0).any())
    again = s.sim.keypoint_cloud(kps, views3(), n_points=K, width=s.w, height=s.h, seed=SEED, crop=crop)
    assert all(same_bits(again[name], out[name]) for name in out)
    # another keypoint view than views[0]
    other = s.sim.keypoint_cloud(kps, views3(), keypoint_view=views3()[1], n_points=K, width=s.w, height=s.h,
                                 seed=SEED, crop=crop)
    assert same_bits(other["points"], out["points"])
    assert same_bits(other["feats"], s.sim.keypoint_features(cloud["points"], kps, views3()[1], cloud["colors"],
                                                             cloud["count"], width=s.w, height=s.h))
    # a crop that excludes everything: empty clouds, zero rows
    empty = s.sim.keypoint_cloud(kps, views3(), n_points=K, width=s.w, height=s.h, seed=SEED,
                                 crop=((10.0, 10.0, 10.0), (11.0, 11.0, 11.0)))
    assert bool((empty["count"] == 0).all()) and bool((empty["feats"] == 0).all())
    # one env alone declared empty: its rows are zero, the others' are untouched
    count = cloud["count"].clone()
    count[1] = 0
    part = s.sim.keypoint_features(cloud["points"], kps, views3()[0], cloud["colors"], count, width=s.w, height=s.h)
    assert bool((part[1] == 0).all()) and same_bits(part[0], feats[0]) and same_bits(part[2], feats[2])


# ------------------------------------------------------------------ end to end
def seeded_state7(seed):
    """net_helpers.seeded_state's recipe with inp_dim = 7: the state_dict of
    get_model(14, 7, 4).  The recipe reads its input width from the module's
    NUM_INPUT, which is 7 while this runs and 6 again afterwards."""
    import net_helpers

    before = net_helpers.NUM_INPUT
    net_helpers.NUM_INPUT = 7
    try:
        return net_helpers.seeded_state(seed)
    finally:
        net_helpers.NUM_INPUT = before


def test_seven_channel_policy_end_to_end(scenes):
    from net_helpers import NUM_CLASSES, STATE_SEED, segnet_np
    from pandasim import CloudSegNet
    from test_gpu_net import forward_by_public_calls

    s, n = scenes["stack"], 512
    assert s.B == 1
    kps = torch.cat([s.object_px, s.object_px + torch.tensor([4, 1], dtype=torch.int32, device=DEV)], 1)
    out = s.sim.keypoint_cloud(kps, views3(), n_points=n, width=s.w, height=s.h, seed=SEED)
    assert int(out["count"][0]) > 0 and len(torch.unique(out["cond"])) == 3
    state = seeded_state7(STATE_SEED)
    net = CloudSegNet(state, DEV)
    assert (net.num_classes, net.num_input_channels) == (NUM_CLASSES, 7) and [m.c_in for m in net.sa1] == [10] * 3
    pred = s.sim.predict_waypoints(net, out["points"], out["feats"], SEED)
    head, g1 = s.sim.segment_cloud(net, out["points"], out["feats"], SEED)
    dec = s.sim.decode_waypoints(head, g1.xyz, net.num_classes, g1.centroid, g1.scale)
    for name in ("waypoints", "quats", "euler_deg", "counts", "first_idx"):
        assert same_bits(getattr(pred, name), getattr(dec, name)), name
    written, w1, w2 = forward_by_public_calls(s.sim, net, out["points"], out["feats"], SEED)
    assert same_bits(head, written)
    idx = dict(fps1=w1.fps_idx.cpu().numpy(), group1=[t.cpu().numpy() for t in w1.group_idx],
               fps2=w2.fps_idx.cpu().numpy(), group2=[t.cpu().numpy() for t in w2.group_idx])
    nx, feats = w1.xyz.cpu().numpy(), out["feats"].cpu().numpy()
    h64 = segnet_np(state, nx, feats, idx, np.float64)
    h32 = segnet_np(state, nx, feats, idx, np.float32)
    tol = 4 * np.abs(h32 - h64).max() + 1e-6 * np.abs(h64).max()  # tests/test_gpu_net.py's bound
    err = np.abs(head.cpu().numpy().astype(np.float64) - h64).max()
    print(f"max |gpu - f64| = {err:.3e}, tol = {tol:.3e}, max |head| = {np.abs(h64).max():.3f}")
    assert head.shape == (1, n, NUM_CLASSES + 14) and 0 < tol < 1e-4 * np.abs(h64).max()
    assert err <= tol


# ------------------------------------------------------------ raw entry point
def test_raw_entry_point_refuses_without_launching(scenes):
    from pandasim import _lib as L
    from pandasim.sim import _ptr

    s = scenes["push"]
    sim, pts = s.sim, s.cloud["points"]
    cv, vis, poses = sim._cloud_view(s.w, s.h, s.view), sim._visual(), sim._target_poses().contiguous()
    kps = s.object_px.contiguous()
    feats = torch.full((s.B, K, 4), -7.0, device=DEV)
    values = (C.c_float * 4)(1.0, 2.0, 3.0, 4.0)

    def call(n_kp=1, radius=3, threshold=0.1, points=pts, out=feats, width=s.w):
        return raw_call(sim, "ps_cloud_keypoint_features", sim._ctx, _ptr(sim.state), C.byref(cv), width, s.h,
                        C.byref(vis), _ptr(poses), _ptr(kps), n_kp, radius, threshold, values, _ptr(points),
                        _ptr(s.cloud["colors"]), None, K, _ptr(out), 4, 0, None, sim._stream())

    for kw, text in ((dict(n_kp=0), "n_kp"), (dict(n_kp=5), "n_kp"), (dict(radius=9), "radius"),
                     (dict(radius=-1), "radius"), (dict(points=None), "null"), (dict(out=None), "null"),
                     (dict(threshold=0.0), "threshold"), (dict(threshold=float("nan")), "threshold"),
                     (dict(width=0), "image")):
        assert call(**kw) == -1, kw
        assert text in L.lib().ps_last_error(sim._ctx).decode(), kw
    torch.cuda.synchronize()
    assert bool((feats == -7.0).all())  # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert same_bits(feats, s.features(s.object_px)[0])
