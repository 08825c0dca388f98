"""CPU tests of the keypoint conditioning (ps_cloud_keypoint_features,
PandaSim.keypoint_features / project_to_pixels): the numpy restatement
(tests/keypoint_reference.py) that tests/test_gpu_keypoint.py holds the kernel
to, itself held to the golden recorded with the reference's own scikit-learn
calls (tests/golden/make_keypoint_golden.py); the new ABI symbol; the Python
layer's argument checks; and project_to_pixels against render()'s host
arithmetic on the render goldens' cameras.
"""
import math
import os

import numpy as np
import pytest
import torch

from cloud_helpers import assert_abi_topic
from keypoint_reference import keypoint_cond_np, keypoint_min_dist_np, patch_offsets_np, patch_pixels_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYPOINT_SYMBOLS = ("ps_cloud_keypoint_features",)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "keypoint_golden.npz")))


def golden_targets(g):
    """The golden's targets in the restatement's slot order [n_kp, P, 3]: NaN
    where a slot's pixel is outside the image."""
    w, h, radius = int(g["width"]), int(g["height"]), int(g["radius"])
    out = []
    for k, kp in enumerate(g["keypoints"]):
        pix, inside = patch_pixels_np(kp, radius, w, h)
        by_pixel = {tuple(p): t for p, t in zip(g[f"patch{k}"].tolist(), g[f"targets{k}"])}
        out.append([by_pixel[tuple(p)] if ok else [np.nan] * 3 for p, ok in zip(pix.tolist(), inside)])
    return np.array(out, np.float64)


def test_patch_sizes_and_slot_order():
    from pandasim import patch_size

    for radius, want in ((0, 1), (1, 5), (3, 29), (8, 197)):
        off = patch_offsets_np(radius)
        assert len(off) == want == patch_size(radius)
        assert (off[:, 0] ** 2 + off[:, 1] ** 2 <= radius * radius).all()
        assert off.tolist() == sorted(off.tolist())  # dx ascending, then dy ascending
        every = [(dx, dy) for dx in range(-9, 10) for dy in range(-9, 10) if dx * dx + dy * dy <= radius * radius]
        assert sorted(map(tuple, off.tolist())) == every


def test_patch_equals_the_references_radius_neighbours(golden):
    w, h, radius = int(golden["width"]), int(golden["height"]), int(golden["radius"])
    for k, kp in enumerate(golden["keypoints"]):
        pix, inside = patch_pixels_np(kp, radius, w, h)
        assert set(map(tuple, pix[inside].tolist())) == set(map(tuple, golden[f"patch{k}"].tolist())), k
        assert inside.sum() == len(golden[f"patch{k}"])
    assert len(golden["patch0"]) == 29 and len(golden["patch1"]) == 11  # interior, clipped at the corner
    # a disc wholly outside the image has no pixel
    for kp in ((-4, 10), (10, -4), (w + 3, 5), (5, h + 3), (-1000, -1000), (-1, -1), (-1, 10), (10, -1)):
        assert not patch_pixels_np(kp, radius, w, h)[1].any()


def test_labels_equal_the_references_nearest_neighbour_marks(golden):
    thr, n_kp = float(golden["threshold"]), len(golden["keypoints"])
    gd = np.stack([golden[f"dists{k}"] for k in range(n_kp)], -1)
    # the fixture keeps every point clear of the threshold: no point is excluded
    assert np.abs(gd - thr).min() > 1e-9
    targets = golden_targets(golden)
    dist = keypoint_min_dist_np(golden["points"], targets)
    assert np.abs(dist - gd).max() < 1e-12
    for k in range(n_kp):
        assert np.array_equal(np.where(dist[:, k] < thr)[0], golden[f"marked{k}"]), k
    cond = keypoint_cond_np(golden["points"], targets, thr, (1.0, 2.0))
    assert cond.dtype == np.float32 and np.array_equal(cond, golden["cond"])
    assert {0.0, 1.0, 2.0} == set(np.unique(cond).tolist())


def test_a_later_keypoint_overwrites_and_an_absent_one_marks_nothing():
    pts = np.array([[0, 0, 0], [1, 0, 0], [5, 5, 5]], np.float64)
    targets = np.array([[[0, 0, 0.05], [np.nan] * 3], [[0.5, 0, 0], [0.04, 0, 0]], [[np.nan] * 3, [np.nan] * 3]])
    assert keypoint_cond_np(pts, targets, 0.1, (1.0, 2.0, 3.0)).tolist() == [2.0, 0.0, 0.0]
    assert keypoint_cond_np(pts, targets, 0.6, (7.0, 0.5, 3.0)).tolist() == [0.5, 0.5, 0.0]
    # strict: a point exactly at the threshold is not marked
    assert keypoint_cond_np(np.array([[0.25, 0, 0]]), np.zeros((1, 1, 3)), 0.25, (1.0,)).tolist() == [0.0]


def test_abi_symbol_is_declared_exported_and_bound():
    src = assert_abi_topic(KEYPOINT_SYMBOLS, "keypoint", ("PS_CLOUD_KEYPOINT_MAX", "PS_CLOUD_KEYPOINT_MAX_RADIUS"))
    assert "#define PS_CLOUD_KEYPOINT_MAX 4" in src and "#define PS_CLOUD_KEYPOINT_MAX_RADIUS 8" in src


def _args(**over):
    B, K = 2, 7
    a = dict(num_envs=B, points=torch.zeros(B, K, 3), keypoints=torch.zeros(B, 2, 2, dtype=torch.int32),
             colors=torch.zeros(B, K, 3, dtype=torch.uint8), count=torch.zeros(B, dtype=torch.int32), radius=3,
             threshold=0.1, values=None)
    a.update(over)
    return a


def test_keypoint_features_args_accepts_and_fills_defaults():
    from pandasim import keypoint_features_args

    assert keypoint_features_args(**_args()) == (7, 2, 3, 0.1, [1.0, 2.0])
    got = keypoint_features_args(**_args(keypoints=torch.zeros(4, 2, dtype=torch.int64), colors=None, count=None,
                                         radius=0, values=(5, 6, 7, 8)))
    assert got == (7, 4, 0, 0.1, [5.0, 6.0, 7.0, 8.0])
    assert keypoint_features_args(**_args(radius=8, threshold=1e3))[2:4] == (8, 1e3)


@pytest.mark.parametrize("name,over", [
    ("points", dict(points=torch.zeros(2, 7, 3, dtype=torch.float64))),
    ("points", dict(points=torch.zeros(2, 7, 2))),
    ("points", dict(points=torch.zeros(3, 7, 3))),
    ("points", dict(points=torch.zeros(2, 0, 3))),
    ("keypoints", dict(keypoints=torch.zeros(2, 2, 2))),  # floating point
    ("keypoints", dict(keypoints=torch.zeros(2, 2, 3, dtype=torch.int32))),
    ("keypoints", dict(keypoints=torch.zeros(3, 2, 2, dtype=torch.int32))),
    ("keypoints", dict(keypoints=torch.zeros(2, dtype=torch.int32))),
    ("n_kp", dict(keypoints=torch.zeros(2, 0, 2, dtype=torch.int32))),
    ("n_kp", dict(keypoints=torch.zeros(2, 5, 2, dtype=torch.int32))),
    ("colors", dict(colors=torch.zeros(2, 7, 3))),
    ("colors", dict(colors=torch.zeros(2, 6, 3, dtype=torch.uint8))),
    ("count", dict(count=torch.zeros(3, dtype=torch.int32))),
    ("count", dict(count=torch.zeros(2, 1, dtype=torch.int32))),
    ("count", dict(count=torch.zeros(2, dtype=torch.int64))),
    ("radius", dict(radius=-1)),
    ("radius", dict(radius=9)),
    ("radius", dict(radius=2.5)),
    ("threshold", dict(threshold=0.0)),
    ("threshold", dict(threshold=-0.1)),
    ("threshold", dict(threshold=math.inf)),
    ("threshold", dict(threshold=math.nan)),
    ("values", dict(values=(1.0,))),
    ("values", dict(values=(1.0, 2.0, 3.0))),
    ("values", dict(values=("a", "b"))),
])
def test_keypoint_features_args_rejects(name, over):
    from pandasim import keypoint_features_args

    with pytest.raises(ValueError, match=name):
        keypoint_features_args(**_args(**over))


def test_project_to_pixels_is_renders_waypoint_projection(render_golden):
    """On the render goldens' cameras and waypoints: the reference's own
    waypoints_proj, and render()'s host loop restated here, exactly."""
    from pandasim import project_to_pixels

    for k in range(int(render_golden["n_cameras"])):
        c = {n[len(f"c{k}_"):]: v for n, v in render_golden.items() if n.startswith(f"c{k}_")}
        w, h = int(c["camera"][0]), int(c["camera"][1])
        view, proj = tuple(float(x) for x in c["view"]), tuple(float(x) for x in c["proj"])
        rng = np.random.default_rng(k)
        pts = np.concatenate([c["waypoints"], rng.uniform(-0.6, 0.6, (195, 3))])
        PV = np.matmul(np.asarray(proj).reshape([4, 4], order="F"), np.asarray(view).reshape([4, 4], order="F"))
        want = []
        for point in pts:
            x, y, z, ww = np.matmul(PV, np.array([point[0], point[1], point[2], 1]))
            x, y = (x / ww + 1) / 2 * w, (y / ww + 1) / 2 * h
            want.append([int(x), int(h - y)])
        got = project_to_pixels(torch.from_numpy(pts), view, proj, w, h)
        assert got.dtype == torch.int32 and got.shape == (len(pts), 2)
        assert np.array_equal(got.numpy(), np.array(want)), k
        assert np.array_equal(got.numpy()[:len(c["waypoints"])], c["waypoints_proj"]), k
        # batched, and f32 points are widened
        both = project_to_pixels(torch.from_numpy(pts.astype(np.float32)).reshape(2, -1, 3), view, proj, w, h)
        assert both.shape == (2, len(pts) // 2, 2)
