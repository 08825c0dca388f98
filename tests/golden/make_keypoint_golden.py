"""Generate the golden vectors of the keypoint conditioning with the
scikit-learn calls the reference makes (envs/task_classes/run_policy.py:202-285,
the same in generate_dset.py:105-195), on a small synthetic case:

    pix2pix_neighborhood    NearestNeighbors(radius=3).fit(pixels)
                            .radius_neighbors(keypoint) over the [i, j] list of
                            every pixel of the image (i the column, j the row)
    point2point_neighborhood
                            NearestNeighbors(n_neighbors=1).fit(target)
                            .kneighbors(source), marked where dists < 0.1
    take_rgbd               keypoint_cond = 0; the start keypoint's marks = 1.0,
                            then the end keypoint's = 2.0

Run where scikit-learn is installed:
    python tests/golden/make_keypoint_golden.py

The case: a 64 x 48 image, 400 points, two keypoints, the second at the image
corner (0, 0) so that its disc is clipped.  The world point of a pixel stands in
for sim.deproject: a smooth synthetic surface (surface() below), since the
neighbourhood calls do not care where the targets come from.  The script
refuses a case in which a point's distance lies within 1e-9 of the threshold,
or in which either keypoint marks fewer than 8 points or all but 8.

Output: tests/golden/keypoint_golden.npz (data only).
"""
import os

import numpy as np
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "keypoint_golden.npz")
WIDTH, HEIGHT, N_POINTS, SEED = 64, 48, 400, 20
KEYPOINTS = np.array([[40, 21], [0, 0]])  # (column, row): interior, corner


def pix2pix_neighborhood(width, height, keypoint, radius=3):
    """The pixels [column, row] within `radius` of the keypoint, by a radius
    query over the list of all image pixels (column-major, as the reference
    lists them)."""
    pixels = np.stack(np.meshgrid(np.arange(width), np.arange(height), indexing="ij"), -1).reshape(-1, 2)
    found = NearestNeighbors(radius=radius).fit(pixels).radius_neighbors(np.reshape(keypoint, (-1, 2)),
                                                                         return_distance=False)
    return pixels[found[0]]


def point2point_neighborhood(source_points, target_points, thresh=0.1):
    """The source points whose nearest target lies closer than `thresh`, and
    every source point's distance to its nearest target."""
    dists, _ = NearestNeighbors(n_neighbors=1).fit(target_points).kneighbors(source_points, return_distance=True)
    return np.where(dists < thresh)[0], dists[:, 0]


def surface(pixels):
    """A world point per pixel (column, row): a tilted, gently curved sheet
    about 0.6 m wide."""
    c, r = pixels[:, 0].astype(np.float64), pixels[:, 1].astype(np.float64)
    x = -0.3 + 0.6 * c / WIDTH
    y = -0.25 + 0.5 * r / HEIGHT
    z = 0.05 + 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y) + 0.2 * x
    return np.stack([x, y, z], -1)


def main():
    rng = np.random.default_rng(SEED)
    # points scattered about the sheet: near enough that both keypoints mark some
    at = np.stack([rng.integers(0, WIDTH, N_POINTS), rng.integers(0, HEIGHT, N_POINTS)], -1)
    points = surface(at) + rng.normal(size=(N_POINTS, 3)) * 0.05
    out = dict(width=WIDTH, height=HEIGHT, keypoints=KEYPOINTS, points=points, threshold=0.1, radius=3)
    cond = np.zeros(N_POINTS)
    for k, (kp, value) in enumerate(zip(KEYPOINTS, (1.0, 2.0))):
        pixels = pix2pix_neighborhood(WIDTH, HEIGHT, kp)
        targets = surface(pixels)
        idxs, dists = point2point_neighborhood(points, targets)
        assert np.abs(dists - 0.1).min() > 1e-9, "a point sits on the threshold: change SEED"
        assert 8 <= len(idxs) <= N_POINTS - 8, (k, len(idxs))
        cond[idxs] = value
        out[f"patch{k}"], out[f"targets{k}"], out[f"dists{k}"], out[f"marked{k}"] = pixels, targets, dists, idxs
        print(f"keypoint {k} at {kp.tolist()}: {len(pixels)} pixels, {len(idxs)} points marked, "
              f"closest to the threshold {np.abs(dists - 0.1).min():.3e}")
    out["cond"] = cond
    assert len(out["patch0"]) == 29 and len(out["patch1"]) < 29
    np.savez(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; cond counts {np.unique(cond, return_counts=True)}")


if __name__ == "__main__":
    main()
