"""CPU tests of the PointNet++ feature propagation (ps_cloud_three_nn /
_interpolate / _feature_propagation, PandaSim.propagate_features): the numpy
restatement (tests/cloud_reference.py) that tests/test_gpu_propagate.py holds
the kernels to bit for bit, itself held to the golden recorded from the
reference's PointNetFeaturePropagation in float64
(tests/golden/make_propagate_golden.py), the new ABI symbols, and the Python layer's argument checks.

The bound of the restatement against the f64 golden, per cloud:
    |restatement - golden| <= K * eps_f32 * max|points2|,  K = 12.
Derivation, u = eps_f32 / 2 the unit roundoff, first order, every quantity
positive until the last sum so relative errors add and do not amplify:
    d = a - b                       1 u   (the inputs are exact)
    d * d                           3 u   (2 from d, 1 from the product)
    (dx2 + dy2) + dz2               5 u   (two sums)
    d2 + 1e-8f                      6 u   (the constant's own rounding is within the 5 u; one sum)
    w = 1 / that                    7 u
    norm = (w0 + w1) + w2           9 u
    weight = w / norm              17 u   (7 + 9 + 1)
    p * weight                     18 u
    (t0 + t1) + t2                 20 u * sum |p_k| weight_k <= 20 u * max|points2|
20 u = 10 eps_f32.  One more eps_f32 covers the higher-order terms and the sum
of the rounded weights exceeding 1 by 17 u; one more the yardstick's own error:
the f64 reference computes d2 as -2ab + a^2 + b^2, wrong by about 4e-16 where a
dense point is a coarse point, which is 4e-8 = 0.3 eps_f32 of the 1e-8 it is
added to.  Rows marked ambiguous in the golden (3rd and 4th nearest within
4e-6 in f32) are skipped, those and no others.
"""
import os

import numpy as np
import pytest

from cloud_helpers import assert_abi_topic
from cloud_reference import propagate_np, three_nn_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("A", "B", "C", "D", "E")
SHAPES = {"A": (300, 64, 0, 8), "B": (1000, 128, 5, 8), "C": (128, 1, 3, 16), "D": (7, 3, 0, 1),
          "E": (5000, 512, 0, 4)}  # N, S, D1, D2
MAX_SKIPPED = 0.05
K_BOUND = 12
EPS = float(np.finfo(np.float32).eps)
PROPAGATE_SYMBOLS = ("ps_cloud_three_nn", "ps_cloud_interpolate", "ps_cloud_feature_propagation")


# -------------------------------------------------------------- the golden
_golden, _restated = {}, {}


def case_of(name):
    """A case's inputs as the kernels take them (f32) and the recorded results:
    xyz1, xyz2, points2, points1 (None with D1 = 0), out (f64), ambiguous, nn."""
    if not _golden:
        _golden.update(np.load(os.path.join(ROOT, "tests", "golden", "propagate_golden.npz")))
    g = _golden
    xyz1, cidx = g[f"{name}_xyz1"], g[f"{name}_coarse_idx"].astype(np.int64)
    c = {"xyz1": xyz1, "xyz2": np.stack([xyz1[b][cidx[b]] for b in range(xyz1.shape[0])]),
         "points2": g[f"{name}_points2"].astype(np.float32), "points1": g[f"{name}_points1"].astype(np.float32),
         "out": g[f"{name}_out"], "ambiguous": g[f"{name}_ambiguous"], "nn": g[f"{name}_nn"].astype(np.int32)}
    if c["points1"].shape[2] == 0:
        c["points1"] = None
    return c


def restated(name):
    """The restatement on a case's inputs, computed once: out, idx, weight."""
    if name not in _restated:
        c = case_of(name)
        _restated[name] = propagate_np(c["xyz1"], c["xyz2"], c["points2"], c["points1"])
    return _restated[name]


@pytest.mark.parametrize("name", CASES)
def test_golden_has_the_shapes_the_cases_say(name):
    c = case_of(name)
    n, s, d1, d2 = SHAPES[name]
    assert c["xyz1"].shape == (2, n, 3) and c["xyz1"].dtype == np.float32
    assert c["xyz2"].shape == (2, s, 3) and c["points2"].shape == (2, s, d2)
    assert (c["points1"] is None) == (d1 == 0) and (d1 == 0 or c["points1"].shape == (2, n, d1))
    assert c["out"].shape == (2, n, d1 + d2) and c["out"].dtype == np.float64
    # every coarse point is one of the dense points: distances that are truly 0
    assert all(len(np.unique(c["xyz2"][b], axis=0)) == s for b in range(2))


@pytest.mark.parametrize("name", CASES)
def test_restatement_within_the_bound_of_the_f64_golden(name):
    c = case_of(name)
    out, idx, weight = restated(name)
    keep = ~c["ambiguous"]
    worst = 0.0
    for b in range(2):
        scale = EPS * float(np.abs(c["points2"][b]).max())
        err = np.abs(out[b].astype(np.float64) - c["out"][b])[keep[b]]
        worst = max(worst, float(err.max()) / scale)
        print(f"case {name} cloud {b}: worst error {err.max():.3e} = {err.max() / scale:.2f} eps_f32 max|points2|")
        assert float(err.max()) <= K_BOUND * scale, (name, b, float(err.max()) / scale)
    print(f"case {name}: worst error / (eps_f32 * max|points2|) = {worst:.2f}, bound {K_BOUND}")
    if c["points1"] is not None:  # the dense features pass through untouched
        d1 = c["points1"].shape[2]
        assert np.array_equal(out[..., :d1], c["points1"]) and np.array_equal(c["out"][..., :d1], c["points1"])
    if SHAPES[name][1] > 1:
        got, want = np.sort(idx, -1), np.sort(c["nn"], -1)
        assert np.array_equal(got[keep], want[keep]), name
        assert np.abs(weight.sum(-1) - 1).max() <= 4 * EPS
    else:
        assert np.array_equal(out[..., SHAPES[name][2]:], np.repeat(c["points2"], SHAPES[name][0], axis=1))


@pytest.mark.parametrize("name", CASES)
def test_skipped_share_is_at_most_five_percent(name):
    share = float(case_of(name)["ambiguous"].mean())
    print(name, f"{100 * share:.2f} % of the rows skipped")
    assert share <= MAX_SKIPPED, (name, share)


def test_ties_go_to_the_lowest_index_and_zero_distance_is_finite():
    xyz2 = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [2, 0, 0]], np.float32)
    xyz1 = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0, 0]], np.float32)
    idx, w = three_nn_np(xyz1, xyz2)
    assert idx.tolist() == [[0, 3, 1], [1, 2, 0], [0, 1, 2]]
    assert np.isfinite(w).all() and w[0, 0] == w[0, 1] == np.float32(0.5) and w[0, 2] < 1e-7


# ----------------------------------------------------------------- the ABI
def test_header_and_signatures_carry_the_new_symbols():
    from pandasim import _lib as L

    assert_abi_topic(PROPAGATE_SYMBOLS, "propagate", ("PS_CLOUD_MAX_POINTS", "PS_CLOUD_MAX_FEATURES",
                                                      "PS_CLOUD_MAX_PROP_FEATURES", "PS_CLOUD_MAX_DENSE_POINTS"))
    lib = L.lib()
    assert L.CLOUD_MAX_PROP_FEATURES == 2048 and L.CLOUD_MAX_DENSE_POINTS == 1 << 20 and L.CLOUD_MAX_FEATURES == 16
    # a NULL context is refused before anything else is looked at
    assert L.ERRORS[lib.ps_cloud_three_nn(None, None, 5, None, 3, None, None, None)] == "PS_ERR_ARG"
    assert L.ERRORS[lib.ps_cloud_feature_propagation(None, None, 5, None, 3, None, 0, None, 1, None, None, None,
                                                     None)] == "PS_ERR_ARG"


def test_python_surface_exists():
    import pandasim

    assert hasattr(pandasim.PandaSim, "propagate_features") and hasattr(pandasim.PandaVecEnv, "propagate_features")


def test_argument_checks():
    import torch

    from pandasim.cloudnet import propagate_features_args

    ok = dict(num_envs=3, xyz1=torch.zeros(3, 100, 3), xyz2=torch.zeros(3, 10, 3), points2=torch.zeros(3, 10, 8),
              points1=None)

    def call(**kw):
        return propagate_features_args(**{**ok, **kw})

    assert call() == (100, 10, 0, 8)
    assert call(points1=torch.zeros(3, 100, 5)) == (100, 10, 5, 8)
    assert call(xyz2=torch.zeros(3, 1, 3), points2=torch.zeros(3, 1, 8)) == (100, 1, 0, 8)
    assert call(xyz2=torch.zeros(3, 3, 3), points2=torch.zeros(3, 3, 2048)) == (100, 3, 0, 2048)
    assert call(xyz1=torch.zeros(3, 1, 3), points1=torch.zeros(3, 1, 2048)) == (1, 10, 2048, 8)
    assert call(xyz2=torch.zeros(3, 200, 3), points2=torch.zeros(3, 200, 1)) == (100, 200, 0, 1)  # S above N
    for bad in (dict(xyz2=torch.zeros(3, 2, 3), points2=torch.zeros(3, 2, 8)),  # S = 2
                dict(xyz2=torch.zeros(3, 0, 3), points2=torch.zeros(3, 0, 8)),
                dict(xyz2=torch.zeros(3, 8193, 3), points2=torch.zeros(3, 8193, 1)),
                dict(xyz1=torch.zeros(3, 0, 3)), dict(xyz1=torch.zeros(3, 100, 2)), dict(xyz1=torch.zeros(4, 100, 3)),
                dict(xyz1=torch.zeros(3, 100, 3, dtype=torch.float64)), dict(xyz1=torch.zeros(100, 3)),
                dict(xyz2=torch.zeros(2, 10, 3)), dict(xyz2=torch.zeros(3, 10, 4)),
                dict(xyz2=torch.zeros(3, 10, 3, dtype=torch.float16)),
                dict(points2=torch.zeros(3, 9, 8)), dict(points2=torch.zeros(3, 10)),
                dict(points2=torch.zeros(3, 10, 0)), dict(points2=torch.zeros(3, 10, 2049)),
                dict(points2=torch.zeros(3, 10, 8, dtype=torch.float64)),
                dict(points2=torch.zeros(3, 10, 8, dtype=torch.int32)),
                dict(points1=torch.zeros(3, 99, 5)), dict(points1=torch.zeros(2, 100, 5)),
                dict(points1=torch.zeros(3, 100)), dict(points1=torch.zeros(3, 100, 0)),
                dict(points1=torch.zeros(3, 100, 2049)), dict(points1=torch.zeros(3, 100, 5, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):  # N above 2^20, without allocating it
        call(xyz1=torch.zeros(1, 1, 3).expand(3, (1 << 20) + 1, 3))
