"""CPU tests of the PointNet++ front end (ps_cloud_normalize / _fps /
_ball_query / _group / _set_abstraction, PandaSim.group_cloud): the numpy
restatement (tests/cloud_reference.py) that tests/test_gpu_group.py holds the
kernels to, itself held to the golden recorded from the reference (tests/golden/make_group_golden.py), the
new ABI symbols, and the Python layer's argument checks.

The restatement computes the squared distance directly, d = x - c and
(d.x*d.x + d.y*d.y) + d.z*d.z in f32 with every product and sum rounded; the
reference's query_ball_point expands it (-2ab + a^2 + b^2), so a row holding a
point within 4e-6 of r^2 (`ambiguous` in the golden) may differ and is skipped
-- those rows and no others.
"""
import os

import numpy as np
import pytest

from cloud_helpers import assert_abi_topic
from cloud_reference import ball_query_np, fps_np, group_rows_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("A", "B", "C", "D1", "D2", "E")
QUERY_CASES = ("A", "B", "E")
MAX_SKIPPED = 0.05
GROUP_SYMBOLS = ("ps_cloud_normalize", "ps_cloud_fps", "ps_cloud_ball_query", "ps_cloud_group",
                 "ps_cloud_set_abstraction")


def row_hash(grouped):
    """make_group_golden.py's hash of every (cloud, centre) row of [B, S, K, C] f32."""
    b, s = grouped.shape[:2]
    bits = np.ascontiguousarray(grouped, np.float32).view(np.uint32).reshape(b, s, -1).astype(np.uint64)
    w = (2 * np.arange(bits.shape[2], dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    return (bits * w).sum(-1, dtype=np.uint64)


def grouped_centres(s):
    return np.unique(np.linspace(0, s - 1, 4).astype(np.int64))


# -------------------------------------------------------------- the golden
_golden = {}


def group_golden():
    if not _golden:
        _golden.update(np.load(os.path.join(ROOT, "tests", "golden", "group_golden.npz")))
    return _golden


def case_of(name):
    """A case's inputs and recorded results: xyz, start, feats (f32), fps_idx,
    scales [(radius, nsample)], and per scale group_idx (i32), ambiguous,
    grouped_hash, grouped_rows."""
    g = group_golden()
    c = {k: g[f"{name}_{k}"] for k in ("xyz", "start", "fps_idx")}
    c["feats"] = g[f"{name}_feats"].astype(np.float32)
    c["scales"] = [(float(r), int(k)) for r, k in g[f"{name}_scales"]]
    for k in range(len(c["scales"])):
        c[f"group_idx_{k}"] = g[f"{name}_group_idx_{k}"].astype(np.int32)
        for f in ("ambiguous", "grouped_hash", "grouped_rows"):
            c[f"{f}_{k}"] = g[f"{name}_{f}_{k}"]
    return c


_restated = {}


def restated(name):
    """The restatement on a case's inputs, computed once: fps_idx [B, S] and per
    scale group_idx and grouped (around the restatement's own fps_idx)."""
    if name not in _restated:
        c = case_of(name)
        nb, s = c["fps_idx"].shape
        r = {"fps_idx": np.stack([fps_np(c["xyz"][b], c["start"][b], s) for b in range(nb)])}
        for k, (radius, nsample) in enumerate(c["scales"]):
            r[f"group_idx_{k}"] = np.stack([ball_query_np(c["xyz"][b], r["fps_idx"][b], radius, nsample)
                                            for b in range(nb)])
            r[f"grouped_{k}"] = group_rows_np(c["xyz"], c["feats"], r["fps_idx"], r[f"group_idx_{k}"])
        _restated[name] = r
    return _restated[name]


def assert_matches_golden(name, k, group_idx, grouped, what):
    """group_idx [B, S, nsample] and grouped [B, S, nsample, D + 3] against the
    golden of case `name`, scale k, on every row that is not ambiguous."""
    c = case_of(name)
    keep = ~c[f"ambiguous_{k}"]
    assert np.array_equal(group_idx[keep], c[f"group_idx_{k}"][keep]), (what, name, k, "group_idx")
    assert np.array_equal(row_hash(grouped)[keep], c[f"grouped_hash_{k}"][keep]), (what, name, k, "grouped hash")
    rows = grouped_centres(group_idx.shape[1])
    got, want = grouped[:, rows].view(np.uint32), c[f"grouped_rows_{k}"].view(np.uint32)
    assert np.array_equal(got[keep[:, rows]], want[keep[:, rows]]), (what, name, k, "grouped rows")


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_golden_fps(name):
    c = case_of(name)
    assert c["xyz"].shape[0] == 3 and c["xyz"].dtype == np.float32
    assert np.array_equal(restated(name)["fps_idx"], c["fps_idx"])
    assert np.array_equal(c["fps_idx"][:, 0], c["start"])


def test_exhausted_cloud_returns_index_zero():
    """Case C: once every distinct point is taken all distances are 0 and the
    arg-max is index 0, as in the reference."""
    c = case_of("C")
    for b in range(3):
        distinct = len(np.unique(c["xyz"][b], axis=0))
        assert distinct <= 20 < c["fps_idx"].shape[1]
        assert not c["fps_idx"][b, distinct:].any()


@pytest.mark.parametrize("name", QUERY_CASES)
def test_restatement_equals_the_golden_ball_query_and_group(name):
    c, r = case_of(name), restated(name)
    for k in range(len(c["scales"])):
        assert_matches_golden(name, k, r[f"group_idx_{k}"], r[f"grouped_{k}"], "restatement")


@pytest.mark.parametrize("name", QUERY_CASES)
def test_skipped_share_is_at_most_five_percent(name):
    c = case_of(name)
    assert len(c["scales"]) == (2 if name == "A" else 3)
    for k in range(len(c["scales"])):
        share = float(c[f"ambiguous_{k}"].mean())
        print(name, c["scales"][k], f"{100 * share:.2f} % of the rows skipped")
        assert share <= MAX_SKIPPED, (name, k, share)


def test_golden_has_duplicates_where_the_cases_say():
    for name, distinct in (("A", 100), ("B", 300), ("C", 20)):
        xyz = case_of(name)["xyz"]
        assert all(len(np.unique(xyz[b], axis=0)) <= distinct < xyz.shape[1] for b in range(3))
    assert case_of("D1")["xyz"].shape == (3, 1, 3) and case_of("D2")["fps_idx"].shape == (3, 2)
    assert case_of("E")["xyz"].shape == (3, 5000, 3) and case_of("E")["fps_idx"].shape == (3, 512)


# ----------------------------------------------------------------- the ABI
def test_header_and_signatures_carry_the_new_symbols():
    import ctypes as C

    from pandasim import _lib as L

    src = assert_abi_topic(GROUP_SYMBOLS, "group",
                           ("PS_CLOUD_MAX_POINTS", "PS_CLOUD_MAX_SCALES", "PS_CLOUD_MAX_FEATURES"))
    lib = L.lib()
    assert L.CLOUD_MAX_POINTS >= 8192 and L.CLOUD_MAX_FEATURES == 16
    assert "ps_cloud_scale" in src and C.sizeof(L.CloudScale) == 32
    assert L.lib().ps_cloud_ball_query.argtypes[5] is C.c_double  # the radius, squared in f64 as the reference's
    # a NULL context is refused before anything else is looked at
    assert L.ERRORS[lib.ps_cloud_fps(None, None, 5, None, 1, None, None)] == "PS_ERR_ARG"


def test_python_surface_exists():
    import pandasim
    from pandasim import cloudnet

    assert hasattr(pandasim.PandaSim, "group_cloud") and hasattr(pandasim.PandaVecEnv, "group_cloud")
    assert set(cloudnet.GroupedCloud.__slots__) == {"xyz", "centroid", "scale", "fps_idx", "new_xyz", "group_idx",
                                               "grouped"}


def test_start_is_the_clouds_counter_draw():
    from pandasim.cloudnet import fps_start
    from test_cloud_cpu import rank

    for seed in (0, 12345, (1 << 64) - 1):
        for env in (0, 1, 255):
            for n in (1, 257, 5000, 8192):
                assert fps_start(seed, env, n) == rank(seed, env, n)
                assert 0 <= fps_start(seed, env, n) < n
    assert fps_start(0, 0, 1000) == 883  # test_cloud_cpu's known answer


def test_argument_checks():
    import torch

    from pandasim.cloudnet import group_cloud_args

    pts = torch.zeros(3, 100, 3)
    ok = dict(num_envs=3, points=pts, feats=None, npoint=10, radii=(0.1, 0.2), nsamples=(4, 8), seed=0, start=None)

    def call(**kw):
        return group_cloud_args(**{**ok, **kw})

    n, s, d, radii, nsamples, first = call()
    assert (n, s, d, radii, nsamples) == (100, 10, 0, [0.1, 0.2], [4, 8])
    assert first.dtype == torch.int32 and first.shape == (3,) and call(seed=0)[5].tolist() == first.tolist()
    assert call(feats=torch.zeros(3, 100, 16))[2] == 16
    assert call(start=[0, 99, 5])[5].tolist() == [0, 99, 5]
    for bad in (dict(npoint=101), dict(npoint=0),  # S outside 1..N
                dict(radii=(0.1,), nsamples=(4, 8)), dict(radii=(), nsamples=()),
                dict(radii=(0.1,) * 5, nsamples=(4,) * 5),
                dict(radii=(0.0, 0.2)), dict(radii=(float("inf"), 0.2)), dict(radii=(float("nan"), 0.2)),
                dict(nsamples=(0, 8)),
                dict(feats=torch.zeros(3, 99, 4)), dict(feats=torch.zeros(2, 100, 4)), dict(feats=torch.zeros(3, 100)),
                dict(feats=torch.zeros(3, 100, 4, dtype=torch.float64)),
                dict(feats=torch.zeros(3, 100, 3, dtype=torch.uint8)), dict(feats=torch.zeros(3, 100, 17)),
                dict(start=[0, 100, 5]), dict(start=[0, -1, 5]), dict(start=[0, 1]), dict(start=[0.0, 1.0, 2.0]),
                dict(points=torch.zeros(3, 100, 2)), dict(points=torch.zeros(4, 100, 3)),
                dict(points=torch.zeros(3, 100, 3, dtype=torch.float64)), dict(points=torch.zeros(3, 8193, 3)),
                dict(points=torch.zeros(3, 0, 3), npoint=1)):
        with pytest.raises(ValueError):
            call(**bad)
