"""CPU tests of the shared MLP with max-pool (ps_cloud_mlp, ps_cloud_group_mlp,
PandaSim.shared_mlp / abstract_features, pandasim.fold_batchnorm): the numpy
restatement (tests/cloud_reference.py) that tests/test_gpu_mlp.py holds the
kernels to on every element, itself held to the golden recorded from the
reference's own modules in float64 (tests/golden/make_mlp_golden.py), the exact
fmaf it is built on, the batch-norm fold, the new ABI symbols, and every refusal of the argument functions.

The restatement is include/pandasim.h's chain: y = b; for k ascending
y = fmaf(x[k], W[o][k], y); ReLU; the maximum over each group.  fma32 is an
exact fmaf: the f64 product of two f32 is exact (48 bits), it is added to the
accumulator with an error-free sum (TwoSum), the f64 sum is rounded to odd, and
the cast to f32 then rounds once (f64 has more than two bits beyond f32's 24).

The bound of the restatement against the f64 golden is derived, not chosen: an
error e is carried through the layers beside the values.  With u = 2^-24 the
unit roundoff of f32, W' and b' the folded f32 parameters, x the restated
input of a layer and e_in the bound on its distance from the reference's:
    the chain's roundings   (C_in + 1) u (|W'| |x| + |b'|)   C_in fmaf steps,
                                                             first order
    the incoming error      |W'| e_in
    the fold's roundings    u (|W'| (|x| + e_in) + |b'|)     W' and b' are each
                                                             one rounding of the
                                                             exact fold
and e_out is their sum times 1.01, which covers the second-order terms
(C_in u < 2e-4 here) and the reference's own f64 roundings (1e-16 relative).
ReLU and max are 1-Lipschitz: e passes through ReLU unchanged and a pooled
value takes the largest e of its group.  The centred coordinates of a grouped
row enter with e = u |x|: ps_cloud_group subtracts in f32, one rounding, where
the reference run in f64 subtracts exactly.
"""
import ctypes
import ctypes.util
import os
from types import SimpleNamespace

import numpy as np
import pytest

from cloud_helpers import assert_abi_topic
from cloud_reference import fma32, group_rows_np, mlp_np, mlp_with_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLP_SYMBOLS = ("ps_cloud_mlp", "ps_cloud_group_mlp")
CASES = ("msg", "all", "fp")


# ------------------------------------------------------------- the golden
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "mlp_golden.npz")))
    return _golden


def raw_layers(prefix):
    g, out, k = golden(), [], 0
    while f"{prefix}_l{k}_conv_w" in g:
        out.append({n: g[f"{prefix}_l{k}_{n}"] for n in ("conv_w", "conv_b", "gamma", "beta", "mean", "var", "eps")})
        k += 1
    return out


def folded(prefix):
    from pandasim import fold_batchnorm

    return [(*fold_batchnorm(p["conv_w"], p["conv_b"], p["gamma"], p["beta"], p["mean"], p["var"], float(p["eps"])),
             True) for p in raw_layers(prefix)]


def case_of(name):
    """-> a list of parts (rows [B, R, C0] f32, layer prefix, pool, column
    offset, the rows as the f64 reference has them) and the f64 golden
    [B, R / pool, width]."""
    g = golden()
    if name == "msg":
        parts, off = [], 0
        for i in range(2):
            rows = group_rows_np(g["msg_xyz"], g["msg_feats"], g["msg_centre_idx"], g[f"msg_group_idx{i}"])
            k = rows.shape[2]
            exact = group_rows_np(g["msg_xyz"].astype(np.float64), g["msg_feats"], g["msg_centre_idx"],
                                  g[f"msg_group_idx{i}"], np.float64)
            parts.append((rows.reshape(2, -1, rows.shape[-1]), f"msg_s{i}", k, off,
                          exact.reshape(2, -1, rows.shape[-1])))
            off += raw_layers(f"msg_s{i}")[-1]["conv_w"].shape[0]
        return parts, g["msg_out"]
    if name == "all":
        rows = np.concatenate([g["all_xyz"], g["all_feats"]], -1)  # sample_and_group_all: xyz first
        return [(rows, "all", rows.shape[1], 0, rows.astype(np.float64))], g["all_out"]
    rows = np.concatenate([g["fp_points1"], np.repeat(g["fp_points2"], g["fp_points1"].shape[1], axis=1)], -1)
    return [(rows, "fp", 1, 0, rows.astype(np.float64))], g["fp_out"]


_restated = {}


def restated(name):
    """The restatement of a golden case and its bound, computed once."""
    if name not in _restated:
        parts, want = case_of(name)
        got, bound = np.zeros(want.shape, np.float32), np.zeros(want.shape)
        for rows, prefix, pool, off, _ in parts:
            y, e = mlp_with_bound(rows, folded(prefix), pool, centred=3 if name == "msg" else 0)
            got[..., off:off + y.shape[-1]], bound[..., off:off + y.shape[-1]] = y, e
        got.setflags(write=False)
        bound.setflags(write=False)
        _restated[name] = (got, bound)
    return _restated[name]


# --------------------------------------------------------------- the tests
def test_fma32_is_the_c_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    libm.fmaf.restype = ctypes.c_float
    rng = np.random.default_rng(5)
    f = np.float32
    n = 4000
    a = rng.normal(size=n).astype(f) * f(2.0) ** rng.integers(-20, 20, n).astype(f)
    b = rng.normal(size=n).astype(f) * f(2.0) ** rng.integers(-20, 20, n).astype(f)
    c = rng.normal(size=n).astype(f) * f(2.0) ** rng.integers(-40, 40, n).astype(f)
    c[:1000] = (-(a[:1000].astype(np.float64) * b[:1000])).astype(f)  # cancellation: the product's own rounding
    # adversarial: products exactly half way between two f32, nudged by a c far below the last bit
    x = (f(1) + f(2.0 ** -12)) * np.ones(600, f)                     # x * x = 1 + 2^-11 + 2^-24: a tie
    tiny = np.concatenate([f(2.0) ** -rng.integers(30, 100, 200).astype(f),
                           -(f(2.0) ** -rng.integers(30, 100, 200).astype(f)), np.zeros(200, f)])
    a, b, c = np.concatenate([a, x, x]), np.concatenate([b, x, -x]), np.concatenate([c, tiny, tiny])
    # sums that are ties in f64 first: c large against the product (double rounding would miss these)
    big = (f(1) + f(2.0 ** -23) * rng.integers(0, 1 << 20, 500).astype(f))
    a, b, c = (np.concatenate([a, (f(1) + f(2.0 ** -12)) * np.ones(500, f)]),
               np.concatenate([b, f(2.0 ** -25) * (f(1) + f(2.0 ** -12)) * np.ones(500, f)]), np.concatenate([c, big]))
    got = fma32(a, b, c)
    want = np.array([libm.fmaf(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], f)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and it is not the twice-rounded a * b + c everywhere (the cases above bite)
    twice = (a.astype(np.float64) * b + c).astype(f)
    assert (twice != want).any()


def test_chain_is_k_ordered_and_starts_at_the_bias():
    f = np.float32
    x = np.array([[f(2.0 ** 24), f(1), f(-2.0 ** 24), f(1)]])
    w = np.array([[1, 1, 1, 1]], f)
    # ((((b + 2^24) + 1) - 2^24) + 1: the first 1 is absorbed, the second is not
    assert mlp_np(x, [(w, np.zeros(1, f), False)])[0, 0] == 1.0
    assert mlp_np(x[:, [0, 2, 1, 3]], [(w, np.zeros(1, f), False)])[0, 0] == 2.0
    # relu and a pool over a group of all-negative rows without relu
    rows = np.array([[-1.0], [-3.0], [2.0], [-5.0]], f)
    assert mlp_np(rows, [(np.ones((1, 1), f), np.zeros(1, f), False)], pool=2).ravel().tolist() == [-1.0, 2.0]
    assert mlp_np(rows, [(np.ones((1, 1), f), np.zeros(1, f), True)], pool=1).ravel().tolist() == [0, 0, 2.0, 0]


@pytest.mark.parametrize("name", CASES)
def test_golden_has_the_shapes_the_cases_say(name):
    parts, want = case_of(name)
    shapes = {"msg": (2, 16, 192), "all": (2, 1, 256), "fp": (2, 70, 32)}
    assert want.shape == shapes[name] and want.dtype == np.float64
    widths = {"msg_s0": (9, 32, 32, 64), "msg_s1": (9, 64, 96, 128), "all": (32, 64, 128, 256), "fp": (45, 64, 32)}
    for rows, prefix, pool, off, _ in parts:
        raw = raw_layers(prefix)
        assert (rows.shape[-1], *[p["conv_w"].shape[0] for p in raw]) == widths[prefix]
        assert rows.dtype == np.float32 and rows.shape[1] % pool == 0
        for p in raw:  # statistics that are not trivial
            assert p["var"].min() >= 0.5 and np.abs(p["mean"]).max() > 0.1 and np.abs(p["beta"]).max() > 0.1


@pytest.mark.parametrize("name", CASES)
def test_fold_batchnorm_is_the_reference_conv_then_bn(name):
    """The reference's layer in f64 numpy, from the raw parameters, meets the
    golden to f64 rounding; the fold is that layer's (W', b') rounded once."""
    from pandasim import fold_batchnorm

    parts, want = case_of(name)
    for rows, prefix, pool, off, exact in parts:
        x = exact.reshape(-1, exact.shape[-1])
        for p in raw_layers(prefix):
            w, b, s = p["conv_w"].astype(np.float64), p["conv_b"].astype(np.float64), None
            y = x @ w.T + b
            y = (y - p["mean"]) / np.sqrt(p["var"].astype(np.float64) + float(p["eps"])) * p["gamma"] + p["beta"]
            x = np.maximum(y, 0.0)
            s = p["gamma"].astype(np.float64) / np.sqrt(p["var"].astype(np.float64) + float(p["eps"]))
            wf, bf = fold_batchnorm(p["conv_w"], p["conv_b"], p["gamma"], p["beta"], p["mean"], p["var"],
                                    float(p["eps"]))
            assert wf.dtype == bf.dtype == np.float32 and wf.shape == w.shape and bf.shape == b.shape
            assert np.array_equal(wf, (w * s[:, None]).astype(np.float32))
            assert np.array_equal(bf, ((b - p["mean"]) * s + p["beta"]).astype(np.float32))
            # a conv weight with its trailing 1s, and tensors, fold the same
            import torch

            w4, _ = fold_batchnorm(torch.from_numpy(p["conv_w"])[:, :, None, None], None, p["gamma"], p["beta"],
                                   p["mean"], p["var"], float(p["eps"]))
            assert np.array_equal(w4, wf)
        pooled = x.reshape(2, -1, pool, x.shape[-1]).max(axis=2)
        got = want[..., off:off + pooled.shape[-1]]
        assert np.abs(pooled - got).max() <= 1e-12 * max(1.0, np.abs(got).max()), prefix


@pytest.mark.parametrize("name", CASES)
def test_restatement_within_the_derived_bound_of_the_f64_golden(name):
    _, want = case_of(name)
    got, bound = restated(name)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / bound).max())
    print(f"{name}: worst |restatement - golden| = {err.max():.3e}, worst error / bound = {ratio:.3f}, "
          f"bound at most {bound.max():.3e} ({bound.max() / max(np.abs(want).max(), 1e-30):.2e} of max|golden|)")
    assert (bound > 0).all() and np.isfinite(bound).all()
    assert (err <= bound).all(), (name, ratio)
    # the bound is a rounding-level one, not a loose one
    assert bound.max() <= 1e-3 * max(1.0, np.abs(want).max())


def test_header_and_signatures_carry_the_new_symbols():
    import ctypes as C

    from pandasim import _lib as L

    assert_abi_topic(MLP_SYMBOLS, "mlp",
                     ("PS_CLOUD_MLP_MAX_LAYERS", "PS_CLOUD_MLP_MAX_HIDDEN", "PS_CLOUD_MLP_MAX_LAST"))
    assert (L.CLOUD_MLP_MAX_LAYERS, L.CLOUD_MLP_MAX_HIDDEN, L.CLOUD_MLP_MAX_LAST) == (4, 512, 1024)
    # ps_cloud_mlp_layer: two pointers and two i32
    assert C.sizeof(L.CloudMlpLayer) == 24 and L.CloudMlpLayer.c_out.offset == 16 and L.CloudMlpLayer.relu.offset == 20
    # the limits cover every layer of model.py, model_cls_off.py and model_cls_off_rot.py
    nets = {"sa1": (9, [[32, 32, 64], [64, 64, 128], [64, 96, 128]]), "sa2": (323, [[128, 128, 256], [128, 196, 256]]),
            "sa3": (515, [[256, 512, 1024]]), "fp3": (1536, [[256, 256]]), "fp2": (576, [[256, 128]]),
            "fp1": (150, [[128, 128]]), "head": (128, [[128], [128]])}
    for c0, mlps in nets.values():
        assert c0 <= L.CLOUD_MAX_PROP_FEATURES + 3
        for widths in mlps:
            assert len(widths) <= 4 and max(widths[:-1], default=1) <= 512 and widths[-1] <= 1024


def test_python_surface_exists():
    import pandasim

    for name in ("shared_mlp", "abstract_features"):
        assert hasattr(pandasim.PandaSim, name) and hasattr(pandasim.PandaVecEnv, name)
    assert callable(pandasim.fold_batchnorm) and isinstance(pandasim.CloudMlp, type)


def fake_mlp(c_in, widths):
    return SimpleNamespace(c_in=c_in, widths=list(widths), array=None)


def test_fold_batchnorm_refusals():
    from pandasim import fold_batchnorm

    w, v = np.ones((4, 3), np.float32), np.ones(4, np.float32)
    fold_batchnorm(w, v, v, v, v, v)
    for bad in (dict(conv_w=np.ones(4, np.float32)), dict(conv_w=np.ones((4, 3, 2), np.float32)),
                dict(conv_b=np.ones(3)), dict(gamma=np.ones(5)), dict(beta=np.ones((4, 1))), dict(mean=np.ones(3)),
                dict(var=np.ones(2)), dict(var=-v), dict(eps=-1.0), dict(var=0 * v, eps=0.0)):
        args = dict(conv_w=w, conv_b=v, gamma=v, beta=v, mean=v, var=v, eps=1e-5)
        args.update(bad)
        with pytest.raises(ValueError):
            fold_batchnorm(**args)


def test_cloud_mlp_layer_refusals():
    from pandasim.cloudnet import cloud_mlp_layers

    f = np.float32
    lay = lambda o, i: (np.zeros((o, i), f), np.zeros(o, f), True)  # noqa: E731
    got = cloud_mlp_layers([lay(32, 9), lay(64, 32), (np.zeros((5, 64), f), np.zeros(5, f), 0)])
    assert [w.shape for w, _, _ in got] == [(32, 9), (64, 32), (5, 64)] and [r for _, _, r in got] == [True, True, False]
    cloud_mlp_layers([lay(512, 2051), lay(512, 512), lay(512, 512), lay(1024, 512)])  # the largest network
    nan = np.zeros((4, 4), f)
    nan[1, 2] = np.nan
    for bad in ([], [lay(8, 8)] * 5,                                   # the number of layers
                [(np.zeros((4, 4), f), np.zeros(4, f))],               # not a triple
                [(np.zeros((4, 4)), np.zeros(4, f), True)],            # f64 weights
                [(np.zeros((4, 4), f), np.zeros(4), True)],            # f64 bias
                [(np.zeros((4, 4, 1), f), np.zeros(4, f), True)],      # a conv weight with its trailing 1
                [(np.zeros((4, 4), f), np.zeros(5, f), True)],         # bias of another length
                [(nan, np.zeros(4, f), True)],                         # not finite
                [(np.zeros((4, 4), f), np.full(4, np.inf, f), True)],
                [lay(4, 2052)],                                        # C0 above 2051
                [(np.zeros((4, 0), f), np.zeros(4, f), True)],         # C0 = 0
                [(np.zeros((0, 4), f), np.zeros(0, f), True)],         # no outputs
                [lay(513, 4), lay(4, 513)],                            # a hidden width above 512
                [lay(1025, 4)],                                        # the last above 1024
                [lay(8, 4), lay(8, 7)]):                               # widths that do not chain
        with pytest.raises(ValueError):
            cloud_mlp_layers(bad)


def test_shared_mlp_argument_checks():
    import torch

    from pandasim.cloudnet import shared_mlp_args

    mlp = fake_mlp(9, [32, 64])
    ok = dict(num_envs=3, rows=torch.zeros(3, 12, 9), layers=mlp, pool=4, out=None, out_offset=0)
    assert shared_mlp_args(**ok) == (12, 9, 64)
    assert shared_mlp_args(**dict(ok, rows=torch.zeros(3, 3, 4, 9))) == (12, 9, 64)
    assert shared_mlp_args(**dict(ok, out=torch.zeros(3, 3, 100), out_offset=36)) == (12, 9, 64)
    for bad in (dict(rows=torch.zeros(2, 12, 9)), dict(rows=torch.zeros(3, 12)), dict(rows=torch.zeros(3, 12, 9).double()),
                dict(rows=torch.zeros(3, 12, 8)), dict(rows=torch.zeros(3, 0, 9)), dict(layers=[(1, 2, 3)]),
                dict(pool=0), dict(pool=5), dict(pool=2.5), dict(pool=True), dict(out_offset=1), dict(out_offset=-1),
                dict(out=torch.zeros(3, 3, 100), out_offset=37), dict(out=torch.zeros(3, 4, 100)),
                dict(out=torch.zeros(3, 3, 100).double()), dict(out=torch.zeros(3, 3, 200)[:, :, ::2]),
                dict(out=torch.zeros(3, 300)), dict(out=torch.zeros(3, 3, 100), out_offset=0.5)):
        with pytest.raises(ValueError):
            shared_mlp_args(**dict(ok, **bad))


def test_abstract_features_argument_checks():
    import torch

    from pandasim.cloudnet import abstract_features_args

    i32 = torch.int32
    ok = dict(num_envs=2, xyz=torch.zeros(2, 50, 3), feats=torch.zeros(2, 50, 6), centre_idx=torch.zeros(2, 8, dtype=i32),
              group_idx=[torch.zeros(2, 8, 4, dtype=i32), torch.zeros(2, 8, 16, dtype=i32)],
              mlps=[fake_mlp(9, [32, 64]), fake_mlp(9, [128])])
    assert abstract_features_args(**ok) == (50, 8, 6, [0, 64], 192)
    assert abstract_features_args(**dict(ok, feats=None, mlps=[fake_mlp(3, [5]), fake_mlp(3, [7])]))[2:] == (0, [0, 5], 12)
    assert abstract_features_args(**dict(ok, feats=torch.zeros(2, 50, 320),
                                         mlps=[fake_mlp(323, [5]), fake_mlp(323, [7])]))[2] == 320
    for bad in (dict(xyz=torch.zeros(3, 50, 3)), dict(xyz=torch.zeros(2, 50, 4)), dict(xyz=torch.zeros(2, 50, 3).double()),
                dict(xyz=torch.zeros(2, 8193, 3), feats=None), dict(feats=torch.zeros(2, 49, 6)),
                dict(feats=torch.zeros(2, 50, 6).double()), dict(feats=torch.zeros(2, 50, 2049)),
                dict(feats=torch.zeros(2, 50, 0)), dict(centre_idx=torch.zeros(2, 8)),
                dict(centre_idx=torch.zeros(3, 8, dtype=i32)), dict(centre_idx=torch.zeros(2, 51, dtype=i32)),
                dict(centre_idx=torch.zeros(2, 0, dtype=i32)), dict(mlps=None), dict(mlps=ok["mlps"][:1]), dict(mlps=[]),
                dict(group_idx=[torch.zeros(2, 8, 4), torch.zeros(2, 8, 16, dtype=i32)]),
                dict(group_idx=[torch.zeros(2, 7, 4, dtype=i32), torch.zeros(2, 8, 16, dtype=i32)]),
                dict(group_idx=[torch.zeros(2, 8, 0, dtype=i32), torch.zeros(2, 8, 16, dtype=i32)]),
                dict(group_idx=[torch.zeros(2, 8, dtype=i32), torch.zeros(2, 8, 16, dtype=i32)]),
                dict(mlps=[fake_mlp(9, [32]), fake_mlp(8, [32])]), dict(mlps=[fake_mlp(9, [32]), "x"])):
        with pytest.raises(ValueError):
            abstract_features_args(**dict(ok, **bad))
