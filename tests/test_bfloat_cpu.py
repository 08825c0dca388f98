"""CPU tests of the bfloat16 shared MLP (ps_cloud_mlp_bfloat,
ps_cloud_group_mlp_bfloat, CloudMlp / CloudSegNet precision="bfloat16",
pandasim.round_bfloat16): the rounding helper, the float64 restatement of
include/pandasim.h's specification with its bounds (tests/bfloat_reference.py)
held to the golden recorded from the reference's own modules, the new ABI
topic, every new refusal of the Python layer, and that float32 objects are
what they were.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from bfloat_reference import (UB, dyadic_net, dyadic_rows, exact_in_f32, golden_bound, mlp_bfloat_np,
                              mlp_bfloat_with_bound)
from cloud_helpers import assert_abi_topic
from test_mlp_cpu import CASES, case_of, folded

BFLOAT_SYMBOLS = ("ps_cloud_mlp_bfloat", "ps_cloud_group_mlp_bfloat")


def f32_of_bits(*bits):
    return np.array(bits, np.uint32).view(np.float32)


# ------------------------------------------------------- the rounding helper
def test_round_bfloat16_on_the_cases_that_matter():
    from pandasim import round_bfloat16

    cases = [  # f32 bits -> bf16 bits
        (0x3F800000, 0x3F80),  # 1.0
        (0x3F808000, 0x3F80),  # a tie, the kept bit even: down
        (0x3F818000, 0x3F82),  # a tie, the kept bit odd: up
        (0x3F808001, 0x3F81),  # just above a tie
        (0x3F807FFF, 0x3F80),  # just below
        (0x3FFF8000, 0x4000),  # a tie that carries into the exponent: 1.99.. -> 2.0
        (0x3FFFFFFF, 0x4000),
        (0x00000000, 0x0000), (0x80000000, 0x8000),  # +0, -0
        (0x7F7F0000, 0x7F7F),  # the largest finite bf16
        (0x7F7F7FFF, 0x7F7F),  # the last f32 that rounds to it
        (0x7F7F8000, 0x7F80),  # the first that rounds to infinity (a tie, odd: up)
        (0xFF7F8000, 0xFF80),
        (0x7F800000, 0x7F80),  # infinity stays
        (0xBF818000, 0xBF82),  # sign does not change the parity rule
    ]
    bits, vals = round_bfloat16(f32_of_bits(*[c[0] for c in cases]))
    assert bits.dtype == np.uint16 and vals.dtype == np.float32
    assert bits.tolist() == [c[1] for c in cases]
    assert np.array_equal(vals.view(np.uint32), bits.astype(np.uint32) << 16)
    nan_bits, nan_vals = round_bfloat16(f32_of_bits(0x7FC00000, 0x7F800001, 0xFFFFFFFF))
    assert np.isnan(nan_vals).all()
    # shape is kept
    assert round_bfloat16(np.zeros((3, 5), np.float32))[0].shape == (3, 5)


def test_round_bfloat16_is_torchs_conversion():
    from pandasim import round_bfloat16

    rng = np.random.default_rng(12)
    rand = rng.integers(0, 2 ** 32, 6000, dtype=np.uint64).astype(np.uint32)
    # adversarial: every low half around the tie, on random high halves of both parities
    high = rng.integers(0, 2 ** 16, 4000, dtype=np.uint64).astype(np.uint32) << 16
    low = np.tile(np.array([0x7FFE, 0x7FFF, 0x8000, 0x8001, 0x8002, 0x0000, 0x0001, 0xFFFF], np.uint32), 500)
    a = np.concatenate([rand, high | low]).view(np.float32)
    a = a[np.isfinite(a)]
    assert a.size > 9000
    bits, vals = round_bfloat16(a)
    want = torch.tensor(a).to(torch.bfloat16)
    assert np.array_equal(bits.view(np.int16), want.view(torch.int16).numpy())
    assert np.array_equal(vals.view(np.uint32), want.float().numpy().view(np.uint32))


# ------------------------------------------------------------ the restatement
def test_restatement_rounds_operands_and_keeps_the_last_layer():
    f = np.float32
    x = np.array([[f(1) + f(2.0 ** -8), f(3)]])      # 1 + 2^-8 is a tie: rounds to 1
    w = np.array([[f(1) + f(3 * 2.0 ** -8), f(0.5)]])  # a tie, odd: rounds up to 1 + 2^-6
    b = np.array([f(2.0 ** -20)])
    y = mlp_bfloat_np(x, [(w, b, False)])
    assert y.dtype == np.float64 and y[0, 0] == 1 * (1 + 2.0 ** -6) + 1.5 + 2.0 ** -20  # not rounded to bf16
    # between layers y is rounded again: 1 + 2^-6 + 1.5 + 2^-20 -> bf16
    y2 = mlp_bfloat_np(x, [(w, b, True), (np.ones((1, 1), f), np.zeros(1, f), False)])
    assert y2[0, 0] == 2.515625
    # relu and the pool
    rows = np.array([[-1.0], [-3.0], [2.0], [-5.0]], f)
    one = [(np.ones((1, 1), f), np.zeros(1, f), False)]
    assert mlp_bfloat_np(rows, one, pool=2).ravel().tolist() == [-1.0, 2.0]
    assert mlp_bfloat_np(rows, [(np.ones((1, 1), f), np.zeros(1, f), True)]).ravel().tolist() == [0, 0, 2.0, 0]


def test_bound_terms():
    f = np.float32
    rng = np.random.default_rng(2)
    x = rng.normal(size=(1, 5, 7)).astype(f)
    w, b = rng.normal(size=(3, 7)).astype(f), rng.normal(size=3).astype(f)
    from bfloat_reference import bf

    y, e = mlp_bfloat_with_bound(x, [(w, b, False)])
    mag = np.abs(bf(x[0])) @ np.abs(bf(w)).T + np.abs(b.astype(np.float64))
    assert np.allclose(e[0], 8 * 2.0 ** -23 * mag, rtol=1e-12)  # (c_in + 1) 2^-23 (|Wh||xh| + |b|), no carried term
    # a carried error enters as |Wh| (e_in + 2^-8 |x|)
    e_in = np.full(x.shape, 1e-3)
    _, e2 = mlp_bfloat_with_bound(x, [(w, b, False)], e_in=e_in)
    extra = (e_in[0] + UB * np.abs(x[0].astype(np.float64))) @ np.abs(bf(w)).T
    assert np.allclose(e2[0], e[0] + extra, rtol=1e-12)
    # the pooled bound is the group's largest
    _, e3 = mlp_bfloat_with_bound(x, [(w, b, False)], pool=5)
    assert np.array_equal(e3[0, 0], e[0].max(axis=0))


def test_dyadic_data_is_exact_in_f32_and_wide_ranged_data_is_not():
    layers = dyadic_net(1, 45, [96, 33, 40])
    rows = dyadic_rows(2, (2, 10, 45))
    assert exact_in_f32(rows, layers)
    # 2^12 and 2^-14 in one sum: 27 bits apart, more than f32 holds
    rows[0, 0, :2] = [2.0 ** 12, 2.0 ** -14]
    assert not exact_in_f32(rows, layers)


@pytest.mark.parametrize("name", CASES)
def test_restatement_within_the_bfloat_bound_of_the_f64_golden(name):
    parts, want = case_of(name)
    got, bound = np.zeros(want.shape), np.zeros(want.shape)
    for rows, prefix, pool, off, _ in parts:
        y, e = golden_bound(rows, folded(prefix), pool, centred=3 if name == "msg" else 0)
        got[..., off:off + y.shape[-1]], bound[..., off:off + y.shape[-1]] = y, e
    err = np.abs(got - want)
    print(f"{name}: worst |bf16 restatement - golden| = {err.max():.3e} ({err.max() / np.abs(want).max():.2e} of "
          f"max|golden|), worst error / bound = {(err / bound).max():.3f}")
    assert (bound > 0).all() and np.isfinite(bound).all()
    assert (err <= bound).all()
    # bf16 rounding shows: the restatement is not the f32 one
    assert err.max() > 1e-5 * np.abs(want).max()


# ---------------------------------------------------------------- the ABI
def test_header_and_signatures_carry_the_bfloat_topic():
    from pandasim import _lib as L

    assert_abi_topic(BFLOAT_SYMBOLS, "bfloat", ())
    assert C.sizeof(L.CloudMlpBfloatLayer) == 24
    assert L.CloudMlpBfloatLayer.c_out.offset == 16 and L.CloudMlpBfloatLayer.relu.offset == 20
    assert L.CloudMlpBfloatLayer is not L.CloudMlpLayer
    assert L.MLP_SYMBOLS == ("ps_cloud_mlp", "ps_cloud_group_mlp")


def test_python_surface():
    import pandasim

    assert callable(pandasim.round_bfloat16) and "round_bfloat16" in pandasim.__all__


# --------------------------------------------------- refusals and the f32 objects
def lay(o, i, value=0.0):
    return (np.full((o, i), value, np.float32), np.zeros(o, np.float32), True)


def test_cloud_mlp_precisions():
    from pandasim import CloudMlp
    from pandasim import _lib as L

    rng = np.random.default_rng(5)
    layers = [(rng.normal(size=(12, 9)).astype(np.float32), rng.normal(size=12).astype(np.float32), True),
              (rng.normal(size=(5, 12)).astype(np.float32), rng.normal(size=5).astype(np.float32), False)]
    plain, named = CloudMlp(layers, "cpu"), CloudMlp(layers, "cpu", precision="float32")
    for m in (plain, named):
        assert m.precision == "float32" and isinstance(m.array, L.CloudMlpLayer * 2)
        assert (m.c_in, m.widths, m.relu, len(m)) == (9, [12, 5], [True, False], 2)
        assert all(w.dtype == torch.float32 and np.array_equal(w.numpy(), l[0]) for w, l in zip(m.W, layers))
        assert all(np.array_equal(b.numpy(), l[1]) for b, l in zip(m.b, layers))
        assert [(a.W, a.b, a.c_out, a.relu) for a in m.array] == [(w.data_ptr(), b.data_ptr(), w.shape[0], int(r))
                                                                    for w, b, r in zip(m.W, m.b, m.relu)]
    half = CloudMlp(layers, "cpu", precision="bfloat16")
    assert half.precision == "bfloat16" and isinstance(half.array, L.CloudMlpBfloatLayer * 2)
    assert (half.c_in, half.widths, half.relu, len(half)) == (9, [12, 5], [True, False], 2)
    from pandasim import round_bfloat16

    for w, b, (w32, b32, _), a in zip(half.W, half.b, layers, half.array):
        assert w.dtype == torch.int16 and w.shape == (w32.shape[0], (w32.shape[1] + 7) & ~7)
        got = w.numpy().view(np.uint16)
        assert np.array_equal(got[:, :w32.shape[1]], round_bfloat16(w32)[0]) and (got[:, w32.shape[1]:] == 0).all()
        assert b.dtype == torch.float32 and np.array_equal(b.numpy(), b32)
        assert (a.W, a.b, a.c_out) == (w.data_ptr(), b.data_ptr(), w32.shape[0])
    with pytest.raises(ValueError):
        CloudMlp(layers, "cpu", precision="float16")
    with pytest.raises(ValueError):
        CloudMlp(layers, "cpu", precision=None)
    # a finite f32 weight that rounds to infinity in bf16
    big = f32_of_bits(0x7F7F8000)[0]
    CloudMlp([lay(4, 4, big)], "cpu")
    with pytest.raises(ValueError):
        CloudMlp([lay(4, 4, big)], "cpu", precision="bfloat16")
    CloudMlp([lay(4, 4, f32_of_bits(0x7F7F7FFF)[0])], "cpu", precision="bfloat16")


def test_mixed_precisions_are_refused():
    from types import SimpleNamespace

    from pandasim.cloudnet import abstract_features_args

    def fake(precision=None):
        m = SimpleNamespace(c_in=9, widths=[32], array=None)
        if precision:
            m.precision = precision
        return m

    i32 = torch.int32
    ok = dict(num_envs=2, xyz=torch.zeros(2, 50, 3), feats=torch.zeros(2, 50, 6), centre_idx=torch.zeros(2, 8, dtype=i32),
              group_idx=[torch.zeros(2, 8, 4, dtype=i32), torch.zeros(2, 8, 16, dtype=i32)])
    for pair in (("bfloat16", "bfloat16"), ("float32", "float32"), (None, "float32")):
        assert abstract_features_args(**ok, mlps=[fake(pair[0]), fake(pair[1])])[3:] == ([0, 32], 64)
    for pair in (("bfloat16", "float32"), ("float32", "bfloat16"), (None, "bfloat16")):
        with pytest.raises(ValueError):
            abstract_features_args(**ok, mlps=[fake(pair[0]), fake(pair[1])])


def test_segnet_precisions():
    from net_helpers import STATE_SEED, seeded_state
    from pandasim import CloudSegNet
    from pandasim import _lib as L

    state = seeded_state(STATE_SEED)
    plain, half = CloudSegNet(state, "cpu"), CloudSegNet(state, "cpu", precision="bfloat16")
    assert plain.precision == "float32" and half.precision == "bfloat16"
    assert plain.widths == half.widths and plain.num_classes == half.num_classes == 4
    every = lambda net: net.sa1 + net.sa2 + [net.sa3, net.fp3, net.fp2, net.fp1, net.head]  # noqa: E731
    assert all(m.precision == "float32" and isinstance(m.array[0], L.CloudMlpLayer) for m in every(plain))
    assert all(m.precision == "bfloat16" and isinstance(m.array[0], L.CloudMlpBfloatLayer) for m in every(half))
    assert [m.c_in for m in every(plain)] == [m.c_in for m in every(half)]
    with pytest.raises(ValueError):
        CloudSegNet(state, "cpu", precision="half")
