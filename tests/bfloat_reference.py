"""What the bfloat16 shared MLP's tests share (tests/test_bfloat_cpu.py,
tests/test_gpu_bfloat.py): include/pandasim.h's bfloat16 specification restated
in float64 numpy, the bound a kernel may differ from it by, the bound of the
restatement against exact arithmetic on unrounded operands, dyadic data on
which every f32 sum is exact, and the network's wiring in that arithmetic.

The restatement: per layer xh = bf16(f32(x)) (round to nearest even), Wh =
bf16(W), y = b + xh Wh^T summed in f64, ReLU; the last y is returned as f64.

The kernel's bound (mlp_bfloat_with_bound), per layer, with e_in the bound on
the kernel's input against the restatement's x:
    accumulation   (c_in + 1) 2^-23 (|Wh| |xh| + |b|)
        any order of the c_in + 1 f32 additions, each rounded to nearest or
        truncated at f32 width (hence 2^-23, not 2^-24); the products of two
        bf16 values are exact in f32
    incoming       |Wh| (e_in + 2^-8 |x|), only where e_in > 0 (layer 0 rounds
        the very same f32 input on both sides)
        the second term: the two sides may round nearly equal values to
        different bf16 neighbours
ReLU and max are 1-Lipschitz: e passes through ReLU unchanged and a pooled
value takes the largest e of its group.
"""
import numpy as np

from cloud_reference import U, group_rows_np, propagate_np
from net_helpers import chain_np, fold_np

UB = 2.0 ** -8  # the unit roundoff of bfloat16 (8 bits of precision)


def bf(a):
    """f32(a) rounded to bfloat16, as float64 values."""
    from pandasim import round_bfloat16

    return round_bfloat16(np.asarray(a, dtype=np.float32))[1].astype(np.float64)


def _layers64(layers):
    return [(bf(w), np.asarray(b, np.float32).astype(np.float64), bool(relu)) for w, b, relu in layers]


def mlp_bfloat_np(rows, layers, pool=1):
    """rows [..., R, C0] f32 -> [..., R / pool, C_n] f64."""
    return mlp_bfloat_with_bound(rows, layers, pool, bound=False)[0]


def mlp_bfloat_with_bound(rows, layers, pool=1, e_in=None, bound=True):
    """The restatement and, beside it, the bound on a kernel's distance from it
    (this module's docstring); e_in is the bound the rows already carry (None:
    the kernel reads these very f32 rows)."""
    rows = np.asarray(rows)
    lead, r, c0 = rows.shape[:-2], rows.shape[-2], rows.shape[-1]
    x = rows.reshape(-1, c0).astype(np.float64)
    e = np.zeros(x.shape) if e_in is None else np.asarray(e_in, np.float64).reshape(-1, c0)
    for k, (wh, b, relu) in enumerate(_layers64(layers)):
        xh = bf(x)
        y = xh @ wh.T + b[None, :]
        if bound:
            mag = np.abs(xh) @ np.abs(wh).T + np.abs(b)[None, :]
            carried = (e + np.where(e > 0, UB * np.abs(x), 0.0)) @ np.abs(wh).T
            e = (wh.shape[1] + 1) * 2.0 ** -23 * mag + carried
        x = np.maximum(y, 0.0) if relu else y
    shape = (*lead, r // pool, pool, x.shape[-1])
    return x.reshape(shape).max(axis=-2), (e.reshape(shape).max(axis=-2) if bound else None)


def exact_in_f32(rows, layers):
    """True if every partial sum of every layer, in any order, is exactly
    representable in f32: every term is a multiple of a common power of two q
    and sum |terms| = |Wh| |xh| + |b| stays below 2^24 q.  Checked on the
    restatement's own values, layer by layer."""
    x = np.asarray(rows, np.float64).reshape(-1, np.asarray(rows).shape[-1])
    for wh, b, relu in _layers64(layers):
        xh = bf(x)  # a hidden y need not be a bf16 value: both sides round the same exact y alike
        # the finest bit set in any operand: products are multiples of qx * qw, b of qb
        def quantum(a):
            a = np.abs(a[a != 0])
            if a.size == 0:
                return np.inf
            m, ex = np.frexp(a)
            low = (m * 2.0 ** 53).astype(np.int64)
            tz = np.log2((low & -low).astype(np.float64))
            return float(2.0 ** (ex - 53 + tz).min())

        q = min(quantum(xh) * quantum(wh), quantum(b))
        mag = np.abs(xh) @ np.abs(wh).T + np.abs(b)[None, :]
        if not mag.max() < 2.0 ** 24 * q:
            return False
        y = xh @ wh.T + b[None, :]
        x = np.maximum(y, 0.0) if relu else y
    return True


def dyadic_net(seed, c0, widths, relus=None):
    """Layers of small integers times powers of two: weights in {-1, 0, 1} (odd
    layers: halves), dense in the first layer, so that every k of it counts,
    and about 6 per row behind it, so that the sums do not grow past f32's 24
    bits; biases in -2..2 quarters.  With dyadic_rows every partial sum is a
    small multiple of a fixed power of two (exact_in_f32 asserts it)."""
    rng = np.random.default_rng(seed)
    layers, c_in = [], c0
    for k, c_out in enumerate(widths):
        w = rng.integers(-1, 2, size=(c_out, c_in)).astype(np.float32)
        if k > 0:
            w = w * (rng.random((c_out, c_in)) < min(1.0, 6.0 / c_in)) * np.float32(0.5 if k & 1 else 1.0)
        w = w.astype(np.float32)
        b = (rng.integers(-2, 3, size=c_out) * 0.25).astype(np.float32)
        layers.append((w, b, True if relus is None else bool(relus[k])))
        c_in = c_out
    return layers


def dyadic_rows(seed, shape):
    """Integers in -3..3 (bf16 values)."""
    return np.random.default_rng(seed).integers(-3, 4, size=shape).astype(np.float32)


def golden_bound(rows, layers, pool=1, centred=0):
    """The restatement and the bound on its distance from exact arithmetic on
    the unrounded operands (the f64 golden of the reference's layers).  With x
    the restated input of a layer, e_in the bound on its distance from the
    exact one x*, W' and b' the folded f32 parameters (each one rounding of the
    exact fold), u = 2^-24 and ub = 2^-8:
        |bf16(f32(x)) - x*| <= e_in + (ub + u) |x|     the activation's roundings
        |Wh - W'|           <= ub |W'|                 the weight's rounding
        |x*|                <= |x| + e_in
    so  e_out = |Wh| (e_in + (ub + u) |x|) + (ub + u) |W'| (|x| + e_in) + u |b'|,
    times 1.01 for the f64 roundings on both sides.  The last `centred` input
    columns are f32 differences, one rounding from the reference's: u |x|."""
    rows = np.asarray(rows)
    lead, r, c0 = rows.shape[:-2], rows.shape[-2], rows.shape[-1]
    x = rows.reshape(-1, c0).astype(np.float64)
    e = np.zeros(x.shape)
    if centred:
        e[:, c0 - centred:] = U * np.abs(x[:, c0 - centred:])
    for (w, b, relu), (wh, b64, _) in zip(layers, _layers64(layers)):
        aw, ax = np.abs(np.asarray(w, np.float64)), np.abs(x)
        e = 1.01 * ((e + (UB + U) * ax) @ np.abs(wh).T + (UB + U) * ((ax + e) @ aw.T) + U * np.abs(b64)[None, :])
        y = bf(x) @ wh.T + b64[None, :]
        x = np.maximum(y, 0.0) if relu else y
    shape = (*lead, r // pool, pool, x.shape[-1])
    return x.reshape(shape).max(axis=-2), e.reshape(shape).max(axis=-2)


# ------------------------------------------------------------ the network
def segnet_bfloat_np(state, xyz, colors, idx):
    """net_helpers.segnet_np's wiring with every shared MLP in the bfloat16
    arithmetic (weights folded to f32 as CloudSegNet folds them, then rounded)
    and everything between them in the kernels' f32 arithmetic, on given
    indices -> head [B, N, 18] f64 and the bound a kernel run may differ by,
    carried through the layers (the f32 steps between the MLPs are linear
    interpolations and copies: the bound passes through them by the same
    weights, plus their own f32 roundings at 4 u of the magnitudes)."""
    f = np.float32
    x = np.asarray(xyz, f)
    l0 = np.concatenate([x, np.asarray(colors, f)], -1)
    nb = x.shape[0]
    take = lambda a, i: np.stack([a[b][i[b]] for b in range(nb)])  # noqa: E731

    def chain(convs, bns):
        return [(w, b, True) for w, b in chain_np(state, convs, bns, f)]

    def msg(name, pts, feats, efeats, fps, groups):
        outs, errs = [], []
        for i, gi in enumerate(groups):
            rows = group_rows_np(pts, feats.astype(f), fps, gi)
            erows = group_rows_np(np.zeros_like(pts), efeats, fps, gi, np.float64)  # e of the features, 0 of xyz
            nbk = rows.shape[:3]
            y, e = mlp_bfloat_with_bound(rows.reshape(nb, -1, rows.shape[-1]),
                                         chain(f"{name}.conv_blocks.{i}", f"{name}.bn_blocks.{i}"), nbk[2],
                                         e_in=erows.reshape(nb, -1, rows.shape[-1]))
            outs.append(y)
            errs.append(e)
        return np.concatenate(outs, -1), np.concatenate(errs, -1)

    def prop(xyz1, xyz2, p2, e2, p1, e1):
        """propagate_np on the f32 values; the bound by the same idx / weight."""
        out, pidx, w = propagate_np(xyz1, xyz2, p2.astype(f), None if p1 is None else p1.astype(f))
        if xyz2.shape[1] == 1:
            ei = np.repeat(e2, xyz1.shape[1], axis=1)
        else:
            ei = np.stack([(e2[b][pidx[b]] * w[b][..., None].astype(np.float64)).sum(1) for b in range(nb)])
        d2 = p2.shape[-1]
        ei = ei + 4 * U * np.abs(out[..., out.shape[-1] - d2:].astype(np.float64))
        return out, (ei if e1 is None else np.concatenate([e1, ei], -1))

    z0 = np.zeros(l0.shape)
    l1, e1 = msg("sa1", x, l0, z0, idx["fps1"], idx["group1"])
    x1 = take(x, idx["fps1"])
    l2, e2 = msg("sa2", x1, l1, e1 + U * np.abs(l1), idx["fps2"], idx["group2"])
    x2 = take(x1, idx["fps2"])
    rows3 = np.concatenate([x2, l2.astype(f)], -1)
    e3in = np.concatenate([np.zeros(x2.shape), e2 + U * np.abs(l2)], -1)
    l3, e3 = mlp_bfloat_with_bound(rows3, chain("sa3.mlp_convs", "sa3.mlp_bns"), rows3.shape[1], e_in=e3in)
    origin = np.zeros((nb, 1, 3), f)
    r, er = prop(x2, origin, l3, e3 + U * np.abs(l3), l2, e2 + U * np.abs(l2))
    l2, e2 = mlp_bfloat_with_bound(r, chain("fp3.mlp_convs", "fp3.mlp_bns"), 1, e_in=er)
    r, er = prop(x1, x2, l2, e2 + U * np.abs(l2), l1, e1 + U * np.abs(l1))
    l1, e1 = mlp_bfloat_with_bound(r, chain("fp2.mlp_convs", "fp2.mlp_bns"), 1, e_in=er)
    r, er = prop(x, x1, l1, e1 + U * np.abs(l1), np.concatenate([x, l0], -1), np.zeros((*x.shape[:2], 9)))
    l0, e0 = mlp_bfloat_with_bound(r, chain("fp1.mlp_convs", "fp1.mlp_bns"), 1, e_in=er)
    w1, b1 = fold_np(state, "conv1", "bn1", f)
    w2, b2 = fold_np(state, "conv2", None, f)
    return mlp_bfloat_with_bound(l0.astype(f), [(w1, b1, True), (w2, b2, False)], 1, e_in=e0 + U * np.abs(l0))
