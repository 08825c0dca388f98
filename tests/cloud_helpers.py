"""What the PointNet++ test modules share besides the arithmetic
(tests/cloud_reference.py): the ABI assertions common to the three topics' CPU
tests, and the GPU tests' plumbing.  No fixtures: each module keeps its own.
"""
import ctypes as C
import os
import re

import numpy as np
import torch

from pandasim import _lib as L
from pandasim.sim import PandaSim, _ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SENTINEL = -12345.5  # what the shared MLP's tests fill an output with before a call


def assert_abi_topic(symbols, topic, macros):
    """The symbols added under `topic` (_lib.SIGNATURES' group): declared in
    include/pandasim.h with as many parameters as SIGNATURES binds, exported
    and bound returning int, and listed by _lib as `symbols`, in that order;
    the ABI version is 6; each PS_* limit in `macros` equals _lib's constant
    of that name without the prefix.  Returns the header's text."""
    src = open(os.path.join(ROOT, "include", "pandasim.h")).read()
    names = set(re.findall(r"\b(ps_[a-z_]+)\s*\(", src))
    lib = L.lib()
    for s in symbols:
        assert s in names and s in L.exported_symbols() and hasattr(lib, s), s
        assert L.SIGNATURES[s][2] == topic
        assert getattr(lib, s).restype is C.c_int and len(getattr(lib, s).argtypes) == len(L.SIGNATURES[s][0])
        decl = re.search(rf"\bint {s}\s*\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[s][0]), s
    assert getattr(L, f"{topic.upper()}_SYMBOLS") == symbols
    assert lib.ps_abi_version() == int(re.search(r"#define PS_ABI_VERSION (\d+)", src).group(1)) == 6
    for macro in macros:
        assert int(re.search(rf"#define {macro} (\d+)", src).group(1)) == getattr(L, macro[len("PS_"):]), macro
    return src


def make_sims(batches):
    """{B: a PandaSim context of B envs} for the clouds of a test module."""
    return {n: PandaSim("reach", num_envs=n, device=DEV) for n in batches}


def dev(a, dtype=None):
    """An array on the device; None stays None."""
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def bits(t):
    """A tensor or array on the host, f32 as its u32 bit patterns."""
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def raw_call(sim, name, *args):
    """The library's entry point `name` through ctypes -> its return code."""
    with torch.cuda.device(sim.device):
        return getattr(L.lib(), name)(*args)


def raw_group(sim, xyz, feats, centre_idx, gidx, new_xyz=False):
    """ps_cloud_group on device tensors -> grouped [B, S, K, D + 3]; with
    new_xyz also the centres [B, S, 3] (the entry point's optional output)."""
    nb, n = xyz.shape[:2]
    d, (s, k) = 0 if feats is None else feats.shape[2], gidx.shape[1:]
    out = torch.empty(nb, s, k, d + 3, device=DEV)
    centres = torch.empty(nb, s, 3, device=DEV) if new_xyz else None
    assert raw_call(sim, "ps_cloud_group", sim._ctx, _ptr(xyz), _ptr(feats), n, d, _ptr(centre_idx), s, _ptr(gidx), k,
                    _ptr(out), _ptr(centres), sim._stream()) == 0
    return (out, centres) if new_xyz else out


# ------------------------------------------- the shared MLP, f32 and bfloat16
def net(seed, c0, widths, relus=None, scale=1.0):
    """Seeded layers [(W, b, relu)] of the given widths; every layer has ReLU
    unless `relus` says otherwise."""
    rng = np.random.default_rng(seed)
    layers, c_in = [], c0
    for k, c_out in enumerate(widths):
        w = (rng.normal(size=(c_out, c_in)) * scale / np.sqrt(c_in)).astype(np.float32)
        b = (rng.normal(size=c_out) * 0.2).astype(np.float32)
        layers.append((w, b, True if relus is None else bool(relus[k])))
        c_in = c_out
    return layers


def upload(layers, precision="float32"):
    from pandasim import CloudMlp

    return CloudMlp(layers, DEV, precision=precision)


def raw_mlp(sim, rows, mlp, pool=1, out=None, offset=0, expect=0, suffix=""):
    """ps_cloud_mlp (suffix "_bfloat": its bfloat16 twin) on a device tensor
    rows [B, R, C0]; -> out."""
    nb, r, c0 = rows.shape
    if out is None:
        out = torch.full((nb, r // pool, mlp.widths[-1]), SENTINEL, device=DEV)
    assert raw_call(sim, "ps_cloud_mlp" + suffix, sim._ctx, _ptr(rows), r, c0, mlp.array, len(mlp), pool, _ptr(out),
                    out.shape[2], offset, sim._stream()) == expect
    return out


def raw_group_mlp(sim, xyz, feats, centre_idx, gidx, mlp, out=None, offset=0, expect=0, suffix=""):
    """ps_cloud_group_mlp (suffix "_bfloat": its bfloat16 twin) -> out."""
    nb, n = xyz.shape[:2]
    d, (s, k) = 0 if feats is None else feats.shape[2], gidx.shape[1:]
    if out is None:
        out = torch.full((nb, s, mlp.widths[-1]), SENTINEL, device=DEV)
    assert raw_call(sim, "ps_cloud_group_mlp" + suffix, sim._ctx, _ptr(xyz), _ptr(feats), n, d, _ptr(centre_idx), s,
                    _ptr(gidx), k, mlp.array, len(mlp), _ptr(out), out.shape[2], offset, sim._stream()) == expect
    return out


def random_groups(seed, nb, n, s, k, d):
    """A cloud with features and group indices padded as the ball query pads
    them: each row's tail repeats its first index."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, size=(nb, n, 3)).astype(np.float32)
    feats = rng.normal(size=(nb, n, d)).astype(np.float32) if d else None
    centre = np.stack([rng.permutation(n)[:s] for _ in range(nb)]).astype(np.int32)
    gidx = np.sort(rng.integers(0, n, size=(nb, s, k)), axis=-1).astype(np.int32)
    fill = rng.integers(1, k + 1, size=(nb, s))
    for b in range(nb):
        for c in range(s):
            gidx[b, c, fill[b, c]:] = gidx[b, c, 0]  # duplicate rows
    return xyz, feats, centre, gidx
