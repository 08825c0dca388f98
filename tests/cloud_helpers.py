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
