"""The one-lane step kernels against the bits of the build before the chunked
LDS layout of the gripper rows: tests/golden/
pgs_lds_layout_<task>.npz hold, for every task in ee control at 130 envs (two
waves and a two-lane tail) and 64 envs (one wave), the scripted actions of
tests/pgs_layout_cases.py and the whole state and step()'s returns after 1
and 25 steps, recorded by scripts/record_pgs_lds_fixtures.py from that build.
Replaying the actions must give every array bit for bit (tolerance 0)."""
import numpy as np
import pytest

import pgs_layout_cases as C

pytestmark = pytest.mark.gpu


def test_fixtures_load_every_gripper_slot():
    """The recorded contact-cache rows use each of the four gripper slots in
    some env, so an error in any slot's rows shows."""
    used = np.zeros(4, np.int64)
    for task in C.TASKS:
        fx = np.load(C.fixture_path(task))
        for B in C.BATCHES:
            for s in C.RECORD_AT:
                pack = fx[f"b{B}_s{s}_f"][C.WRID_ROW].astype(np.int64)
                for k in range(4):
                    used[k] += int((((pack >> (5 * k)) & 31) != 0).sum())
    assert (used > 0).all(), used.tolist()


@pytest.mark.parametrize("B", C.BATCHES)
@pytest.mark.parametrize("task", C.TASKS)
def test_one_lane_step_keeps_the_recorded_bits(task, B):
    fx = np.load(C.fixture_path(task))
    arrays, _, _ = C.run_case(task, B, actions=fx[f"b{B}_actions"])
    names = sorted(k for k in fx.files if k.startswith(f"b{B}_s"))
    assert len(names) == 11 * len(C.RECORD_AT) and {n[len(f"b{B}_"):] for n in names} == set(arrays)
    bad = []
    for n in names:
        want, got = fx[n], arrays[n[len(f"b{B}_"):]]
        assert want.shape == got.shape and want.dtype == got.dtype, n
        diff = C.bits(want) != C.bits(got)
        if diff.any():
            bad.append((n, int(diff.sum())))
    assert not bad, f"{task} x{B}: arrays that differ from the recorded bits (name, differing bytes): {bad}"
