#!/usr/bin/env python
"""Records tests/golden/pgs_lds_layout_<task>.npz from the library that is
loaded (PANDASIM_LIB, or the product): the runs of tests/pgs_layout_cases.py
-- six tasks, ee control, one-lane kernel, 130 and 64 envs, the state and
step()'s returns after 1 and 25 scripted steps, and the actions themselves.

Run it on the build whose bits are to be kept (the parent of a change that
must not move them).  It refuses to write a fixture set that could not see an
error in a gripper slot: over the recorded contact-cache rows every one of
the four slots must be in use in at least one env.

    python scripts/record_pgs_lds_fixtures.py [OUT_DIR]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "panda-lang-manip_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pgs_layout_cases as C  # noqa: E402


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    slot_envs = np.zeros(4, np.int64)  # envs with slot k in use, over every recorded WRID row
    for task in C.TASKS:
        data = {}
        for B in C.BATCHES:
            arrays, actions, used = C.run_case(task, B)
            data[f"b{B}_actions"] = actions
            for k, v in arrays.items():
                data[f"b{B}_{k}"] = v
            for s in C.RECORD_AT:
                pack = arrays[f"s{s}_f"][C.WRID_ROW].astype(np.int64)
                for k in range(4):
                    slot_envs[k] += int((((pack >> (5 * k)) & 31) != 0).sum())
            print(json.dumps({"task": task, "envs": B, "max_slots_in_use_by_step": used.max(1).tolist(),
                              "envs_with_4_slots_by_step": (used == 4).sum(1).tolist()}), flush=True)
        path = os.path.join(out_dir, os.path.basename(C.fixture_path(task)))
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        print(json.dumps({"task": task, "file": os.path.basename(path), "bytes": size}), flush=True)
        assert size <= 1 << 20, f"{path}: {size} B exceeds the committed-file limit"
    print(json.dumps({"recorded_envs_with_slot_in_use": slot_envs.tolist()}), flush=True)
    assert (slot_envs > 0).all(), f"a gripper slot is never in use in the recorded rows: {slot_envs.tolist()}"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else C.GOLDEN_DIR)
