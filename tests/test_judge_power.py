"""CPU: the parity classifier (tests/parity_judge.judge) has power (VERDICT r04
weak 1 / item 1).  The "GPU" is the oracle in fp32-like arithmetic
(tests/judge_power.py); with a deliberate model error of 1-2 % -- the kind of
error a wrong constant in include/panda_model.h would be -- the teacher-forced
workloads of the GPU tests must yield 'beyond' samples (the GPU test's
assertion would fail), and without one they must yield none.

A mutation can only be seen where it moves the observation by more than the
tight bounds within one step: a 12 % change of btMultiBody's damping (0.04 ->
0.045) moves a motor-driven arm's end effector by < 2e-5 m per step (the
POSITION_CONTROL rows overwrite the damped velocity), so on the random
workload it is invisible to any per-step check at these bounds; it shows where
an object slides (the scripted push).  profiles/r05_judge_power.jsonl has the
full scan at 64 envs and the smallest mutation of each kind that is detected
(scripts/judge_power_scan.py).
"""
import functools

import pytest

import judge_power as J

B = 16  # envs per workload here; the committed scan uses the GPU tests' 64


@functools.lru_cache(maxsize=None)
def _judged_64(task, control, workload, mutation):
    """One judge_workload run at the GPU tests' 64 envs, shared by the tests below (read only)."""
    return J.judge_workload(task, control, workload, mutation, B=64)


@pytest.mark.parametrize("task,control,workload", [("push", "ee", "random"), ("reach", "joints", "random"),
                                                   ("pick_and_place", "ee", "random"), ("push", "ee", "push"),
                                                   ("slide", "ee", "push"), ("stack", "ee", "random"),
                                                   ("flip", "ee", "random"), ("stack", "ee", "stack_push"),
                                                   ("flip", "ee", "push")])
def test_unmutated_fp32_oracle_has_no_beyond_samples(task, control, workload):
    counts, *_ = J.classify_workload(task, control, workload, "none", B=B)
    print(task, control, workload, counts)
    assert counts["beyond"] == 0
    # a blocked gripper leaves next to nothing untight (parity_judge.NOT_TIGHT_CAP)
    if task not in ("pick_and_place", "stack", "flip"):
        assert counts["conditioned"] + counts["bif"] <= 0.005 * sum(counts.values()) + 1


@pytest.mark.parametrize("task,control,workload,mutation", [
    ("reach", "ee", "random", "motor_kp_x1.01"),
    ("push", "ee", "random", "motor_kp_x1.01"),
    ("reach", "joints", "random", "motor_kp_x1.01"),
    ("push", "ee", "push", "cube_mass_x1.02"),
    ("push", "ee", "push", "cube_friction_0.51"),
    ("push", "ee", "push", "finger_box_+0.5mm"),
    ("push", "ee", "push", "link_damping_0.045"),
    ("pick_and_place", "ee", "push", "cube_mass_x1.02"),
])
def test_model_errors_are_beyond(task, control, workload, mutation):
    """Each mutation yields beyond samples, and most samples whose fp64 effect
    alone leaves the tight bounds are classified beyond, not absorbed as
    conditioned or ill-conditioned."""
    counts, worst, effect, visible = J.classify_workload(task, control, workload, mutation, B=B)
    print(task, control, workload, mutation, counts, f"samples the mutation moves beyond the tight bounds: {visible}",
          {k: f"{v:.1e}" for k, v in effect.items()})
    assert visible > 0
    assert counts["beyond"] > 0
    assert counts["beyond"] >= 0.5 * visible


# Round 6: the second cube and the cube-cube rows of
# Stack, and Flip's quaternion observation.  At the GPU tests' 64 envs: with 16
# the pair-friction case has too few visible samples for the half-beyond
# criterion to be a measurement (10 of 26 at 16 envs, 56 of 108 at 64:
# profiles/r06_judge_power.log).
@pytest.mark.parametrize("task,control,workload,mutation", [
    ("stack", "ee", "stack_push", "cube2_mass_x1.02"),
    ("stack", "ee", "stack_push", "pair_friction_x1.02"),
    ("stack", "ee", "stack_push", "cube_mass_x1.02"),
    ("flip", "ee", "push", "cube_mass_x1.02"),
    ("flip", "ee", "push", "cube_friction_0.51"),
])
def test_model_errors_are_beyond_stack_flip(task, control, workload, mutation):
    r = _judged_64(task, control, workload, mutation)
    counts, worst, effect, visible = r["counts"], r["worst"], r["effect"], r["visible"]
    print(task, control, workload, mutation, counts, f"samples the mutation moves beyond the tight bounds: {visible}",
          {k: f"{v:.1e}" for k, v in effect.items()})
    assert visible > 0
    assert counts["beyond"] > 0
    assert counts["beyond"] >= 0.5 * visible
    if task == "flip":
        # the mutation moves Flip's quaternion observation itself
        assert effect["obj_rot"] > J.TOL["flip"]["obj_rot"]
    if mutation in ("cube2_mass_x1.02", "pair_friction_x1.02"):
        # ... and the second cube's, through the cube-cube rows
        assert effect["obj2_pos"] > J.TOL["stack"]["obj2_pos"] and effect["obj2_rot"] > J.TOL["stack"]["obj2_rot"]


# The whole verdict of test_gpu_parity.test_judged_contact_workloads
# (parity_judge.contact_workload_failures: the resting-stack escape
# at_pgs_resolution, its 0.5 % cap, the caps on the other classes) on the same
# stand-in runs.  The escape excuses beyond samples of a real model error too
# -- 6 of 14 at cube 2's mass x 1.002 before it asked for a stack at rest --
# so the factors where it excused the most are run here.  Every one of these
# verdicts fails through its unexcused beyond samples alone (78 and 11 at cube
# 2's mass x 1.005 and x 1.002), so these cases hold whatever the escape's
# bounds and the caps are: those are pinned by test_escape_boundaries and
# test_verdict_caps_at_896_samples below.
@pytest.mark.parametrize("task,control,workload,mutation", [
    ("stack", "ee", "stack_push", "cube2_mass_x1.02"),
    ("stack", "ee", "stack_push", "pair_friction_x1.02"),
    ("stack", "ee", "stack_push", "cube_mass_x1.02"),
    ("stack", "ee", "stack_push", "cube2_mass_x1.005"),
    ("stack", "ee", "stack_push", "cube2_mass_x1.002"),
    ("stack", "ee", "stack_push", "pair_friction_x1.005"),
    ("flip", "ee", "push", "cube_mass_x1.02"),
    ("flip", "ee", "push", "cube_friction_0.51"),
])
def test_contact_verdict_fails_on_model_errors(task, control, workload, mutation):
    r = _judged_64(task, control, workload, mutation)
    fails, excused, unexcused = J.workload_verdict(task, r)
    print(task, workload, mutation, r["counts"], f"beyond / excused / unexcused: {len(r['beyond'])} / {len(excused)} / "
          f"{len(unexcused)}; past loose {len(r['past_loose'])}; fired:", [f.split(":")[0] for f in fails])
    assert fails != []


@pytest.mark.parametrize("task,control,workload", [("stack", "ee", "stack_push"), ("stack", "ee", "push"),
                                                   ("flip", "ee", "push")])
def test_contact_verdict_passes_the_unmutated_stand_in(task, control, workload):
    r = _judged_64(task, control, workload, "none")
    fails, excused, unexcused = J.workload_verdict(task, r)
    print(task, workload, "none", r["counts"], f"beyond / excused / unexcused: {len(r['beyond'])} / {len(excused)} / "
          f"{len(unexcused)}; past loose {len(r['past_loose'])}; fired:", fails)
    assert fails == []


# The verdict's constants, pinned on synthetic samples at and just past each
# boundary.  The figures are written out here, not read from parity_judge: an
# edit to PGS_RESOLUTION, REST_SPEED, a cap or the classes' TOL fails a case.
_STACK_GROUPS = ("ee_pos", "ee_vel", "width", "obj_pos", "obj_rot", "obj_vel", "obj_avel",
                 "obj2_pos", "obj2_rot", "obj2_vel", "obj2_avel")
_AT_REST = {"pair_after": 4, "v": 7.2e-4, "w": 1.68e-2}  # at both resting-speed bounds


def _errs(**over):
    """Every velocity-free group at its tight bound, the objects' velocities at the escape's bounds."""
    e = {k: J.TOL["stack"][k] for k in _STACK_GROUPS}
    e.update({k: 6.4e-4 if k.endswith("_vel") else 3.2e-2 for k in _STACK_GROUPS if k.startswith("obj") and "vel" in k})
    e.update(over)
    return e


def test_escape_boundaries():
    from parity_judge import at_pgs_resolution as esc

    assert [J.TOL["stack"][k] for k in _STACK_GROUPS[:5]] == [2e-5, 2e-3, 2e-4, 2e-5, 1e-4]
    assert esc("stack", _errs(), _AT_REST)  # on every bound at once
    for k, bound in (("obj_vel", 6.4e-4), ("obj2_vel", 6.4e-4), ("obj_avel", 3.2e-2), ("obj2_avel", 3.2e-2)):
        assert not esc("stack", _errs(**{k: bound * 1.01}), _AT_REST), k
    for k in ("ee_pos", "ee_vel", "width", "obj_pos", "obj_rot", "obj2_pos", "obj2_rot"):
        assert not esc("stack", _errs(**{k: J.TOL["stack"][k] * 1.01}), _AT_REST), k
    assert not esc("stack", _errs(), dict(_AT_REST, v=7.2e-4 * 1.01))
    assert not esc("stack", _errs(), dict(_AT_REST, w=1.68e-2 * 1.01))
    assert not esc("stack", _errs(), dict(_AT_REST, pair_after=0))
    # Flip has one cube: no pair, never excused
    flip = {k: v for k, v in _errs().items() if not k.startswith("obj2")}
    assert not esc("flip", flip, {"pair_after": 0, "v": 0.0, "w": 0.0})


def test_verdict_caps_at_896_samples():
    """64 envs x 14 steps: 0.5 % = 4.48, 6 % = 53.76, 8 % = 71.68, 1 % = 8.96."""
    from parity_judge import contact_workload_failures as verdict

    n = 896
    excused, wrong = (0, 0, _errs(), _AT_REST), (0, 0, _errs(obj_pos=1e-3), _AT_REST)

    def fired(resolution=4, conditioned=53, bif=71, loose=8, unexcused=0):
        counts = {"tight": n - conditioned - bif - resolution - unexcused, "conditioned": conditioned, "bif": bif,
                  "beyond": resolution + unexcused}
        fails = verdict("stack", n, counts, [excused] * resolution + [wrong] * unexcused, [(0, 0, {})] * loose)
        return [f.split(":")[0] for f in fails]

    assert fired() == []  # on every cap at once
    assert fired(resolution=5) == ["resolution"]
    assert fired(conditioned=54) == ["conditioned"]
    assert fired(bif=72) == ["bif"]
    assert fired(loose=9) == ["past loose"]
    assert fired(unexcused=1) == ["beyond"]
    assert fired(resolution=5, conditioned=54, bif=72, loose=9, unexcused=1) == [
        "beyond", "resolution", "conditioned", "bif", "past loose"]


def test_damping_error_on_a_motor_driven_arm_is_below_the_bounds():
    """The undetectable case, stated: on the random Reach workload the damping
    mutation's own effect stays inside the tight bounds, so every sample is
    tight -- the classifier is not hiding it, the step does not show it."""
    counts, worst, effect, visible = J.classify_workload("reach", "ee", "random", "link_damping_0.045", B=B)
    print(counts, {k: f"{v:.1e}" for k, v in effect.items()})
    assert visible == 0 and counts["tight"] == sum(counts.values())
    assert 0 < effect["ee_pos"] < 2e-5
