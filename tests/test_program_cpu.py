"""CPU tests of the motion programs (ps_motion_program;
pandasim.panda_cartesian.MotionProgram, Panda.run; pandasim.skills): the ABI
symbol and its refusals, the builder's lowering on CPU tensors, the host
checks, and the three skills of run_policy.py:189-193, 287-339 as segment
lists written out by hand from its lines.  No kernel is launched.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from cloud_helpers import assert_abi_topic
from pandasim import _lib as L
from pandasim import skills
from pandasim.panda_cartesian import MotionProgram, Panda, program_flags

MOVE, GRASP, RELEASE, WAIT = 0, 1, 2, 3
B = 3


# ------------------------------------------------------------------- the ABI
def test_symbol_and_constants_match_the_header():
    src = assert_abi_topic(("ps_motion_program",), "program", ("PS_PROGRAM_MAX_SEGMENTS", "PS_PROGRAM_MAX_WAIT"))
    for name, value in (("MOVE", MOVE), ("GRASP", GRASP), ("RELEASE", RELEASE), ("WAIT", WAIT)):
        assert int(re.search(rf"\bPS_SEG_{name} = (\d+)", src).group(1)) == getattr(L, f"SEG_{name}") == value
    assert (L.PROGRAM_MAX_SEGMENTS, L.PROGRAM_MAX_WAIT) == (32, 1000)


def test_refusals_need_no_device():
    """Every PS_ERR_ARG case returns before anything is enqueued: the pointers
    below are never dereferenced on the device."""
    lib = L.lib()
    cfg = L.default_config(2, 0, 0)
    ctx = C.c_void_p()
    assert lib.ps_create(C.byref(cfg), 8, 0, C.byref(ctx)) == 0
    x = C.c_void_p(64)

    def call(ctx=ctx, state=x, plan=x, S=2, kinds=(MOVE, WAIT), waits=(0, 5), pos=x, quat=x):
        k = None if kinds is None else (C.c_int32 * len(kinds))(*kinds)
        w = None if waits is None else (C.c_int32 * len(waits))(*waits)
        return lib.ps_motion_program(ctx, state, plan, S, k, w, 0, pos, quat, None, None, None, None, None)

    assert call(ctx=None) == call(state=None) == call(plan=None) == call(kinds=None) == -1
    assert call(S=0) == call(S=-1) == -1
    assert call(S=33, kinds=(GRASP,) * 33, waits=(0,) * 33) == -1
    assert call(kinds=(MOVE, 4)) == call(kinds=(-1, WAIT)) == -1
    assert call(waits=(0, 0)) == call(waits=(0, 1001)) == call(waits=(0, -2)) == call(waits=None) == -1
    assert call(pos=None) == call(quat=None) == -1
    assert b"wait" in lib.ps_last_error(ctx) or b"move" in lib.ps_last_error(ctx)
    lib.ps_destroy(ctx)


# ---------------------------------------------------------------- the builder
def test_lowering_on_cpu_tensors():
    gp = torch.arange(9, dtype=torch.float32).reshape(B, 3)
    p = MotionProgram(B, "cpu")
    assert p.move(gp, [180.0, 0.0, 10.0]) is p
    p.grasp(mask=[1, 0, 2]).move(np.array([0.1, 0.2, 0.3]), gp + 1).wait(7).release(0.02, mask=torch.tensor([0, 1, 1]))
    p.release(torch.tensor([0.01, 0.02, 0.03])).move([0, 0, 0.6], [180, 0, 0])
    assert len(p) == 7
    low = p.lower(False)
    assert low.kinds == [MOVE, GRASP, MOVE, WAIT, RELEASE, RELEASE, MOVE]
    assert low.wait_steps == [0, 0, 0, 7, 0, 0, 0]
    assert low.blocked == [False, True, True, True, False, False, False] and low.blocked_after is False
    assert p.lower(True).blocked == [True, True, True, True, False, False, False]
    z = torch.zeros(B, 3)
    want_pos = torch.stack([gp, z, torch.tensor([0.1, 0.2, 0.3]).expand(B, 3), z, z, z,
                            torch.tensor([0.0, 0.0, 0.6]).expand(B, 3)])
    want_euler = torch.stack([torch.tensor([180.0, 0.0, 10.0]).expand(B, 3), z, gp + 1, z, z, z,
                              torch.tensor([180.0, 0.0, 0.0]).expand(B, 3)])
    assert low.goal_pos.dtype == torch.float32 and low.goal_pos.is_contiguous()
    assert torch.equal(low.goal_pos, want_pos) and torch.equal(low.goal_euler, want_euler)
    one = torch.ones(B)
    assert torch.equal(low.width, torch.stack([one, one, one, one, torch.full((B,), 0.02),
                                               torch.tensor([0.01, 0.02, 0.03]), one]))
    m = torch.ones(7, B, dtype=torch.uint8)
    m[1], m[4] = torch.tensor([1, 0, 1]), torch.tensor([0, 1, 1])
    assert low.mask.dtype == torch.uint8 and torch.equal(low.mask, m)
    # nothing to stack where no segment needs it
    bare = MotionProgram(B, "cpu").grasp().wait(1).lower(False)
    assert bare.goal_pos is None and bare.goal_euler is None and bare.width is None and bare.mask is None
    assert bare.blocked == [True, True] and bare.blocked_after is True


def test_host_checks_name_the_bad_argument():
    p = MotionProgram(B, "cpu")
    for bad, name in ((lambda: p.move(torch.zeros(2, 3), [0, 0, 0]), "goal_pos"),
                      (lambda: p.move([0, 0, 0], torch.zeros(B, 4)), "goal_euler"),
                      (lambda: p.move([0, 0, 0], 5.0), "goal_euler"),
                      (lambda: p.release(torch.zeros(2)), "width"),
                      (lambda: p.grasp(mask=[1, 0]), "mask"),
                      (lambda: p.wait(0), "wait"), (lambda: p.wait(1001), "wait"), (lambda: p.wait(2.5), "wait"),
                      (lambda: p.wait(True), "wait")):
        with pytest.raises(ValueError, match=name):
            bad()
    assert len(p) == 0  # a refused segment is not added
    with pytest.raises(ValueError, match="segments"):
        p.lower(False)  # an empty program
    for _ in range(32):
        p.grasp()
    with pytest.raises(ValueError, match="32 segments"):
        p.grasp()
    assert len(p.lower(False).kinds) == 32
    with pytest.raises(ValueError, match="33 segments"):
        program_flags([GRASP] * 33, [0] * 33, False)
    with pytest.raises(ValueError, match="unknown kind"):
        program_flags([MOVE, 7], [0, 0], False)
    with pytest.raises(ValueError, match="wait_steps"):
        program_flags([MOVE, WAIT], [0], False)
    with pytest.raises(ValueError, match="wait"):
        program_flags([WAIT], [0], False)
    assert program_flags([MOVE, GRASP, WAIT, RELEASE, MOVE], [0, 0, 1000, 0, 0], True) == (
        [True, True, True, False, False], False)


# ------------------------------------------------------------------ Panda.run
class _Sim:
    device = torch.device("cpu")
    num_envs = B

    def __init__(self):
        self.calls = []

    def motion_plan(self):
        return "plan"

    def motion_program(self, plan, program, blocked):
        self.calls.append((plan, program, blocked))
        return "completed", "steps", program.lower(blocked).blocked_after


class _Robot(Panda):
    """A Panda without a sim behind it: run() reaches _Sim.motion_program."""

    def __init__(self, block_gripper=False):
        self.sim, self.block_gripper, self._plan, self.resets = _Sim(), block_gripper, None, 0

    def reset(self):
        self.resets += 1
        self.sim.calls.append("reset")


def test_run_leaves_block_gripper_as_the_calls_would():
    robot = _Robot(block_gripper=False)
    p = MotionProgram(B, "cpu").move([0, 0, 0.1], [180, 0, 0]).grasp(mask=[0, 0, 0])
    assert robot.run(p) == ("completed", "steps") and robot.block_gripper is True  # a grasp sets it whatever its mask
    assert robot.sim.calls == [("plan", p, False)]
    robot.run(MotionProgram(B, "cpu").wait(3))
    assert robot.block_gripper is True and robot.sim.calls[-1][2] is True
    robot.run(MotionProgram(B, "cpu").release().move([0, 0, 0.1], [180, 0, 0]))
    assert robot.block_gripper is False


# ------------------------------------------------------------------ the skills
START = torch.tensor([[0.10, -0.20, 0.05], [0.00, 0.10, 0.02], [-0.10, 0.00, 0.30]])
END = torch.tensor([[0.00, 0.20, 0.25], [0.15, 0.10, 0.20], [-0.10, 0.15, 0.10]])
START_E = torch.tensor([[180.0, 0.0, 0.0], [170.0, 5.0, 0.0], [-175.0, 0.0, 20.0]])
END_E = torch.tensor([[180.0, 0.0, 90.0], [180.0, 45.0, 0.0], [150.0, 0.0, 0.0]])
HOME = (MOVE, (0.0, 0.0, 0.6), (180.0, 0.0, 0.0))


def _segments(program):
    """[(kind, goal_pos, goal_euler) | (kind, width) | (kind, n) | (kind,)] as nested lists."""
    out = []
    for kind, n, pos, euler, width, mask in program.segments:
        assert mask is None
        if kind == MOVE:
            out.append((kind, pos.tolist(), euler.tolist()))
        elif kind == RELEASE:
            out.append((kind, width.tolist()))
        else:
            out.append((kind, n) if kind == WAIT else (kind,))
    return out


def _move(pos, euler):
    pos, euler = torch.as_tensor(pos, dtype=torch.float32), torch.as_tensor(euler, dtype=torch.float32)
    return (MOVE, pos.expand(B, 3).tolist(), euler.expand(B, 3).tolist())


RELEASE_1 = (RELEASE, [1.0] * B)
HOME_SEGMENTS = [_move(HOME[1], HOME[2]), RELEASE_1]


def test_reset_robot_is_reset_move_release():
    robot = _Robot()
    skills.reset_robot(robot)  # run_policy.py:189-193
    assert robot.sim.calls[0] == "reset" and len(robot.sim.calls) == 2
    assert _segments(robot.sim.calls[1][1]) == HOME_SEGMENTS


def test_pour_is_run_policy_325_339():
    robot = _Robot()
    skills.pour(robot, START, END, START_E, END_E)
    up = START + torch.tensor([0.0, 0.0, 0.10])
    want = [_move(up, START_E),       # :327 move(start_pos + [0, 0, 0.10], start_euler)
            _move(START, START_E),    # :328
            (GRASP,),                 # :329
            _move(up, START_E),       # :331
            _move(END, START_E),      # :333
            _move(END, END_E),        # :334
            (WAIT, 50)]               # :337-338
    main, _, home = robot.sim.calls   # :339 reset_robot
    assert _segments(main[1]) == want and robot.sim.calls[1] == "reset" and _segments(home[1]) == HOME_SEGMENTS
    low = main[1].lower(False)
    assert low.kinds == [MOVE, MOVE, GRASP, MOVE, MOVE, MOVE, WAIT] and low.wait_steps == [0, 0, 0, 0, 0, 0, 50]
    assert low.blocked == [False, False, True, True, True, True, True]
    assert tuple(low.goal_pos.shape) == (7, B, 3) and low.width is None and low.mask is None
    assert robot.block_gripper is False  # reset_robot's release


def test_open_is_run_policy_287_309():
    robot = _Robot(block_gripper=True)
    skills.open_(robot, START, END, START_E, END_E)  # (grasp, approach) = (start, end)
    delta = (END - START) / 15
    want = (HOME_SEGMENTS                                              # :292 reset_robot
            + [_move(END, START_E), (WAIT, 50),                         # :293-295 approach_pos, grasp_euler
               _move(START, START_E), (WAIT, 50),                       # :296-298
               (GRASP,)]                                                # :299
            + [_move(START + i * delta, START_E) for i in range(15)]    # :305-306
            + [RELEASE_1])                                              # :308
    assert robot.sim.calls[0] == "reset" and robot.sim.calls[2] == "reset"  # :292, :309
    main, home = robot.sim.calls[1], robot.sim.calls[3]
    assert _segments(main[1]) == want and len(want) == 23 and _segments(home[1]) == HOME_SEGMENTS
    assert main[2] is True  # the robot's flag reaches the first move
    assert main[1].lower(True).blocked == [True] + [False] * 5 + [True] * 16 + [False]


def test_close_is_run_policy_311_323():
    robot = _Robot()
    skills.close(robot, START, END, START_E, END_E)  # (approach, grasp) = (start, end); every move at grasp_euler
    delta = (START - END) / 15
    want = []
    for i in range(15):
        want.append(_move(START - i * delta, END_E))  # :321
        if i == 3:
            want.append((GRASP,))                    # :322-323
    assert len(robot.sim.calls) == 1 and _segments(robot.sim.calls[0][1]) == want
    assert robot.block_gripper is True and robot.resets == 0


def test_execute_dispatches_in_the_reference_argument_order():
    class Decoded:
        waypoints = torch.stack([START, END], 1)
        euler_deg = torch.stack([START_E, END_E], 1)

    for name, fn in (("pour", skills.pour), ("open", skills.open_), ("close", skills.close)):
        a, b = _Robot(), _Robot()
        out = skills.execute(a, Decoded(), name)
        fn(b, START, END, START_E, END_E)
        assert list(out) == [name]
        assert [c if c == "reset" else _segments(c[1]) for c in a.sim.calls] == \
               [c if c == "reset" else _segments(c[1]) for c in b.sim.calls]
    with pytest.raises(ValueError, match="action 'push'"):
        skills.execute(_Robot(), (START, END, START_E, END_E), "push")
    with pytest.raises(ValueError, match="2 names for 3 envs"):
        skills.execute(_Robot(), (START, END, START_E, END_E), ["pour", "open"])
    with pytest.raises(ValueError, match="decoded"):
        skills.execute(_Robot(), (START, END), "pour")
    assert skills.WAIT_STEPS == 50 and skills.LINE_STEPS == 15
