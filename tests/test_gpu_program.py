"""GPU tests of the motion programs (ps_motion_program, Panda.run) in the four
scenes k_motion_program is compiled for.

The yardstick is the project's own sequence of Panda.move / grasp / release
calls (and sim.step() for a wait), which tests/test_gpu_motion.py pins against
the oracle; test_chunk_independence and test_neighbour_independence there
establish that an env's bits depend neither on how its control steps are split
over launches nor on its neighbours.  A program must therefore leave the bits
of the sequence: every comparison here is torch.equal.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_motion_cpu import MOVE_DISTANCES, SCENES, SCHED_B, SCHED_SEED, move_goals

pytestmark = pytest.mark.gpu

B = SCHED_B  # 100: one full wave and a ragged one
MOVE, GRASP, RELEASE, WAIT = 0, 1, 2, 3


def make_robot(task, n=B, seed=SCHED_SEED):
    """A fused env's sim with a Cartesian Panda's primitives on it."""
    from pandasim.envs import PandaVecEnv
    from pandasim.panda_cartesian import Panda

    env = PandaVecEnv(task, "sparse", "ee", n, "cuda", autoreset=False)
    env.reset(seed=seed)
    robot = object.__new__(Panda)
    robot.sim, robot.block_gripper, robot._plan = env.sim, bool(env.sim.cfg.block_gripper), None
    return robot


def schedule(sim, n_moves=4):
    """Per-env goals of n_moves moves in a row: the first is test_motion_cpu's
    schedule from the start (0.02 to 0.10 m, angles (-180, 0, 0) +- 15 degrees,
    its seed); each later one lies MOVE_DISTANCES[(i + 3 k) % 8] from the goal
    before it, so an env's step counts (20 and 2 to 7) differ per segment and
    within a wave.  -> [(goal_pos [B, 3], goal_euler [B, 3])] on the device."""
    n = sim.num_envs
    at = sim.get_link_position("panda", 11).double().cpu().numpy()
    out = []
    for k in range(n_moves):
        goal, euler = move_goals(at, seed=9 + k)
        if k:
            rng = np.random.default_rng(100 + k)
            u = rng.normal(size=(n, 3))
            u[:, 2] = np.abs(u[:, 2]) * (1 if k % 2 else -0.3)
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            d = np.array([MOVE_DISTANCES[(i + 3 * k) % len(MOVE_DISTANCES)] for i in range(n)])
            goal = (at + u * d[:, None]).astype(np.float32).astype(np.float64)
        out.append((torch.from_numpy(goal.astype(np.float32)).cuda(), torch.from_numpy(euler.astype(np.float32)).cuda()))
        at = goal
    return out


def full_segments(sim):
    """[move, move, grasp, move, release(0.01), move]"""
    g = schedule(sim)
    return [("move", *g[0]), ("move", *g[1]), ("grasp",), ("move", *g[2]), ("release", 0.01), ("move", *g[3])]


def build(robot, segments, masks=None):
    from pandasim.panda_cartesian import MotionProgram

    p = MotionProgram(robot.sim.num_envs, robot.sim.device)
    for s, seg in enumerate(segments):
        getattr(p, seg[0])(*seg[1:], mask=None if masks is None else masks[s])
    return p


def run_sequence(robot, segments, masks=None):
    """The segments as Panda calls, one by one (a wait: sim.step() calls) ->
    the control steps each env ran, from the plans' num_steps."""
    steps = torch.zeros(robot.sim.num_envs, dtype=torch.int32, device=robot.sim.device)
    for s, seg in enumerate(segments):
        m = None if masks is None else masks[s]
        if seg[0] == "wait":
            assert m is None
            for _ in range(seg[1]):
                robot.sim.step()
            steps += seg[1]
        else:
            getattr(robot, seg[0])(*seg[1:], mask=m)
            steps += robot._plan.num_steps
    return steps


def snapshot(robot):
    torch.cuda.synchronize()
    return robot.sim.state.clone(), robot._plan.buf.clone()


def restart(robot, state0, blocked):
    robot.sim.state.copy_(state0)
    robot._plan, robot.block_gripper = None, blocked
    robot.sim._call("ps_mark_motor_rows_dirty", robot.sim._ctx)


def columns(sim, state):
    """Every state row as raw words per env: [rows, B] int64."""
    lay, stride, n = sim.layout, sim.layout.stride, sim.num_envs
    f = state[lay.float_offset:lay.goal_offset].view(torch.int32).view(-1, stride)[:, :n].long()
    g = state[lay.goal_offset:lay.elapsed_offset].view(torch.int64).view(-1, stride)[:, :n]
    e = state[lay.elapsed_offset:].view(torch.int32).view(-1, stride)[:, :n].long()
    return torch.cat([f, g, e])


def plan_columns(sim, buf):
    """(f64 rows as words [14, B], i32 rows [4, B]) of a plan buffer."""
    stride, n = sim.layout.stride, sim.num_envs
    split = 14 * stride * 8
    return (buf[:split].view(torch.int64).view(14, stride)[:, :n], buf[split:].view(torch.int32).view(4, stride)[:, :n])


# --------------------------------------------------------- program = sequence
@pytest.mark.parametrize("task", SCENES)
def test_program_equals_sequence(task):
    """[move, move, grasp, move, release(0.01), move] with per-env goals: the
    whole state tensor and the plan buffer equal those of the same calls made
    one by one from the same state; steps is the sum of the primitives'
    num_steps per env; completed is 6.  The same program twice from the same
    state gives the same bits."""
    robot = make_robot(task)
    sim, blocked0 = robot.sim, robot.block_gripper
    state0 = sim.state.clone()
    segments = full_segments(sim)
    want_steps = run_sequence(robot, segments)
    want, flag = snapshot(robot), robot.block_gripper
    assert not torch.equal(want[0], state0)
    got = []
    for _ in range(2):
        restart(robot, state0, blocked0)
        completed, steps = robot.run(build(robot, segments))
        got.append(snapshot(robot))
        assert robot.block_gripper is flag is False
        assert torch.equal(steps, want_steps) and (completed == 6).all()
    per_wave = want_steps[:64]
    print(task, "control steps per env: min", int(want_steps.min()), "max", int(want_steps.max()),
          "distinct in wave 0:", len(set(per_wave.tolist())))
    assert len(set(per_wave.tolist())) >= 8  # ragged within a wave
    assert torch.equal(got[0][0], want[0]) and torch.equal(got[0][1], want[1])
    assert torch.equal(got[1][0], got[0][0]) and torch.equal(got[1][1], got[0][1])


@pytest.mark.parametrize("task", SCENES)
def test_masks(task):
    """A random [S, B] mask: env 7 is masked out of every segment and keeps
    its state and plan bits; envs 1, 65 and 66 start at a later segment; the
    state equals the sequence's with the same per-call masks.  The plan's f64
    rows and kind do too; num_steps, done and blocked are compared where the
    last segment ran (in the sequence a masked plan call zeroes the first two
    and Panda.move writes the whole batch's blocked row; the program keeps the
    env's last segment that ran)."""
    robot = make_robot(task)
    sim, blocked0 = robot.sim, robot.block_gripper
    state0 = sim.state.clone()
    segments = full_segments(sim)
    S = len(segments)
    rng = np.random.default_rng(77)
    mask = (rng.uniform(size=(S, B)) < 0.6).astype(np.uint8)
    mask[:, 7] = 0
    mask[0, [1, 65]] = 0
    mask[:3, 66] = 0
    mask[3:, 66] = 1
    mask[:, 0] = 1
    masks = [torch.from_numpy(mask[s]).cuda() for s in range(S)]
    want_steps = run_sequence(robot, segments, masks)
    want = snapshot(robot)
    restart(robot, state0, blocked0)
    completed, steps = robot.run(build(robot, segments, masks))
    got = snapshot(robot)
    assert torch.equal(steps, want_steps) and (completed == S).all() and int(steps[7]) == 0
    assert torch.equal(got[0], want[0])
    assert torch.equal(columns(sim, got[0])[:, 7], columns(sim, state0)[:, 7])
    (gd, gn), (wd, wn) = plan_columns(sim, got[1]), plan_columns(sim, want[1])
    ran = torch.from_numpy(mask.any(0)).cuda()
    last = torch.from_numpy(mask[S - 1] != 0).cuda()
    assert torch.equal(gd, wd) and torch.equal(gn[3], wn[3])
    assert torch.equal(gn[:3, last], wn[:3, last])
    assert (gd[:, 7] == 0).all() and (gn[:, 7] == 0).all()  # never planned
    assert torch.equal(gn[0, ran], gn[1, ran]) and (gn[0, ran] > 0).all()  # done == num_steps of the last that ran


def copy_env(src, j, dst):
    """env j of src's state into env 0 of dst's."""
    for name in ("f", "goal", "rng"):
        getattr(dst, name)[:, 0] = getattr(src, name)[:, j]
    dst.elapsed[0] = src.elapsed[j]


@pytest.mark.parametrize("task", SCENES)
def test_alone_equals_in_batch(task):
    """Envs 0, 63, 64 and 99 of the batch end with the bits of the same env
    run as a batch of one."""
    robot = make_robot(task)
    sim = robot.sim
    state0 = sim.state.clone()
    segments = full_segments(sim)
    robot.run(build(robot, segments))
    batch = columns(sim, snapshot(robot)[0])
    one = make_robot(task, n=1)
    for j in (0, 63, 64, 99):
        restart(robot, state0, robot.block_gripper)
        one._plan, one.block_gripper = None, bool(sim.cfg.block_gripper)
        copy_env(sim, j, one.sim)
        one.sim._call("ps_mark_motor_rows_dirty", one.sim._ctx)
        own = [tuple(a[j:j + 1].clone() if torch.is_tensor(a) else a for a in seg) for seg in segments]
        completed, _ = one.run(build(one, own))
        alone = columns(one.sim, snapshot(one)[0])
        assert int(completed[0]) == len(segments)
        assert torch.equal(alone[:, 0], batch[:, j]), (task, j)


# ----------------------------------------------------------------------- wait
@pytest.mark.parametrize("task", SCENES)
def test_wait_equals_sim_steps(task):
    """[move, wait(5)] against Panda.move and five sim.step() calls, and
    wait(5) as a launch of its own after a move in an earlier one: the same
    state bits (ps_motion_run leaves ps_step's gains in the state, which
    sim.step() reads; the program's wait takes them as constants)."""
    robot = make_robot(task)
    sim, blocked0 = robot.sim, robot.block_gripper
    state0 = sim.state.clone()
    move = ("move", *schedule(sim, 1)[0])
    want_steps = run_sequence(robot, [move, ("wait", 5)])
    want = snapshot(robot)
    restart(robot, state0, blocked0)
    completed, steps = robot.run(build(robot, [move, ("wait", 5)]))
    got = snapshot(robot)
    diff = (sim.f[:, :B] - want[0][:sim.layout.goal_offset].view(torch.float32).view(-1, sim.layout.stride)[:, :B]).abs()
    print(task, "wait: largest difference of a float row against move + 5 sim.step():", float(diff.max()))
    assert torch.equal(steps, want_steps) and (completed == 2).all()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])  # the plan holds the move, done
    restart(robot, state0, blocked0)
    robot.run(build(robot, [move]))
    completed, steps = robot.run(build(robot, [("wait", 5)]))
    again = snapshot(robot)
    assert (steps == 5).all() and (completed == 1).all()
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])


# ------------------------------------------------------------ the raw entry point
def raw(sim, plan, kinds, waits, blocked0, pos, quat, width=None, mask=None, completed=None, steps=None, over=()):
    """ps_motion_program itself; `over` replaces arguments by name (ctx, state, plan, kinds, waits, pos, quat, S)."""
    from pandasim.sim import _ptr

    over = dict(over)
    S = over.pop("S", len(kinds))
    a = dict(ctx=sim._ctx, state=_ptr(sim.state), plan=_ptr(plan.buf),
             kinds=(C.c_int32 * len(kinds))(*kinds), waits=None if waits is None else (C.c_int32 * len(waits))(*waits),
             pos=_ptr(pos), quat=_ptr(quat))
    a.update(over)
    with torch.cuda.device(sim.device):
        return sim._lib.ps_motion_program(a["ctx"], a["state"], a["plan"], S, a["kinds"], a["waits"], blocked0, a["pos"],
                                          a["quat"], _ptr(width), _ptr(mask), _ptr(completed), _ptr(steps), sim._stream())


def raw_inputs(sim):
    g = schedule(sim, 3)
    pos = torch.stack([g[0][0], g[1][0], g[2][0]]).contiguous()
    quat = sim.euler_xyz_to_quat(torch.stack([g[0][1], g[1][1], g[2][1]])).contiguous()
    return pos, quat


@pytest.mark.parametrize("task", ["reach", "pick_and_place"])
def test_non_finite_goal_stops_the_env(task):
    """Three moves; the third's goal position is NaN (env 3) or infinite (env
    70), its quaternion zero (env 5) or NaN (env 98): those envs report
    completed == 2 and hold the two-move program's bits, state and plan;
    every other env holds the three-move program's."""
    robot = make_robot(task)
    sim, blocked0 = robot.sim, int(robot.block_gripper)
    state0 = sim.state.clone()
    pos, quat = raw_inputs(sim)

    def run(S, p, q):
        sim.state.copy_(state0)
        plan = sim.motion_plan()
        completed = torch.full((B,), -7, dtype=torch.int32, device=sim.device)
        steps = torch.full((B,), -7, dtype=torch.int32, device=sim.device)
        assert raw(sim, plan, [MOVE] * S, None, blocked0, p, q, completed=completed, steps=steps) == 0
        torch.cuda.synchronize()
        return columns(sim, sim.state.clone()), plan_columns(sim, plan.buf.clone()), completed, steps

    full, two = run(3, pos, quat), run(2, pos, quat)
    bad_pos, bad_quat = pos.clone(), quat.clone()
    bad_pos[2, 3, 1] = float("nan")
    bad_pos[2, 70, 0] = float("inf")
    bad_quat[2, 5] = 0.0
    bad_quat[2, 98, 3] = float("nan")
    got = run(3, bad_pos, bad_quat)
    stopped = torch.zeros(B, dtype=torch.bool, device=sim.device)
    stopped[[3, 5, 70, 98]] = True
    assert (got[2][stopped] == 2).all() and (got[2][~stopped] == 3).all()
    assert torch.equal(got[3][stopped], two[3][stopped]) and torch.equal(got[3][~stopped], full[3][~stopped])
    assert torch.equal(got[0][:, stopped], two[0][:, stopped]) and torch.equal(got[0][:, ~stopped], full[0][:, ~stopped])
    for k in range(2):
        assert torch.equal(got[1][k][:, stopped], two[1][k][:, stopped])
        assert torch.equal(got[1][k][:, ~stopped], full[1][k][:, ~stopped])
    assert not torch.equal(full[0][:, stopped], two[0][:, stopped])
    # a NaN goal in the env's first segment: nothing of it is touched
    bad_pos[0, 9] = float("nan")
    first = run(3, bad_pos, bad_quat)
    assert int(first[2][9]) == 0 and int(first[3][9]) == 0
    assert torch.equal(first[0][:, 9], columns(sim, state0)[:, 9]) and (first[1][1][:, 9] == 0).all()


def test_refusals_write_nothing():
    """Each PS_ERR_ARG case leaves the sentinel-filled completed and steps,
    the state and the plan buffer as they were."""
    robot = make_robot("pick_and_place")
    sim = robot.sim
    pos, quat = raw_inputs(sim)
    plan = sim.motion_plan()
    plan.buf.fill_(0x5A)
    completed = torch.full((B,), -7, dtype=torch.int32, device=sim.device)
    steps = torch.full((B,), -7, dtype=torch.int32, device=sim.device)
    before = sim.state.clone(), plan.buf.clone()
    k3, w3 = [MOVE, WAIT, MOVE], [0, 5, 0]
    cases = dict(
        null_ctx=dict(ctx=None), null_state=dict(state=None), null_plan=dict(plan=None), null_kinds=dict(kinds=None),
        no_segments=dict(S=0), negative_segments=dict(S=-2),
        too_many=dict(kinds=(C.c_int32 * 33)(*([GRASP] * 33)), waits=(C.c_int32 * 33)(), S=33),
        unknown_kind=dict(kinds=(C.c_int32 * 3)(MOVE, 4, MOVE)), negative_kind=dict(kinds=(C.c_int32 * 3)(MOVE, -1, MOVE)),
        wait_zero=dict(waits=(C.c_int32 * 3)(0, 0, 0)), wait_over=dict(waits=(C.c_int32 * 3)(0, 1001, 0)),
        wait_null=dict(waits=None), null_goal_pos=dict(pos=None), null_goal_quat=dict(quat=None))
    for name, over in cases.items():
        assert raw(sim, plan, k3, w3, 0, pos, quat, completed=completed, steps=steps, over=over) == -1, name
    torch.cuda.synchronize()
    assert torch.equal(sim.state, before[0]) and torch.equal(plan.buf, before[1])
    assert (completed == -7).all() and (steps == -7).all()
    # the same arguments without a fault run; width and the outputs are optional
    assert raw(sim, plan, [GRASP, RELEASE, WAIT], [0, 0, 1], 0, None, None) == 0
    torch.cuda.synchronize()
    assert not torch.equal(sim.state, before[0])


# --------------------------------------------------------------------- stream
def test_runs_on_the_callers_stream():
    """On a side stream, behind a delay and a copy of the inputs queued on
    that stream before the call (the state and the goals it must see), the
    program leaves the default stream's bits for those inputs, not the bits
    for what the buffers held when the call was enqueued."""
    robot = make_robot("pick_and_place")
    sim, blocked0 = robot.sim, robot.block_gripper
    segments = full_segments(sim)
    goal_a, goal_b = segments[0][1].clone(), segments[0][1] + torch.tensor([0.0, 0.01, 0.02], device=sim.device)
    state_b = sim.state.clone()
    robot.release(0.01)  # A: another state
    state_a = snapshot(robot)[0]
    refs = {}
    for name, (state, goal) in dict(a=(state_a, goal_a), b=(state_b, goal_b)).items():
        restart(robot, state, blocked0)
        segments[0][1].copy_(goal)
        robot.run(build(robot, segments))
        refs[name] = snapshot(robot)
    assert not torch.equal(refs["a"][0], refs["b"][0])
    restart(robot, state_a, blocked0)
    segments[0][1].copy_(goal_a)
    program = build(robot, segments)  # holds views of the goal tensors
    robot._motion_plan()
    big = torch.ones(2048, 2048, device=sim.device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1 << 26)
        else:
            for _ in range(64):
                big = torch.mm(big, big).clamp_(max=1.0)
        sim.state.copy_(state_b)
        segments[0][1].copy_(goal_b)
        completed, _ = robot.run(program)
        got = sim.state.clone(), robot._plan.buf.clone()
    s.synchronize()
    torch.cuda.synchronize()
    assert (completed == len(segments)).all()
    assert torch.equal(got[0], refs["b"][0]) and torch.equal(got[1], refs["b"][1])
