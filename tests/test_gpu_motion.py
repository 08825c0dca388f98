"""GPU tests of the fused motion primitives (ps_plan_move / ps_plan_grasp /
ps_plan_release / ps_motion_run; pandasim.panda_cartesian.Panda) in the four
scenes k_motion is compiled for.

The yardstick is tests/test_motion_cpu.py's composition of the fp64 oracle
(oracle_plan_move, oracle_control_step), whose schedule that file judges with
the reference alone.  Bounds and classes are parity_judge's (judge, TOL, LOOSE,
the caps by the plan's gripper).
"""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as R

import oracle as O
from helpers import oracle_config_for, oracle_env_from, quat_err, snapshot
from parity_judge import LOOSE, NOISE_K, TOL, judge
from parity_judge import groups_for as _groups
from test_motion_cpu import (CAP, EE_LINK, HOLD_TF_STEPS, MOVE_STEPS, RELEASE_TF_WIDTH, SCENES, SCHED_B, SCHED_SEED,
                             motion_obs, move_goals, oracle_control_step, oracle_plan_hold, oracle_plan_move,
                             oracle_run)

pytestmark = pytest.mark.gpu

B = SCHED_B  # 100: a partial second wave

# Joint positions and the end effector's orientation after a teacher-forced
# control step, which parity_judge's groups do not hold (they see the arm only
# through the ee position and velocity, so a wrong slerp angle could hide in
# the arm's null space).  An arm joint's error turns every link after it by
# that angle, so the arm joints and the ee link's rotation take parity_judge's
# rotation bound (obj_rot: 1e-4 rad tight, 5e-3 loose); a finger's travel is
# half the width's, so each finger takes the width's bound (2e-4 m, 1e-2 m).
# Tight samples are held to the tight values; samples the judge puts at an
# ill-conditioned or bifurcated step, to the loose ones.
def _joint_bounds(cls):
    t = TOL["pick_and_place"] if cls == "tight" else LOOSE
    return dict(arm=t["obj_rot"], finger=t["width"], ee_rot=t["obj_rot"])


def _joint_errors(cfg, e_oracle, e_gpu):
    qo, qg = np.array(e_oracle.q), np.array(e_gpu.q)
    ro, rg = (R.from_quat(O.link_state(cfg, e, EE_LINK)[1]) for e in (e_oracle, e_gpu))
    return dict(arm=float(np.abs(qg[:7] - qo[:7]).max()), finger=float(np.abs(qg[7:] - qo[7:]).max()),
                ee_rot=float((rg * ro.inv()).magnitude()))


@pytest.fixture(scope="module")
def ps():
    import pandasim

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return pandasim


def make_sim(task, n=B, seed=SCHED_SEED):
    from pandasim.envs import PandaVecEnv

    env = PandaVecEnv(task, "sparse", "ee", n, "cuda", autoreset=False)
    env.reset(seed=seed)
    return env.sim


def starts_of(sim):
    return sim.get_link_position("panda", EE_LINK).double().cpu().numpy()


def quats_of(sim, euler):
    return sim.euler_xyz_to_quat(torch.from_numpy(np.asarray(euler, np.float32)))


def plan_schedule_move(sim, plan, blocked, mask=None):
    goal, euler = move_goals(starts_of(sim))
    plan.blocked.fill_(int(blocked))
    sim.plan_move(plan, torch.from_numpy(goal.astype(np.float32)), quats_of(sim, euler), mask)
    return goal, euler


# ---------------------------------------------------------------------- plan
@pytest.mark.parametrize("task", SCENES)
def test_plan_matches_the_fp64_composition(ps, task):
    """ps_plan_move against oracle_plan_move from a snapshot: num_steps exactly
    (the schedule's goals are >= 1e-4 m from the branch points; the fp32 FK's
    start is within TOL's 2e-5 m of the oracle's), delta within 2e-5 / num_steps,
    finger_width exactly (the sum of two f32 values in fp64), the start
    quaternion within TOL's 1e-4 up to sign, start within 2e-5 m; masked envs
    get no steps; ps_plan_grasp / ps_plan_release set 30 steps, the blocked
    flag and the width."""
    sim = make_sim(task)
    cfg = oracle_config_for(sim.cfg)
    snap = snapshot(sim)
    plan = sim.motion_plan()
    mask = np.ones(B, np.uint8)
    mask[::7] = 0
    goal, euler = plan_schedule_move(sim, plan, True, mask)
    d, n = plan.d[:, :B].cpu().numpy(), plan.n[:, :B].cpu().numpy()
    worst = dict(start=0.0, delta=0.0, quat=0.0)
    for i in range(B):
        if not mask[i]:
            assert n[0, i] == 0 and n[1, i] == 0
            continue
        ref = oracle_plan_move(cfg, oracle_env_from(cfg, snap, i), goal[i], euler[i])
        assert n[0, i] == ref["num"] == MOVE_STEPS[i % len(MOVE_STEPS)], i
        assert (n[1, i], n[2, i], n[3, i]) == (0, 1, 0)
        worst["start"] = max(worst["start"], np.abs(d[0:3, i] - ref["start"]).max())
        worst["delta"] = max(worst["delta"], np.abs(d[3:6, i] - ref["delta"]).max() * ref["num"])
        assert d[6, i] == ref["width"]
        worst["quat"] = max(worst["quat"], quat_err(d[7:11, i][None], ref["start_quat"][None])[0])
        # the slerp's end: R_start exp(rotvec) is the goal rotation
        end = R.from_quat(d[7:11, i]) * R.from_rotvec(d[11:14, i])
        assert (end * R.from_euler("xyz", euler[i], degrees=True).inv()).magnitude() <= 1e-6
        assert np.linalg.norm(d[11:14, i]) <= np.pi
    print(task, "plan vs fp64 composition", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["start"] <= TOL[task]["ee_pos"] and worst["delta"] <= TOL[task]["ee_pos"]
    assert worst["quat"] <= 1e-4  # parity_judge's tight rotation bound
    sim.plan_grasp(plan, torch.from_numpy(mask))
    n = plan.n[:, :B].cpu().numpy()
    assert (n[0][mask == 1] == 30).all() and (n[0][mask == 0] == 0).all() and (n[1] == 0).all()
    assert (n[2] == 1).all() and (n[3][mask == 1] == 1).all()  # masked envs keep blocked = 1 from the move
    assert (plan.d[6, :B].cpu().numpy()[mask == 1] == 1.0).all()
    w = torch.linspace(0.0, 0.05, B)
    sim.plan_release(plan, w, None)
    n = plan.n[:, :B].cpu().numpy()
    assert (n[0] == 30).all() and (n[2] == 0).all() and (n[3] == 1).all()
    assert np.array_equal(plan.d[6, :B].cpu().numpy(), w.double().numpy())
    sim.plan_release(plan, None, None)
    assert (plan.d[6, :B].cpu().numpy() == 1.0).all()


# ------------------------------------------- teacher-forced against the oracle
@pytest.mark.parametrize("task", SCENES)
def test_motion_parity_teacher_forced(ps, monkeypatch, task):
    """ps_motion_run(max_steps = 1) against one composed oracle control step
    from the same snapshot, per env: the move schedule of test_motion_cpu
    (goals 0.02 to 0.10 m away, goal angles (-180, 0, 0) +- 15 degrees, 2 to 20
    control steps), then the first 5 control steps of release
    (RELEASE_TF_WIDTH, see test_motion_cpu) and of grasp.  The oracle's plan is
    made from the snapshot at plan time.  Classified by parity_judge.judge over
    ee position and velocity, width and the objects' pose and velocity; no
    sample beyond the tight bounds, bifurcated ones within LOOSE, not-tight
    counts within the cap of the plan's gripper.  Every sample's nine joint
    positions and ee orientation are held to _joint_bounds of its class."""
    sim = make_sim(task)
    cfg = oracle_config_for(sim.cfg)
    groups = _groups(task, 7)
    plan = sim.motion_plan()
    scene_blocked = bool(sim.cfg.block_gripper)
    report = {}
    for phase, blocked in (("move", scene_blocked), ("release", False), ("grasp", True)):
        snap0 = snapshot(sim)
        if phase == "move":
            goal, euler = plan_schedule_move(sim, plan, blocked)
            ref = [oracle_plan_move(cfg, oracle_env_from(cfg, snap0, i), goal[i], euler[i]) for i in range(B)]
            steps = max(MOVE_STEPS)
        elif phase == "release":
            sim.plan_release(plan, RELEASE_TF_WIDTH)
            ref, steps = [oracle_plan_hold(RELEASE_TF_WIDTH)] * B, HOLD_TF_STEPS
        else:
            sim.plan_grasp(plan)
            ref, steps = [oracle_plan_hold(1.0)] * B, HOLD_TF_STEPS
        num = plan.num_steps.cpu().numpy()
        assert [r["num"] for r in ref] == list(num)
        counts = {"tight": 0, "conditioned": 0, "bif": 0, "beyond": 0}
        worst, worst_bif, beyond = {k: 0.0 for k in groups}, {k: 0.0 for k in groups}, []
        worst_j, bad_j = dict(arm=0.0, finger=0.0, ee_rot=0.0), []
        for s in range(1, steps + 1):
            snap = snapshot(sim)
            sim.motion_run(plan, 1)
            after = snapshot(sim)
            assert np.array_equal(plan.done.cpu().numpy(), np.minimum(s, num))
            for i in range(B):
                if s > num[i]:
                    assert np.array_equal(after["f"][:, i], snap["f"][:, i])  # a finished env keeps its bits
                    continue

                def step(c, e, act, autoreset=False, stats=None, i=i, s=s):
                    oracle_control_step(c, e, ref[i], s, blocked)
                    return (motion_obs(c, e),)

                with monkeypatch.context() as m:
                    m.setattr(O, "step", step)
                    e = oracle_env_from(cfg, snap, i)
                    o = O.step(cfg, e, None)[0]
                    e_gpu = oracle_env_from(cfg, after, i)
                    og = motion_obs(cfg, e_gpu)
                    cls, errs = judge(cfg, snap, i, None, o, og, groups, task)
                counts[cls] += 1
                jerr, jb = _joint_errors(cfg, e, e_gpu), _joint_bounds(cls)
                for k, v in jerr.items():
                    if cls == "tight":
                        worst_j[k] = max(worst_j[k], v)
                    if v > jb[k]:
                        bad_j.append((s, i, cls, k, f"{v:.2e}"))
                for k, err in errs.items():
                    (worst_bif if cls == "bif" else worst)[k] = max((worst_bif if cls == "bif" else worst)[k], err)
                if cls == "beyond":
                    beyond.append((s, i, {k: f"{v:.2e}" for k, v in errs.items()}))
        total = sum(counts.values())
        report[phase] = counts
        print(task, phase, counts, "worst", {k: f"{v:.2e}" for k, v in worst.items()}, "ill-conditioned worst",
              {k: f"{v:.2e}" for k, v in worst_bif.items()}, "joints and ee rotation of tight samples",
              {k: f"{v:.2e}" for k, v in worst_j.items()}, "beyond", beyond[:8], "joints beyond", bad_j[:8])
        assert total == int(np.minimum(num, steps).sum())
        assert not beyond
        assert not bad_j, bad_j[:8]
        for k, v in worst_bif.items():
            assert v <= LOOSE[k], (k, v)
        assert counts["bif"] + counts["conditioned"] <= CAP[blocked] * total


# ------------------------------------------------------------ independence
def _run_chunks(sim, state0, plan_fn, chunks):
    sim.state.copy_(state0)
    plan = sim.motion_plan()
    plan_fn(plan)
    for c in chunks:
        sim.motion_run(plan, c)
    torch.cuda.synchronize()
    return sim.state.clone(), plan.buf.clone()


@pytest.mark.parametrize("task", SCENES)
def test_chunk_independence(ps, task):
    """One launch of n control steps, n launches of one and launches of 3 +
    (n - 3) leave the same state buffer and plan, bit for bit: the move
    schedule (n = 20, envs finishing after 2 to 20 steps) and a grasp after a
    release (n = 30)."""
    sim = make_sim(task)
    state0 = sim.state.clone()
    goal, euler = move_goals(starts_of(sim))
    gp, gq = torch.from_numpy(goal.astype(np.float32)), quats_of(sim, euler)

    def move(plan):
        sim.plan_move(plan, gp, gq)

    n = max(MOVE_STEPS)
    one = _run_chunks(sim, state0, move, [n])
    assert not torch.equal(one[0], state0)
    for chunks in ([1] * n, [3, n - 3]):
        got = _run_chunks(sim, state0, move, chunks)
        assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1]), chunks
    again = _run_chunks(sim, state0, move, [n, 5])  # nothing left: a further launch changes nothing
    assert torch.equal(again[0], one[0]) and torch.equal(again[1], one[1])
    sim.state.copy_(state0)
    plan = sim.motion_plan()
    sim.plan_release(plan, 0.02)
    sim.motion_run(plan, 3)
    state1 = sim.state.clone()
    one = _run_chunks(sim, state1, lambda p: sim.plan_grasp(p), [30])
    for chunks in ([1] * 30, [3, 27]):
        got = _run_chunks(sim, state1, lambda p: sim.plan_grasp(p), chunks)
        assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1]), chunks


@pytest.mark.parametrize("task", SCENES)
def test_neighbour_independence(ps, task):
    """Step counts 2, 3, 7 and 20 interleaved over the lanes of each wave, every
    fifth env masked off, against each count run as a uniform batch from the
    same states with the same goals: every env's state bits are those of its
    count's uniform batch; masked envs keep their bits."""
    counts, dist = (2, 3, 7, 20), (0.0305, 0.0325, 0.10, 0.02)
    sim = make_sim(task)
    state0 = sim.state.clone()
    starts = starts_of(sim)
    rng = np.random.default_rng(21)
    u = rng.normal(size=(B, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    euler = np.array([-180.0, 0.0, 0.0]) + rng.uniform(-15, 15, size=(B, 3))
    gq = quats_of(sim, euler)
    goals = [torch.from_numpy((starts + u * d).astype(np.float32)) for d in dist]
    which = np.arange(B) % 4
    mask = torch.from_numpy((np.arange(B) % 5 != 0).astype(np.uint8))
    mixed_goal = torch.stack([goals[which[i]][i] for i in range(B)])
    plans = {}

    def run(goal, m):
        sim.state.copy_(state0)
        plan = sim.motion_plan()
        sim.plan_move(plan, goal, gq, m)
        plans["last"] = plan.num_steps.cpu().numpy().copy()
        sim.motion_run(plan, 20)
        torch.cuda.synchronize()
        assert torch.equal(plan.done, plan.num_steps)
        return sim.state.clone()

    mixed = run(mixed_goal, mask)
    assert np.array_equal(plans["last"], np.where(mask.numpy() == 1, np.array(counts)[which], 0))
    lay, stride = sim.layout, sim.layout.stride

    def columns(state):
        """[rows, B] of every state row as raw bytes per env."""
        f = state[lay.float_offset:lay.goal_offset].view(torch.int32).view(-1, stride)[:, :B]
        g = state[lay.goal_offset:lay.elapsed_offset].view(torch.int64).view(-1, stride)[:, :B]
        e = state[lay.elapsed_offset:].view(torch.int32).view(-1, stride)[:, :B]
        return f.cpu().numpy(), g.cpu().numpy(), e.cpu().numpy()

    cm, c0 = columns(mixed), columns(state0)
    for k, c in enumerate(counts):
        uniform = run(goals[k], None)
        assert (plans["last"] == c).all()
        cu = columns(uniform)
        sel = (which == k) & (mask.numpy() == 1)
        assert sel.sum() >= 15
        for a, b in zip(cm, cu):
            diff = (a[:, sel] != b[:, sel]).any(0)
            assert not diff.any(), (task, c, np.flatnonzero(sel)[diff])
    off = mask.numpy() == 0
    for a, b in zip(cm, c0):
        assert np.array_equal(a[:, off], b[:, off])
    assert any(not np.array_equal(a[:, ~off], b[:, ~off]) for a, b in zip(cm, c0))


@pytest.mark.parametrize("task", SCENES)
def test_neighbour_independence_of_kind_and_gripper(ps, task):
    """The lanes of a wave hold, interleaved, a move with a free gripper, a
    move with a blocked one, a release and a grasp (k_motion branches per lane
    on the plan's kind and blocked flag; 2 to 30 control steps).  Every env's
    state bits are those of the batch in which all envs run its own kind."""
    sim = make_sim(task)
    plan0 = sim.motion_plan()  # fingers off their limits first: three control steps of a small release
    sim.plan_release(plan0, 0.01)
    sim.motion_run(plan0, 3)
    state0 = sim.state.clone()
    goal, euler = move_goals(starts_of(sim))
    gp, gq = torch.from_numpy(goal.astype(np.float32)), quats_of(sim, euler)

    def make(kind):
        plan = sim.motion_plan()
        if kind < 2:
            plan.blocked.fill_(kind)
            sim.plan_move(plan, gp, gq)
        elif kind == 2:
            sim.plan_release(plan, 0.01)
        else:
            sim.plan_grasp(plan)
        return plan

    def run(plan):
        sim.state.copy_(state0)
        sim.motion_run(plan, 30)
        torch.cuda.synchronize()
        assert torch.equal(plan.done, plan.num_steps)
        return sim.f[:, :B].clone().view(torch.int32)

    sim.state.copy_(state0)
    plans = [make(k) for k in range(4)]  # all made from state0
    which = torch.arange(B, device=sim.device) % 4
    mixed = sim.motion_plan()
    stride = sim.layout.stride
    sel = torch.arange(stride, device=sim.device) % 4
    for k, p in enumerate(plans):
        mixed.d[:, sel == k] = p.d[:, sel == k]
        mixed.n[:, sel == k] = p.n[:, sel == k]
    assert sorted(set(mixed.n[3, :B].tolist())) == [0, 1] and sorted(set(mixed.n[2, :B].tolist())) == [0, 1]
    got = run(mixed)
    for k, p in enumerate(plans):
        uniform = run(p)
        cols = which == k
        assert torch.equal(got[:, cols], uniform[:, cols]), (task, k)
        assert not torch.equal(uniform[:9, cols], state0[:36 * stride].view(torch.int32).view(9, stride)[:, :B][:, cols])


# ------------------------------------------------------------------ free run
N_FREE = 4  # envs compared with the oracle (each costs five oracle runs)


def _free_run_compare(sim, cfg, task, snap, run_oracle, label):
    """ee position and width of envs 0..N_FREE-1 against the composed oracle's
    run from `snap` (run_oracle(env, i) runs env i's primitives); bound: NOISE_K x the oracle's own spread over four runs
    with one ulp of state noise per substep, floored at TOL's tight values."""
    pos = sim.get_link_position("panda", EE_LINK).double().cpu().numpy()
    width = (sim.f[7, :B] + sim.f[8, :B]).double().cpu().numpy()
    worst = dict(ee_pos=0.0, width=0.0, bound_pos=0.0, bound_width=0.0)
    ok = True
    for i in range(N_FREE):
        e = oracle_env_from(cfg, snap, i)
        run_oracle(e, i)
        p, w = O.link_state(cfg, e, EE_LINK)[0], e.q[7] + e.q[8]
        sp = sw = 0.0
        try:
            for seed in range(1, 5):
                O.set_state_noise(1.0, seed)
                n = oracle_env_from(cfg, snap, i)
                run_oracle(n, i)
                sp = max(sp, np.abs(O.link_state(cfg, n, EE_LINK)[0] - p).max())
                sw = max(sw, abs(n.q[7] + n.q[8] - w))
        finally:
            O.set_state_noise(0.0)
        bp, bw = max(NOISE_K * sp, TOL[task]["ee_pos"]), max(NOISE_K * sw, TOL[task]["width"])
        ep, ew = np.abs(pos[i] - p).max(), abs(width[i] - w)
        if ep / bp >= worst["ee_pos"] / max(worst["bound_pos"], 1e-300):
            worst["ee_pos"], worst["bound_pos"] = ep, bp
        if ew / bw >= worst["width"] / max(worst["bound_width"], 1e-300):
            worst["width"], worst["bound_width"] = ew, bw
        ok = ok and ep <= bp and ew <= bw
    print("MEASURED free run", label, {k: f"{v:.2e}" for k, v in worst.items()})
    return ok, worst


def test_free_run_move_reach(ps):
    """A whole move of 0.06 m with a 30 degree yaw change in the Reach scene
    (4 control steps, gripper blocked), free running."""
    sim = make_sim("reach")
    cfg = oracle_config_for(sim.cfg)
    snap = snapshot(sim)
    goal = (starts_of(sim) + np.array([0.04, -0.04, 0.02])).astype(np.float32)
    euler = np.array([-180.0, 0.0, 30.0])
    plan = sim.motion_plan()
    plan.blocked.fill_(1)
    sim.plan_move(plan, torch.from_numpy(goal), quats_of(sim, euler))
    assert (plan.num_steps == 4).all()
    sim.motion_run(plan, 4)

    pos = sim.get_link_position("panda", EE_LINK).double().cpu().numpy()
    assert np.abs(pos - goal).max() < 0.03  # the arm went there

    def runner(e, i):
        oracle_run(cfg, e, oracle_plan_move(cfg, e, goal[i].astype(np.float64), euler), True)

    ok, worst = _free_run_compare(sim, cfg, "reach", snap, runner, "reach move 0.06 m, 30 deg yaw")
    assert ok, worst


def test_free_run_grasp_release_pick_and_place(ps):
    """PickAndPlace with the cube between the pads: the cube is placed under
    the gripper, the fingers open (release, 3 control steps), the hand moves
    down to the cube (12 control steps), then a whole grasp and a whole
    release, free running; compared after the grasp and after the release."""
    sim = make_sim("pick_and_place")
    cfg = oracle_config_for(sim.cfg)
    start = starts_of(sim)
    sim.set_base_pose("object", torch.from_numpy(np.concatenate([start[:, :2], np.full((B, 1), 0.02)], 1)),
                      [0.0, 0.0, 0.0, 1.0])
    snap = snapshot(sim)
    down = np.concatenate([start[:, :2], np.full((B, 1), 0.02)], 1).astype(np.float32)
    euler = np.array([-180.0, 0.0, 0.0])
    plan = sim.motion_plan()
    sim.plan_release(plan, 1.0)
    sim.motion_run(plan, 3)
    plan.blocked.fill_(0)
    sim.plan_move(plan, torch.from_numpy(down), quats_of(sim, euler))
    n_down = int(plan.num_steps.max())
    assert (plan.num_steps == n_down).all()
    sim.motion_run(plan, n_down)
    sim.plan_grasp(plan)
    sim.motion_run(plan, 30)

    def approach_and_grasp(e, i):
        oracle_run(cfg, e, oracle_plan_hold(1.0), False, last=3)
        oracle_run(cfg, e, oracle_plan_move(cfg, e, down[i].astype(np.float64), euler), False)
        oracle_run(cfg, e, oracle_plan_hold(1.0), True)

    ok1, worst1 = _free_run_compare(sim, cfg, "pick_and_place", snap, approach_and_grasp, "pick_and_place approach + grasp")
    width = (sim.f[7, :B] + sim.f[8, :B]).cpu().numpy()
    assert (width[:N_FREE] > 0.03).all()  # the pads hold the 4 cm cube
    sim.plan_release(plan, 1.0)
    sim.motion_run(plan, 30)

    def runner2(e, i):
        approach_and_grasp(e, i)
        oracle_run(cfg, e, oracle_plan_hold(1.0), False)

    ok2, worst2 = _free_run_compare(sim, cfg, "pick_and_place", snap, runner2, "pick_and_place ... + release")
    assert ok1 and ok2, (worst1, worst2)


# -------------------------------------------------------------------- Python
def test_python_panda_matches_the_raw_calls(ps):
    """panda_cartesian.Panda.move / grasp / release on the plugin path's sim
    leave the state bits of the raw ABI calls; its set_action + sim.step()
    agrees with ps_motion_run(max_steps = 1) of the equivalent hold plan within
    parity_judge.TOL (ee position, width)."""
    from pandasim.panda_cartesian import Panda

    env = ps.make("PandaPickAndPlace-v3", num_envs=B, fused=False)
    env.reset(seed=5)
    sim = env.sim
    robot = Panda(sim, block_gripper=False, base_position=np.array([-0.6, 0.0, 0.0]), control_type="ee")
    state0 = sim.state.clone()
    goal = starts_of(sim) + np.array([0.03, 0.02, -0.04])
    euler = [-175.0, 5.0, 20.0]
    n = robot.move(goal, euler, chunk=4)
    assert n == 4 or n == 3
    assert robot.release(width=0.01) == 30 and robot.block_gripper is False
    assert robot.grasp(mask=torch.arange(B) % 2) == 30 and robot.block_gripper is True
    torch.cuda.synchronize()
    via_robot = sim.state.clone()
    sim.state.copy_(state0)
    plan = sim.motion_plan()
    sim.plan_move(plan, goal, sim.euler_xyz_to_quat(euler))
    sim.motion_run(plan, n)
    sim.plan_release(plan, 0.01)
    sim.motion_run(plan, 30)
    sim.plan_grasp(plan, torch.arange(B) % 2)
    sim.motion_run(plan, 30)
    torch.cuda.synchronize()
    assert torch.equal(sim.state, via_robot)
    # one hold step through the plugin path
    robot.block_gripper = False
    state1 = sim.state.clone()
    w = 0.004
    robot.set_action(torch.tensor([[0.0, 0.0, 0.0, w]]).expand(B, 4), euler_xyz=robot.get_ee_orientation())
    sim.step()
    pos_p, width_p = starts_of(sim), (sim.f[7, :B] + sim.f[8, :B]).double().cpu().numpy()
    sim.state.copy_(state1)
    sim.plan_release(plan, w)
    sim.motion_run(plan, 1)
    pos_f, width_f = starts_of(sim), (sim.f[7, :B] + sim.f[8, :B]).double().cpu().numpy()
    err = dict(ee_pos=np.abs(pos_p - pos_f).max(), width=np.abs(width_p - width_f).max())
    print("plugin set_action + step vs fused hold step", {k: f"{v:.2e}" for k, v in err.items()})
    assert err["ee_pos"] <= TOL["pick_and_place"]["ee_pos"] and err["width"] <= TOL["pick_and_place"]["width"]


def test_motion_run_any_context_and_errors(ps):
    """A joints-control context runs the primitives; NULL buffers and
    max_steps < 1 are PS_ERR_ARG and change nothing."""
    from pandasim.envs import PandaVecEnv
    from pandasim.sim import _ptr

    env = PandaVecEnv("slide", "sparse", "joints", 8, "cuda", autoreset=False)
    env.reset(seed=1)
    sim = env.sim
    plan = sim.motion_plan()
    sim.plan_grasp(plan)
    before = sim.state.clone()
    lib = sim._lib
    assert lib.ps_motion_run(sim._ctx, _ptr(sim.state), _ptr(plan.buf), 0, sim._stream()) == -1
    assert lib.ps_motion_run(sim._ctx, None, _ptr(plan.buf), 1, sim._stream()) == -1
    assert lib.ps_motion_run(sim._ctx, _ptr(sim.state), None, 1, sim._stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(sim.state, before) and int(plan.done.sum()) == 0
    sim.motion_run(plan, 2)
    assert (plan.done == 2).all() and not torch.equal(sim.state, before)
    assert torch.equal(sim.goal, before[sim.layout.goal_offset:sim.layout.rng_offset].view(torch.float64).view(6, -1))
    # the gain rows hold ps_step's values: a fused step needs no ps_mark_motor_rows_dirty
    assert (sim.f[27:36, :8] == 0.1).all() and (sim.f[36:45, :8] == 1.0).all() and (sim.f[45:54, :8] == 0.0).all()
