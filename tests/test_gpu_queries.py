"""GPU tests of the engine-level query kernels behind the plugin path's
pandasim.sim calls (getLinkState, calculateInverseKinematics,
getBasePositionAndOrientation / getEulerFromQuaternion, np_random.uniform):

  * k_link_state on all 12 links against the fp64 oracle, whose velocities
    tests/test_oracle.py ties to finite differences of its own positions;
  * k_ik<LINK>, all 12 instantiations, against the oracle's IK;
  * k_base_state's Euler angles on both sides of both gimbal-lock switches
    against the fp64 formula, its other outputs bit for bit;
  * k_rng_seed / k_rng_uniform / k_rng_rotation bit for bit against numpy's
    own Generator(PCG64(SeedSequence(seed))) and the oracle's goal stream,
    with masks.

Bounds.  Each bound is four times the worst error measured on an MI355X
(the *_MEASURED tables below; every test prints its figures before it
asserts), capped by the ceiling of the quantity: parity_judge._TIGHT for the
link and base states (position 2e-5 m, quaternion and object rotation 1e-4,
velocities 2e-3), test_ik_parity's median 1e-5 / max 2e-3 rad for IK.  The
errors are fp32 rounding of a kinematic chain (no dynamics), and 4 x the
rounding of a sum of at most nine terms is still rounding: the margin is for
another seed, not for another kernel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
from helpers import (DOF_HI, DOF_LO, NEUTRAL_Q, NUM_LINKS, f32, link_sample, oracle_config_for, oracle_env_with,
                     oracle_link_states, quat_err, quat_to_matrix, rotation_branch, snapshot)
from pandasim import _lib as L
from parity_judge import _TIGHT, _obs_err

pytestmark = pytest.mark.gpu

LINKS = list(range(NUM_LINKS))


@pytest.fixture(scope="module")
def ps():
    import pandasim

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return pandasim


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    """Bit pattern of a float32 / float64 tensor (NaN-proof equality)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _bound(measured, ceiling):
    return min(4.0 * measured, ceiling)


def kat_sim(B):
    """The known-answer scene: the robot alone, its base at the origin."""
    from pandasim.sim import PandaSim

    cfg = L.default_config(0, 0, 0)
    cfg.has_table = cfg.has_plane = 0
    cfg.base[0] = 0.0
    return PandaSim(config=cfg, num_envs=B)


def set_joints(sim, q, qd=None):
    sim.set_rows(L.F_Q, torch.from_numpy(np.asarray(q, np.float32)))
    sim.set_rows(L.F_QD, torch.from_numpy(np.asarray(np.zeros_like(q) if qd is None else qd, np.float32)))


# ------------------------------------------------------------ ps_link_state
LINK_CEIL = (_TIGHT["ee_pos"], _TIGHT["obj_rot"], _TIGHT["ee_vel"], _TIGHT["obj_avel"])
# worst |GPU - oracle| on an MI355X per link: position (m), quaternion, linear
# velocity (m/s), angular velocity (rad/s); the asserted bound is 4 x each
LINK_MEASURED = {
    0: (7.63e-09, 9.76e-08, 8.15e-09, 0.0),  # link 0 turns about z: omega = (0, 0, qd[0]) exactly
    1: (2.08e-08, 8.15e-08, 3.20e-08, 1.31e-07),
    2: (6.57e-08, 1.27e-07, 9.34e-08, 1.93e-07),
    3: (6.60e-08, 1.31e-07, 1.44e-07, 2.69e-07),
    4: (1.02e-07, 1.08e-07, 2.80e-07, 3.33e-07),
    5: (9.72e-08, 1.42e-07, 2.97e-07, 4.87e-07),
    6: (1.13e-07, 1.48e-07, 2.72e-07, 5.11e-07),
    7: (9.73e-08, 1.48e-07, 3.43e-07, 5.11e-07),
    8: (1.35e-07, 1.80e-07, 3.71e-07, 5.11e-07),
    9: (1.39e-07, 1.80e-07, 4.19e-07, 5.11e-07),
    10: (1.37e-07, 1.80e-07, 3.72e-07, 5.11e-07),
    11: (1.36e-07, 1.80e-07, 4.90e-07, 5.11e-07),
}
# the same with the base of the registered tasks (-0.6, 0, 0): links 9 and 11
LINK_BASE_MEASURED = {9: (1.39e-07, 1.80e-07, 4.19e-07, 5.11e-07), 11: (1.36e-07, 1.80e-07, 4.90e-07, 5.11e-07)}
SIGN_MARGIN = 1e-4  # fp64 branch predicates this far from switching: the fp32 branch is the same


def _link_state_raw(sim, link, want=(True, True, True, True)):
    """ps_link_state with any subset of its outputs; the others are passed as NULL."""
    B = sim.num_envs
    outs = [torch.full((B, n), float("nan"), device=sim.device) if w else None for n, w in zip((3, 4, 3, 3), want)]
    sim._call("ps_link_state", sim._ctx, _ptr(sim.state), int(link), *[_ptr(o) for o in outs], sim._stream())
    return outs


@pytest.fixture(scope="module")
def link_case(ps):
    """258 envs (four blocks of 64 and a ragged one of 2): the 256
    configurations of helpers.link_sample, the neutral pose and all joints at
    0, in the known-answer scene; the oracle's link states of all 12 links
    from the fp32 state read back."""
    q, qd = link_sample(256, 0)
    q = np.vstack([q, f32(NEUTRAL_Q), np.zeros(9)])
    qd = np.vstack([qd, qd[:2]])
    sim = kat_sim(len(q))
    set_joints(sim, q, qd)
    snap = snapshot(sim)
    qs, qds = snap["f"][L.F_Q:L.F_Q + 9].T, snap["f"][L.F_QD:L.F_QD + 9].T
    assert np.array_equal(qs, q) and np.array_equal(qds, qd)
    cfg = oracle_config_for(sim.cfg)
    ref = {link: oracle_link_states(cfg, qs, qds, link) for link in LINKS}
    return dict(sim=sim, q=qs, qd=qds, ref=ref)


def _link_errors(gpu, ref):
    pos, quat, v, w = [t.cpu().numpy().astype(np.float64) for t in gpu]
    branch, margin = rotation_branch(quat_to_matrix(ref[1]))
    return (np.abs(pos - ref[0]).max(), quat_err(quat, ref[1], margin >= SIGN_MARGIN).max(),
            np.abs(v - ref[2]).max(), np.abs(w - ref[3]).max())


def test_link_sample_reaches_every_rotation_branch(link_case):
    """A condition on the inputs: over the links, each of getRotation's four
    branches (trace > 0, i = 0, 1, 2) is taken by at least 16 samples, and by
    at least 16 whose predicates are SIGN_MARGIN away from switching (the
    samples whose quaternion sign is compared too)."""
    counts, firm = np.zeros(4, int), np.zeros(4, int)
    for link in LINKS:
        branch, margin = rotation_branch(quat_to_matrix(link_case["ref"][link][1]))
        counts += np.bincount(branch, minlength=4)
        firm += np.bincount(branch[margin >= SIGN_MARGIN], minlength=4)
    print(f"getRotation branches (i=0, i=1, i=2, trace>0): {counts}, {SIGN_MARGIN:g} from a switch: {firm}")
    assert counts.min() >= 16 and firm.min() >= 16


@pytest.mark.parametrize("link", LINKS)
def test_link_state_matches_oracle(link_case, link):
    """Position, quaternion, linear and angular velocity of every link's COM
    frame against O.link_state.  Quaternions are compared up to sign, and
    with their sign where the fp64 branch predicates are SIGN_MARGIN from
    switching.  Bound: 4 x LINK_MEASURED[link], at most LINK_CEIL."""
    sim = link_case["sim"]
    err = _link_errors(sim.link_state(link), link_case["ref"][link])
    print(f"MEASURED link_state link={link} pos={err[0]:.3g} quat={err[1]:.3g} v={err[2]:.3g} w={err[3]:.3g}")
    for name, e, m, c in zip(("pos", "quat", "v", "w"), err, LINK_MEASURED[link], LINK_CEIL):
        assert e <= _bound(m, c), (link, name, e, _bound(m, c))


@pytest.mark.parametrize("link", LINKS)
def test_link_state_null_outputs(link_case, link):
    """Each output alone (the other three NULL) carries the bits of the call with all four."""
    sim = link_case["sim"]
    full = _link_state_raw(sim, link)
    assert all(torch.isfinite(t).all() for t in full)
    for k in range(4):
        want = [j == k for j in range(4)]
        one = _link_state_raw(sim, link, want)
        assert [o is not None for o in one] == want
        assert torch.equal(_bits(one[k]), _bits(full[k])), (link, k)
    for a, b in zip(sim.link_state(link), full):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("link", [9, 11])
def test_link_state_base_offset(ps, link_case, link):
    """A registered task's scene (base at (-0.6, 0, 0)): the fp32 base is
    added to the position and to nothing else -- bit for bit the known-answer
    scene's outputs -- and the result agrees with the oracle of that scene."""
    from pandasim.sim import PandaSim

    sim = PandaSim(task="reach", num_envs=len(link_case["q"]))
    base = np.array([sim.cfg.base[k] for k in range(3)], np.float32)
    assert base[0] != 0.0
    set_joints(sim, link_case["q"], link_case["qd"])
    got = sim.link_state(link)
    kat = link_case["sim"].link_state(link)
    assert np.array_equal(got[0].cpu().numpy(), kat[0].cpu().numpy() + base)  # one fp32 add
    for a, b in zip(got[1:], kat[1:]):
        assert torch.equal(_bits(a), _bits(b))
    cfg = oracle_config_for(sim.cfg)
    ref = oracle_link_states(cfg, link_case["q"], link_case["qd"], link)
    assert np.allclose(ref[0] - link_case["ref"][link][0], base.astype(np.float64), atol=1e-12)
    err = _link_errors(got, ref)
    print(f"MEASURED link_state_base link={link} pos={err[0]:.3g} quat={err[1]:.3g} v={err[2]:.3g} w={err[3]:.3g}")
    for name, e, m, c in zip(("pos", "quat", "v", "w"), err, LINK_BASE_MEASURED[link], LINK_CEIL):
        assert e <= _bound(m, c), (link, name, e, _bound(m, c))


# ---------------------------------------------------- ps_inverse_kinematics
IK_CEIL = (1e-5, 2e-3)  # test_ik_parity: median, max (rad; m for the fingers)
IK_PROBE = 1e-6         # m: target moved by this much on each axis, both ways
IK_PROBE_SKIP = 2e-4    # rad: a sample whose oracle answer moves more may be skipped ...
IK_SKIP_CAP = 0.02      # ... at most this share of a link's samples (today: none)
# (median, max) over the samples of max_d |q_gpu - q_oracle| on an MI355X, per link
IK_MEASURED = {
    0: (3.62e-08, 2.44e-07), 1: (7.35e-08, 1.87e-07), 2: (6.51e-08, 3.02e-07), 3: (8.93e-08, 3.76e-07),
    4: (1.14e-07, 3.60e-07), 5: (1.27e-07, 4.56e-07), 6: (1.51e-07, 4.95e-07), 7: (1.51e-07, 4.13e-07),
    8: (1.49e-07, 4.21e-07), 9: (1.68e-07, 4.05e-07), 10: (1.72e-07, 4.55e-07), 11: (1.40e-07, 6.56e-07),
}
IK_EXTRA_MEASURED = {
    (9, "negated"): (2.28e-07, 5.16e-07), (9, "scaled"): (1.83e-07, 6.64e-07),
    (9, "far_turn"): (3.13e-07, 2.50e-06), (9, "far_target"): (1.69e-07, 4.96e-07),
    (11, "negated"): (2.44e-07, 5.21e-07), (11, "scaled"): (1.58e-07, 7.78e-07),
    (11, "far_turn"): (2.98e-07, 3.39e-06), (11, "far_target"): (1.47e-07, 5.07e-07),
}


def _ik_untouched(link):
    """DoFs that cannot move `link`: arm joints above it, the fingers unless it is one, then the other finger."""
    arm = list(range(link + 1, 7)) if link <= 5 else []
    return arm + {9: [8], 10: [7]}.get(link, [7, 8])


def _ik_inputs(cfg, link, n, rng):
    """Start joints inside the limits and a target pose: O.link_state's of a
    second configuration (arm joints moved by U(-0.3, 0.3), fingers by
    U(-0.01, 0.01) clipped to their range); all rounded to fp32."""
    q0 = f32(DOF_LO + (DOF_HI - DOF_LO) * rng.uniform(0.1, 0.9, (n, 9)))
    q1 = q0 + np.concatenate([rng.uniform(-0.3, 0.3, (n, 7)), rng.uniform(-0.01, 0.01, (n, 2))], axis=1)
    q1[:, 7:] = np.clip(q1[:, 7:], 0.0, 0.04)
    pos, quat, _, _ = oracle_link_states(cfg, q1, np.zeros_like(q1), link)
    return q0, f32(pos), f32(quat)


def _ik_oracle(cfg, q0, link, pos, orn):
    return np.array([O.inverse_kinematics(cfg, q0[i], link, pos[i], orn[i]) for i in range(len(q0))])


def _ik_probe(cfg, q0, link, pos, orn, ref):
    """Largest move [n] of the oracle's answer when the target moves by +-IK_PROBE on one axis."""
    move = np.zeros(len(q0))
    for axis in range(3):
        for sign in (-1.0, 1.0):
            p = pos.copy()
            p[:, axis] += sign * IK_PROBE
            move = np.maximum(move, np.abs(_ik_oracle(cfg, q0, link, p, orn) - ref).max(axis=1))
    return move


def _ik_check(sim, cfg, link, q0, pos, orn, measured, tag):
    """GPU IK against the oracle's on the same fp32 inputs: untouched DoFs bit
    for bit, the others within 4 x measured (median and max over the samples,
    capped by IK_CEIL) on every sample the probe does not mark."""
    set_joints(sim, q0)
    snap = snapshot(sim)
    qs = snap["f"][L.F_Q:L.F_Q + 9].T
    assert np.array_equal(qs, q0)
    got = sim.inverse_kinematics("panda", link, torch.from_numpy(pos), torch.from_numpy(orn)).cpu().numpy()
    assert np.isfinite(got).all()
    ref = _ik_oracle(cfg, qs, link, pos, orn)
    still = _ik_untouched(link)
    assert np.array_equal(got[:, still], q0[:, still].astype(np.float32)), (link, tag)
    assert np.array_equal(ref[:, still], q0[:, still])
    moved = [d for d in range(9) if d not in still]
    assert np.abs(ref[:, moved] - q0[:, moved]).max(axis=0).min() > 1e-4  # every other DoF does move
    move = _ik_probe(cfg, qs, link, pos, orn, ref)
    skip = move > IK_PROBE_SKIP
    assert skip.mean() <= IK_SKIP_CAP, (link, tag, int(skip.sum()))
    err = np.abs(got.astype(np.float64) - ref).max(axis=1)[~skip]
    print(f"MEASURED ik link={link} {tag} median={np.median(err):.3g} max={err.max():.3g} "
          f"probe_move={move.max():.3g} skipped={int(skip.sum())}")
    assert np.median(err) <= _bound(measured[0], IK_CEIL[0]), (link, tag, np.median(err))
    assert err.max() <= _bound(measured[1], IK_CEIL[1]), (link, tag, err.max())
    return got, ref


@pytest.fixture(scope="module")
def ik_scene(ps):
    """A registered task's scene (the base is not at the origin: the kernel
    takes it off the target), 128 envs; and one of 130 for the extra cases."""
    from pandasim.sim import PandaSim

    sims = {B: PandaSim(task="reach", num_envs=B) for B in (128, 130)}
    return sims, oracle_config_for(sims[128].cfg)


@pytest.fixture(scope="module")
def ik_samples(ik_scene):
    rng = np.random.default_rng(1)
    return {link: _ik_inputs(ik_scene[1], link, 128, rng) for link in LINKS}


@pytest.mark.parametrize("link", LINKS)
def test_ik_matches_oracle(ik_scene, ik_samples, link):
    """All 12 instantiations of k_ik (system sizes 1..7, and 8 with the finger
    column of links 9 and 10) on position and orientation targets.

    With the oracle alone: moving the target by +-1e-6 m on an axis moves its
    answer by at most 3.5e-6 rad on these inputs, so no sample hangs on the
    1e-4 m stopping rule (the damped solve runs its 20 iterations) and none
    is skipped; the probe stays as a guard for another seed."""
    sims, cfg = ik_scene
    q0, pos, orn = ik_samples[link]
    _ik_check(sims[128], cfg, link, q0, pos, orn, IK_MEASURED[link], "base")


def _quat_mul(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


@pytest.mark.parametrize("case", ["negated", "scaled", "far_turn", "far_target"])
@pytest.mark.parametrize("link", [9, 11])
def test_ik_extra_cases(ik_scene, link, case):
    """On the end effector and one finger link (130 envs, a ragged block):
    negated: -q is the same rotation; whichever of q and -q lies across from
      the current orientation takes the `angle > pi` wrap;
    scaled: 3 q, which the kernel normalises as btTransform does;
    far_turn: an orientation 171..179 deg from the start's (the wrap and the
      45 deg clamp at once);
    far_target: a position 0.5 m from the start's (the 45 deg clamp)."""
    sims, cfg = ik_scene
    rng = np.random.default_rng(100 + link)
    q0, pos, orn = _ik_inputs(cfg, link, 130, rng)
    base_orn = orn
    if case == "negated":
        orn = -orn
    elif case == "scaled":
        orn = f32(3.0 * orn)
    elif case == "far_turn":
        _, cur, _, _ = oracle_link_states(cfg, q0, np.zeros_like(q0), link)
        axis = rng.normal(size=(130, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        half = np.radians(rng.uniform(171.0, 179.0, 130)) / 2
        orn = f32(_quat_mul(np.concatenate([axis * np.sin(half)[:, None], np.cos(half)[:, None]], axis=1), cur))
        R0, R1 = quat_to_matrix(cur), quat_to_matrix(orn)
        turn = np.degrees(np.arccos(np.clip((np.einsum("nij,nij->n", R0, R1) - 1) / 2, -1, 1)))
        assert turn.min() > 170.0
    else:
        cur, _, _, _ = oracle_link_states(cfg, q0, np.zeros_like(q0), link)
        d = rng.normal(size=(130, 3))
        pos = f32(cur + 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True))
    got, ref = _ik_check(sims[130], cfg, link, q0, pos, orn, IK_EXTRA_MEASURED[link, case], case)
    if case in ("negated", "scaled"):
        # the same rotation, so the oracle's answer is the base target's: to the rounding of 3 q, and of the
        # angle, which the oracle keeps in a float as computeIK does (a wrapped 2 pi - a: 5e-7 rad)
        same = _ik_oracle(cfg, q0, link, pos, base_orn)
        assert np.abs(same - ref).max() < 2e-6
    if case in ("far_turn", "far_target"):
        # some sample's joint ends further away than one clamped step could take it
        assert np.abs(ref - q0).max() > np.pi / 4


# ------------------------------------------------------------ ps_base_state
EULER_CEIL = _TIGHT["obj_rot"]
# worst angle between the GPU's and the fp64 formula's orientation on an MI355X (rad)
# (5.23e-6 at sarg = +-0.99998, where asin amplifies the rounding of sarg by 1 / sqrt(1 - sarg^2) = 158;
# 1.8e-7 on the locked samples)
EULER_MEASURED = {("push", 0): 5.23e-06, ("stack", 0): 5.23e-06, ("stack", 1): 5.23e-06}
LOCK = 0.99999


def _euler_ref(q):
    """getEulerFromQuaternion in fp64 (the formula test_euler_from_quaternion_branches pins) -> rpy [n, 3], sarg [n]."""
    x, y, z, w = np.asarray(q, np.float64).T
    sarg = -2.0 * (x * z - w * y)
    roll = np.arctan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z)
    pitch = np.arcsin(np.clip(sarg, -1.0, 1.0))
    yaw = np.arctan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z)
    lo, hi = sarg <= -LOCK, sarg >= LOCK
    roll = np.where(lo | hi, 0.0, roll)
    pitch = np.where(lo, -0.5 * np.pi, np.where(hi, 0.5 * np.pi, pitch))
    yaw = np.where(lo, 2.0 * np.arctan2(x, -y), np.where(hi, 2.0 * np.arctan2(-x, y), yaw))
    return np.stack([roll, pitch, yaw], -1), sarg


def _quat_from_euler(e):
    r, p, y = (np.asarray(e, np.float64) * 0.5).T
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy], -1)


def _orientation_sample(rng, n=130):
    """Quaternions [n, 4] and the count of samples meant to be locked: exact
    pitch +-90 deg with several yaws; sarg = +-0.9999, +-0.99998 (unlocked)
    and +-0.999995 (locked) built from Euler angles with two roll / yaw
    pairs; the identity; a 180 deg turn about each axis; random unit
    quaternions for the rest (106)."""
    qs = [_quat_from_euler([[0.0, s * np.pi / 2, yaw]]) for s in (-1, 1) for yaw in (0.0, 0.7, -2.4, 3.0)]
    for sarg in (0.9999, 0.99998, 0.999995):
        for s in (-1, 1):
            qs += [_quat_from_euler([[roll, np.arcsin(s * sarg), yaw]]) for roll, yaw in ((0.3, -1.1), (-2.0, 2.5))]
    qs += [np.array([[0.0, 0.0, 0.0, 1.0]]), np.array([[1.0, 0, 0, 0]]), np.array([[0, 1.0, 0, 0]]),
           np.array([[0, 0, 1.0, 0]])]
    fixed = np.concatenate(qs)
    rnd = rng.normal(size=(n - len(fixed), 4))
    assert len(rnd) >= 100
    return np.concatenate([fixed, rnd / np.linalg.norm(rnd, axis=1, keepdims=True)])


def _base_state_raw(sim, obj, want=(True,) * 5):
    B = sim.num_envs
    outs = [torch.full((B, n), float("nan"), device=sim.device) if w else None
            for n, w in zip((3, 4, 3, 3, 3), want)]
    sim._call("ps_base_state", sim._ctx, _ptr(sim.state), int(obj), *[_ptr(o) for o in outs], sim._stream())
    return outs


@pytest.mark.parametrize("task,bodies", [("push", ["object"]), ("stack", ["object1", "object2"])])
def test_base_state(ps, task, bodies):
    """ps_base_state of every object of a one- and a two-object scene, 130
    envs.  Euler angles against the fp64 formula on the fp32 quaternion read
    back, as the angle between the two orientations (parity_judge._obs_err);
    locked samples give roll = 0 and pitch = +-fp32(pi/2) exactly.  Position,
    quaternion and velocities are copies of the rows written.  Bound: 4 x
    EULER_MEASURED, at most EULER_CEIL."""
    from pandasim.sim import PandaSim, euler_from_quaternion

    B = 130
    sim = PandaSim(task=task, num_envs=B)
    rng = np.random.default_rng(4)
    for obj, body in enumerate(bodies):
        quat = _orientation_sample(rng, B)[rng.permutation(B)]
        sim.set_base_pose(body, torch.from_numpy(rng.uniform(-1.0, 1.0, (B, 3))), torch.from_numpy(quat))
        row = L.OBJECT_ROWS[obj]
        sim.set_rows(row + 7, torch.from_numpy(rng.uniform(-2.0, 2.0, (B, 3))))
        sim.set_rows(row + 10, torch.from_numpy(rng.uniform(-9.0, 9.0, (B, 3))))
    for obj, body in enumerate(bodies):
        row = L.OBJECT_ROWS[obj]
        written = [sim.rows(row, 3), sim.rows(row + 3, 4), None, sim.rows(row + 7, 3), sim.rows(row + 10, 3)]
        full = _base_state_raw(sim, obj)
        for k in (0, 1, 3, 4):
            assert torch.equal(_bits(full[k]), _bits(written[k])), (body, k)
        assert written[3].abs().max() > 1.0 and written[4].abs().max() > 1.0
        # NULL outputs: each alone carries the bits of the full call; so does the wrapper
        for k in range(5):
            want = [j == k for j in range(5)]
            one = _base_state_raw(sim, obj, want)
            assert [o is not None for o in one] == want
            assert torch.equal(_bits(one[k]), _bits(full[k])), (body, k)
        for a, b in zip(sim._base_state(body), full):
            assert torch.equal(_bits(a), _bits(b))
        assert torch.equal(_bits(sim.get_base_rotation(body)), _bits(full[2]))
        # Euler angles
        q = written[1].double().cpu().numpy()
        ref, sarg = _euler_ref(q)
        assert np.abs(np.abs(sarg) - LOCK).min() > 1e-6  # no sample hangs on the switch
        locked = np.abs(sarg) >= LOCK
        assert (sarg[locked] > 0).sum() >= 6 and (sarg[locked] < 0).sum() >= 6
        near = ~locked & (np.abs(sarg) > 0.9998)
        assert (sarg[near] > 0).sum() >= 4 and (sarg[near] < 0).sum() >= 4
        got = full[2].cpu().numpy()
        assert np.all(got[locked, 0] == 0.0)
        assert np.array_equal(got[locked, 1], (np.sign(sarg[locked]) * np.float32(np.pi / 2)).astype(np.float32))
        err = np.array([_obs_err(got[i], ref[i], "obj_rot", slice(None), task) for i in range(B)])
        print(f"MEASURED base_state {task} obj={obj} euler_angle={err.max():.3g} "
              f"(locked {err[locked].max():.3g}, near {err[near].max():.3g})")
        assert err.max() <= _bound(EULER_MEASURED[task, obj], EULER_CEIL), (body, err.max())
        # the host helper (ghosts and the robot base) is the same formula: fp64 rounding, amplified by
        # at most 1 / sqrt(1 - 0.99999^2) = 224 in asin
        host = euler_from_quaternion(torch.from_numpy(q)).numpy()
        herr = np.array([_obs_err(host[i], ref[i], "obj_rot", slice(None), task) for i in range(B)])
        assert herr.max() < 1e-12
        assert np.all(host[locked, 0] == 0.0) and np.array_equal(host[locked, 1], ref[locked, 1])


def test_base_state_of_a_missing_object_is_unsupported(ps):
    from pandasim.sim import PandaSim

    sim = PandaSim(task="push", num_envs=4)
    out = torch.zeros(4, 3, device=sim.device)
    for obj in (1, 2, -1):
        rc = sim._lib.ps_base_state(sim._ctx, _ptr(sim.state), obj, _ptr(out), None, None, None, None, sim._stream())
        assert L.ERRORS[rc] == "PS_ERR_UNSUPPORTED"
    reach = PandaSim(task="reach", num_envs=4)
    rc = reach._lib.ps_base_state(reach._ctx, _ptr(reach.state), 0, _ptr(out), None, None, None, None,
                                  reach._stream())
    assert L.ERRORS[rc] == "PS_ERR_UNSUPPORTED"
    with pytest.raises(L.PandasimError):
        sim._call("ps_base_state", sim._ctx, _ptr(sim.state), 1, _ptr(out), None, None, None, None, sim._stream())


# ------------------------------------------------------- per-env generators
RNG_B = 130
SPECIAL_SEEDS = [0, 1, 2**32 - 1, 2**32, 2**63 + 7, 2**64 - 1]  # tests/test_oracle.py::test_pcg64_matches_numpy
DRAWS = [  # successive Generator.uniform(low, high) calls: n = 1, 3, 8; negative and equal bounds
    ([-0.3], [0.7]),
    ([-0.15, -0.15, 0.0], [0.15, 0.15, 0.0]),
    ([-5.0, -1e-3, 2.0, -7.25, 0.0, 1e6, -1.0, 0.1], [-2.0, 1e-3, 2.0, 3.5, 1.0, 1e6 + 1.0, -1.0, 0.3]),
]
SENTINEL = -12345.678


def _seeds(rng, n=RNG_B):
    rest = rng.integers(0, 2**64, size=n - len(SPECIAL_SEEDS), dtype=np.uint64, endpoint=False)
    return np.concatenate([np.array(SPECIAL_SEEDS, dtype=np.uint64), rest])


def _numpy_gens(seeds):
    return [np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(s)))) for s in seeds]


def _seed(sim, seeds, mask=None):
    sim.seed(torch.from_numpy(seeds.view(np.int64)), mask=None if mask is None else torch.from_numpy(mask))


def _uniform_raw(sim, low, high, mask):
    """ps_rng_uniform into a buffer pre-filled with SENTINEL."""
    n = len(low)
    out = torch.full((sim.num_envs, n), SENTINEL, dtype=torch.float64, device=sim.device)
    m = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(sim.device)
    sim._call("ps_rng_uniform", sim._ctx, _ptr(sim.state), _ptr(m), n, (C.c_double * n)(*low),
              (C.c_double * n)(*high), _ptr(out), sim._stream())
    return out.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64),
                          np.ascontiguousarray(b, np.float64).view(np.uint64))


def test_rng_uniform_matches_numpy(ps):
    """sim.seed + sim.uniform with n = 1, 3 and 8 (PS_MAX_UNIFORM) in
    succession against numpy's own Generator of each env's seed, bit for bit;
    the state rows after seeding are the oracle's SeedSequence restatement."""
    from pandasim.sim import PandaSim

    sim = PandaSim(task="reach", num_envs=RNG_B)
    seeds = _seeds(np.random.default_rng(5))
    _seed(sim, seeds)
    rows = snapshot(sim)["rng"]
    assert np.array_equal(rows[:4].T, np.array([O.pcg64_seed(int(s)) for s in seeds]))
    assert np.array_equal(rows[4], seeds ^ np.uint64(0x5851F42D4C957F2D))
    gens = _numpy_gens(seeds)
    assert len(DRAWS[-1][0]) == L.PS_MAX_UNIFORM
    for rep in range(2):
        for low, high in DRAWS:
            got = sim.uniform(low, high).cpu().numpy()
            want = np.array([g.uniform(low, high) for g in gens])
            assert got.shape == (RNG_B, len(low)) and _same_bits(got, want), (rep, low)
    # scalar bounds are one draw
    got = sim.uniform(-1.0, 1.0).cpu().numpy()
    assert _same_bits(got, np.array([[g.uniform(-1.0, 1.0)] for g in gens]))


def test_rng_masks(ps):
    """A masked-out env's output rows and its stream stay put, in
    ps_rng_uniform and in ps_rng_seed."""
    from pandasim.sim import PandaSim

    sim = PandaSim(task="reach", num_envs=RNG_B)
    seeds = _seeds(np.random.default_rng(6))
    _seed(sim, seeds)
    gens = _numpy_gens(seeds)
    mask = np.arange(RNG_B) % 3 == 0
    assert mask[-1] and not mask[-2]  # the ragged block has both kinds
    for low, high in DRAWS:
        before = snapshot(sim)["rng"]
        got = _uniform_raw(sim, low, high, mask)
        after = snapshot(sim)["rng"]
        want = np.array([g.uniform(low, high) if m else np.full(len(low), SENTINEL) for g, m in zip(gens, mask)])
        assert _same_bits(got, want), low
        assert np.array_equal(after[:, ~mask], before[:, ~mask])
        assert np.all((after[:2, mask] != before[:2, mask]).any(axis=0))
        assert np.array_equal(after[2:, mask], before[2:, mask])  # increment and goal stream
    # the next unmasked draw is every stream's next value: the masked-out ones did not advance
    low, high = DRAWS[1]
    assert _same_bits(_uniform_raw(sim, low, high, None), np.array([g.uniform(low, high) for g in gens]))
    # an all-zero mask draws nothing
    before = snapshot(sim)["rng"]
    assert np.all(_uniform_raw(sim, low, high, np.zeros(RNG_B, bool)) == SENTINEL)
    assert np.array_equal(snapshot(sim)["rng"], before)
    # masked seeding re-seeds the masked envs only
    new = _seeds(np.random.default_rng(7))[::-1].copy()
    _seed(sim, new, mask)
    fresh = _numpy_gens(new)
    gens = [f if m else g for f, g, m in zip(fresh, gens, mask)]
    after = snapshot(sim)["rng"]
    assert np.array_equal(after[:, ~mask], before[:, ~mask])
    assert np.array_equal(after[:4, mask].T, np.array([O.pcg64_seed(int(s)) for s in new[mask]]))
    assert np.array_equal(after[4, mask], new[mask] ^ np.uint64(0x5851F42D4C957F2D))
    for low, high in DRAWS:
        assert _same_bits(sim.uniform(low, high).cpu().numpy(), np.array([g.uniform(low, high) for g in gens]))


def test_rng_rotation(ps):
    """sim.random_rotation: three successive draws bit-equal to O.flip_goal
    from the same auxiliary state, unit to 1e-12; a mask leaves the other
    envs' goal streams and output rows alone; the PCG64 streams never move."""
    from pandasim.sim import PandaSim

    sim = PandaSim(task="flip", num_envs=RNG_B)
    seeds = _seeds(np.random.default_rng(8))
    _seed(sim, seeds)
    start = snapshot(sim)["rng"]
    aux = [int(a) for a in start[4]]

    def expect(which):
        out = np.full((RNG_B, 4), SENTINEL)
        for i in np.flatnonzero(which):
            aux[i], out[i] = O.flip_goal(aux[i])
        return out

    everyone = np.ones(RNG_B, bool)
    for _ in range(3):
        got = sim.random_rotation().cpu().numpy()
        assert _same_bits(got, expect(everyone))
        assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() < 1e-12
        assert np.array_equal(snapshot(sim)["rng"][4], np.array(aux, dtype=np.uint64))
    mask = np.arange(RNG_B) % 3 == 0
    for _ in range(2):
        out = torch.full((RNG_B, 4), SENTINEL, dtype=torch.float64, device=sim.device)
        m = torch.from_numpy(mask.astype(np.uint8)).to(sim.device)
        sim._call("ps_rng_rotation", sim._ctx, _ptr(sim.state), _ptr(m), _ptr(out), sim._stream())
        assert _same_bits(out.cpu().numpy(), expect(mask))
        assert np.array_equal(snapshot(sim)["rng"][4], np.array(aux, dtype=np.uint64))
    got = sim.random_rotation(mask=torch.from_numpy(mask)).cpu().numpy()
    assert _same_bits(got[mask], expect(mask)[mask])
    assert _same_bits(sim.random_rotation().cpu().numpy(), expect(everyone))
    assert np.array_equal(snapshot(sim)["rng"][:4], start[:4])


def test_rng_argument_checks(ps):
    from pandasim.sim import PandaSim

    sim = PandaSim(task="reach", num_envs=4)
    before = snapshot(sim)["rng"]
    for low, high in (([], []), ([0.0] * 9, [1.0] * 9), ([0.0, 0.0], [1.0]), ([0.0], [1.0, 1.0])):
        with pytest.raises(ValueError):
            sim.uniform(low, high)
    out = torch.full((4, 9), SENTINEL, dtype=torch.float64, device=sim.device)
    lo, hi = (C.c_double * 9)(*[0.0] * 9), (C.c_double * 9)(*[1.0] * 9)
    for n in (0, 9, -1):
        rc = sim._lib.ps_rng_uniform(sim._ctx, _ptr(sim.state), None, n, lo, hi, _ptr(out), sim._stream())
        assert L.ERRORS[rc] == "PS_ERR_ARG"
    assert sim._lib.ps_rng_uniform(sim._ctx, _ptr(sim.state), None, 1, None, hi, _ptr(out),
                                   sim._stream()) == -1
    assert sim._lib.ps_rng_seed(sim._ctx, _ptr(sim.state), None, None, sim._stream()) == -1
    assert sim._lib.ps_rng_rotation(sim._ctx, _ptr(sim.state), None, None, sim._stream()) == -1
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL) and np.array_equal(snapshot(sim)["rng"], before)
