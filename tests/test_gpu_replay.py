"""GPU tests of the device-resident HER replay (pandasim.HerReplay over
ps_replay_*): the kernels against the numpy restatement of the specification
(tests/replay_reference.py), bit for bit -- the ring after a store, the prefix
sum and search across scan blocks, every output of a sample -- and the
relabelled rewards against ps_compute_reward itself."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_reference as R
from pandasim import HerReplay
from pandasim import _lib as L
from pandasim.envs import PandaVecEnv
from pandasim.replay import her_ratio, her_threshold
from pandasim.utils import THRESHOLD, angle_distance, distance
from replay_env_run import run_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("obs", "ag", "dg", "action", "next_obs", "next_ag", "reward", "terminated", "ep_end")


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def new_pair(task, reward, B, T, strategy="future", n_sampled_goal=4, seed=0):
    """An env (for its context and dims only), its buffer and the restatement.
    The ring is smaller than an episode here, which the class refuses for users:
    the capacity check is lifted for the construction."""
    env = PandaVecEnv(task, reward, "ee", B, DEV, autoreset=False)
    steps, env.max_episode_steps = env.max_episode_steps, 1
    buf = HerReplay(env, T, n_sampled_goal, strategy, seed)
    env.max_episode_steps = steps
    ref = R.ReplayRef(B, T, env.obs_dim, env.goal_dim, env.action_dim, task, reward)
    return env, buf, ref


def feed(buf, ref, first, steps, final=True):
    if first is not None:
        buf.begin(dict(zip(("observation", "achieved_goal", "desired_goal"), map(dev, first))))
        ref.begin(*first)
    for s in steps:
        s = s if final else {**s, "final_obs": None, "final_ag": None}
        info = {"final_observation": dev(s["final_obs"]), "final_achieved_goal": dev(s["final_ag"])} if final else {}
        buf.add(dev(s["actions"]), {"observation": dev(s["obs"]), "achieved_goal": dev(s["ag"]),
                                    "desired_goal": dev(s["dg"])}, dev(s["reward"]), dev(s["terminated"]),
                dev(s["truncated"]).bool(), info)
        ref.store(**s)


def assert_ring_equal(buf, ref):
    assert (buf.n_stores, buf.pos, buf.stored) == (ref.n_stores, ref.pos, ref.stored)
    for name in FIELDS:
        want = getattr(ref, name)
        want = want.reshape(ref.T, ref.B, -1)
        assert torch.equal(buf.field(name).cpu(), torch.from_numpy(want)), name
    assert torch.equal(buf.cur_len.cpu(), torch.from_numpy(ref.cur_len)), "cur_len"
    O, G = ref.O, ref.G
    pend = buf.pending.cpu()
    assert torch.equal(pend[:, :O], torch.from_numpy(ref.pend_obs)), "pending obs"
    assert torch.equal(pend[:, O:O + G], torch.from_numpy(ref.pend_ag)), "pending ag"
    assert torch.equal(pend[:, O + G:O + 2 * G], torch.from_numpy(ref.pend_dg)), "pending dg"
    assert not pend[:, O + 2 * G:].any() and not buf.ring[:, :, buf.layout.off_ep_end + 1:].any()  # the padding


def assert_sample_equal(got, want):
    for name, w in want.items():
        g = getattr(got, name).cpu()
        assert g.dtype == torch.from_numpy(w).dtype, name
        assert torch.equal(g, torch.from_numpy(np.ascontiguousarray(w))), name


# ------------------------------------------------------------ store, bit for bit
@pytest.mark.parametrize("B,final", [(130, True), (1, True), (130, False)])
def test_store_bit_for_bit(B, final):
    """B = 130: two full waves and a ragged tail of rows; T = 5, 23 stores of
    random rows with the scripted episodes (1 to 7 steps)."""
    env, buf, ref = new_pair("push", "sparse", B, 5)
    first, steps = R.synthetic_steps(B, 23, env.obs_dim, env.goal_dim, env.action_dim, seed=B)
    assert_ring_equal(buf, ref)  # ps_replay_init
    done = 0
    for upto in (4, 5, 6, 23):
        feed(buf, ref, first if done == 0 else None, steps[done:upto], final)
        done = upto
        assert_ring_equal(buf, ref)
    assert len(buf) == 5 * B and buf.nbytes == buf.layout.bytes == buf.buf.numel()
    assert buf.valid_count() == int(ref.prefix()[-1])


# ------------------------------------------------ prefix and search across blocks
def test_prefix_and_search_across_scan_blocks():
    """One workgroup of k_replay_prefix scans 1 024 envs: B = 1 025 is one more
    than that, and puts one env in a second block.  Reach (O = 6), T = 3, uneven
    cur_len."""
    assert L.REPLAY_SCAN_BLOCK == 1024
    check_scan_blocks(L.REPLAY_SCAN_BLOCK + 1)


def test_search_in_a_second_scan_block():
    """40 envs in the second block: a few dozen of the 1 000 samples fall there
    (about 2.6 % of the valid transitions are theirs), so the rank relative to
    the first block's total and the search within the second block are checked
    by many samples, not by the one that B = 1 025 gives."""
    want = check_scan_blocks(L.REPLAY_SCAN_BLOCK + 40)
    assert (want["env_idx"] >= L.REPLAY_SCAN_BLOCK).sum() >= 10
    assert len(set(want["env_idx"][want["env_idx"] >= L.REPLAY_SCAN_BLOCK].tolist())) >= 8


def check_scan_blocks(B):
    env, buf, ref = new_pair("reach", "sparse", B, 3)
    assert env.obs_dim == 6
    first, steps = R.synthetic_steps(B, 5, env.obs_dim, env.goal_dim, env.action_dim, seed=3)
    feed(buf, ref, first, steps)
    assert len(set(ref.cur_len.tolist())) >= 3 and ref.valid_counts()[L.REPLAY_SCAN_BLOCK:].sum() > 0  # uneven
    want = ref.sample(1000, 0, 0, R.FUTURE, R.her_threshold(0.8))
    got = buf.sample(1000)
    assert torch.equal(got.env_idx.cpu(), torch.from_numpy(want["env_idx"]))
    assert torch.equal(got.slot.cpu(), torch.from_numpy(want["slot"]))
    assert int(got.n_valid.item()) == int(ref.prefix()[-1])
    assert_sample_equal(got, want)
    return want


# ----------------------------------------------------------- sample, bit for bit
THRESHOLD_ENVS = 30


def threshold_offsets(task):
    """f32 values d for which the task's f32 distance of (base + d e_0, base),
    base = 0 (Flip: of (d e_0, e_0)), is the f32 threshold exactly, one ulp
    below and one ulp above.  Flip's 1 - fl(m^2) with m^2 in [0.5, 1) is a
    multiple of 2^-24 and the f32 threshold 0.2 is an odd multiple of 2^-26, so
    no pair has the threshold itself or the ulp above it as its distance: Flip
    takes the nearest distances either side of the threshold that a pair has
    (within four steps of 2^-24)."""
    thr = np.float32(THRESHOLD[task])
    lo, hi = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    centre = np.float32(np.sqrt(1.0 - float(thr))) if task == "flip" else thr
    cand = [centre]
    for _ in range(8):
        cand = [np.nextafter(cand[0], np.float32(0))] + cand + [np.nextafter(cand[-1], np.float32(1))]
    G = {"flip": 4, "stack": 6}.get(task, 3)
    found = {}
    for d in cand:
        a, g = np.zeros(G, np.float32), np.zeros(G, np.float32)
        a[0] = d
        if task == "flip":
            g[0] = 1.0
        dist = np.float32((angle_distance if task == "flip" else distance)(torch.from_numpy(a[None]),
                                                                           torch.from_numpy(g[None])).item())
        found.setdefault(dist, d)
    if task == "flip":
        below, above = max(k for k in found if k < thr), min(k for k in found if k > thr)
        assert float(thr) - 4 * 2.0 ** -24 < below < thr < above < float(thr) + 4 * 2.0 ** -24
        return [found[below], found[above]]
    assert lo in found and thr in found and hi in found
    return [found[lo], found[thr], found[hi]]


def with_threshold_pairs(task, steps):
    """The first 30 envs, env b with offset b mod 3 (Flip: b mod 2): next_ag is
    `base` at an episode's last step and base + d e_0 before it, so that a
    `final` relabel of any earlier transition is a pair at the threshold."""
    offsets = threshold_offsets(task)
    for env_b in range(THRESHOLD_ENVS):
        d = offsets[env_b % len(offsets)]
        for s in steps:
            ag = np.zeros(s["final_ag"].shape[1], np.float32)
            if s["terminated"][env_b] or s["truncated"][env_b]:
                if task == "flip":
                    ag[0] = 1.0
            else:
                ag[0] = d
            s["final_ag"][env_b] = ag
    return steps


@pytest.mark.parametrize("task,reward", [("push", "sparse"), ("push", "dense"), ("stack", "sparse"), ("flip", "sparse")])
def test_sample_bit_for_bit(task, reward):
    B, T, M = 130, 5, 1000
    env, buf, ref = new_pair(task, reward, B, T)
    assert env.goal_dim == {"push": 3, "stack": 6, "flip": 4}[task]
    first, steps = R.synthetic_steps(B, 23, env.obs_dim, env.goal_dim, env.action_dim, seed=7)
    feed(buf, ref, first, with_threshold_pairs(task, steps))
    assert_ring_equal(buf, ref)
    thr32 = np.float32(THRESHOLD[task])
    n_variants = 2 if task == "flip" else 3
    seen = set()
    for strategy in (R.FUTURE, R.FINAL):
        for n_goal, ratio in ((0, 0.0), (4, 0.8), (None, 1.0)):
            buf.strategy, buf.threshold = strategy, R.her_threshold(ratio)
            if n_goal is not None:
                assert buf.threshold == her_threshold(her_ratio(n_goal))  # the class's own threshold
            got = buf.sample(M, draw=3)
            want = ref.sample(M, 0, 3, strategy, R.her_threshold(ratio))
            assert_sample_equal(got, want)
            rel = got.relabelled.bool()
            assert rel.float().mean().item() == pytest.approx(ratio, abs=0.06)
            # relabelled: the env's own compute_reward / compute_success (ps_compute_reward) on the sampled pairs
            r = env.compute_reward(got.next_ag, got.dg)
            ok = env.compute_success(got.next_ag, got.dg)
            assert torch.equal(got.reward[rel], r[rel]) and torch.equal(got.success.bool(), ok)
            # the others: the stored values
            t, b = got.slot.long(), got.env_idx.long()
            assert torch.equal(got.reward[~rel], buf.field("reward")[t, b, 0][~rel])
            assert torch.equal(got.dg[~rel], buf.field("dg")[t, b][~rel])
            assert (got.goal_slot[~rel] == -1).all()
            if strategy == R.FINAL and ratio == 1.0:
                # the pairs at the threshold were drawn, and fall on the side their distance says
                e = buf.field("ep_end")[t, b, 0]
                for v in range(n_variants):
                    hit = (b < THRESHOLD_ENVS) & (b % n_variants == v) & (e != got.slot)
                    assert hit.any(), v
                    d = (angle_distance if task == "flip" else distance)(got.next_ag[hit].cpu(), got.dg[hit].cpu())
                    assert len(set(d.tolist())) == 1
                    seen.add(np.float32(d[0].item()))
                    assert (got.success[hit].bool().cpu() == (d < thr32)).all()
                    if reward == "sparse":
                        assert (got.reward[hit].cpu() == -(d > thr32).float()).all()
    lo, hi = np.nextafter(thr32, np.float32(0)), np.nextafter(thr32, np.float32(1))
    if task == "flip":
        assert len(seen) == 2 and min(seen) < thr32 < max(seen)
    else:
        assert seen == {lo, thr32, hi}


# --------------------------------------------------------- empty and degenerate
def test_empty_and_degenerate():
    B, T = 3, 3
    env, buf, ref = new_pair("push", "sparse", B, T)
    first, steps = R.synthetic_steps(B, 5, env.obs_dim, env.goal_dim, env.action_dim, seed=2, lengths=(5,))
    feed(buf, ref, first, steps[:4])  # an episode longer than the ring, still running
    assert_ring_equal(buf, ref)
    got = buf.sample(7)
    assert int(got.n_valid.item()) == 0 and buf.valid_count() == 0
    assert (got.env_idx == -1).all() and (got.slot == -1).all() and (got.goal_slot == -1).all()
    for name in ("obs", "ag", "dg", "action", "next_obs", "next_ag", "reward", "terminated", "success", "relabelled"):
        assert not getattr(got, name).any(), name
    assert_sample_equal(got, ref.sample(7, 0, 0, R.FUTURE, R.her_threshold(0.8)))
    feed(buf, ref, None, steps[4:])  # ... then its end: the T slots it left become valid
    assert_ring_equal(buf, ref)
    assert ref.valid_counts().tolist() == [T] * B and (ref.ep_end == 4 % T).all()
    assert_sample_equal(buf.sample(1), ref.sample(1, 0, 1, R.FUTURE, R.her_threshold(0.8)))  # M = 1
    assert buf.valid_count() == T * B
    # begin(mask) in mid-episode closes the masked envs' episode at their last stored slot
    _, more = R.synthetic_steps(B, 2, env.obs_dim, env.goal_dim, env.action_dim, seed=5, lengths=(50,))
    feed(buf, ref, None, more)
    mask = np.array([1, 0, 1], np.uint8)
    buf.begin(dict(zip(("observation", "achieved_goal", "desired_goal"), map(dev, first))), dev(mask))
    ref.begin(*first, mask=mask)
    assert_ring_equal(buf, ref)
    assert ref.cur_len.tolist() == [0, 2, 0]


# -------------------------------------------------------------- through the env
@pytest.fixture(scope="module")
def env_run():
    return run_env()


def test_through_the_env(env_run):
    env, buf, actions, first, trace, batch = env_run
    ref = R.ReplayRef(env.num_envs, buf.capacity, env.obs_dim, env.goal_dim, env.action_dim, "push", "sparse")
    ref.begin(*(x.cpu().numpy() for x in first))
    ends = 0
    for s, tr in enumerate(trace):
        obs, ag, dg, fo, fa, r, te, tu = (x.cpu().numpy() for x in tr)
        ref.store(actions[s].cpu().numpy(), obs, ag, dg, fo, fa, r, te, tu)
        done = (te | tu).astype(bool)
        if done.any() and s >= len(trace) - buf.capacity:
            # at an episode's end the stored next_obs is final_observation, not the reset observation
            stored = buf.field("next_obs")[s % buf.capacity].cpu().numpy()
            assert np.array_equal(stored[done], fo[done]) and not np.array_equal(stored[done], obs[done])
            ends += int(done.sum())
    assert ends >= env.num_envs  # every env ended an episode within the ring (TimeLimit 50, T = 60)
    assert_ring_equal(buf, ref)
    assert_sample_equal(batch, ref.sample(512, 0, 0, R.FUTURE, R.her_threshold(0.8)))
    rel = batch.relabelled.bool()
    t, b = batch.slot.long(), batch.env_idx.long()
    assert (~rel).any() and torch.equal(batch.reward[~rel], buf.field("reward")[t, b, 0][~rel])  # the env's own reward
    assert torch.equal(batch.reward[rel], env.compute_reward(batch.next_ag, batch.dg)[rel])


def test_side_stream_sees_the_steps_queued_before():
    """add and sample on a side stream are ordered behind the step queued before
    them there: the same ring, step outputs and batch as on the default stream.
    Both runs happen in a fresh process (tests/replay_env_run.py): a side stream
    made here would stay live in this one, and tests/test_gpu_streams.py counts
    on its two side streams being the only ones ("no more than these are ever
    live"; its control rows lose their power otherwise)."""
    import os
    import subprocess
    import sys

    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "replay_env_run.py")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "side stream == default stream" in r.stdout, r.stdout[-2000:]


# -------------------------------------------------------------------- refusals
def test_refusals_leave_the_buffer_untouched():
    B, T = 8, 4
    env, buf, ref = new_pair("push", "sparse", B, T)
    first, steps = R.synthetic_steps(B, 3, env.obs_dim, env.goal_dim, env.action_dim, seed=4)
    feed(buf, ref, first, steps)
    torch.cuda.synchronize()
    before = buf.buf.clone()
    lib, ctx, p, st = env.sim._lib, env.sim._ctx, L._ptr, env.sim._stream()
    s = {k: dev(v) for k, v in steps[0].items()}
    out = buf.sample(4)
    torch.cuda.synchronize()
    before = buf.buf.clone()
    fields = {k: t.data_ptr() for k, t in out._asdict().items()}
    batch = L.ReplayBatch(**fields)
    rp = p(buf.buf)

    def store(ctx_=ctx, replay=rp, cap=T, pos=3, **kw):
        a = {**{k: p(v) for k, v in s.items()}, **kw}
        return lib.ps_replay_store(ctx_, replay, cap, pos, a["actions"], a["obs"], a["ag"], a["dg"], a["final_obs"],
                                   a["final_ag"], a["reward"], a["terminated"], a["truncated"], st)

    def sample(ctx_=ctx, replay=rp, cap=T, pos_next=3, stored=3, strategy=0, thr=1 << 31, M=4, batch_=batch):
        return lib.ps_replay_sample(ctx_, replay, cap, pos_next, stored, strategy, 0, 0, thr, M,
                                    None if batch_ is None else C.byref(batch_), st)

    def begin(ctx_=ctx, replay=rp, cap=T, pos_next=3, stored=3, obs=s["obs"]):
        return lib.ps_replay_begin(ctx_, replay, cap, pos_next, stored, p(obs), p(s["ag"]), p(s["dg"]), None, st)

    def without(name):
        return L.ReplayBatch(**{**fields, name: None})

    refused = [
        store(ctx_=None), store(replay=None), store(cap=0), store(pos=-1), store(pos=T), store(actions=None),
        store(reward=None), store(truncated=None), store(dg=None),
        begin(ctx_=None), begin(replay=None), begin(cap=0), begin(pos_next=T), begin(stored=T + 1), begin(obs=None),
        begin(pos_next=2, stored=3),
        sample(ctx_=None), sample(replay=None), sample(cap=0), sample(pos_next=-1), sample(stored=T + 1),
        sample(pos_next=0, stored=0), sample(M=0), sample(M=-5), sample(strategy=2), sample(strategy=-1),
        sample(thr=(1 << 32) + 1), sample(batch_=None), sample(batch_=without("obs")),
        sample(batch_=without("action")), sample(batch_=without("dg")),
        lib.ps_replay_init(ctx, None, T, st), lib.ps_replay_init(None, rp, T, st), lib.ps_replay_init(ctx, rp, 0, st),
        # a buffer that is not 16-byte aligned (the kernels move 128-bit words)
        store(replay=C.c_void_p(buf.buf.data_ptr() + 4)), begin(replay=C.c_void_p(buf.buf.data_ptr() + 8)),
        sample(replay=C.c_void_p(buf.buf.data_ptr() + 4)), lib.ps_replay_init(ctx, C.c_void_p(buf.buf.data_ptr() + 12), T, st),
    ]
    assert refused == [-1] * len(refused)
    torch.cuda.synchronize()
    assert torch.equal(buf.buf, before)
    # the same calls with good arguments go through (nullable outputs left out, threshold 2^32)
    assert sample(thr=1 << 32, batch_=without("ag")) == 0 and begin() == 0 and store() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="max_episode_steps"):
        HerReplay(env, env.max_episode_steps - 1)
    # a tensor that is not on the buffer's device is refused by the class, before its address reaches a kernel
    obs = {"observation": s["obs"], "achieved_goal": s["ag"], "desired_goal": s["dg"]}
    n = buf.n_stores
    with pytest.raises(ValueError, match="actions is on cpu"):
        buf.add(s["actions"].cpu(), obs, s["reward"], s["terminated"], s["truncated"], {})
    with pytest.raises(ValueError, match="reward is on cpu"):
        buf.add(s["actions"], obs, s["reward"].cpu(), s["terminated"], s["truncated"], {})
    with pytest.raises(ValueError, match="achieved_goal is on cpu"):
        buf.begin({**obs, "achieved_goal": s["ag"].cpu()})
    assert buf.n_stores == n
