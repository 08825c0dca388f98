"""CPU tests of the device-resident HER replay (include/pandasim.h,
"Device-resident HER replay"): the numpy restatement (tests/replay_reference.py)
against the properties the specification promises, the host-side argument
checks of pandasim.replay, and ps_replay_layout_of.  No kernel is launched; the
GPU tests (tests/test_gpu_replay.py) hold the kernels to this restatement bit
for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_reference as R
from pandasim import replay as PR

LENGTHS = (1, 2, 3, 4, 5, 6, 7)


def filled(B, T, n_steps, O=6, G=3, A=3, seed=0, task="push", reward_type="sparse", lengths=LENGTHS):
    ref = R.ReplayRef(B, T, O, G, A, task, reward_type)
    first, steps = R.synthetic_steps(B, n_steps, O, G, A, seed, lengths)
    ref.begin(*first)
    for s in steps:
        ref.store(**s)
    return ref


# ------------------------------------------------------------ scripted streams
def test_scripted_streams_valid_slots_and_episode_ends():
    """B = 5, T = 4, 19 stores, episodes of 1 to 7 steps (shorter than, equal
    to and longer than the ring).  The expectation is kept step by step, by
    global step number, apart from the restatement's own bookkeeping."""
    B, T, N = 5, 4, 19
    ref = R.ReplayRef(B, T, 6, 3, 3)
    first, steps = R.synthetic_steps(B, N, 6, 3, 3)
    assert {len_ for eps in R.episode_lengths(B) for len_ in eps} == set(LENGTHS)
    ref.begin(*first)
    episode = [[] for _ in range(B)]   # episode number of every step of env b
    end_of = [dict() for _ in range(B)]  # episode number -> the step it ended at
    current = [0] * B
    for n, s in enumerate(steps):
        ref.store(**s)
        for b in range(B):
            episode[b].append(current[b])
            if s["terminated"][b] or s["truncated"][b]:
                end_of[b][current[b]] = n
                current[b] += 1
        in_ring = range(n + 1 - min(n + 1, T), n + 1)
        for b in range(B):
            want = [m % T for m in in_ring if episode[b][m] in end_of[b]]
            running = [m % T for m in in_ring if episode[b][m] not in end_of[b]]
            assert ref.valid_slots(b) == want, (n, b)           # exactly the stored - cur_len oldest
            assert len(want) == min(n + 1, T) - ref.cur_len[b]
            assert not set(running) & set(ref.valid_slots(b))   # no slot of a running episode is valid
            for m in in_ring:
                if episode[b][m] in end_of[b]:
                    end = end_of[b][episode[b][m]]
                    assert end >= m and ref.ep_end[m % T, b] == end % T, (n, b, m)  # its own episode's end
                    assert ref.ep_end[m % T, b] >= 0
    ended = {episode[b].count(k) for b in range(B) for k in end_of[b]}  # the lengths of the episodes that ended
    assert ended == {1, 2, 3, 4, 5, 6, 7}  # shorter than, equal to and longer than T
    assert ref.prefix()[-1] == ref.valid_counts().sum()


def test_begin_mid_episode_closes_the_episode():
    B, T = 3, 6
    ref = R.ReplayRef(B, T, 6, 3, 3)
    first, steps = R.synthetic_steps(B, 4, 6, 3, 3, lengths=(50,))  # no episode ends by itself
    ref.begin(*first)
    for s in steps:
        ref.store(**s)
    assert ref.valid_counts().tolist() == [0, 0, 0] and (ref.ep_end == -1).all()
    mask = np.array([1, 0, 1], np.uint8)
    new = tuple(x + 1 for x in first)
    ref.begin(*new, mask=mask)
    assert ref.cur_len.tolist() == [0, 4, 0]
    assert ref.valid_counts().tolist() == [4, 0, 4]
    assert (ref.ep_end[:4, 0] == 3).all() and (ref.ep_end[:4, 2] == 3).all() and (ref.ep_end[:, 1] == -1).all()
    assert (ref.ep_end[4:] == -1).all()
    assert np.array_equal(ref.pend_obs[0], new[0][0]) and np.array_equal(ref.pend_obs[1], steps[-1]["obs"][1])
    # the next transition of a masked env starts from the observation begin recorded
    first2, steps2 = R.synthetic_steps(B, 1, 6, 3, 3, seed=9, lengths=(50,))
    ref.store(**steps2[0])
    assert np.array_equal(ref.obs[4, 0], new[0][0]) and np.array_equal(ref.obs[4, 1], steps[-1]["obs"][1])


# --------------------------------------------------------- sampling properties
M_BIG = 200_000


@pytest.fixture(scope="module")
def ring():
    ref = filled(64, 10, 25, seed=1)
    assert 400 <= ref.prefix()[-1] <= 600  # V of about 500
    return ref


@pytest.fixture(scope="module")
def draws(ring):
    return {s: ring.indices(M_BIG, 7, 0, s, R.her_threshold(0.8)) for s in (R.FUTURE, R.FINAL)}


def test_every_valid_transition_is_drawn_uniformly(ring, draws):
    b, t, _, _, V = draws[R.FUTURE]
    valid = {(e, s) for e in range(ring.B) for s in ring.valid_slots(e)}
    assert len(valid) == V
    pairs, counts = np.unique(np.stack([b, t], 1), axis=0, return_counts=True)
    assert {tuple(p) for p in pairs.tolist()} == valid  # all of them and nothing else
    mean = M_BIG / V
    assert np.abs(counts - mean).max() <= 5 * np.sqrt(mean), (counts.min(), counts.max(), mean)


def test_relabelled_share(ring, draws):
    _, _, relabel, _, _ = draws[R.FUTURE]
    assert abs(relabel.mean() - 0.8) <= 4 * np.sqrt(0.8 * 0.2 / M_BIG)
    assert R.her_threshold(0.8) == 3435973837 == PR.her_threshold(PR.her_ratio(4))
    assert not ring.indices(5000, 7, 0, R.FUTURE, R.her_threshold(0.0))[2].any()
    assert ring.indices(5000, 7, 0, R.FUTURE, R.her_threshold(1.0))[2].all()
    assert (R.her_threshold(0.0), R.her_threshold(1.0)) == (0, 1 << 32)


def test_goal_slot_lies_within_the_episode(ring, draws):
    T = ring.T
    for strategy in (R.FUTURE, R.FINAL):
        b, t, _, g, _ = draws[strategy]
        e = ring.ep_end[t, b]
        assert (e >= 0).all()
        assert (((g - t) % T) <= ((e - t) % T)).all()  # between slot and ep_end in ring order
        if strategy == R.FINAL:
            assert np.array_equal(g, e)
    assert (draws[R.FUTURE][3] != draws[R.FINAL][3]).any()


def test_future_offsets_are_uniform_over_an_episode_of_seven():
    ref = filled(1, 8, 7, lengths=(7,))
    assert ref.valid_counts().tolist() == [7] and (ref.ep_end[:7, 0] == 6).all()
    b, t, relabel, g, V = ref.indices(M_BIG, 3, 5, R.FUTURE, R.her_threshold(1.0))
    assert V == 7 and relabel.all()
    off = (g - t) % ref.T
    for slot in range(7):
        n = 7 - slot
        here = off[t == slot]
        counts = np.bincount(here, minlength=n)
        assert len(counts) == n  # never past the episode's end
        mean = len(here) / n
        assert np.abs(counts - mean).max() <= 5 * np.sqrt(mean), (slot, counts)


def test_same_and_different_draws(ring):
    thr = R.her_threshold(0.8)
    a, b, c = (ring.sample(512, 11, d, R.FUTURE, thr) for d in (4, 4, 5))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["env_idx"], c["env_idx"]) and not np.array_equal(a["obs"], c["obs"])
    d = ring.sample(512, 12, 4, R.FUTURE, thr)
    assert not np.array_equal(a["env_idx"], d["env_idx"])
    # relabelled rows carry the goal slot's next_ag and its recomputed reward, the others the stored ones
    rel = a["relabelled"].astype(bool)
    assert rel.any() and (~rel).any()
    assert np.array_equal(a["dg"][rel], ring.next_ag[a["goal_slot"][rel], a["env_idx"][rel]])
    assert np.array_equal(a["dg"][~rel], ring.dg[a["slot"][~rel], a["env_idx"][~rel]])
    assert np.array_equal(a["reward"][~rel], ring.reward[a["slot"][~rel], a["env_idx"][~rel]])
    assert set(np.unique(a["reward"][rel])) <= {-1.0, 0.0} and (a["goal_slot"][~rel] == -1).all()


def test_hash_and_mulhi_agree_with_python_integers():
    rng = np.random.default_rng(0)
    z = rng.integers(0, 1 << 64, size=200, dtype=np.uint64)
    w = rng.integers(0, 1 << 64, size=200, dtype=np.uint64)
    assert R.mix(z).tolist() == [R.mix_int(int(x)) for x in z]
    assert R.mulhi64(z, w).tolist() == [(int(x) * int(y)) >> 64 for x, y in zip(z, w)]
    assert R.mix_int(0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0


def test_empty_ring_samples_zeros():
    ref = filled(4, 5, 3, lengths=(50,))
    out = ref.sample(16, 0, 0, R.FUTURE, R.her_threshold(0.8))
    assert out["n_valid"][0] == 0 and (out["env_idx"] == -1).all() and (out["slot"] == -1).all()
    assert not out["obs"].any() and not out["reward"].any() and not out["relabelled"].any()


# ------------------------------------------------------------------ host checks
def test_constructor_checks_need_no_device():
    assert PR.replay_args(50, 50) == (0, 3435973837)
    assert PR.replay_args(100, 50, 0, "final") == (1, 0)
    with pytest.raises(ValueError, match="max_episode_steps"):
        PR.replay_args(49, 50)
    with pytest.raises(ValueError, match="strategy"):
        PR.replay_args(50, 50, 4, "episode")
    with pytest.raises(ValueError, match="n_sampled_goal"):
        PR.replay_args(50, 50, -1)
    with pytest.raises(ValueError, match="capacity_steps"):
        PR.replay_args(50.5, 50)
    with pytest.raises(ValueError, match="empty"):
        PR.replay_sample_args(8, 0)
    with pytest.raises(ValueError, match="batch_size"):
        PR.replay_sample_args(0, 5)
    assert PR.replay_sample_args(8, 5) == 8


def test_add_checks_shapes_and_dtypes():
    B, O, G, A = 4, 18, 3, 3
    good = dict(actions=torch.zeros(B, A), obs_dict={"observation": torch.zeros(B, O), "achieved_goal": torch.zeros(B, G),
                                                      "desired_goal": torch.zeros(B, G)},
                reward=torch.zeros(B), terminated=torch.zeros(B, dtype=torch.bool),
                truncated=torch.zeros(B, dtype=torch.uint8), info={})
    assert PR.replay_add_args(B, O, G, A, **good) == (None, None)
    fo, fa = torch.zeros(B, O), torch.zeros(B, G)
    got = PR.replay_add_args(B, O, G, A, **{**good, "info": {"final_observation": fo, "final_achieved_goal": fa}})
    assert got[0] is fo and got[1] is fa
    bad = [("actions", torch.zeros(B, A + 1)), ("actions", torch.zeros(B, A, dtype=torch.float64)),
           ("reward", torch.zeros(B, 1)), ("terminated", torch.zeros(B)), ("truncated", torch.zeros(B + 1, dtype=torch.bool)),
           ("actions", torch.zeros(A, B).t()), ("actions", [[0.0] * A] * B),
           ("obs_dict", {**good["obs_dict"], "observation": torch.zeros(B, O - 1)}),
           ("obs_dict", {**good["obs_dict"], "desired_goal": torch.zeros(B, G, dtype=torch.float64)}),
           ("obs_dict", {"observation": torch.zeros(B, O)}),
           ("info", {"final_observation": fo}), ("info", {"final_observation": fo[:, :-1].contiguous(),
                                                          "final_achieved_goal": fa})]
    for key, value in bad:
        with pytest.raises(ValueError, match="HerReplay.add"):
            PR.replay_add_args(B, O, G, A, **{**good, key: value})
    with pytest.raises(ValueError, match="mask"):
        PR.replay_obs_args("HerReplay.begin", B, O, G, good["obs_dict"], mask=torch.zeros(B))
    # the device HerReplay passes (its envs'): a tensor elsewhere is refused, whichever argument it is.  The "meta"
    # device stands for the GPU here: the checks read no data
    assert PR.replay_add_args(B, O, G, A, **good, device="cpu") == (None, None)
    meta = {k: (v.to("meta") if isinstance(v, torch.Tensor) else v) for k, v in good.items()}
    meta["obs_dict"] = {k: v.to("meta") for k, v in good["obs_dict"].items()}
    meta["info"] = {"final_observation": fo.to("meta"), "final_achieved_goal": fa.to("meta")}
    assert PR.replay_add_args(B, O, G, A, **meta, device="meta")[0] is meta["info"]["final_observation"]
    for key in ("actions", "reward", "terminated", "truncated"):
        with pytest.raises(ValueError, match=f"HerReplay.add: {key} is on cpu"):
            PR.replay_add_args(B, O, G, A, **{**meta, key: good[key]}, device="meta")
    for key in good["obs_dict"]:
        with pytest.raises(ValueError, match=f"{key} is on cpu"):
            PR.replay_add_args(B, O, G, A, **{**meta, "obs_dict": {**meta["obs_dict"], key: good["obs_dict"][key]}},
                               device="meta")
        with pytest.raises(ValueError, match=f"HerReplay.begin: {key} is on cpu"):
            PR.replay_obs_args("HerReplay.begin", B, O, G, {**meta["obs_dict"], key: good["obs_dict"][key]}, device="meta")
    with pytest.raises(ValueError, match="final_achieved_goal'\\] is on cpu"):
        PR.replay_add_args(B, O, G, A, **{**meta, "info": {**meta["info"], "final_achieved_goal": fa}}, device="meta")
    with pytest.raises(ValueError, match="mask is on cpu"):
        PR.replay_obs_args("HerReplay.begin", B, O, G, meta["obs_dict"], mask=torch.zeros(B, dtype=torch.bool), device="meta")


# --------------------------------------------------------------------- layout
def test_replay_layout_without_gpu():
    from pandasim import _lib as L

    lib = L.lib()
    B = 64
    for task in (0, 1, 4, 5):  # Reach, Push, Stack, Flip
        cfg = L.default_config(task, 0, 0)
        ctx = C.c_void_p()
        assert lib.ps_create(C.byref(cfg), B, 0, C.byref(ctx)) == 0
        lays = [PR.replay_layout(ctx, T) for T in (1, 2, 3, 50)]
        lay = lays[0]
        O, G, A = lib.ps_obs_dim(ctx), lib.ps_goal_dim(ctx), lib.ps_action_dim(ctx)
        assert (lay.obs_dim, lay.goal_dim, lay.action_dim, lay.num_envs) == (O, G, A, B)
        assert lay.row_floats % 4 == 0 and 0 <= lay.row_floats - (2 * O + 3 * G + A + 3) < 4  # a multiple of 16 B
        assert lay.pending_floats % 4 == 0 and 0 <= lay.pending_floats - (O + 2 * G) < 4
        offs = [lay.off_obs, lay.off_ag, lay.off_dg, lay.off_action, lay.off_next_obs, lay.off_next_ag, lay.off_reward,
                lay.off_terminated, lay.off_ep_end]
        assert offs == list(np.cumsum([0, O, G, G, A, O, G, 1, 1])) and lay.off_ep_end < lay.row_floats
        step = B * lay.row_floats * 4  # (64 rows of a multiple of 16 B: no alignment slack)
        assert [x.bytes - lay.bytes for x in lays] == [0, step, 2 * step, 49 * step]  # linear in capacity
        assert [x.capacity for x in lays] == [1, 2, 3, 50]
        sections = [lay.ring_offset, lay.cur_len_offset, lay.pending_offset, lay.prefix_offset, lay.block_sum_offset,
                    lay.bytes]
        assert sections[0] == 0 and all(a < b and b % 16 == 0 for a, b in zip(sections, sections[1:]))
        bad = L.ReplayLayout()
        assert lib.ps_replay_layout_of(ctx, 0, C.byref(bad)) == -1
        assert lib.ps_replay_layout_of(ctx, (1 << 20) + 1, C.byref(bad)) == -1
        assert lib.ps_replay_layout_of(None, 4, C.byref(bad)) == -1
        lib.ps_destroy(ctx)
    assert "HerReplay" in __import__("pandasim").__all__
