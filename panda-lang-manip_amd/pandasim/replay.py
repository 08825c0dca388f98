"""Device-resident hindsight experience replay for ``PandaVecEnv``.

The counterpart of stable-baselines3's ``HerReplayBuffer`` as the reference's
``examples/train_push.py`` uses it (``DDPG(..., replay_buffer_class=
HerReplayBuffer)`` on ``PandaPush-v3``; ``env.compute_reward`` relabels,
core.py:226), for B envs at once and without leaving the GPU: the ring lives
in one device buffer, ``add`` is one launch per env step (ps_replay_store) and
``sample`` one call without a host synchronisation (ps_replay_sample), with
the ``future`` / ``final`` goal selection and the reward recomputation inside
the sampling kernel.  The specification is include/pandasim.h, "Device-resident
HER replay" (DESIGN.md §14); tests/replay_reference.py restates it in numpy.

    env = pandasim.make("PandaPush-v3", num_envs=4096)
    buf = pandasim.HerReplay(env, capacity_steps=100)
    obs, _ = env.reset(seed=0)
    buf.begin(obs)
    for _ in range(200):
        out = env.step(policy(obs), copy=False)
        buf.add(actions, *out)
        batch = buf.sample(4096)          # device tensors, no sync

The argument checks are plain functions that need no device (replay_args,
replay_add_args, replay_sample_args), as program_flags and shared_mlp_args are.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib as L

STRATEGIES = {"future": L.REPLAY_FUTURE, "final": L.REPLAY_FINAL}


class ReplaySample(NamedTuple):
    """One batch: device tensors, named as include/pandasim.h names them."""
    obs: torch.Tensor          # [M, O] f32
    ag: torch.Tensor           # [M, G]
    dg: torch.Tensor           # [M, G]  the stored goal, or the hindsight goal where relabelled
    action: torch.Tensor       # [M, A]
    next_obs: torch.Tensor     # [M, O]
    next_ag: torch.Tensor      # [M, G]
    reward: torch.Tensor       # [M] f32  stored, or compute_reward(next_ag, dg) where relabelled
    terminated: torch.Tensor   # [M] u8
    success: torch.Tensor      # [M] u8   is_success(next_ag, dg)
    relabelled: torch.Tensor   # [M] u8
    env_idx: torch.Tensor      # [M] i32
    slot: torch.Tensor         # [M] i32
    goal_slot: torch.Tensor    # [M] i32  -1 where not relabelled
    n_valid: torch.Tensor      # [1] i64  the valid transitions the batch was drawn from


def her_ratio(n_sampled_goal: int) -> float:
    """HerReplayBuffer's share of relabelled samples: 1 - 1 / (n_sampled_goal + 1)."""
    return 1.0 - 1.0 / (n_sampled_goal + 1)


def her_threshold(ratio: float) -> int:
    """round(ratio * 2^32): a sample is relabelled when the high half of its
    second hash word is below it."""
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"HerReplay: her_ratio = {ratio!r} (0 to 1)")
    return int(round(ratio * 4294967296.0))


def _whole(name: str, v, low: int) -> int:
    if isinstance(v, bool) or int(v) != v or v < low:
        raise ValueError(f"HerReplay: {name} = {v!r} (a whole number from {low})")
    return int(v)


def replay_args(capacity_steps, max_episode_steps: int, n_sampled_goal=4, strategy="future"):
    """The constructor's checks (ValueError; no device) -> (strategy id,
    relabelling threshold)."""
    T = _whole("capacity_steps", capacity_steps, 1)
    if T < max_episode_steps:
        raise ValueError(f"HerReplay: capacity_steps = {T} is below the env's max_episode_steps = "
                         f"{max_episode_steps}: an episode longer than the ring overwrites its own first "
                         "transitions before it ends, so they could never be sampled")
    if T > L.REPLAY_MAX_CAPACITY:
        raise ValueError(f"HerReplay: capacity_steps = {T} (at most {L.REPLAY_MAX_CAPACITY})")
    n = _whole("n_sampled_goal", n_sampled_goal, 0)
    if strategy not in STRATEGIES:
        raise ValueError(f"HerReplay: unknown strategy {strategy!r} (one of {sorted(STRATEGIES)}; "
                         "'episode' is not built)")
    return STRATEGIES[strategy], her_threshold(her_ratio(n))


def _want(what: str, name: str, t, shape, dtypes=(torch.float32,), device=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if device is not None and t.device != torch.device(device):
        raise ValueError(f"{what}: {name} is on {t.device}, the buffer's envs are on {device}: the kernel reads "
                         "the tensor's memory as it is (move it with .to(device))")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise ValueError(f"{what}: {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous, got strides {t.stride()}")


def replay_obs_args(what: str, num_envs: int, obs_dim: int, goal_dim: int, obs_dict, mask=None, device=None):
    """An observation dict's checks -> (observation, achieved_goal, desired_goal).
    With `device`, every tensor must be on it (HerReplay passes its own: the
    kernels take the tensors' addresses)."""
    B = int(num_envs)
    for key in ("observation", "achieved_goal", "desired_goal"):
        if key not in obs_dict:
            raise ValueError(f"{what}: the observation has no {key!r}")
    _want(what, "observation", obs_dict["observation"], (B, obs_dim), device=device)
    _want(what, "achieved_goal", obs_dict["achieved_goal"], (B, goal_dim), device=device)
    _want(what, "desired_goal", obs_dict["desired_goal"], (B, goal_dim), device=device)
    if mask is not None:
        _want(what, "mask", mask, (B,), (torch.uint8, torch.bool), device=device)
    return obs_dict["observation"], obs_dict["achieved_goal"], obs_dict["desired_goal"]


def replay_add_args(num_envs: int, obs_dim: int, goal_dim: int, action_dim: int, actions, obs_dict, reward,
                    terminated, truncated, info=None, device=None):
    """add's checks (ValueError; no device needed to run them) ->
    (final_observation, final_achieved_goal), each None when info does not
    carry it.  With `device`, every tensor must be on it."""
    B, what = int(num_envs), "HerReplay.add"
    _want(what, "actions", actions, (B, action_dim), device=device)
    replay_obs_args(what, B, obs_dim, goal_dim, obs_dict, device=device)
    _want(what, "reward", reward, (B,), device=device)
    _want(what, "terminated", terminated, (B,), (torch.uint8, torch.bool), device)
    _want(what, "truncated", truncated, (B,), (torch.uint8, torch.bool), device)
    fo = fa = None
    if info:
        fo, fa = info.get("final_observation"), info.get("final_achieved_goal")
        if (fo is None) != (fa is None):
            raise ValueError(f"{what}: info carries one of final_observation / final_achieved_goal without the other")
        if fo is not None:
            _want(what, "info['final_observation']", fo, (B, obs_dim), device=device)
            _want(what, "info['final_achieved_goal']", fa, (B, goal_dim), device=device)
    return fo, fa


def replay_sample_args(batch_size, stored: int) -> int:
    M = _whole("batch_size", batch_size, 1)
    if M > L.REPLAY_MAX_BATCH:
        raise ValueError(f"HerReplay: batch_size = {M} (at most {L.REPLAY_MAX_BATCH})")
    if stored < 1:
        raise ValueError("HerReplay.sample: the buffer is empty (nothing was added yet)")
    return M


def replay_layout(ctx, capacity_steps: int) -> L.ReplayLayout:
    """ps_replay_layout_of of a context (no device needed)."""
    lay = L.ReplayLayout()
    L.check(L.lib().ps_replay_layout_of(ctx, int(capacity_steps), C.byref(lay)), ctx, "ps_replay_layout_of")
    return lay


def _u8(t):
    return None if t is None else (t.view(torch.uint8) if t.dtype == torch.bool else t)


class HerReplay:
    """A ring of ``capacity_steps`` time slots of the env's B envs on its
    device.  ``capacity_steps`` must be at least the env's max_episode_steps:
    a longer episode would overwrite its own first transitions before they
    become valid (the kernels allow it; the class refuses what a user cannot
    mean)."""

    def __init__(self, env, capacity_steps: int, n_sampled_goal: int = 4, strategy: str = "future", seed: int = 0):
        self.strategy, self.threshold = replay_args(capacity_steps, env.max_episode_steps, n_sampled_goal, strategy)
        self.env, self.sim = env, env.sim
        self.capacity = int(capacity_steps)
        self.num_envs, self.device = env.num_envs, env.device
        self.obs_dim, self.goal_dim, self.action_dim = env.obs_dim, env.goal_dim, env.action_dim
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.layout = lay = replay_layout(self.sim._ctx, self.capacity)
        try:
            self.buf = torch.empty(lay.bytes, dtype=torch.uint8, device=self.device)  # ps_replay_init zeroes it
        except RuntimeError as e:  # torch.cuda.OutOfMemoryError is one
            raise L.PandasimError(f"HerReplay: cannot allocate the replay buffer of {lay.bytes} bytes "
                                  f"({self.capacity} steps x {self.num_envs} envs x {lay.row_floats * 4} B): {e}") from e
        T, B, R = self.capacity, self.num_envs, lay.row_floats
        ring = self.buf[lay.ring_offset:lay.ring_offset + T * B * R * 4]
        self.ring = ring.view(torch.float32).view(T, B, R)        # the rows as floats ...
        self.ring_i32 = ring.view(torch.int32).view(T, B, R)      # ... and as words (terminated, ep_end)
        self.cur_len = self.buf[lay.cur_len_offset:lay.cur_len_offset + B * 4].view(torch.int32)
        self.pending = self.buf[lay.pending_offset:lay.pending_offset + B * lay.pending_floats * 4] \
            .view(torch.float32).view(B, lay.pending_floats)
        self.n_stores = 0
        self.draw = 0
        self.sim._call("ps_replay_init", self.sim._ctx, L._ptr(self.buf), self.capacity, self.sim._stream())

    # ------------------------------------------------------------ counters
    @property
    def pos(self) -> int:
        """The slot the next add writes."""
        return self.n_stores % self.capacity

    @property
    def stored(self) -> int:
        return min(self.n_stores, self.capacity)

    def __len__(self) -> int:
        """stored * B: an upper bound of the valid transitions, without a sync."""
        return self.stored * self.num_envs

    @property
    def nbytes(self) -> int:
        return int(self.layout.bytes)

    def field(self, name: str) -> torch.Tensor:
        """A [T, B, width] view of one field of the ring (obs, ag, dg, action,
        next_obs, next_ag, reward: f32; terminated, ep_end: i32)."""
        lay = self.layout
        width = {"obs": lay.obs_dim, "ag": lay.goal_dim, "dg": lay.goal_dim, "action": lay.action_dim,
                 "next_obs": lay.obs_dim, "next_ag": lay.goal_dim, "reward": 1, "terminated": 1, "ep_end": 1}[name]
        off = getattr(lay, "off_" + name)
        src = self.ring_i32 if name in ("terminated", "ep_end") else self.ring
        return src[:, :, off:off + width]

    # --------------------------------------------------------------- calls
    def begin(self, obs_dict, mask=None) -> None:
        """After env.reset(): the first observation of the masked envs' next
        episode (all envs without mask).  A masked env whose episode was still
        running has it closed at its last stored transition."""
        obs, ag, dg = replay_obs_args("HerReplay.begin", self.num_envs, self.obs_dim, self.goal_dim, obs_dict, mask,
                                      self.device)
        self.sim._call("ps_replay_begin", self.sim._ctx, L._ptr(self.buf), self.capacity, self.pos, self.stored,
                       L._ptr(obs), L._ptr(ag), L._ptr(dg), L._ptr(_u8(mask)), self.sim._stream())

    def add(self, actions, obs_dict, reward, terminated, truncated, info=None) -> None:
        """One env step of every env: `actions` and what env.step(actions)
        returned.  With step(copy=False) the tensors are the env's own output
        buffers; the kernel reads them in stream order, before the next step
        overwrites them."""
        fo, fa = replay_add_args(self.num_envs, self.obs_dim, self.goal_dim, self.action_dim, actions, obs_dict,
                                 reward, terminated, truncated, info, self.device)
        p = L._ptr
        self.sim._call("ps_replay_store", self.sim._ctx, p(self.buf), self.capacity, self.pos, p(actions),
                       p(obs_dict["observation"]), p(obs_dict["achieved_goal"]), p(obs_dict["desired_goal"]), p(fo),
                       p(fa), p(reward), p(_u8(terminated)), p(_u8(truncated)), self.sim._stream())
        self.n_stores += 1

    def sample(self, batch_size: int, draw: Optional[int] = None) -> ReplaySample:
        """A batch of `batch_size` transitions, relabelled with the buffer's
        strategy and ratio; no host synchronisation.  `draw` replays an earlier
        call's batch (the default counts up per call)."""
        M = replay_sample_args(batch_size, self.stored)
        if draw is None:
            draw, self.draw = self.draw, self.draw + 1
        dev, O, G, A = self.device, self.obs_dim, self.goal_dim, self.action_dim
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        u = lambda: torch.empty(M, dtype=torch.uint8, device=dev)  # noqa: E731
        i = lambda: torch.empty(M, dtype=torch.int32, device=dev)  # noqa: E731
        out = ReplaySample(obs=f(M, O), ag=f(M, G), dg=f(M, G), action=f(M, A), next_obs=f(M, O), next_ag=f(M, G),
                           reward=f(M), terminated=u(), success=u(), relabelled=u(), env_idx=i(), slot=i(),
                           goal_slot=i(), n_valid=torch.empty(1, dtype=torch.int64, device=dev))
        self._sample(M, draw, out._asdict())
        return out

    def _sample(self, M: int, draw: int, outputs: dict) -> None:
        batch = L.ReplayBatch(**{k: t.data_ptr() for k, t in outputs.items()})
        self.sim._call("ps_replay_sample", self.sim._ctx, L._ptr(self.buf), self.capacity, self.pos, self.stored,
                       self.strategy, self.seed, int(draw) & 0xFFFFFFFFFFFFFFFF, self.threshold, M, C.byref(batch),
                       self.sim._stream())

    def valid_count(self) -> int:
        """The valid transitions (those of finished episodes) as of now: runs
        the prefix sum through a one-sample call and reads it back (a sync)."""
        if self.stored == 0:
            return 0
        f = lambda n: torch.empty(1, n, dtype=torch.float32, device=self.device)  # noqa: E731
        n_valid = torch.empty(1, dtype=torch.int64, device=self.device)
        # one sample into the three outputs the call requires, and the count
        self._sample(1, 0, dict(obs=f(self.obs_dim), action=f(self.action_dim), dg=f(self.goal_dim), n_valid=n_valid))
        return int(n_valid.item())
