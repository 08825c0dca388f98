"""The HER replay buffer of include/pandasim.h ("Device-resident HER replay"),
restated in numpy: the ring with its back-fill, begin, the valid transitions and
their prefix sum, the integer hash with mulhi64, and both hindsight strategies.
Written from the specification, one env at a time where the kernels work per
128-bit word; it shares no code with pandasim.replay.  The relabelled reward is
the project's host-side float32 arithmetic (pandasim.utils on CPU tensors:
distance / angle_distance, each operation rounded once), with the threshold
rounded to float32 as ps_compute_reward's f32 / f32 branch does."""
import numpy as np
import torch

FUTURE, FINAL = 0, 1
MASK64 = (1 << 64) - 1
U = np.uint64


def mix(z):
    """splitmix64's finaliser on uint64 arrays (wrapping)."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=U) + U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def mix_int(z: int) -> int:
    """mix on one Python integer (the second, independent statement of it)."""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def mulhi64(a, b):
    """The high 64 bits of the 128-bit product of uint64 arrays."""
    a, b = np.asarray(a, dtype=U), np.asarray(b, dtype=U)
    lo32 = U(0xFFFFFFFF)
    al, ah, bl, bh = a & lo32, a >> U(32), b & lo32, b >> U(32)
    with np.errstate(over="ignore"):
        ll, hl, lh, hh = al * bl, ah * bl, al * bh, ah * bh
        cross = (ll >> U(32)) + (hl & lo32) + lh
        return hh + (hl >> U(32)) + (cross >> U(32))


def her_threshold(ratio: float) -> int:
    return int(round(ratio * 2 ** 32))


def reward_and_success(task: str, reward_type: str, next_ag: np.ndarray, dg: np.ndarray):
    """compute_reward / is_success of float32 pairs [n, G] -> (f32 [n], bool [n])."""
    from pandasim.utils import THRESHOLD, goal_reward_and_success

    thr = float(np.float32(THRESHOLD[task]))
    a = torch.from_numpy(np.ascontiguousarray(next_ag, dtype=np.float32))
    g = torch.from_numpy(np.ascontiguousarray(dg, dtype=np.float32))
    r, ok = goal_reward_and_success(a, g, reward_type, distance_threshold=thr, task=task)
    return r.numpy().astype(np.float32), ok.numpy()


class ReplayRef:
    def __init__(self, num_envs, capacity, obs_dim, goal_dim, action_dim, task="push", reward_type="sparse"):
        self.B, self.T, self.O, self.G, self.A = num_envs, capacity, obs_dim, goal_dim, action_dim
        self.task, self.reward_type = task, reward_type
        B, T, f = num_envs, capacity, np.float32
        self.obs, self.next_obs = np.zeros((T, B, obs_dim), f), np.zeros((T, B, obs_dim), f)
        self.ag, self.dg, self.next_ag = (np.zeros((T, B, goal_dim), f) for _ in range(3))
        self.action = np.zeros((T, B, action_dim), f)
        self.reward = np.zeros((T, B), f)
        self.terminated = np.zeros((T, B), np.int32)
        self.ep_end = np.full((T, B), -1, np.int32)
        self.cur_len = np.zeros(B, np.int32)
        self.pend_obs, self.pend_ag, self.pend_dg = np.zeros((B, obs_dim), f), np.zeros((B, goal_dim), f), \
            np.zeros((B, goal_dim), f)
        self.n_stores = 0

    # ------------------------------------------------------------------ ring
    @property
    def pos(self):
        return self.n_stores % self.T

    @property
    def stored(self):
        return min(self.n_stores, self.T)

    def _close(self, b, last):
        """ep_end of env b's last cur_len slots, ending at `last`, becomes `last`."""
        for k in range(int(self.cur_len[b])):
            self.ep_end[(last - k) % self.T, b] = last
        self.cur_len[b] = 0

    def begin(self, obs, ag, dg, mask=None):
        for b in range(self.B):
            if mask is not None and not mask[b]:
                continue
            self.pend_obs[b], self.pend_ag[b], self.pend_dg[b] = obs[b], ag[b], dg[b]
            if self.cur_len[b] > 0:
                self._close(b, (self.pos - 1) % self.T)

    def store(self, actions, obs, ag, dg, final_obs, final_ag, reward, terminated, truncated):
        pos = self.pos
        nobs = obs if final_obs is None else final_obs
        nag = ag if final_ag is None else final_ag
        for b in range(self.B):
            self.obs[pos, b], self.ag[pos, b], self.dg[pos, b] = self.pend_obs[b], self.pend_ag[b], self.pend_dg[b]
            self.action[pos, b], self.next_obs[pos, b], self.next_ag[pos, b] = actions[b], nobs[b], nag[b]
            self.reward[pos, b] = reward[b]
            self.terminated[pos, b] = 1 if terminated[b] else 0
            self.ep_end[pos, b] = -1
            self.cur_len[b] = min(self.cur_len[b] + 1, self.T)
            if terminated[b] or truncated[b]:
                self._close(b, pos)
            self.pend_obs[b], self.pend_ag[b], self.pend_dg[b] = obs[b], ag[b], dg[b]
        self.n_stores += 1

    # ----------------------------------------------------------------- valid
    def oldest(self):
        return (self.pos - self.stored) % self.T

    def valid_counts(self):
        return (self.stored - self.cur_len).astype(np.int64)

    def valid_slots(self, b):
        """Env b's valid slots, oldest first."""
        return [(self.oldest() + j) % self.T for j in range(int(self.valid_counts()[b]))]

    def prefix(self):
        return np.cumsum(self.valid_counts())

    # ---------------------------------------------------------------- sample
    def indices(self, M, seed, draw, strategy, threshold):
        """-> env b, slot t, relabel, goal slot g (int64 / bool arrays), V."""
        v, P = self.valid_counts(), self.prefix()
        V = int(P[-1])
        if V == 0:
            minus = np.full(M, -1, np.int64)
            return minus, minus.copy(), np.zeros(M, bool), minus.copy(), 0
        h = mix_int(mix_int(seed & MASK64) ^ (draw & MASK64))
        i = np.arange(M, dtype=U)
        w = [mix(U(h) ^ (U(4) * i + U(k))) for k in range(3)]
        r = mulhi64(w[0], np.full(M, V, U)).astype(np.int64)
        b = np.searchsorted(P, r, side="right")  # the least env with P[b] > r
        j = r - (P[b] - v[b])
        t = (self.oldest() + j) % self.T
        relabel = (w[1] >> U(32)).astype(np.int64) < threshold
        e = self.ep_end[t, b].astype(np.int64)
        n = ((e - t) % self.T) + 1
        if strategy == FUTURE:
            g = (t + mulhi64(w[2], n.astype(U)).astype(np.int64)) % self.T
        else:
            g = e
        return b, t, relabel, g, V

    def sample(self, M, seed, draw, strategy, threshold):
        b, t, relabel, g, V = self.indices(M, seed, draw, strategy, threshold)
        f = np.float32
        if V == 0:
            z = lambda *s: np.zeros(s, f)  # noqa: E731
            return dict(obs=z(M, self.O), ag=z(M, self.G), dg=z(M, self.G), action=z(M, self.A),
                        next_obs=z(M, self.O), next_ag=z(M, self.G), reward=z(M), terminated=np.zeros(M, np.uint8),
                        success=np.zeros(M, np.uint8), relabelled=np.zeros(M, np.uint8),
                        env_idx=np.full(M, -1, np.int32), slot=np.full(M, -1, np.int32),
                        goal_slot=np.full(M, -1, np.int32), n_valid=np.zeros(1, np.int64))
        next_ag = self.next_ag[t, b]
        dg = np.where(relabel[:, None], self.next_ag[g, b], self.dg[t, b])
        rew, ok = reward_and_success(self.task, self.reward_type, next_ag, dg)
        reward = np.where(relabel, rew, self.reward[t, b]).astype(f)
        return dict(obs=self.obs[t, b], ag=self.ag[t, b], dg=dg, action=self.action[t, b],
                    next_obs=self.next_obs[t, b], next_ag=next_ag, reward=reward,
                    terminated=self.terminated[t, b].astype(np.uint8), success=ok.astype(np.uint8),
                    relabelled=relabel.astype(np.uint8), env_idx=b.astype(np.int32), slot=t.astype(np.int32),
                    goal_slot=np.where(relabel, g, -1).astype(np.int32), n_valid=np.array([V], np.int64))


# ------------------------------------------------------------ scripted streams
def episode_lengths(num_envs, lengths=(1, 2, 3, 4, 5, 6, 7)):
    """Env b runs episodes of lengths[b % len], lengths[(b + 1) % len], ... steps."""
    return [[lengths[(b + k) % len(lengths)] for k in range(len(lengths))] for b in range(num_envs)]


def scripted_done(num_envs, n_steps, lengths=(1, 2, 3, 4, 5, 6, 7)):
    """terminated / truncated [n_steps, B] u8 of the scripted episodes: an
    episode of even length ends terminated, one of odd length truncated."""
    term, trunc = np.zeros((n_steps, num_envs), np.uint8), np.zeros((n_steps, num_envs), np.uint8)
    for b, eps in enumerate(episode_lengths(num_envs, lengths)):
        s, k = 0, 0
        while True:
            s += eps[k % len(eps)]
            if s > n_steps:
                break
            (term if eps[k % len(eps)] % 2 == 0 else trunc)[s - 1, b] = 1
            k += 1
    return term, trunc


def synthetic_steps(num_envs, n_steps, obs_dim, goal_dim, action_dim, seed=0, lengths=(1, 2, 3, 4, 5, 6, 7)):
    """Random float32 step outputs with the scripted episode ends: a first
    observation triple and n_steps tuples as ReplayRef.store takes them."""
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    term, trunc = scripted_done(num_envs, n_steps, lengths)
    first = (r(num_envs, obs_dim), r(num_envs, goal_dim), r(num_envs, goal_dim))
    steps = [dict(actions=r(num_envs, action_dim), obs=r(num_envs, obs_dim), ag=r(num_envs, goal_dim),
                  dg=r(num_envs, goal_dim), final_obs=r(num_envs, obs_dim), final_ag=r(num_envs, goal_dim),
                  reward=r(num_envs), terminated=term[s], truncated=trunc[s]) for s in range(n_steps)]
    return first, steps
