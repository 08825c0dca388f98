// ps_replay.h — the device-resident HER replay buffer (include/pandasim.h,
// "Device-resident HER replay"): the view of the caller's buffer that the
// kernels of replay_kernels.hip take by value, the host function that lays the
// buffer out, and the integer hash of the sampler (host and device: the host
// folds seed and draw, the device draws per sample).
#pragma once

#include "ps_common.h"

namespace ps {

constexpr int kReplayScanBlock = 1024;  // envs one workgroup of k_replay_prefix scans

struct ReplayView {
    float *ring;         // [T][B][R] rows of 32-bit words
    int32_t *cur_len;    // [B]
    float *pending;      // [B][Pf]: obs, ag, dg of the transition the next store completes
    int32_t *prefix;     // [B] inclusive scan of v within each block of kReplayScanBlock envs
    int64_t *block_sum;  // [ceil(B / kReplayScanBlock)] inclusive scan of the blocks' totals
    int32_t T, B, R, Pf, O, G, A;
    int32_t off_action, off_next_obs, off_next_ag, off_reward, off_terminated, off_ep_end;
    // (obs, ag and dg lead the row, in the pending row's order: off_obs = 0, off_ag = O, off_dg = O + G)
};

PS_HD uint64_t replay_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

inline int64_t replay_align(int64_t x) { return (x + 255) / 256 * 256; }

inline void replay_layout(int64_t num_envs, int capacity, int O, int G, int A, ps_replay_layout *l) {
    const int words = 2 * O + 3 * G + A + 3;
    l->capacity = capacity;
    l->num_envs = (int32_t)num_envs;
    l->row_floats = (words + 3) / 4 * 4;
    l->pending_floats = (O + 2 * G + 3) / 4 * 4;
    l->obs_dim = O;
    l->goal_dim = G;
    l->action_dim = A;
    l->off_obs = 0;
    l->off_ag = O;
    l->off_dg = O + G;
    l->off_action = O + 2 * G;
    l->off_next_obs = l->off_action + A;
    l->off_next_ag = l->off_next_obs + O;
    l->off_reward = l->off_next_ag + G;
    l->off_terminated = l->off_reward + 1;
    l->off_ep_end = l->off_reward + 2;
    const int64_t nb = (num_envs + kReplayScanBlock - 1) / kReplayScanBlock;
    l->ring_offset = 0;
    l->cur_len_offset = replay_align((int64_t)capacity * num_envs * l->row_floats * 4);
    l->pending_offset = l->cur_len_offset + replay_align(num_envs * 4);
    l->prefix_offset = l->pending_offset + replay_align(num_envs * l->pending_floats * 4);
    l->block_sum_offset = l->prefix_offset + replay_align(num_envs * 4);
    l->bytes = l->block_sum_offset + replay_align(nb * 8);
}

inline ReplayView replay_view(const ps_replay_layout &l, void *replay) {
    char *p = (char *)replay;
    ReplayView v;
    v.ring = (float *)(p + l.ring_offset);
    v.cur_len = (int32_t *)(p + l.cur_len_offset);
    v.pending = (float *)(p + l.pending_offset);
    v.prefix = (int32_t *)(p + l.prefix_offset);
    v.block_sum = (int64_t *)(p + l.block_sum_offset);
    v.T = l.capacity;
    v.B = l.num_envs;
    v.R = l.row_floats;
    v.Pf = l.pending_floats;
    v.O = l.obs_dim;
    v.G = l.goal_dim;
    v.A = l.action_dim;
    v.off_action = l.off_action;
    v.off_next_obs = l.off_next_obs;
    v.off_next_ag = l.off_next_ag;
    v.off_reward = l.off_reward;
    v.off_terminated = l.off_terminated;
    v.off_ep_end = l.off_ep_end;
    return v;
}

}  // namespace ps
