// replay_kernels.hip — the device-resident HER replay buffer and the C ABI
// entry points that launch it (include/pandasim.h, ps_replay_*): the fused
// store of one env step (k_replay_store), the episode close of a reset
// (k_replay_begin), the prefix sum of the envs' valid transitions
// (k_replay_prefix, k_replay_prefix_blocks) and the relabelling sampler
// (k_replay_sample).  The ring is [T][B][row], one transition's fields
// contiguous and the row a multiple of 16 bytes: a store writes one slot of all
// envs as one contiguous run of 128-bit words, a sample reads one row with the
// 128-bit loads of a 16-lane group.
#include "ps_ctx.h"
#include "ps_replay.h"
#include "ps_reward.h"

namespace {

constexpr int kReplayBlock = 256;
constexpr int kSampleLanes = 16;  // lanes that copy one sampled row

PS_D int ring_mod(int x, int T) {  // x in (-T, 2T)
    return x < 0 ? x + T : (x >= T ? x - T : x);
}
PS_D int64_t row_index(const ReplayView &v, int t, int b) { return ((int64_t)t * v.B + b) * v.R; }

// the step's outputs a store reads (device pointers; final_obs / final_ag may be NULL)
struct ReplayStoreIn {
    const float *actions, *obs, *ag, *dg, *final_obs, *final_ag, *reward;
    const uint8_t *terminated, *truncated;
};

// ep_end = -1 of every row (the buffer is zero already: ps_replay_init)
__global__ __launch_bounds__(kReplayBlock) void k_replay_init(ReplayView v) {
    const int64_t q = (int64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    if (q >= (int64_t)v.T * v.B) return;
    ((int32_t *)v.ring)[q * v.R + v.off_ep_end] = -1;
}

// ep_end of the `len` slots ending at `last` (backwards, mod T) becomes `end`
PS_D void close_episode(const ReplayView &v, int b, int end, int last, int len) {
    int32_t *ring = (int32_t *)v.ring;
    int t = last;
    for (int k = 0; k < len; k++) {
        ring[row_index(v, t, b) + v.off_ep_end] = end;
        t = t == 0 ? v.T - 1 : t - 1;
    }
}

// the word `w` (< O + 2 G) of env b's observation triple, as the pending row holds it
PS_D float triple_word(const ReplayView &v, int b, int w, const float *obs, const float *ag, const float *dg) {
    if (w < v.O) return obs[(int64_t)b * v.O + w];
    if (w < v.O + v.G) return ag[(int64_t)b * v.G + (w - v.O)];
    return dg[(int64_t)b * v.G + (w - v.O - v.G)];
}

// One lane per 128-bit word of the pending rows; a lane owns its word (nobody
// else reads or writes it).  Word 0's lane closes the env's running episode.
__global__ __launch_bounds__(kReplayBlock) void k_replay_begin(ReplayView v, int pos_next, const float *obs,
                                                               const float *ag, const float *dg,
                                                               const uint8_t *mask) {
    const int C = v.Pf / 4, np = v.O + 2 * v.G;
    const int64_t q = (int64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    if (q >= (int64_t)v.B * C) return;
    const int b = (int)(q / C), c = (int)(q % C);
    if (mask && !mask[b]) return;
    float x[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int w = 4 * c + k;
        x[k] = w < np ? triple_word(v, b, w, obs, ag, dg) : 0.0f;
    }
    *(float4 *)(v.pending + (int64_t)b * v.Pf + 4 * c) = make_float4(x[0], x[1], x[2], x[3]);
    if (c == 0) {
        const int len = v.cur_len[b];
        if (len > 0) {
            const int last = ring_mod(pos_next - 1, v.T);
            close_episode(v, b, last, last, len < v.T ? len : v.T);
            v.cur_len[b] = 0;
        }
    }
}

// One lane per 128-bit word of slot `pos`: the slot of all envs is one
// contiguous run, so a wave stores 1 KB of consecutive memory.  The leading
// O + 2 G words of a row are the pending row's; the lane that moves a pending
// word into the ring writes the new pending word in its place (it owns it),
// so no lane reads what another writes.  The lane holding the row's ep_end
// does the env's bookkeeping: about B / episode length of them walk back over
// their episode, the others store one word.
__global__ __launch_bounds__(kReplayBlock) void k_replay_store(ReplayView v, int pos, ReplayStoreIn in) {
    const int C = v.R / 4, np = v.O + 2 * v.G;
    const int64_t q = (int64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    if (q >= (int64_t)v.B * C) return;
    const int b = (int)(q / C), c = (int)(q % C);
    const bool has_pending = 4 * c < np;
    float4 *pend = (float4 *)(v.pending + (int64_t)b * v.Pf + 4 * c);
    float4 p4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (has_pending) p4 = *pend;
    const float p[4] = {p4.x, p4.y, p4.z, p4.w};
    const float *nobs = in.final_obs ? in.final_obs : in.obs, *nag = in.final_ag ? in.final_ag : in.ag;
    float x[4], fresh[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int w = 4 * c + k;
        fresh[k] = 0.0f;
        if (w < np) {
            x[k] = p[k];
            fresh[k] = triple_word(v, b, w, in.obs, in.ag, in.dg);
        } else if (w < v.off_next_obs) {
            x[k] = in.actions[(int64_t)b * v.A + (w - v.off_action)];
        } else if (w < v.off_next_ag) {
            x[k] = nobs[(int64_t)b * v.O + (w - v.off_next_obs)];
        } else if (w < v.off_reward) {
            x[k] = nag[(int64_t)b * v.G + (w - v.off_next_ag)];
        } else if (w == v.off_reward) {
            x[k] = in.reward[b];
        } else if (w == v.off_terminated) {
            x[k] = __int_as_float(in.terminated[b] ? 1 : 0);
        } else if (w == v.off_ep_end) {
            const bool done = in.terminated[b] || in.truncated[b];
            const int len = min(v.cur_len[b] + 1, v.T);
            // the slots before pos; this lane's own word carries pos's
            if (done) close_episode(v, b, pos, ring_mod(pos - 1, v.T), len - 1);
            v.cur_len[b] = done ? 0 : len;
            x[k] = __int_as_float(done ? pos : -1);
        } else {
            x[k] = 0.0f;
        }
    }
    *(float4 *)(v.ring + row_index(v, pos, b) + 4 * c) = make_float4(x[0], x[1], x[2], x[3]);
    if (has_pending) *pend = make_float4(fresh[0], fresh[1], fresh[2], fresh[3]);
}

// Inclusive scan of v_b = stored - cur_len[b] within each block of
// kReplayScanBlock envs, the blocks' totals beside: the wave scans by
// __shfl_up, its 16 totals go through LDS and the first wave scans them.  No
// atomics; k_replay_prefix_blocks scans the totals, and the sampler searches
// the two levels.
__global__ __launch_bounds__(kReplayScanBlock) void k_replay_prefix(ReplayView v, int stored) {
    __shared__ int32_t wave_total[kReplayScanBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = (int64_t)blockIdx.x * kReplayScanBlock + tid;
    int32_t x = b < v.B ? stored - v.cur_len[b] : 0;
    x = x < 0 ? 0 : x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_total[wave] = x;
    __syncthreads();
    if (wave == 0) {
        int32_t s = lane < kReplayScanBlock / 64 ? wave_total[lane] : 0;
#pragma unroll
        for (int d = 1; d < kReplayScanBlock / 64; d <<= 1) {
            const int32_t y = __shfl_up(s, d, 64);
            if (lane >= d) s += y;
        }
        if (lane < kReplayScanBlock / 64) wave_total[lane] = s;
    }
    __syncthreads();
    if (wave > 0) x += wave_total[wave - 1];
    if (b < v.B) v.prefix[b] = x;
    if (tid == kReplayScanBlock - 1) v.block_sum[blockIdx.x] = x;
}

// the second pass: one workgroup scans the (at most 1 024) block totals in place
__global__ __launch_bounds__(kReplayScanBlock) void k_replay_prefix_blocks(ReplayView v, int nb) {
    __shared__ long long wave_total[kReplayScanBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long x = tid < nb ? (long long)v.block_sum[tid] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_total[wave] = x;
    __syncthreads();
    if (wave == 0) {
        long long s = lane < kReplayScanBlock / 64 ? wave_total[lane] : 0;
#pragma unroll
        for (int d = 1; d < kReplayScanBlock / 64; d <<= 1) {
            const long long y = __shfl_up(s, d, 64);
            if (lane >= d) s += y;
        }
        if (lane < kReplayScanBlock / 64) wave_total[lane] = s;
    }
    __syncthreads();
    if (wave > 0) x += wave_total[wave - 1];
    if (tid < nb) v.block_sum[tid] = (int64_t)x;
}

// A group of 16 lanes per sample.  Every lane of the group does the index
// arithmetic (the same addresses: one request each), then the lanes read the
// row by 128-bit words and scatter its fields to the batch; lane 0 relabels.
__global__ __launch_bounds__(kReplayBlock) void k_replay_sample(ReplayView v, int oldest, int stored, int strategy,
                                                                int task, int reward_type, uint64_t h,
                                                                uint64_t threshold, int64_t M, ps_replay_batch out) {
    const int64_t gid = (int64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    const int64_t i = gid / kSampleLanes;
    const int lane = (int)(gid % kSampleLanes);
    if (i >= M) return;
    const int nb = (v.B + kReplayScanBlock - 1) / kReplayScanBlock;
    const int64_t V = v.block_sum[nb - 1];
    if (gid == 0 && out.n_valid) out.n_valid[0] = V;
    const int C = v.R / 4;
    int b = -1, t = -1, g = -1;
    bool relabel = false;
    const float *row = nullptr;
    if (V > 0) {
        const uint64_t w0 = replay_mix(h ^ (uint64_t)(4 * i)), w1 = replay_mix(h ^ (uint64_t)(4 * i + 1)),
                       w2 = replay_mix(h ^ (uint64_t)(4 * i + 2));
        const int64_t r = (int64_t)__umul64hi(w0, (uint64_t)V);
        // the least block whose inclusive total exceeds r, then the least env in it
        int lo = 0, hi = nb - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (v.block_sum[mid] > r) hi = mid; else lo = mid + 1;
        }
        const int32_t rr = (int32_t)(r - (lo > 0 ? v.block_sum[lo - 1] : 0));
        hi = min(v.B, (lo + 1) * kReplayScanBlock) - 1;
        lo = lo * kReplayScanBlock;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (v.prefix[mid] > rr) hi = mid; else lo = mid + 1;
        }
        b = lo;
        const int vb = max(stored - v.cur_len[b], 0);
        int j = rr - (v.prefix[b] - vb);
        // within [0, v_b) for the pos_next / stored of the buffer's own stores; scalars of another history
        // (include/pandasim.h: unspecified samples) are kept inside the ring, here and at ep_end below
        j = j < 0 ? 0 : (j >= v.T ? v.T - 1 : j);
        t = ring_mod(oldest + j, v.T);
        row = v.ring + row_index(v, t, b);
        int e = ((const int32_t *)row)[v.off_ep_end];
        if (e < 0 || e >= v.T) e = t;
        relabel = (w1 >> 32) < threshold;
        const int n = ring_mod(e - t, v.T) + 1;
        g = strategy == PS_REPLAY_FUTURE ? (int)(((int64_t)t + (int64_t)__umul64hi(w2, (uint64_t)n)) % v.T) : e;
    }
    for (int c = lane; c < C; c += kSampleLanes) {
        float4 x4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (row) x4 = *(const float4 *)(row + 4 * c);
        const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int w = 4 * c + k;
            if (w < v.O) {
                out.obs[i * v.O + w] = x[k];
            } else if (w < v.O + v.G) {
                if (out.ag) out.ag[i * v.G + (w - v.O)] = x[k];
            } else if (w < v.off_action) {
                // dg: lane 0, below
            } else if (w < v.off_next_obs) {
                out.action[i * v.A + (w - v.off_action)] = x[k];
            } else if (w < v.off_next_ag) {
                if (out.next_obs) out.next_obs[i * v.O + (w - v.off_next_obs)] = x[k];
            } else if (w < v.off_reward) {
                if (out.next_ag) out.next_ag[i * v.G + (w - v.off_next_ag)] = x[k];
            }
        }
    }
    if (lane != 0) return;
    float reward = 0.0f;
    bool success = false, term = false;
    if (row) {
        const float *a = row + v.off_next_ag;
        const float *d = relabel ? v.ring + row_index(v, g, b) + v.off_next_ag : row + v.O + v.G;
        float rw;
        goal_pair_reward_f32(task, reward_type, a, d, rw, success);
        reward = relabel ? rw : row[v.off_reward];
        term = ((const int32_t *)row)[v.off_terminated] != 0;
        for (int k = 0; k < v.G; k++) out.dg[i * v.G + k] = d[k];
    } else {
        for (int k = 0; k < v.G; k++) out.dg[i * v.G + k] = 0.0f;
    }
    if (out.reward) out.reward[i] = reward;
    if (out.success) out.success[i] = success;
    if (out.terminated) out.terminated[i] = term;
    if (out.relabelled) out.relabelled[i] = relabel;
    if (out.env_idx) out.env_idx[i] = b;
    if (out.slot) out.slot[i] = t;
    if (out.goal_slot) out.goal_slot[i] = relabel ? g : -1;
}

// the checks every replay call shares; fills the layout
int replay_args(ps_ctx *c, const void *replay, int capacity, ps_replay_layout *l) {
    if (!c) return PS_ERR_ARG;
    if (!replay) return fail(c, PS_ERR_ARG, "replay: null buffer");
    // every section starts at a multiple of 256 bytes and is read and written by 128-bit words
    if ((uintptr_t)replay % 16 != 0) return fail(c, PS_ERR_ARG, "replay: the buffer is not 16-byte aligned");
    if (capacity < 1 || capacity > PS_REPLAY_MAX_CAPACITY) return fail(c, PS_ERR_ARG, "replay: capacity out of range");
    if (c->num_envs > PS_REPLAY_MAX_ENVS) return fail(c, PS_ERR_ARG, "replay: more than PS_REPLAY_MAX_ENVS envs");
    replay_layout(c->num_envs, capacity, ps_obs_dim(c), ps_goal_dim(c), ps_action_dim(c), l);
    return PS_OK;
}

// pos_next and stored of a ring after n_stores stores, for some n_stores
bool replay_counts_ok(int capacity, int pos_next, int stored) {
    if (pos_next < 0 || pos_next >= capacity || stored < 0 || stored > capacity) return false;
    return stored == capacity || pos_next == stored;
}

}  // namespace

// ------------------------------------------------------------------- C ABI
extern "C" {

int ps_replay_layout_of(const ps_ctx *c, int capacity, ps_replay_layout *out) {
    if (!c || !out || capacity < 1 || capacity > PS_REPLAY_MAX_CAPACITY || c->num_envs > PS_REPLAY_MAX_ENVS)
        return PS_ERR_ARG;
    replay_layout(c->num_envs, capacity, ps_obs_dim(c), ps_goal_dim(c), ps_action_dim(c), out);
    return PS_OK;
}

int ps_replay_init(ps_ctx *c, void *replay, int capacity, void *stream) {
    ps_replay_layout l;
    if (int rc = replay_args(c, replay, capacity, &l)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(replay, 0, (size_t)l.bytes, st) != hipSuccess) return fail(c, PS_ERR_HIP, "replay init: memset failed");
    hipLaunchKernelGGL(k_replay_init, grid_of((int64_t)l.capacity * l.num_envs, kReplayBlock), dim3(kReplayBlock), 0,
                       st, replay_view(l, replay));
    return check_launch(c);
}

int ps_replay_begin(ps_ctx *c, void *replay, int capacity, int pos_next, int stored, const float *obs,
                    const float *ag, const float *dg, const uint8_t *mask, void *stream) {
    ps_replay_layout l;
    if (int rc = replay_args(c, replay, capacity, &l)) return rc;
    if (!obs || !ag || !dg) return fail(c, PS_ERR_ARG, "replay begin: null observation");
    if (!replay_counts_ok(capacity, pos_next, stored)) return fail(c, PS_ERR_ARG, "replay begin: pos_next or stored out of range");
    hipLaunchKernelGGL(k_replay_begin, grid_of((int64_t)l.num_envs * (l.pending_floats / 4), kReplayBlock),
                       dim3(kReplayBlock), 0, (hipStream_t)stream, replay_view(l, replay), pos_next, obs, ag, dg, mask);
    return check_launch(c);
}

int ps_replay_store(ps_ctx *c, void *replay, int capacity, int pos, const float *actions, const float *obs,
                    const float *ag, const float *dg, const float *final_obs, const float *final_ag,
                    const float *reward, const uint8_t *terminated, const uint8_t *truncated, void *stream) {
    ps_replay_layout l;
    if (int rc = replay_args(c, replay, capacity, &l)) return rc;
    if (!actions || !obs || !ag || !dg || !reward || !terminated || !truncated)
        return fail(c, PS_ERR_ARG, "replay store: null argument");
    if (pos < 0 || pos >= capacity) return fail(c, PS_ERR_ARG, "replay store: pos out of range");
    const ReplayStoreIn in = {actions, obs, ag, dg, final_obs, final_ag, reward, terminated, truncated};
    hipLaunchKernelGGL(k_replay_store, grid_of((int64_t)l.num_envs * (l.row_floats / 4), kReplayBlock),
                       dim3(kReplayBlock), 0, (hipStream_t)stream, replay_view(l, replay), pos, in);
    return check_launch(c);
}

int ps_replay_sample(ps_ctx *c, const void *replay, int capacity, int pos_next, int stored, int strategy,
                     uint64_t seed, uint64_t draw, uint64_t her_threshold, int64_t M, const ps_replay_batch *out,
                     void *stream) {
    ps_replay_layout l;
    if (int rc = replay_args(c, replay, capacity, &l)) return rc;
    if (!out || !out->obs || !out->action || !out->dg) return fail(c, PS_ERR_ARG, "replay sample: null output");
    if (!replay_counts_ok(capacity, pos_next, stored) || stored < 1)
        return fail(c, PS_ERR_ARG, "replay sample: pos_next or stored out of range (or nothing stored)");
    if (M < 1 || M > PS_REPLAY_MAX_BATCH) return fail(c, PS_ERR_ARG, "replay sample: M out of range");
    if (strategy != PS_REPLAY_FUTURE && strategy != PS_REPLAY_FINAL)
        return fail(c, PS_ERR_ARG, "replay sample: unknown strategy");
    if (her_threshold > (1ULL << 32)) return fail(c, PS_ERR_ARG, "replay sample: her_threshold above 2^32");
    hipStream_t st = (hipStream_t)stream;
    // (the prefix sum's workspace is the one part of the buffer a sample writes)
    const ReplayView v = replay_view(l, (void *)replay);
    const int nb = (int)((l.num_envs + kReplayScanBlock - 1) / kReplayScanBlock);
    hipLaunchKernelGGL(k_replay_prefix, dim3(nb), dim3(kReplayScanBlock), 0, st, v, stored);
    if (int rc = check_launch(c)) return rc;
    hipLaunchKernelGGL(k_replay_prefix_blocks, dim3(1), dim3(kReplayScanBlock), 0, st, v, nb);
    if (int rc = check_launch(c)) return rc;
    const uint64_t h = replay_mix(replay_mix(seed) ^ draw);
    const int oldest = ((pos_next - stored) % capacity + capacity) % capacity;
    hipLaunchKernelGGL(k_replay_sample, grid_of(M * kSampleLanes, kReplayBlock), dim3(kReplayBlock), 0, st, v, oldest,
                       stored, strategy, c->cfg.task, c->cfg.reward, h, her_threshold, M, *out);
    return check_launch(c);
}

}  // extern "C"
