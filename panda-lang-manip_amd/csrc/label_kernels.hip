// label_kernels.hip — the ground-truth side of the point-cloud policy, forward
// only, for the context's B clouds on the device (include/pandasim.h):
//
//   k_cloud_labels  record() of the reference's data generation
//                   (task_classes/generate_combined_dset.py:422-484) with the
//                   loader's normalisation of the waypoints
//                   (data_utils/PourDataLoader_cls_off.py:43-45): per point its
//                   class from the two radius tests and the 14 target columns
//                   the head carries behind its logits.  The inverse of
//                   k_cloud_decode.
//   k_cloud_loss    the value of the reference's losses
//                   (models/model_cls_off_rot.py:63-79: F.nll_loss on the
//                   log-softmax, nn.L1Loss on offsets and quaternions) as
//                   per-cloud f64 sums, with the counts of their means, the
//                   accuracy's and the confusion matrix.
//
// k_cloud_labels is per point, without a reduction: one block per (cloud, 256
// points), a lane per point.  The cloud's two waypoints, its centroid and its
// scale are read at addresses the whole block shares, before any store, so
// they arrive once per wave in scalar registers.  A lane reads 24 B and writes
// 60 B; the 14 target columns leave as three 128-bit stores and a 64-bit one
// where the row stride, the column offset and the base address are multiples
// of 16 B, as seven 64-bit stores where they are multiples of 8 B (the plain
// [B, N, 14] target), else as 14 dword stores.
//
// k_cloud_loss has k_cloud_decode's shape and its reasons (decode_kernels.hip):
// a workgroup of 1024 owns a cloud and walks its rows once, thread t the rows
// t, t + 1024, ...; five f64 partial sums per thread meet in an LDS tree by
// halving (40 KiB), the four counts by wave shuffles and one LDS word per wave,
// the confusion matrix by integer LDS atomics (whole numbers: any order gives
// the same).  No atomics on floating-point values, nothing shared between
// workgroups.
#include <stdint.h>

#include "ps_cloud_math.h"

namespace {

constexpr int kLabelBlock = 256;
constexpr int kLabelColumns = PS_CLOUD_LABEL_COLUMNS;
constexpr int kLossThreads = 1024;
constexpr int kLossWaves = kLossThreads / 64;
constexpr int kLossSums = 5;    // nll, |d| start offset, end offset, start quaternion, end quaternion
constexpr int kLossCounts = 4;  // labelled, in the start set, in the end set, predicted right
static_assert(kLabelColumns == 14, "two offsets of 3 and two quaternions of 4");
static_assert(PS_CLOUD_DECODE_MAX_CLASSES * PS_CLOUD_DECODE_MAX_CLASSES <= kLossThreads,
              "one thread per cell of the confusion matrix");

// the 14 columns of one row, V floats per store (the launcher picks V from the
// alignment of the rows)
template <int V>
PS_D void store_columns(float *row, const float (&v)[kLabelColumns]) {
    if constexpr (V == 4) {
        float4 *r4 = reinterpret_cast<float4 *>(row);
        r4[0] = make_float4(v[0], v[1], v[2], v[3]);
        r4[1] = make_float4(v[4], v[5], v[6], v[7]);
        r4[2] = make_float4(v[8], v[9], v[10], v[11]);
        *reinterpret_cast<float2 *>(row + 12) = make_float2(v[12], v[13]);
    } else if constexpr (V == 2) {
        float2 *r2 = reinterpret_cast<float2 *>(row);
#pragma unroll
        for (int k = 0; k < kLabelColumns / 2; k++) r2[k] = make_float2(v[2 * k], v[2 * k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < kLabelColumns; k++) row[k] = v[k];
    }
}

template <int V>
__global__ __launch_bounds__(kLabelBlock) void k_cloud_labels(const float *points, const float *xyz,
                                                              const float *centroid, const float *scale,
                                                              const float *waypoints, const float *quats, float r2,
                                                              const int32_t *count, int n, int32_t *cls,
                                                              float *target, int ld, int offset) {
#pragma clang fp contract(off)
    const int64_t env = blockIdx.x;
    // the same addresses for the whole block
    const float sc = scale[env];
    const bool empty = count && count[env] == 0;
    float w[2][3], wn[2][3], q[2][4];
#pragma unroll
    for (int k = 0; k < 2; k++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            w[k][c] = waypoints[(env * 2 + k) * 3 + c];
            wn[k][c] = (w[k][c] - centroid[env * 3 + c]) / sc;  // ps_cloud_normalize's expression
        }
#pragma unroll
        for (int c = 0; c < 4; c++) q[k][c] = quats[(env * 2 + k) * 4 + c];
    }
    const int64_t j = (int64_t)blockIdx.y * kLabelBlock + threadIdx.x;
    if (j >= n) return;
    const int64_t at = env * n + j;
    const float *p = points + at * 3, *x = xyz + at * 3;
    const float px = p[0], py = p[1], pz = p[2];
    // a NaN distance is in no set: the comparison is false
    const bool in0 = !empty && dist2(px, py, pz, w[0][0], w[0][1], w[0][2]) <= r2;
    const bool in1 = !empty && dist2(px, py, pz, w[1][0], w[1][1], w[1][2]) <= r2;
    const bool off0 = in0 && sc > 0.0f, off1 = in1 && sc > 0.0f;  // a cloud of scale 0: zero offsets
    float v[kLabelColumns];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float xc = x[c];
        v[c] = off0 ? xc - wn[0][c] : 0.0f;
        v[3 + c] = off1 ? xc - wn[1][c] : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        v[6 + c] = in0 ? q[0][c] : 0.0f;
        v[10 + c] = in1 ? q[1][c] : 0.0f;
    }
    cls[at] = empty ? -1 : (int)in0 + 2 * (int)in1;
    store_columns<V>(target + at * ld + offset, v);
}

__global__ __launch_bounds__(kLossThreads) void k_cloud_loss(const float *head, int n, int ld, int nc,
                                                             const int32_t *cls, const float *target, int ld_t,
                                                             int t_off, uint32_t mask0, uint32_t mask1, double *sums,
                                                             int32_t *counts, int32_t *confusion) {
#pragma clang fp contract(off)
    __shared__ double red[kLossSums * kLossThreads];
    __shared__ int32_t s_cnt[kLossCounts][kLossWaves];
    __shared__ int32_t s_conf[PS_CLOUD_DECODE_MAX_CLASSES * PS_CLOUD_DECODE_MAX_CLASSES];
    const int t = threadIdx.x;
    const int64_t env = blockIdx.x;
    const float *rows = head + env * n * ld;
    const float *trows = target + env * n * ld_t + t_off;
    const int32_t *truth = cls + env * n;
    if (confusion) {
        if (t < nc * nc) s_conf[t] = 0;
        __syncthreads();
    }
    double sum[kLossSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt[kLossCounts] = {0, 0, 0, 0};
    for (int i = t; i < n; i += kLossThreads) {
        const int c = truth[i];
        if (c < 0 || c >= nc) continue;  // -1, or anything else that is no class: ignored everywhere
        const float *row = rows + (int64_t)i * ld;
        const float *tr = trows + (int64_t)i * ld_t;
        double m = (double)row[0];
        for (int k = 1; k < nc; k++) {
            const double xk = (double)row[k];
            if (xk > m) m = xk;
        }
        double s = 0.0;
        for (int k = 0; k < nc; k++) s += exp((double)row[k] - m);
        const double lse = m + log(s);
        sum[0] += lse - (double)row[c];
        const int pred = cloud_argmax(row, nc);
        cnt[0] += 1;
        cnt[3] += pred == c ? 1 : 0;
        if (confusion) atomicAdd(&s_conf[c * nc + pred], 1);
        if ((mask0 >> c) & 1u) {
            cnt[1] += 1;
#pragma unroll
            for (int k = 0; k < 3; k++) sum[1] += fabs((double)row[nc + k] - (double)tr[k]);
#pragma unroll
            for (int k = 0; k < 4; k++) sum[3] += fabs((double)row[nc + 6 + k] - (double)tr[6 + k]);
        }
        if ((mask1 >> c) & 1u) {
            cnt[2] += 1;
#pragma unroll
            for (int k = 0; k < 3; k++) sum[2] += fabs((double)row[nc + 3 + k] - (double)tr[3 + k]);
#pragma unroll
            for (int k = 0; k < 4; k++) sum[4] += fabs((double)row[nc + 10 + k] - (double)tr[10 + k]);
        }
    }
#pragma unroll
    for (int k = 0; k < kLossSums; k++) red[k * kLossThreads + t] = sum[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kLossCounts; k++) cnt[k] += __shfl_down(cnt[k], off);
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kLossCounts; k++) s_cnt[k][t >> 6] = cnt[k];
    }
    __syncthreads();
    for (int h = kLossThreads / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < kLossSums; k++) red[k * kLossThreads + t] += red[k * kLossThreads + t + h];
        }
        __syncthreads();
    }
    if (t < kLossSums) sums[env * kLossSums + t] = red[t * kLossThreads];
    if (t < kLossCounts) {
        int total = 0;
        for (int w = 0; w < kLossWaves; w++) total += s_cnt[t][w];
        counts[env * kLossCounts + t] = total;
    }
    if (confusion && t < nc * nc) confusion[env * nc * nc + t] = s_conf[t];
}

inline bool aligned_to(const void *p, int64_t a, int64_t b, int bytes) {
    return (uintptr_t)p % bytes == 0 && (a * 4) % bytes == 0 && (b * 4) % bytes == 0;
}

}  // namespace

extern "C" {

int ps_cloud_waypoint_labels(ps_ctx *c, const float *points, const float *xyz, const float *centroid,
                             const float *scale, const float *waypoints, const float *quats, double radius,
                             const int32_t *count, int n, int32_t *cls, float *target, int ld, int out_offset,
                             void *stream) {
    if (!c || !points || !xyz || !centroid || !scale || !waypoints || !quats || !cls || !target)
        return fail(c, PS_ERR_ARG, "null argument");
    if (n < 1 || n > PS_CLOUD_MAX_DENSE_POINTS) return fail(c, PS_ERR_ARG, "N outside 1..2^20");
    if (!(radius > 0.0) || radius == __builtin_inf()) return fail(c, PS_ERR_ARG, "radius must be positive and finite");
    if (out_offset < 0 || ld > PS_CLOUD_LABEL_MAX_LD || (int64_t)out_offset + kLabelColumns > ld)
        return fail(c, PS_ERR_ARG, "the 14 target columns do not fit ld (at most 4096)");
    const float rf = (float)radius;
    const float r2 = rf * rf;
    const dim3 grid((unsigned)c->num_envs, (unsigned)((n + kLabelBlock - 1) / kLabelBlock));
    hipStream_t st = (hipStream_t)stream;
#define PS_LABELS_LAUNCH(V)                                                                                       \
    hipLaunchKernelGGL(k_cloud_labels<V>, grid, dim3(kLabelBlock), 0, st, points, xyz, centroid, scale, waypoints, \
                       quats, r2, count, n, cls, target, ld, out_offset)
    if (aligned_to(target, ld, out_offset, 16))
        PS_LABELS_LAUNCH(4);
    else if (aligned_to(target, ld, out_offset, 8))
        PS_LABELS_LAUNCH(2);
    else
        PS_LABELS_LAUNCH(1);
#undef PS_LABELS_LAUNCH
    return check_launch(c);
}

int ps_cloud_policy_loss(ps_ctx *c, const float *head, int n, int ld, int nc, const int32_t *cls, const float *target,
                         int ld_t, int target_offset, uint32_t start_mask, uint32_t end_mask, double *sums,
                         int32_t *counts, int32_t *confusion, void *stream) {
    if (!c || !head || !cls || !target || !sums || !counts) return fail(c, PS_ERR_ARG, "null argument");
    if (n < 1 || n > PS_CLOUD_MAX_DENSE_POINTS) return fail(c, PS_ERR_ARG, "N outside 1..2^20");
    if (nc < 2 || nc > PS_CLOUD_DECODE_MAX_CLASSES) return fail(c, PS_ERR_ARG, "nc outside 2..16");
    if (ld < nc + kLabelColumns || ld > PS_CLOUD_DECODE_MAX_LD)
        return fail(c, PS_ERR_ARG, "ld outside nc + 14 .. 4096");
    if (target_offset < 0 || ld_t > PS_CLOUD_LABEL_MAX_LD || (int64_t)target_offset + kLabelColumns > ld_t)
        return fail(c, PS_ERR_ARG, "the 14 target columns do not fit ld_t (at most 4096)");
    if (start_mask == 0 || end_mask == 0 || (start_mask >> nc) != 0 || (end_mask >> nc) != 0)
        return fail(c, PS_ERR_ARG, "a class mask is empty or names a class at or above nc");
    hipLaunchKernelGGL(k_cloud_loss, dim3((unsigned)c->num_envs), dim3(kLossThreads), 0, (hipStream_t)stream, head, n,
                       ld, nc, cls, target, ld_t, target_offset, start_mask, end_mask, sums, counts, confusion);
    return check_launch(c);
}

}  // extern "C"
