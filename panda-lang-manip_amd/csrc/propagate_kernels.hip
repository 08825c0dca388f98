// propagate_kernels.hip — the interpolation of PointNetFeaturePropagation.forward
// (pointnet2_utils.py:276-310) for the context's B clouds: per dense point the
// three nearest coarse points, inverse-distance weights, the weighted sum of
// their features behind the dense point's own.  Three kernels over the same
// two device functions (nn3_of_block, interp_rows), so that the fused call is
// the two single calls' arithmetic:
//   k_cloud_three_nn      a block stages its cloud's S coarse points in LDS
//                         (x[S], y[S], z[S], as k_cloud_fps) and finds the
//                         3-NN of kPropBlock / L dense points, L = 1 or 4
//                         lanes per dense point; the best three (distance,
//                         index) of a lane live in registers, the insertion is
//                         selects only; L lanes merge by two xor-shuffles;
//   k_cloud_interpolate   a block writes kInterpRows rows of out, lanes
//                         across the channels of consecutive rows;
//   k_cloud_propagate     the first, idx and weight left in LDS, then the
//                         second on the same rows.
// There is no distance matrix and no sort: B * N * S distances are computed
// and dropped, B * N * 3 kept.
#include "ps_cloud_math.h"

namespace {

constexpr int kPropBlock = 256;
constexpr int kPropSplit = 4;    // lanes per dense point of the split walk
constexpr int kInterpRows = 64;  // rows of out per block of k_cloud_interpolate
// One lane per dense point gives B * ceil(N / 256) blocks.  Below eight blocks
// per compute unit of the 256 (full occupancy of this kernel) the walk is
// split over 4 lanes: 64 points per block, four times the blocks, a quarter of
// the walk each -- and a quarter of the rows of out per block, which is what
// the fused kernel's second, memory-bound half wants when blocks are few.
constexpr int64_t kSplitBelowBlocks = 2048;
constexpr int kPropMaxS = PS_CLOUD_MAX_POINTS;
constexpr int kPropMaxN = PS_CLOUD_MAX_DENSE_POINTS;

// The best three of a walk, ascending by (distance, index).
struct Nn3 {
    float d0, d1, d2;
    int i0, i1, i2;
};

PS_D Nn3 nn3_empty() { return Nn3{INFINITY, INFINITY, INFINITY, 0, 0, 0}; }

// Insert (d, i); lt0..lt2 tell whether it sorts before each kept entry.
PS_D void nn3_put(Nn3 &b, float d, int i, bool lt0, bool lt1, bool lt2) {
    b.d2 = lt1 ? b.d1 : (lt2 ? d : b.d2);
    b.i2 = lt1 ? b.i1 : (lt2 ? i : b.i2);
    b.d1 = lt0 ? b.d0 : (lt1 ? d : b.d1);
    b.i1 = lt0 ? b.i0 : (lt1 ? i : b.i1);
    b.d0 = lt0 ? d : b.d0;
    b.i0 = lt0 ? i : b.i0;
}

// A walk in ascending index order: a strict < leaves equal distances to the
// lower index, which came first.
PS_D void nn3_insert_ascending(Nn3 &b, float d, int i) { nn3_put(b, d, i, d < b.d0, d < b.d1, d < b.d2); }

// Any order (the merge of the split walk): (distance, then lowest index).
PS_D bool nn3_before(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }
PS_D void nn3_insert(Nn3 &b, float d, int i) {
    nn3_put(b, d, i, nn3_before(d, i, b.d0, b.i0), nn3_before(d, i, b.d1, b.i1), nn3_before(d, i, b.d2, b.i2));
}

// The block's `P = kPropBlock / L` dense points p0 .. p0 + P - 1 of cloud
// `env`: idx and weight into s_idx[P * 3], s_w[P * 3] (LDS).  Ends with a
// barrier.  sx/sy/sz: dynamic LDS of 3 * s floats.
template <int L>
PS_D void nn3_of_block(const float *xyz1, int n, const float *xyz2, int s, int64_t env, int p0, float *cloud,
                       int32_t *s_idx, float *s_w) {
#pragma clang fp contract(off)
    constexpr int P = kPropBlock / L;
    const int t = threadIdx.x;
    if (s == 1) {  // the reference's repeat
        for (int e = t; e < P * 3; e += kPropBlock) {
            s_idx[e] = 0;
            s_w[e] = e % 3 == 0 ? 1.0f : 0.0f;
        }
        __syncthreads();
        return;
    }
    float *sx = cloud, *sy = cloud + s, *sz = cloud + 2 * s;
    const float *q = xyz2 + env * s * 3;
    for (int j = t; j < s; j += kPropBlock) {
        sx[j] = q[(int64_t)j * 3 + 0];
        sy[j] = q[(int64_t)j * 3 + 1];
        sz[j] = q[(int64_t)j * 3 + 2];
    }
    __syncthreads();
    const int local = t / L, part = t % L;
    const int gp = p0 + local < n ? p0 + local : n - 1;  // a lane past the cloud repeats its last point
    const float *a = xyz1 + (env * n + gp) * 3;
    const float ax = a[0], ay = a[1], az = a[2];
    Nn3 b = nn3_empty();
#pragma unroll 4
    for (int j = part; j < s; j += L) nn3_insert_ascending(b, dist2(ax, ay, az, sx[j], sy[j], sz[j]), j);
    if constexpr (L > 1) {
        // the L lanes of a point are neighbours in the wave; after exchanging
        // with lane ^ 1 and lane ^ 2 all four hold the same three
#pragma unroll
        for (int off = 1; off < L; off <<= 1) {
            const float e0 = __shfl_xor(b.d0, off), e1 = __shfl_xor(b.d1, off), e2 = __shfl_xor(b.d2, off);
            const int j0 = __shfl_xor(b.i0, off), j1 = __shfl_xor(b.i1, off), j2 = __shfl_xor(b.i2, off);
            nn3_insert(b, e0, j0);
            nn3_insert(b, e1, j1);
            nn3_insert(b, e2, j2);
        }
    }
    if (part == 0) {
        const float w0 = 1.0f / (b.d0 + 1e-8f), w1 = 1.0f / (b.d1 + 1e-8f), w2 = 1.0f / (b.d2 + 1e-8f);
        const float norm = (w0 + w1) + w2;
        s_idx[local * 3 + 0] = b.i0;
        s_idx[local * 3 + 1] = b.i1;
        s_idx[local * 3 + 2] = b.i2;
        s_w[local * 3 + 0] = w0 / norm;
        s_w[local * 3 + 1] = w1 / norm;
        s_w[local * 3 + 2] = w2 / norm;
    }
    __syncthreads();
}

// idx and weight of rows p0 .. p0 + rows - 1 from LDS to global memory, coalesced
PS_D void nn3_store(int n, int64_t env, int p0, int rows, const int32_t *s_idx, const float *s_w, int32_t *idx,
                    float *weight) {
    const int64_t base = (env * n + p0) * 3;
    for (int e = threadIdx.x; e < rows * 3; e += kPropBlock) {
        if (idx) idx[base + e] = s_idx[e];
        if (weight) weight[base + e] = s_w[e];
    }
}

// Rows p0 .. p0 + rows - 1 of out [B, N, d1 + d2], lanes across the channels
// of consecutive rows (the rows of a block are contiguous in out).  idx and
// w hold the rows' three indices and weights at [r * 3 + k], r from 0; the
// indices are inside 0..s-1.  rows * (d1 + d2) <= 256 * 4096 = 2^20: exact in
// f32, so element / channels is the truncated f32 quotient, off by at most
// one and then corrected.
PS_D void interp_rows(const float *points1, int d1, const float *points2, int d2, int n, int s, int64_t env, int p0,
                      int rows, const int32_t *idx, const float *w, float *out) {
#pragma clang fp contract(off)
    const int ch_n = d1 + d2, total = rows * ch_n;
    const float inv = 1.0f / (float)ch_n;
    const float *f2 = points2 + env * s * d2;
    const int64_t row0 = env * n + p0;
    for (int e = threadIdx.x; e < total; e += kPropBlock) {
        int r = (int)((float)e * inv);
        int ch = e - r * ch_n;
        if (ch < 0) {
            r -= 1;
            ch += ch_n;
        } else if (ch >= ch_n) {
            r += 1;
            ch -= ch_n;
        }
        float v;
        if (ch < d1) {
            v = points1[(row0 + r) * d1 + ch];
        } else if (s == 1) {
            v = f2[ch - d1];
        } else {
            const int c = ch - d1;
            const float a0 = f2[(int64_t)idx[r * 3 + 0] * d2 + c], a1 = f2[(int64_t)idx[r * 3 + 1] * d2 + c],
                        a2 = f2[(int64_t)idx[r * 3 + 2] * d2 + c];
            v = (rounded(a0 * w[r * 3 + 0]) + rounded(a1 * w[r * 3 + 1])) + rounded(a2 * w[r * 3 + 2]);
        }
        out[row0 * ch_n + e] = v;
    }
}

// x clouds, y blocks of kPropBlock / L dense points
template <int L>
__global__ __launch_bounds__(kPropBlock) void k_cloud_three_nn(const float *xyz1, int n, const float *xyz2, int s,
                                                               int32_t *idx, float *weight) {
    extern __shared__ __align__(16) float cloud[];  // x[s], y[s], z[s]
    constexpr int P = kPropBlock / L;
    __shared__ int32_t s_idx[P * 3];
    __shared__ float s_w[P * 3];
    const int64_t env = blockIdx.x;
    const int p0 = blockIdx.y * P;
    nn3_of_block<L>(xyz1, n, xyz2, s, env, p0, cloud, s_idx, s_w);
    nn3_store(n, env, p0, n - p0 < P ? n - p0 : P, s_idx, s_w, idx, weight);
}

// x clouds, y blocks of kInterpRows rows; idx and weight from global memory
// into LDS, the indices clamped into the cloud on the way
__global__ __launch_bounds__(kPropBlock) void k_cloud_interpolate(const float *points1, int d1, const float *points2,
                                                                  int d2, int n, int s, const int32_t *idx,
                                                                  const float *weight, float *out) {
    __shared__ int32_t s_idx[kInterpRows * 3];
    __shared__ float s_w[kInterpRows * 3];
    const int64_t env = blockIdx.x;
    const int p0 = blockIdx.y * kInterpRows;
    const int rows = n - p0 < kInterpRows ? n - p0 : kInterpRows;
    if (s > 1) {
        const int64_t base = (env * n + p0) * 3;
        for (int e = threadIdx.x; e < rows * 3; e += kPropBlock) {
            s_idx[e] = clamp_index(idx[base + e], s);
            s_w[e] = weight[base + e];
        }
        __syncthreads();
    }
    interp_rows(points1, d1, points2, d2, n, s, env, p0, rows, s_idx, s_w, out);
}

template <int L>
__global__ __launch_bounds__(kPropBlock) void k_cloud_propagate(const float *xyz1, int n, const float *xyz2, int s,
                                                                const float *points1, int d1, const float *points2,
                                                                int d2, float *out, int32_t *idx, float *weight) {
    extern __shared__ __align__(16) float cloud[];  // x[s], y[s], z[s]
    constexpr int P = kPropBlock / L;
    __shared__ int32_t s_idx[P * 3];
    __shared__ float s_w[P * 3];
    const int64_t env = blockIdx.x;
    const int p0 = blockIdx.y * P;
    const int rows = n - p0 < P ? n - p0 : P;
    nn3_of_block<L>(xyz1, n, xyz2, s, env, p0, cloud, s_idx, s_w);
    if (idx || weight) nn3_store(n, env, p0, rows, s_idx, s_w, idx, weight);
    interp_rows(points1, d1, points2, d2, n, s, env, p0, rows, s_idx, s_w, out);
}

// ------------------------------------------------------------- host side
inline const char *nn_shape_error(int n, int s) {
    if (n < 1 || n > kPropMaxN) return "N outside 1..2^20";
    if (s < 1 || s > kPropMaxS) return "S outside 1..8192";
    if (s == 2) return "S = 2: the reference's interpolation needs three coarse points (or one)";
    return nullptr;
}

inline const char *width_error(const float *points1, int d1, int d2) {
    if (d2 < 1 || d2 > PS_CLOUD_MAX_PROP_FEATURES) return "D2 outside 1..2048";
    if (d1 < 0 || d1 > PS_CLOUD_MAX_PROP_FEATURES) return "D1 outside 0..2048";
    if ((points1 == nullptr) != (d1 == 0)) return "D1 and points1 disagree";
    return nullptr;
}

inline int lanes_per_point(const ps_ctx *c, int n) {
    return c->num_envs * ((n + kPropBlock - 1) / kPropBlock) < kSplitBelowBlocks ? kPropSplit : 1;
}

template <typename K>
inline int coarse_lds(ps_ctx *c, K kernel) {
    // 12 B per coarse point: above 64 KiB a kernel's dynamic LDS has to be allowed first
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * 3 * kPropMaxS)) != hipSuccess)
        return fail(c, PS_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    return PS_OK;
}

inline dim3 point_grid(const ps_ctx *c, int n, int per_block) {
    return dim3((unsigned)c->num_envs, (unsigned)((n + per_block - 1) / per_block));
}

template <int L>
int launch_three_nn(ps_ctx *c, const float *xyz1, int n, const float *xyz2, int s, int32_t *idx, float *weight,
                    hipStream_t st) {
    int rc = coarse_lds(c, k_cloud_three_nn<L>);
    if (rc != PS_OK) return rc;
    hipLaunchKernelGGL(k_cloud_three_nn<L>, point_grid(c, n, kPropBlock / L), dim3(kPropBlock),
                       s > 1 ? sizeof(float) * 3 * s : 0, st, xyz1, n, xyz2, s, idx, weight);
    return check_launch(c);
}

template <int L>
int launch_propagate(ps_ctx *c, const float *xyz1, int n, const float *xyz2, int s, const float *points1, int d1,
                     const float *points2, int d2, float *out, int32_t *idx, float *weight, hipStream_t st) {
    int rc = coarse_lds(c, k_cloud_propagate<L>);
    if (rc != PS_OK) return rc;
    hipLaunchKernelGGL(k_cloud_propagate<L>, point_grid(c, n, kPropBlock / L), dim3(kPropBlock),
                       s > 1 ? sizeof(float) * 3 * s : 0, st, xyz1, n, xyz2, s, points1, d1, points2, d2, out, idx,
                       weight);
    return check_launch(c);
}

}  // namespace

extern "C" {

int ps_cloud_three_nn(ps_ctx *c, const float *xyz1, int n, const float *xyz2, int s, int32_t *idx, float *weight,
                      void *stream) {
    if (!c || !xyz1 || !xyz2 || !idx || !weight) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = nn_shape_error(n, s)) return fail(c, PS_ERR_ARG, e);
    return lanes_per_point(c, n) == 1 ? launch_three_nn<1>(c, xyz1, n, xyz2, s, idx, weight, (hipStream_t)stream)
                                      : launch_three_nn<kPropSplit>(c, xyz1, n, xyz2, s, idx, weight,
                                                                    (hipStream_t)stream);
}

int ps_cloud_interpolate(ps_ctx *c, const float *points1, int d1, const float *points2, int d2, int n, int s,
                         const int32_t *idx, const float *weight, float *out, void *stream) {
    if (!c || !points2 || !idx || !weight || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = nn_shape_error(n, s)) return fail(c, PS_ERR_ARG, e);
    if (const char *e = width_error(points1, d1, d2)) return fail(c, PS_ERR_ARG, e);
    hipLaunchKernelGGL(k_cloud_interpolate, point_grid(c, n, kInterpRows), dim3(kPropBlock), 0, (hipStream_t)stream,
                       points1, d1, points2, d2, n, s, idx, weight, out);
    return check_launch(c);
}

int ps_cloud_feature_propagation(ps_ctx *c, const float *xyz1, int n, const float *xyz2, int s, const float *points1,
                                 int d1, const float *points2, int d2, float *out, int32_t *idx, float *weight,
                                 void *stream) {
    if (!c || !xyz1 || !xyz2 || !points2 || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = nn_shape_error(n, s)) return fail(c, PS_ERR_ARG, e);
    if (const char *e = width_error(points1, d1, d2)) return fail(c, PS_ERR_ARG, e);
    hipStream_t st = (hipStream_t)stream;
    return lanes_per_point(c, n) == 1
               ? launch_propagate<1>(c, xyz1, n, xyz2, s, points1, d1, points2, d2, out, idx, weight, st)
               : launch_propagate<kPropSplit>(c, xyz1, n, xyz2, s, points1, d1, points2, d2, out, idx, weight, st);
}

}  // extern "C"
