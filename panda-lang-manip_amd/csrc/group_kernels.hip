// group_kernels.hip — the PointNet++ front end of the point-cloud observation
// (pointnet2_utils.py: pc_normalize, farthest_point_sample, query_ball_point,
// index_points and the centring of PointNetSetAbstractionMsg.forward), for the
// context's B clouds of N points each.  Four kernels:
//   k_cloud_normalize  one block per cloud: f64 centroid in a fixed order, the
//                      largest radius, (p - c) / scale;
//   k_cloud_fps        one block of 1 024 lanes per cloud: the points in LDS
//                      (for the centre of each iteration), every lane's own
//                      <= 8 points and running distances in registers, the
//                      arg-max as a 64-bit key (distance bits, ~index) reduced
//                      by shuffles in the wave and through LDS across waves;
//   k_cloud_query      one wave per centre, up to four radii in the same scan
//                      of the cloud's points from LDS in index order: ballot +
//                      popcount compaction, no sort and no distance matrix;
//   k_cloud_group      one lane per output element: the gathers and the
//                      centring.
// ps_cloud_set_abstraction launches the same kernels on the same arguments as
// the four single calls, so its result is theirs bit for bit.
//
// The squared distance is (dx*dx + dy*dy) + dz*dz with every product and sum
// rounded to f32 (dist2): the form that reproduces the reference's FPS index
// for index; an FMA or another tie-break gives other indices.
#include "ps_cloud_math.h"

namespace {

constexpr int kGroupMaxN = PS_CLOUD_MAX_POINTS;  // 12 B of LDS per point: 96 KiB
constexpr int kFpsBlock = 1024;
constexpr int kFpsPer = kGroupMaxN / kFpsBlock;  // points a lane owns (i = lane + k * 1024)
constexpr int kFpsWaves = kFpsBlock / 64;
constexpr int kNormBlock = 256;
constexpr int kQueryBlock = 256;
constexpr int kQueryCentres = 64;  // centres of one block (16 per wave), which stages the cloud once
constexpr int kGatherBlock = 256;
constexpr int kGatherMaxBlocks = 1024;  // per (cloud, scale); the rest by a grid stride
static_assert(kFpsPer * kFpsBlock == kGroupMaxN && kFpsPer == 8, "a lane owns at most 8 points");

// rounded(), dist2() and clamp_index() are ps_cloud_math.h's, shared with
// propagate_kernels.hip

// ------------------------------------------------------------- normalise
// The mean's order: lane t of 256 adds rows t, t + 256, ... in f64, the 256
// partial sums are added by halving (t += t + 128, + 64, ... + 1).  The block
// size is part of the definition, not of the launch.
__global__ __launch_bounds__(kNormBlock) void k_cloud_normalize(const float *points, int n, float *xyz_out,
                                                                float *centroid, float *scale) {
#pragma clang fp contract(off)
    __shared__ double part[3][kNormBlock];
    __shared__ float wmax[kNormBlock / 64];
    const int t = threadIdx.x;
    const int64_t env = blockIdx.x;
    const float *p = points + env * n * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = t; i < n; i += kNormBlock) {
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] += (double)p[(int64_t)i * 3 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) part[k][t] = s[k];
    __syncthreads();
    for (int h = kNormBlock / 2; h >= 1; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < 3; k++) part[k][t] += part[k][t + h];
        }
        __syncthreads();
    }
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = (float)(part[k][0] / (double)n);
    // the largest radius: sqrt is monotone, so the root of the largest square
    float m = 0.0f;
    for (int i = t; i < n; i += kNormBlock) {
        const float *q = p + (int64_t)i * 3;
        m = fmaxf(m, dist2(q[0], q[1], q[2], c[0], c[1], c[2]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((t & 63) == 0) wmax[t >> 6] = m;
    __syncthreads();
    m = wmax[0];
#pragma unroll
    for (int w = 1; w < kNormBlock / 64; w++) m = fmaxf(m, wmax[w]);
    const float sc = sqrtf(m);
    if (t < 3) centroid[env * 3 + t] = t == 0 ? c[0] : (t == 1 ? c[1] : c[2]);
    if (t == 0) scale[env] = sc;
    float *out = xyz_out + env * n * 3;
    for (int e = t; e < n * 3; e += kNormBlock) {
        const int k = e % 3;
        const float ck = k == 0 ? c[0] : (k == 1 ? c[1] : c[2]);
        out[e] = sc > 0.0f ? (p[e] - ck) / sc : 0.0f;
    }
}

// ------------------------------------------------- farthest point sampling
// dist >= +0 always (a sum of squares, or the initial 1e10), so its bits order
// as the floats do; ~index in the low word makes the largest key the lowest
// index among equal distances.  A lane without points holds key 0, below every
// real key.
__global__ __launch_bounds__(kFpsBlock) void k_cloud_fps(const float *xyz, int n, const int32_t *start, int s,
                                                         int32_t *idx) {
    extern __shared__ __align__(16) float cloud[];  // x[n], y[n], z[n]
    __shared__ unsigned long long best[2][kFpsWaves];
    float *sx = cloud, *sy = cloud + n, *sz = cloud + 2 * n;
    const int t = threadIdx.x;
    const int64_t env = blockIdx.x;
    const float *p = xyz + env * n * 3;
    float px[kFpsPer], py[kFpsPer], pz[kFpsPer], dist[kFpsPer];
#pragma unroll
    for (int k = 0; k < kFpsPer; k++) {
        const int i = t + k * kFpsBlock;
        px[k] = py[k] = pz[k] = 0.0f;
        dist[k] = 1e10f;
        if (i < n) {
            px[k] = sx[i] = p[(int64_t)i * 3 + 0];
            py[k] = sy[i] = p[(int64_t)i * 3 + 1];
            pz[k] = sz[i] = p[(int64_t)i * 3 + 2];
        }
    }
    int far = clamp_index(start[env], n);
    __syncthreads();
    for (int it = 0; it < s; it++) {
        if (t == 0) idx[env * s + it] = far;
        const float cx = sx[far], cy = sy[far], cz = sz[far];
        unsigned long long key = 0ull;
#pragma unroll
        for (int k = 0; k < kFpsPer; k++) {
            const int i = t + k * kFpsBlock;
            if (i < n) {
                const float d2 = dist2(px[k], py[k], pz[k], cx, cy, cz);
                if (d2 < dist[k]) dist[k] = d2;
                const unsigned long long mine =
                    ((unsigned long long)__float_as_uint(dist[k]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
                key = mine > key ? mine : key;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long other = __shfl_xor(key, off);
            key = other > key ? other : key;
        }
        // two buffers: a wave two iterations ahead cannot exist (the barrier of
        // the iteration between needs every wave past these reads)
        if ((t & 63) == 0) best[it & 1][t >> 6] = key;
        __syncthreads();
        key = best[it & 1][0];
#pragma unroll
        for (int w = 1; w < kFpsWaves; w++) {
            const unsigned long long other = best[it & 1][w];
            key = other > key ? other : key;
        }
        far = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    }
}

// ------------------------------------------------------------- ball query
struct QueryArgs {
    float r2[PS_CLOUD_MAX_SCALES];
    int nsample[PS_CLOUD_MAX_SCALES];
    int32_t *gidx[PS_CLOUD_MAX_SCALES];  // [B, S, nsample]
    int n_scales;
};

// x clouds, y blocks of kQueryCentres centres.  A wave takes a centre and
// walks the cloud 64 points at a time in index order; per radius the ballot of
// "not d2 > r2" is compacted behind the indices already kept.  A radius whose
// row is full drops out; the walk ends when all are full.
__global__ __launch_bounds__(kQueryBlock) void k_cloud_query(const float *xyz, int n, const int32_t *centre_idx, int s,
                                                             QueryArgs Q) {
    extern __shared__ __align__(16) float cloud[];  // x[n], y[n], z[n]
    float *sx = cloud, *sy = cloud + n, *sz = cloud + 2 * n;
    const int t = threadIdx.x, lane = t & 63;
    const int64_t env = blockIdx.x;
    const float *p = xyz + env * n * 3;
    for (int i = t; i < n; i += kQueryBlock) {
        sx[i] = p[(int64_t)i * 3 + 0];
        sy[i] = p[(int64_t)i * 3 + 1];
        sz[i] = p[(int64_t)i * 3 + 2];
    }
    __syncthreads();
    const int c_begin = blockIdx.y * kQueryCentres;
    const int c_end = c_begin + kQueryCentres < s ? c_begin + kQueryCentres : s;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c = c_begin + (t >> 6); c < c_end; c += kQueryBlock / 64) {
        const int ci = clamp_index(centre_idx[env * s + c], n);
        const float cx = sx[ci], cy = sy[ci], cz = sz[ci];
        const int64_t row = env * s + c;
        int cnt[PS_CLOUD_MAX_SCALES], first[PS_CLOUD_MAX_SCALES];
#pragma unroll
        for (int q = 0; q < PS_CLOUD_MAX_SCALES; q++) {
            cnt[q] = 0;
            first[q] = ci;  // the centre itself is always within the radius (d2 = 0)
        }
        bool open = true;
        for (int base = 0; base < n && open; base += 64) {
            const int i = base + lane;
            const bool in = i < n;
            const float d2 = in ? dist2(sx[i], sy[i], sz[i], cx, cy, cz) : 0.0f;
            open = false;
#pragma unroll
            for (int q = 0; q < PS_CLOUD_MAX_SCALES; q++) {
                if (q < Q.n_scales && cnt[q] < Q.nsample[q]) {
                    const bool ok = in && !(d2 > Q.r2[q]);
                    const unsigned long long m = __ballot(ok);
                    if (m) {
                        if (cnt[q] == 0) first[q] = base + (__ffsll((long long)m) - 1);
                        const int pos = cnt[q] + __popcll(m & below);
                        if (ok && pos < Q.nsample[q]) Q.gidx[q][row * Q.nsample[q] + pos] = i;
                        const int more = Q.nsample[q] - cnt[q], found = __popcll(m);
                        cnt[q] += found < more ? found : more;
                    }
                    open = open || cnt[q] < Q.nsample[q];
                }
            }
        }
        // fewer than nsample within the radius: the rest repeats the first
#pragma unroll
        for (int q = 0; q < PS_CLOUD_MAX_SCALES; q++) {
            if (q < Q.n_scales)
                for (int j = cnt[q] + lane; j < Q.nsample[q]; j += 64) Q.gidx[q][row * Q.nsample[q] + j] = first[q];
        }
    }
}

// ------------------------------------------------------ gather and centre
struct GroupArgs {
    const int32_t *gidx[PS_CLOUD_MAX_SCALES];  // [B, S, nsample]
    float *out[PS_CLOUD_MAX_SCALES];           // [B, S, nsample, d + 3], may be NULL
    int nsample[PS_CLOUD_MAX_SCALES];
};

// x clouds, y blocks of a grid stride over one scale's elements, z scales.
// Element (row, channel): a feature channel of point gidx[row], or that
// point's coordinate minus the centre's.  Scale 0 also writes new_xyz.
__global__ __launch_bounds__(kGatherBlock) void k_cloud_group(const float *xyz, const float *feats, int n, int d,
                                                              const int32_t *centre_idx, int s, GroupArgs G,
                                                              float *new_xyz) {
#pragma clang fp contract(off)
    const int64_t env = blockIdx.x;
    const float *p = xyz + env * n * 3;
    const int32_t *gidx = nullptr;
    float *out = nullptr;
    int ns = 0;
#pragma unroll
    for (int q = 0; q < PS_CLOUD_MAX_SCALES; q++)
        if (q == (int)blockIdx.z) {
            gidx = G.gidx[q];
            out = G.out[q];
            ns = G.nsample[q];
        }
    const int64_t step = (int64_t)gridDim.y * kGatherBlock, e0 = (int64_t)blockIdx.y * kGatherBlock + threadIdx.x;
    if (out) {
        const int ch_n = d + 3;
        const int64_t rows = (int64_t)s * ns, total = rows * ch_n;
        for (int64_t e = e0; e < total; e += step) {
            const int64_t r = e / ch_n;
            const int ch = (int)(e - r * ch_n);
            const int i = clamp_index(gidx[env * rows + r], n);
            float v;
            if (ch < d) {
                v = feats[(env * n + i) * d + ch];
            } else {
                const int ci = clamp_index(centre_idx[env * s + r / ns], n);
                v = p[(int64_t)i * 3 + (ch - d)] - p[(int64_t)ci * 3 + (ch - d)];
            }
            out[env * total + e] = v;
        }
    }
    if (blockIdx.z == 0 && new_xyz) {
        for (int64_t e = e0; e < (int64_t)s * 3; e += step) {
            const int ci = clamp_index(centre_idx[env * s + e / 3], n);
            new_xyz[env * s * 3 + e] = p[(int64_t)ci * 3 + (int)(e % 3)];
        }
    }
}

// ------------------------------------------------------------- host side
inline const char *shape_error(int n, int s) {
    if (n < 1 || n > kGroupMaxN) return "N outside 1..8192";
    if (s < 1 || s > n) return "S outside 1..N";
    return nullptr;
}

inline const char *scale_error(double radius, int nsample) {
    if (!(radius > 0.0) || !(radius <= 3.0e38)) return "radius not positive and finite";
    if (nsample < 1) return "nsample < 1";
    return nullptr;
}

// the reference compares f32 distances with f32(r * r), r a double
inline float radius2(double radius) { return (float)(radius * radius); }

template <typename K>
inline int cloud_lds(ps_ctx *c, K kernel, int n) {
    // 12 B per point: above 64 KiB a kernel's dynamic LDS has to be allowed first
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * 3 * kGroupMaxN)) != hipSuccess)
        return fail(c, PS_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    (void)n;
    return PS_OK;
}

int launch_normalize(ps_ctx *c, const float *points, int n, float *xyz, float *centroid, float *scale, hipStream_t st) {
    hipLaunchKernelGGL(k_cloud_normalize, dim3((unsigned)c->num_envs), dim3(kNormBlock), 0, st, points, n, xyz,
                       centroid, scale);
    return check_launch(c);
}

int launch_fps(ps_ctx *c, const float *xyz, int n, const int32_t *start, int s, int32_t *idx, hipStream_t st) {
    int rc = cloud_lds(c, k_cloud_fps, n);
    if (rc != PS_OK) return rc;
    hipLaunchKernelGGL(k_cloud_fps, dim3((unsigned)c->num_envs), dim3(kFpsBlock), sizeof(float) * 3 * n, st, xyz, n,
                       start, s, idx);
    return check_launch(c);
}

int launch_query(ps_ctx *c, const float *xyz, int n, const int32_t *centre_idx, int s, const QueryArgs &Q,
                 hipStream_t st) {
    int rc = cloud_lds(c, k_cloud_query, n);
    if (rc != PS_OK) return rc;
    hipLaunchKernelGGL(k_cloud_query, dim3((unsigned)c->num_envs, (unsigned)((s + kQueryCentres - 1) / kQueryCentres)),
                       dim3(kQueryBlock), sizeof(float) * 3 * n, st, xyz, n, centre_idx, s, Q);
    return check_launch(c);
}

int launch_group(ps_ctx *c, const float *xyz, const float *feats, int n, int d, const int32_t *centre_idx, int s,
                 const GroupArgs &G, int n_scales, float *new_xyz, hipStream_t st) {
    int64_t most = (int64_t)s * 3;
    for (int q = 0; q < n_scales; q++)
        if (G.out[q] && (int64_t)s * G.nsample[q] * (d + 3) > most) most = (int64_t)s * G.nsample[q] * (d + 3);
    int64_t blocks = (most + kGatherBlock - 1) / kGatherBlock;
    if (blocks > kGatherMaxBlocks) blocks = kGatherMaxBlocks;
    hipLaunchKernelGGL(k_cloud_group, dim3((unsigned)c->num_envs, (unsigned)blocks, (unsigned)n_scales),
                       dim3(kGatherBlock), 0, st, xyz, feats, n, d, centre_idx, s, G, new_xyz);
    return check_launch(c);
}

}  // namespace

extern "C" {

int ps_cloud_normalize(ps_ctx *c, const float *points, int n, float *xyz_out, float *centroid, float *scale,
                       void *stream) {
    if (!c || !points || !xyz_out || !centroid || !scale) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = shape_error(n, 1)) return fail(c, PS_ERR_ARG, e);
    return launch_normalize(c, points, n, xyz_out, centroid, scale, (hipStream_t)stream);
}

int ps_cloud_fps(ps_ctx *c, const float *xyz, int n, const int32_t *start, int s, int32_t *idx, void *stream) {
    if (!c || !xyz || !start || !idx) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = shape_error(n, s)) return fail(c, PS_ERR_ARG, e);
    return launch_fps(c, xyz, n, start, s, idx, (hipStream_t)stream);
}

int ps_cloud_ball_query(ps_ctx *c, const float *xyz, int n, const int32_t *centre_idx, int s, double radius,
                        int nsample, int32_t *group_idx, void *stream) {
    if (!c || !xyz || !centre_idx || !group_idx) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = shape_error(n, s)) return fail(c, PS_ERR_ARG, e);
    if (const char *e = scale_error(radius, nsample)) return fail(c, PS_ERR_ARG, e);
    QueryArgs Q;
    memset(&Q, 0, sizeof Q);
    Q.r2[0] = radius2(radius);
    Q.nsample[0] = nsample;
    Q.gidx[0] = group_idx;
    Q.n_scales = 1;
    return launch_query(c, xyz, n, centre_idx, s, Q, (hipStream_t)stream);
}

int ps_cloud_group(ps_ctx *c, const float *xyz, const float *feats, int n, int d, const int32_t *centre_idx, int s,
                   const int32_t *group_idx, int nsample, float *out, float *new_xyz, void *stream) {
    if (!c || !xyz || !centre_idx || !group_idx || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = shape_error(n, s)) return fail(c, PS_ERR_ARG, e);
    if (nsample < 1) return fail(c, PS_ERR_ARG, "nsample < 1");
    if (d < 0 || d > PS_CLOUD_MAX_FEATURES || (feats == nullptr) != (d == 0))
        return fail(c, PS_ERR_ARG, "D outside 0..16, or D and feats disagree");
    GroupArgs G;
    memset(&G, 0, sizeof G);
    G.gidx[0] = group_idx;
    G.out[0] = out;
    G.nsample[0] = nsample;
    return launch_group(c, xyz, feats, n, d, centre_idx, s, G, 1, new_xyz, (hipStream_t)stream);
}

int ps_cloud_set_abstraction(ps_ctx *c, const float *points, const float *feats, int n, int d, const int32_t *start,
                             int s, const ps_cloud_scale *scales, int n_scales, int normalize, float *xyz,
                             float *centroid, float *scale, int32_t *fps_idx, float *new_xyz, void *stream) {
    if (!c || !points || !start || !scales || !fps_idx) return fail(c, PS_ERR_ARG, "null argument");
    if (normalize && (!xyz || !centroid || !scale)) return fail(c, PS_ERR_ARG, "normalize without xyz, centroid, scale");
    if (const char *e = shape_error(n, s)) return fail(c, PS_ERR_ARG, e);
    if (n_scales < 1 || n_scales > PS_CLOUD_MAX_SCALES) return fail(c, PS_ERR_ARG, "n_scales outside 1..4");
    if (d < 0 || d > PS_CLOUD_MAX_FEATURES || (feats == nullptr) != (d == 0))
        return fail(c, PS_ERR_ARG, "D outside 0..16, or D and feats disagree");
    QueryArgs Q;
    GroupArgs G;
    memset(&Q, 0, sizeof Q);
    memset(&G, 0, sizeof G);
    for (int q = 0; q < n_scales; q++) {
        if (const char *e = scale_error(scales[q].radius, scales[q].nsample)) return fail(c, PS_ERR_ARG, e);
        if (!scales[q].group_idx) return fail(c, PS_ERR_ARG, "a scale without group_idx");
        Q.r2[q] = radius2(scales[q].radius);
        Q.nsample[q] = G.nsample[q] = scales[q].nsample;
        Q.gidx[q] = scales[q].group_idx;
        G.gidx[q] = scales[q].group_idx;
        G.out[q] = scales[q].grouped;
    }
    Q.n_scales = n_scales;
    hipStream_t st = (hipStream_t)stream;
    int rc = PS_OK;
    const float *cloud = points;
    if (normalize) {
        rc = launch_normalize(c, points, n, xyz, centroid, scale, st);
        if (rc != PS_OK) return rc;
        cloud = xyz;
    }
    rc = launch_fps(c, cloud, n, start, s, fps_idx, st);
    if (rc != PS_OK) return rc;
    rc = launch_query(c, cloud, n, fps_idx, s, Q, st);
    if (rc != PS_OK) return rc;
    return launch_group(c, cloud, feats, n, d, fps_idx, s, G, n_scales, new_xyz, st);
}

}  // extern "C"
