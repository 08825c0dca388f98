// mlp_kernels.hip — the shared MLP of the PointNet++ models at inference
// (pointnet2_utils.py:196-200, :253-257, :312-314): up to four pointwise
// linear layers (batch norm folded in by the caller) with ReLU and a max-pool
// over groups of G rows, on the f32-input MFMA (v_mfma_f32_32x32x2_f32).
//
// One kernel, k_cloud_mlp<GATHER>: a workgroup of 1, 2 or 4 waves owns a tile
// of 32 rows.  The tile's activations stay in LDS from the first layer to the
// last ([row][channel], two buffers the layers alternate between); the waves
// share the rows and split a layer's output channels in chunks of 32, so an
// MFMA's 32 x 32 result is 32 rows (in its registers) by 32 channels (on its
// lanes).  A wave stages its chunk's weights W[32 outputs][32 k] through a
// slab of LDS of its own: coalesced along k from global memory, the next slab
// in flight while the current one is multiplied.  Rows come from memory
// directly or, with GATHER, through group_idx as ps_cloud_group composes them,
// so the grouped tensor never exists.  A first layer wider than kMlpKChunk is
// streamed through LDS in chunks of k with the accumulators kept.  The last
// layer's result goes from the accumulators to `out` (G = 1) or into the
// maximum of its group; a group longer than a tile is walked tile by tile by
// one workgroup with the running maximum in LDS.
//
// The arithmetic (include/pandasim.h): an accumulator starts as the bias and
// takes k in ascending order, one MFMA per two k; k is padded to a multiple of
// 8 with zero operands on both sides.  k is never split.
//
// LDS order of k: within each aligned 8 channels, channel c sits at position
// 4 * (c & 1) + (c >> 1), so that the lanes of half h = lane >> 5 (which hold
// k = 2 s + h of MFMA s) read their four operands of four MFMAs as one 128-bit
// word at 4 h.
#include "ps_cloud_math.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMlpRows = 32;      // rows of a tile: the MFMA's M
constexpr int kMlpChunk = 32;     // output channels of one accumulator: the MFMA's N
constexpr int kMlpMaxWaves = 4;
constexpr int kMlpKChunk = 512;   // most input channels resident in LDS (= the hidden limit)
constexpr int kMlpSlab = 32;      // k of one weight slab
constexpr int kMlpSlabPitch = 36; // floats per slab row: 16-byte aligned, 4 banks past a multiple of 32
constexpr int kMlpMaxHidden = PS_CLOUD_MLP_MAX_HIDDEN;
constexpr int kMlpMaxLast = PS_CLOUD_MLP_MAX_LAST;
constexpr int kMlpMaxC0 = PS_CLOUD_MAX_PROP_FEATURES + 3;
constexpr int64_t kMlpMaxBlocks = 1 << 20;

struct MlpNet {
    const float *W[PS_CLOUD_MLP_MAX_LAYERS];
    const float *b[PS_CLOUD_MLP_MAX_LAYERS];
    int c_out[PS_CLOUD_MLP_MAX_LAYERS];
    int relu[PS_CLOUD_MLP_MAX_LAYERS];
    int n_layers;
    int c0;
};

// Where the rows come from: `rows` [B, R, c0], or (GATHER) the rows of
// ps_cloud_group: feats[gidx] then xyz[gidx] - xyz[centre_idx], R = s * k.
struct MlpRows {
    const float *rows;
    const float *xyz, *feats;
    const int32_t *centre_idx, *gidx;
    int n, d, s, k;
    int R;
};

PS_D int k_slot(int c) { return (c & ~7) | ((c & 1) << 2) | ((c >> 1) & 3); }

// the lanes of a wave have written LDS that other lanes of it read next
PS_D void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One slab's weights of this lane: rows 2 t + h of the chunk, column j.
struct Slab {
    float w[16];
};

PS_D void slab_load(Slab &s, const float *W, int c_in, int c_out, int o0, int k, int h) {
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const int o = o0 + 2 * t + h;
        s.w[t] = (o < c_out && k < c_in) ? W[(int64_t)o * c_in + k] : 0.0f;
    }
}

// acc += x[rows][k0 .. k0 + kcp) * W[o0 .. o0 + 31][k0 ..]^T, k ascending.
// xin: the tile's LDS rows holding those kcp (a multiple of 8) columns from
// column 0; wst: this wave's slab.
PS_D void mma_chunk(f32x16 &acc, const float *xin, int pitch, int kcp, const float *W, int c_in, int c_out, int o0,
                    int k0, float *wst) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int slot = k_slot(j);
    Slab cur;
    slab_load(cur, W, c_in, c_out, o0, k0 + j, h);
    for (int ks = 0; ks < kcp; ks += kMlpSlab) {
#pragma unroll
        for (int t = 0; t < 16; t++) wst[(2 * t + h) * kMlpSlabPitch + slot] = cur.w[t];
        wave_sync();
        if (ks + kMlpSlab < kcp) slab_load(cur, W, c_in, c_out, o0, k0 + ks + kMlpSlab + j, h);
        const int steps = (kcp - ks < kMlpSlab ? kcp - ks : kMlpSlab) >> 3;
        const float *xa = xin + j * pitch + ks + 4 * h;
        const float *wb = wst + j * kMlpSlabPitch + 4 * h;
        for (int q = 0; q < steps; q++) {
            const float4 a = *(const float4 *)(xa + 8 * q);
            const float4 b = *(const float4 *)(wb + 8 * q);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
        wave_sync();
    }
}

// the tile row that register r of lane half h holds
PS_D int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// x clouds' units, grid stride.  Dynamic LDS: buf0 [32][pitch0], buf1
// [32][pitch1], a slab per wave, the running maximum [pool_n].
template <bool GATHER>
__global__ __launch_bounds__(kMlpMaxWaves * 64) void k_cloud_mlp(MlpNet M, MlpRows S, int G, float *out,
                                                                  int64_t out_stride, int out_offset, int64_t units,
                                                                  int64_t units_per_cloud, int pitch0, int pitch1) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float lds[];
    __shared__ int32_t s_gi[kMlpRows];
    __shared__ float s_centre[kMlpRows * 3];
    const int tid = threadIdx.x, nthreads = blockDim.x, nw = nthreads >> 6;
    const int wave = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    float *buf0 = lds, *buf1 = buf0 + kMlpRows * pitch0;
    float *wst = buf1 + kMlpRows * pitch1 + wave * (kMlpRows * kMlpSlabPitch);
    float *pool = buf1 + kMlpRows * pitch1 + nw * (kMlpRows * kMlpSlabPitch);
    const int R = S.R, groups = R / G;
    const int c0 = M.c0, nkc = (c0 + kMlpKChunk - 1) / kMlpKChunk;
    const int tiles = G > kMlpRows ? (G + kMlpRows - 1) / kMlpRows : 1;

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int64_t env = unit / units_per_cloud;
        const int u = (int)(unit - env * units_per_cloud);
        // the unit's groups g0 .. g0 + ngroups - 1 of its cloud
        int g0, ngroups;
        if (G > kMlpRows) {
            g0 = u;
            ngroups = 1;
        } else {
            const int per = kMlpRows / G;
            g0 = u * per;
            ngroups = groups - g0 < per ? groups - g0 : per;
        }
        for (int tt = 0; tt < tiles; tt++) {
            const int r0 = g0 * G + tt * kMlpRows;  // the tile's first row of its cloud
            const int nrows = G > kMlpRows ? (G - tt * kMlpRows < kMlpRows ? G - tt * kMlpRows : kMlpRows) : ngroups * G;
            if (GATHER && tid < kMlpRows) {
                int gi = 0;
                float cx = 0.0f, cy = 0.0f, cz = 0.0f;
                if (tid < nrows) {
                    const int r = r0 + tid;
                    gi = clamp_index(S.gidx[env * R + r], S.n);
                    const int ci = clamp_index(S.centre_idx[env * S.s + r / S.k], S.n);
                    const float *c = S.xyz + (env * S.n + ci) * 3;
                    cx = c[0], cy = c[1], cz = c[2];
                }
                s_gi[tid] = gi;
                s_centre[tid * 3 + 0] = cx;
                s_centre[tid * 3 + 1] = cy;
                s_centre[tid * 3 + 2] = cz;
            }
            int c_in = c0;
            for (int l = 0; l < M.n_layers; l++) {
                const float *W = nullptr, *bias = nullptr;
                int c_out = 0, relu = 0;
#pragma unroll
                for (int q = 0; q < PS_CLOUD_MLP_MAX_LAYERS; q++)
                    if (q == l) {
                        W = M.W[q];
                        bias = M.b[q];
                        c_out = M.c_out[q];
                        relu = M.relu[q];
                    }
                const bool last = l == M.n_layers - 1;
                // layer l reads buf0 if l is even, buf1 if odd, and writes the other
                const float *xin = (l & 1) ? buf1 : buf0;
                float *xout = (l & 1) ? buf0 : buf1;
                const int pin = (l & 1) ? pitch1 : pitch0, pout = (l & 1) ? pitch0 : pitch1;
                const int nch = (c_out + kMlpChunk - 1) / kMlpChunk, npass = (nch + nw - 1) / nw;
                for (int pass = 0; pass < npass; pass++) {
                    const int oc = pass * nw + wave, o0 = oc * kMlpChunk;
                    const bool active = oc < nch;
                    const int ch = o0 + j;
                    const float b0 = (active && ch < c_out) ? bias[ch] : 0.0f;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[r] = b0;
                    if (l == 0) {
                        for (int kc = 0; kc < nkc; kc++) {
                            const int k0 = kc * kMlpKChunk;
                            const int kw = c0 - k0 < kMlpKChunk ? c0 - k0 : kMlpKChunk, kcp = (kw + 7) & ~7;
                            if (nkc > 1 || pass == 0) {
                                __syncthreads();  // the rows' indices are written, buf0 is read no more
                                for (int e = tid; e < kMlpRows * kcp; e += nthreads) {
                                    const int i = e / kcp, kk = e - i * kcp, k = k0 + kk;
                                    float v = 0.0f;
                                    if (i < nrows && kk < kw) {
                                        if (GATHER) {
                                            const int64_t p = env * S.n + s_gi[i];
                                            v = k < S.d ? S.feats[p * S.d + k]
                                                        : S.xyz[p * 3 + (k - S.d)] - s_centre[i * 3 + (k - S.d)];
                                        } else {
                                            v = S.rows[(env * R + r0 + i) * c0 + k];
                                        }
                                    }
                                    buf0[i * pitch0 + k_slot(kk)] = v;
                                }
                                __syncthreads();
                            }
                            if (active) mma_chunk(acc, buf0, pitch0, kcp, W, c_in, c_out, o0, k0, wst);
                        }
                    } else if (active) {
                        mma_chunk(acc, xin, pin, (c_in + 7) & ~7, W, c_in, c_out, o0, 0, wst);
                    }
                    if (!active) continue;
                    if (relu) {
#pragma unroll
                        for (int r = 0; r < 16; r++) acc[r] = acc[r] > 0.0f ? acc[r] : 0.0f;
                    }
                    if (!last) {
                        // channels past c_out of the chunk are exact zeros (zero weights and bias)
                        float *o = xout + o0 + k_slot(j);
#pragma unroll
                        for (int r = 0; r < 16; r++) o[acc_row(r, h) * pout] = acc[r];
                    } else if (G == 1) {
                        if (ch < c_out) {
                            float *o = out + (env * R + r0) * out_stride + out_offset + ch;
#pragma unroll
                            for (int r = 0; r < 16; r++)
                                if (acc_row(r, h) < nrows) o[(int64_t)acc_row(r, h) * out_stride] = acc[r];
                        }
                    } else {
                        // G > 32: the one group's rows of this tile; else each whole group of the tile
                        const int span = G > kMlpRows ? nrows : G;
                        for (int g = 0; g < ngroups; g++) {
                            const int lo = g * span, hi = lo + span;
                            float m = -INFINITY;
#pragma unroll
                            for (int r = 0; r < 16; r++) {
                                const int row = acc_row(r, h);
                                m = (row >= lo && row < hi) ? fmaxf(m, acc[r]) : m;
                            }
                            m = fmaxf(m, __shfl_xor(m, 32));
                            if (h == 0 && ch < c_out) {
                                if (tt > 0) m = fmaxf(m, pool[ch]);  // written by this lane, a tile ago
                                if (tt == tiles - 1)
                                    out[(env * groups + g0 + g) * out_stride + out_offset + ch] = m;
                                else
                                    pool[ch] = m;
                            }
                        }
                    }
                }
                __syncthreads();  // xout is whole, xin is free
                c_in = c_out;
            }
        }
    }
}

// ------------------------------------------------------------- host side
inline int pitch_of(int width) { return ((width + kMlpChunk - 1) / kMlpChunk) * kMlpChunk + 4; }

inline const char *net_error(const ps_cloud_mlp_layer *layers, int n_layers, int c0, int64_t out_stride,
                             int out_offset) {
    if (n_layers < 1 || n_layers > PS_CLOUD_MLP_MAX_LAYERS) return "n_layers outside 1..4";
    if (c0 < 1 || c0 > kMlpMaxC0) return "C0 outside 1..2051";
    for (int l = 0; l < n_layers; l++) {
        if (!layers[l].W || !layers[l].b) return "a layer without W or b";
        const int most = l == n_layers - 1 ? kMlpMaxLast : kMlpMaxHidden;
        if (layers[l].c_out < 1 || layers[l].c_out > most) return "c_out outside 1..512 (the last: 1..1024)";
    }
    if (out_offset < 0 || out_stride < (int64_t)out_offset + layers[n_layers - 1].c_out)
        return "out_offset < 0 or out_stride < out_offset + the last c_out";
    return nullptr;
}

template <bool GATHER>
int launch_mlp(ps_ctx *c, const ps_cloud_mlp_layer *layers, int n_layers, int c0, MlpRows S, int G, float *out,
               int64_t out_stride, int out_offset, hipStream_t st) {
    MlpNet M;
    memset(&M, 0, sizeof M);
    M.n_layers = n_layers;
    M.c0 = c0;
    int widest = 0, w0 = c0 < kMlpKChunk ? c0 : kMlpKChunk, w1 = 1;
    for (int l = 0; l < n_layers; l++) {
        M.W[l] = layers[l].W;
        M.b[l] = layers[l].b;
        M.c_out[l] = layers[l].c_out;
        M.relu[l] = layers[l].relu != 0;
        if (layers[l].c_out > widest) widest = layers[l].c_out;
        if (l < n_layers - 1) {  // layer 0 writes buf1, layer 1 buf0, layer 2 buf1
            int &w = (l & 1) ? w0 : w1;
            if (layers[l].c_out > w) w = layers[l].c_out;
        }
    }
    int nw = (widest + kMlpChunk - 1) / kMlpChunk;
    nw = nw >= 4 ? 4 : (nw >= 2 ? 2 : 1);
    const int pitch0 = pitch_of(w0), pitch1 = pitch_of(w1);
    const int pool_n = G > kMlpRows ? layers[n_layers - 1].c_out : 0;
    const size_t lds = sizeof(float) * ((size_t)kMlpRows * (pitch0 + pitch1) + (size_t)nw * kMlpRows * kMlpSlabPitch +
                                        pool_n);
    const int groups = S.R / G;
    const int64_t upc = G > kMlpRows ? groups : (groups + kMlpRows / G - 1) / (kMlpRows / G);
    const int64_t units = upc * c->num_envs;
    static_assert(sizeof(float) * (kMlpRows * 2 * (kMlpMaxHidden + 4) + kMlpMaxWaves * kMlpRows * kMlpSlabPitch +
                                   kMlpMaxLast) + 1024 <= 160 * 1024, "the largest network must fit the 160 KiB of LDS");
    if (hipFuncSetAttribute((const void *)k_cloud_mlp<GATHER>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * (kMlpRows * 2 * (kMlpMaxHidden + 4) +
                                                   kMlpMaxWaves * kMlpRows * kMlpSlabPitch + kMlpMaxLast))) != hipSuccess)
        return fail(c, PS_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    const int64_t blocks = units < kMlpMaxBlocks ? units : kMlpMaxBlocks;
    hipLaunchKernelGGL(k_cloud_mlp<GATHER>, dim3((unsigned)blocks), dim3(nw * 64), lds, st, M, S, G, out, out_stride,
                       out_offset, units, upc, pitch0, pitch1);
    return check_launch(c);
}

}  // namespace

extern "C" {

int ps_cloud_mlp(ps_ctx *c, const float *rows, int R, int C0, const ps_cloud_mlp_layer *layers, int n_layers, int G,
                 float *out, int64_t out_stride, int out_offset, void *stream) {
    if (!c || !rows || !layers || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = net_error(layers, n_layers, C0, out_stride, out_offset)) return fail(c, PS_ERR_ARG, e);
    if (R < 1 || G < 1 || R % G != 0) return fail(c, PS_ERR_ARG, "R < 1, G < 1 or R not a multiple of G");
    MlpRows S;
    memset(&S, 0, sizeof S);
    S.rows = rows;
    S.R = R;
    return launch_mlp<false>(c, layers, n_layers, C0, S, G, out, out_stride, out_offset, (hipStream_t)stream);
}

int ps_cloud_group_mlp(ps_ctx *c, const float *xyz, const float *feats, int N, int D, const int32_t *centre_idx, int S,
                       const int32_t *group_idx, int K, const ps_cloud_mlp_layer *layers, int n_layers, float *out,
                       int64_t out_stride, int out_offset, void *stream) {
    if (!c || !xyz || !centre_idx || !group_idx || !layers || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (N < 1 || N > PS_CLOUD_MAX_POINTS) return fail(c, PS_ERR_ARG, "N outside 1..8192");
    if (S < 1 || S > N) return fail(c, PS_ERR_ARG, "S outside 1..N");
    if (K < 1 || (int64_t)S * K > 0x7fffffff) return fail(c, PS_ERR_ARG, "nsample < 1 (or S * nsample >= 2^31)");
    if (D < 0 || D > PS_CLOUD_MAX_PROP_FEATURES || (feats == nullptr) != (D == 0))
        return fail(c, PS_ERR_ARG, "D outside 0..2048, or D and feats disagree");
    if (const char *e = net_error(layers, n_layers, D + 3, out_stride, out_offset)) return fail(c, PS_ERR_ARG, e);
    MlpRows Q;
    memset(&Q, 0, sizeof Q);
    Q.xyz = xyz;
    Q.feats = feats;
    Q.centre_idx = centre_idx;
    Q.gidx = group_idx;
    Q.n = N, Q.d = D, Q.s = S, Q.k = K;
    Q.R = S * K;
    return launch_mlp<true>(c, layers, n_layers, D + 3, Q, K, out, out_stride, out_offset, (hipStream_t)stream);
}

}  // extern "C"
