// mlp_kernels.hip — the shared MLP of the PointNet++ models at inference
// (pointnet2_utils.py:196-200, :253-257, :312-314): up to four pointwise
// linear layers (batch norm folded in by the caller) with ReLU and a max-pool
// over groups of G rows, on the f32-input MFMA (v_mfma_f32_32x32x2_f32).
//
// One kernel, k_cloud_mlp<GATHER>: a workgroup of 1, 2 or 4 waves owns a tile
// of 32 rows.  The tile, its rows' sources, the layers' buffers and the host
// side are ps_mlp_tile.h's, shared with the bfloat16 kernel; this file has the
// f32 multiplication and the kernel body (the layer select and
// the last layer's epilogue measured slower as shared functions).  An MFMA's
// 32 x 32 result is 32 rows (in its registers) by 32 channels (on its lanes).
// A wave stages its chunk's weights W[32 outputs][32 k] through a slab of LDS
// of its own: coalesced along k from global memory, the next slab in flight
// while the current one is multiplied.  A first layer wider than kMlpKChunk is
// streamed through LDS in chunks of k with the accumulators kept.
//
// The arithmetic (include/pandasim.h): an accumulator starts as the bias and
// takes k in ascending order, one MFMA per two k; k is padded to a multiple of
// 8 with zero operands on both sides.  k is never split.
//
// LDS order of k: within each aligned 8 channels, channel c sits at position
// 4 * (c & 1) + (c >> 1), so that the lanes of half h = lane >> 5 (which hold
// k = 2 s + h of MFMA s) read their four operands of four MFMAs as one 128-bit
// word at 4 h.
#include "ps_mlp_tile.h"

namespace {

constexpr int kMlpRows = 32;      // rows of a tile: the MFMA's M
constexpr int kMlpMaxWaves = 4;
constexpr int kMlpSlab = 32;      // k of one weight slab
constexpr int kMlpSlabPitch = 36; // floats per slab row: 16-byte aligned, 4 banks past a multiple of 32

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

// x clouds' units, grid stride.  Dynamic LDS: buf0 [32][pitch0], buf1
// [32][pitch1], a slab per wave, the running maximum [pool_n].
template <bool GATHER>
__global__ __launch_bounds__(kMlpMaxWaves * 64) void k_cloud_mlp(MlpNet<float> M, MlpRows S, int G, float *out,
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
    const int tiles = mlp_tiles<kMlpRows>(G);

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const MlpTile U = mlp_unit<kMlpRows>(unit, units_per_cloud, G, groups);
        for (int tt = 0; tt < tiles; tt++) {
            const MlpTile T = mlp_tile<kMlpRows>(U, tt, G);
            if (GATHER) mlp_gather_prologue<kMlpRows>(S, T, s_gi, s_centre);
            int c_in = c0;
            for (int l = 0; l < M.n_layers; l++) {
                // layer l out of the kernel's arguments (no indexed read of them)
                struct { const float *W; const float *bias; int c_out, relu; } L = {nullptr, nullptr, 0, 0};
#pragma unroll
                for (int q = 0; q < PS_CLOUD_MLP_MAX_LAYERS; q++)
                    if (q == l) {
                        L.W = M.W[q];
                        L.bias = M.b[q];
                        L.c_out = M.c_out[q];
                        L.relu = M.relu[q];
                    }
                const int c_out = L.c_out;
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
                    const float b0 = (active && ch < c_out) ? L.bias[ch] : 0.0f;
                    f32x16 acc[1];
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[0][r] = b0;
                    if (l == 0) {
                        for (int kc = 0; kc < nkc; kc++) {
                            const int k0 = kc * kMlpKChunk;
                            const int kw = c0 - k0 < kMlpKChunk ? c0 - k0 : kMlpKChunk, kcp = (kw + 7) & ~7;
                            if (nkc > 1 || pass == 0) {
                                __syncthreads();  // the rows' indices are written, buf0 is read no more
                                for (int e = tid; e < kMlpRows * kcp; e += nthreads) {
                                    const int i = e / kcp, kk = e - i * kcp, k = k0 + kk;
                                    float v = 0.0f;
                                    if (i < T.nrows && kk < kw) {
                                        if (GATHER) {
                                            const int64_t p = T.env * S.n + s_gi[i];
                                            v = k < S.d ? S.feats[p * S.d + k]
                                                        : S.xyz[p * 3 + (k - S.d)] - s_centre[i * 3 + (k - S.d)];
                                        } else {
                                            v = S.rows[(T.env * R + T.r0 + i) * c0 + k];
                                        }
                                    }
                                    buf0[i * pitch0 + k_slot(kk)] = v;
                                }
                                __syncthreads();
                            }
                            if (active) mma_chunk(acc[0], buf0, pitch0, kcp, L.W, c_in, c_out, o0, k0, wst);
                        }
                    } else if (active) {
                        mma_chunk(acc[0], xin, pin, (c_in + 7) & ~7, L.W, c_in, c_out, o0, 0, wst);
                    }
                    if (!active) continue;
                    mlp_relu(acc, L.relu);
                    if (!last) {
                        // channels past c_out of the chunk are exact zeros (zero weights and bias)
                        float *o = xout + o0 + k_slot(j);
#pragma unroll
                        for (int r = 0; r < 16; r++) o[acc_row(r, h) * pout] = acc[0][r];
                    } else if (G == 1) {
                        if (ch < c_out) {
                            float *o = out + (T.env * R + T.r0) * out_stride + out_offset + ch;
#pragma unroll
                            for (int r = 0; r < 16; r++) {
                                const int row = acc_row(r, h);
                                if (row < T.nrows) o[(int64_t)row * out_stride] = acc[0][r];
                            }
                        }
                    } else {
                        // G > 32: the one group's rows of this tile; else each whole group of the tile
                        const int span = G > kMlpRows ? T.nrows : G;
                        for (int g = 0; g < T.ngroups; g++) {
                            const int lo = g * span, hi = lo + span;
                            float mx = -INFINITY;
#pragma unroll
                            for (int r = 0; r < 16; r++) {
                                const int row = acc_row(r, h);
                                mx = (row >= lo && row < hi) ? fmaxf(mx, acc[0][r]) : mx;
                            }
                            mx = fmaxf(mx, __shfl_xor(mx, 32));
                            if (h == 0 && ch < c_out) {
                                if (tt > 0) mx = fmaxf(mx, pool[ch]);  // written by this lane, a tile ago
                                if (tt == tiles - 1)
                                    out[(T.env * groups + T.g0 + g) * out_stride + out_offset + ch] = mx;
                                else
                                    pool[ch] = mx;
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

constexpr size_t kMlpMaxLds =
    sizeof(float) * (kMlpRows * 2 * (kMlpMaxHidden + 4) + kMlpMaxWaves * kMlpRows * kMlpSlabPitch + kMlpMaxLast);
static_assert(kMlpMaxLds + 1024 <= 160 * 1024, "the largest network must fit the 160 KiB of LDS");

template <bool GATHER>
int launch_mlp(ps_ctx *c, const ps_cloud_mlp_layer *layers, int n_layers, int c0, const MlpRows &S, int G, float *out,
               int64_t out_stride, int out_offset, void *stream) {
    MlpNet<float> M;
    const MlpPlan P = mlp_plan<kMlpRows, kMlpMaxWaves>(c, layers, n_layers, c0, S.R, G, pitch_of, M);
    const size_t lds = sizeof(float) * ((size_t)kMlpRows * (P.pitch0 + P.pitch1) +
                                        (size_t)P.nw * kMlpRows * kMlpSlabPitch + P.pool_n);
    return mlp_launch<float>(c, k_cloud_mlp<GATHER>, P, lds, kMlpMaxLds, M, S, G, out, out_stride, out_offset,
                             (hipStream_t)stream);
}

}  // namespace

extern "C" {

int ps_cloud_mlp(ps_ctx *c, const float *rows, int R, int C0, const ps_cloud_mlp_layer *layers, int n_layers, int G,
                 float *out, int64_t out_stride, int out_offset, void *stream) {
    MlpRows S;
    if (int e = mlp_args(c, rows, R, C0, layers, n_layers, G, out, out_stride, out_offset, S)) return e;
    return launch_mlp<false>(c, layers, n_layers, C0, S, G, out, out_stride, out_offset, stream);
}

int ps_cloud_group_mlp(ps_ctx *c, const float *xyz, const float *feats, int N, int D, const int32_t *centre_idx, int S,
                       const int32_t *group_idx, int K, const ps_cloud_mlp_layer *layers, int n_layers, float *out,
                       int64_t out_stride, int out_offset, void *stream) {
    MlpRows Q;
    if (int e = group_mlp_args(c, xyz, feats, N, D, centre_idx, S, group_idx, K, layers, n_layers, out, out_stride,
                               out_offset, Q))
        return e;
    return launch_mlp<true>(c, layers, n_layers, D + 3, Q, K, out, out_stride, out_offset, stream);
}

}  // extern "C"
