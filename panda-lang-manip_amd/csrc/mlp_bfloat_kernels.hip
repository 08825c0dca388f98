// mlp_bfloat_kernels.hip — the shared MLP of the PointNet++ models at inference
// in reduced precision (include/pandasim.h, "bfloat16 on the matrix cores"):
// the layers of mlp_kernels.hip with operands rounded to bfloat16 and f32
// accumulation, on v_mfma_f32_32x32x16_bf16.  The tile, its rows' sources, the
// layers' buffers and the host side are ps_mlp_tile.h's, one text for this
// kernel and the f32 one; this file has what bfloat16 changes and the kernel
// body (the layer select and the last layer's epilogue
// measured slower as shared functions, so each file has its own).
//
// One kernel, k_cloud_mlp_bfloat<GATHER>: a workgroup of 1, 2, 4 or 8 waves
// owns a tile of 64 rows, kept in LDS as bf16, so a wave carries two
// accumulators (rows 0..31 and 32..63 of the tile) that share every weight
// fragment.  An MFMA operand fragment is 8 consecutive k of one row: one
// 128-bit LDS read of the activations, one 128-bit global read of the weights
// (W is [c_out, ldw] bf16 with ldw a multiple of 8 and 16-byte aligned, so the
// weights need no staging).
//
// A hidden layer is computed transposed, D = W x^T: a lane then holds four
// consecutive channels of its own tile row in every four accumulator
// registers, which it rounds to bf16 (v_cvt_pk_bf16_f32) and writes to the
// other buffer as one 8-byte word.  The last layer is computed as D = x W^T,
// rows in the registers and the channel on the lane as in the f32 kernel, so
// the pooled maximum is taken in registers and `out` is written along the
// channels.  The bias is the initial accumulator in both.  A first layer
// wider than kMlpKChunk is streamed through LDS in chunks of k with the
// accumulators kept.  No atomics, no scratch.
//
// LDS rows have a pitch of (a multiple of 32) + 8 bf16: 16 bytes times an odd
// number, so the 16 rows that a ds_read_b128 lane group reads at one column
// fall on 16 different 16-byte slots of the 256-byte bank row.
#include "ps_mlp_tile.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kBfRows = 64;       // rows of a tile: two MFMA row blocks
constexpr int kBfMaxWaves = 8;
constexpr int kBfKStep = 16;      // k of one MFMA
constexpr int kBfPad = 8;         // bf16 past a row's channels

// two f32 -> two bf16 (round to nearest even) in one dword, a in the low half
PS_D uint32_t pack_bf16(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// acc[m] += x[32 m + .][0 .. kcp) * W[o0 .. o0 + 31][k0 .. k0 + kcp)^T, m = 0, 1.
// xin: the tile's LDS rows holding those kcp (a multiple of 16) columns from
// column 0.  TRANSPOSED: the result's rows are the channels, its columns the
// tile rows (a hidden layer); else rows by channels (the last layer).
template <bool TRANSPOSED>
PS_D void mma_chunk(f32x16 (&acc)[2], const uint16_t *xin, int pitch, int kcp, const uint16_t *W, int ldw, int c_out,
                    int o0, int k0) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const bool orow = o0 + j < c_out;
    const uint16_t *wp = W + (int64_t)(orow ? o0 + j : 0) * ldw + k0 + 8 * h;
    const int wk = ldw - k0 - 8 * h;  // this lane's k below it hold weights
    const uint16_t *x0 = xin + j * pitch + 8 * h, *x1 = x0 + 32 * pitch;
    const bf16x8 zero = {};
    bf16x8 w = (orow && 0 < wk) ? *(const bf16x8 *)wp : zero;
    for (int ks = 0; ks < kcp; ks += kBfKStep) {
        const bf16x8 a0 = *(const bf16x8 *)(x0 + ks), a1 = *(const bf16x8 *)(x1 + ks);
        const bf16x8 wc = w;
        const int kn = ks + kBfKStep;
        if (kn < kcp) w = (orow && kn < wk) ? *(const bf16x8 *)(wp + kn) : zero;
        if (TRANSPOSED) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc, a0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc, a1, acc[1], 0, 0, 0);
        } else {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, wc, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, wc, acc[1], 0, 0, 0);
        }
    }
}

// x clouds' units, grid stride.  Dynamic LDS: buf0 [64][pitch0] bf16, buf1
// [64][pitch1] bf16, the running maximum [pool_n] f32.
template <bool GATHER>
__global__ __launch_bounds__(kBfMaxWaves * 64) void k_cloud_mlp_bfloat(MlpNet<uint16_t> M, MlpRows S, int G, float *out,
                                                                        int64_t out_stride, int out_offset,
                                                                        int64_t units, int64_t units_per_cloud,
                                                                        int pitch0, int pitch1) {
    extern __shared__ __align__(16) unsigned char lds_bf[];
    __shared__ int32_t s_gi[kBfRows];
    __shared__ float s_centre[kBfRows * 3];
    const int tid = threadIdx.x, nthreads = blockDim.x, nw = nthreads >> 6;
    const int wave = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    uint16_t *buf0 = (uint16_t *)lds_bf, *buf1 = buf0 + kBfRows * pitch0;
    float *pool = (float *)(buf1 + kBfRows * pitch1);
    const int R = S.R, groups = R / G;
    const int c0 = M.c0, nkc = (c0 + kMlpKChunk - 1) / kMlpKChunk;
    const int tiles = mlp_tiles<kBfRows>(G);

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const MlpTile U = mlp_unit<kBfRows>(unit, units_per_cloud, G, groups);
        for (int tt = 0; tt < tiles; tt++) {
            const MlpTile T = mlp_tile<kBfRows>(U, tt, G);
            if (GATHER) mlp_gather_prologue<kBfRows>(S, T, s_gi, s_centre);
            int c_in = c0;
            for (int l = 0; l < M.n_layers; l++) {
                // layer l out of the kernel's arguments (no indexed read of them)
                struct { const uint16_t *W; const float *bias; int c_out, relu; } L = {nullptr, nullptr, 0, 0};
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
                const int ldw = (c_in + 7) & ~7;
                // layer l reads buf0 if l is even, buf1 if odd, and writes the other
                const uint16_t *xin = (l & 1) ? buf1 : buf0;
                uint16_t *xout = (l & 1) ? buf0 : buf1;
                const int pin = (l & 1) ? pitch1 : pitch0, pout = (l & 1) ? pitch0 : pitch1;
                const int nch = (c_out + kMlpChunk - 1) / kMlpChunk, npass = (nch + nw - 1) / nw;
                for (int pass = 0; pass < npass; pass++) {
                    const int oc = pass * nw + wave, o0 = oc * kMlpChunk;
                    const bool active = oc < nch;
                    const int ch = o0 + j;
                    f32x16 acc[2];
                    if (last) {
                        const float b0 = (active && ch < c_out) ? L.bias[ch] : 0.0f;
#pragma unroll
                        for (int r = 0; r < 16; r++) acc[0][r] = acc[1][r] = b0;
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int o = o0 + acc_row(r, h);
                            acc[0][r] = acc[1][r] = (active && o < c_out) ? L.bias[o] : 0.0f;
                        }
                    }
                    if (l == 0) {
                        for (int kc = 0; kc < nkc; kc++) {
                            const int k0 = kc * kMlpKChunk;
                            const int kw = c0 - k0 < kMlpKChunk ? c0 - k0 : kMlpKChunk;
                            const int kcp = (kw + kBfKStep - 1) & ~(kBfKStep - 1);
                            if (nkc > 1 || pass == 0) {
                                __syncthreads();  // the rows' indices are written, buf0 is read no more
                                // 2^lg lanes walk a row's pairs of columns, the others the next rows
                                const int kcp2 = kcp >> 1;
                                int lg = 32 - __clz(kcp2 - 1);
                                lg = lg > 6 ? 6 : lg;
                                const int lpr = 1 << lg;
                                for (int i = tid >> lg; i < kBfRows; i += nthreads >> lg) {
                                    const bool row_in = i < T.nrows;
                                    const float *src = nullptr, *pxyz = nullptr;
                                    if (row_in) {
                                        if (GATHER) {
                                            const int64_t p = T.env * S.n + s_gi[i];
                                            src = S.feats + p * S.d;
                                            pxyz = S.xyz + p * 3;
                                        } else {
                                            src = S.rows + (T.env * R + T.r0 + i) * c0;
                                        }
                                    }
                                    for (int c = tid & (lpr - 1); c < kcp2; c += lpr) {
                                        float v[2];
#pragma unroll
                                        for (int e = 0; e < 2; e++) {
                                            const int kk = 2 * c + e, k = k0 + kk;
                                            v[e] = 0.0f;
                                            if (row_in && kk < kw) {
                                                if (GATHER)
                                                    v[e] = k < S.d ? src[k] : pxyz[k - S.d] - s_centre[i * 3 + (k - S.d)];
                                                else
                                                    v[e] = src[k];
                                            }
                                        }
                                        *(uint32_t *)(buf0 + i * pitch0 + 2 * c) = pack_bf16(v[0], v[1]);
                                    }
                                }
                                __syncthreads();
                            }
                            if (active) {
                                if (last)
                                    mma_chunk<false>(acc, buf0, pitch0, kcp, L.W, ldw, c_out, o0, k0);
                                else
                                    mma_chunk<true>(acc, buf0, pitch0, kcp, L.W, ldw, c_out, o0, k0);
                            }
                        }
                    } else if (active) {
                        const int kcp = (c_in + kBfKStep - 1) & ~(kBfKStep - 1);
                        if (last)
                            mma_chunk<false>(acc, xin, pin, kcp, L.W, ldw, c_out, o0, 0);
                        else
                            mma_chunk<true>(acc, xin, pin, kcp, L.W, ldw, c_out, o0, 0);
                    }
                    if (!active) continue;
                    mlp_relu(acc, L.relu);
                    if (!last) {
                        // lane j holds tile rows j and 32 + j; registers 4 g .. 4 g + 3 are the channels
                        // o0 + 8 g + 4 h + 0 .. 3.  Channels past c_out of the chunk are exact zeros
                        // (zero weights and bias).
#pragma unroll
                        for (int m = 0; m < 2; m++) {
                            uint16_t *o = xout + (32 * m + j) * pout + o0 + 4 * h;
#pragma unroll
                            for (int g = 0; g < 4; g++) {
                                uint2 q;
                                q.x = pack_bf16(acc[m][4 * g + 0], acc[m][4 * g + 1]);
                                q.y = pack_bf16(acc[m][4 * g + 2], acc[m][4 * g + 3]);
                                *(uint2 *)(o + 8 * g) = q;
                            }
                        }
                    } else if (G == 1) {
                        if (ch < c_out) {
                            float *o = out + (T.env * R + T.r0) * out_stride + out_offset + ch;
#pragma unroll
                            for (int m = 0; m < 2; m++)
#pragma unroll
                                for (int r = 0; r < 16; r++) {
                                    const int row = 32 * m + acc_row(r, h);
                                    if (row < T.nrows) o[(int64_t)row * out_stride] = acc[m][r];
                                }
                        }
                    } else {
                        // G > 64: the one group's rows of this tile; else each whole group of the tile
                        const int span = G > kBfRows ? T.nrows : G;
                        for (int g = 0; g < T.ngroups; g++) {
                            const int lo = g * span, hi = lo + span;
                            float mx = -INFINITY;
#pragma unroll
                            for (int m = 0; m < 2; m++)
#pragma unroll
                                for (int r = 0; r < 16; r++) {
                                    const int row = 32 * m + acc_row(r, h);
                                    mx = (row >= lo && row < hi) ? fmaxf(mx, acc[m][r]) : mx;
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
inline int pitch_of(int width) { return ((width + kMlpChunk - 1) / kMlpChunk) * kMlpChunk + kBfPad; }

constexpr size_t kBfMaxLds =
    sizeof(uint16_t) * kBfRows * 2 * (kMlpMaxHidden + kBfPad) + sizeof(float) * kMlpMaxLast;
static_assert(kBfMaxLds + 2048 <= 160 * 1024, "the largest network must fit the 160 KiB of LDS");

template <bool GATHER>
int launch_mlp(ps_ctx *c, const ps_cloud_mlp_bfloat_layer *layers, int n_layers, int c0, const MlpRows &S, int G,
               float *out, int64_t out_stride, int out_offset, void *stream) {
    MlpNet<uint16_t> M;
    const MlpPlan P = mlp_plan<kBfRows, kBfMaxWaves>(c, layers, n_layers, c0, S.R, G, pitch_of, M);
    const size_t lds = sizeof(uint16_t) * (size_t)kBfRows * (P.pitch0 + P.pitch1) + sizeof(float) * P.pool_n;
    return mlp_launch<uint16_t>(c, k_cloud_mlp_bfloat<GATHER>, P, lds, kBfMaxLds, M, S, G, out, out_stride, out_offset,
                                (hipStream_t)stream);
}

}  // namespace

extern "C" {

int ps_cloud_mlp_bfloat(ps_ctx *c, const float *rows, int R, int C0, const ps_cloud_mlp_bfloat_layer *layers,
                        int n_layers, int G, float *out, int64_t out_stride, int out_offset, void *stream) {
    MlpRows S;
    if (int e = mlp_args(c, rows, R, C0, layers, n_layers, G, out, out_stride, out_offset, S)) return e;
    return launch_mlp<false>(c, layers, n_layers, C0, S, G, out, out_stride, out_offset, stream);
}

int ps_cloud_group_mlp_bfloat(ps_ctx *c, const float *xyz, const float *feats, int N, int D, const int32_t *centre_idx,
                              int S, const int32_t *group_idx, int K, const ps_cloud_mlp_bfloat_layer *layers,
                              int n_layers, float *out, int64_t out_stride, int out_offset, void *stream) {
    MlpRows Q;
    if (int e = group_mlp_args(c, xyz, feats, N, D, centre_idx, S, group_idx, K, layers, n_layers, out, out_stride,
                               out_offset, Q))
        return e;
    return launch_mlp<true>(c, layers, n_layers, D + 3, Q, K, out, out_stride, out_offset, stream);
}

}  // extern "C"
