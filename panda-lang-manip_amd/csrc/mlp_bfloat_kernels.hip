// mlp_bfloat_kernels.hip — the shared MLP of the PointNet++ models at inference
// in reduced precision (include/pandasim.h, "bfloat16 on the matrix cores"):
// the layers of mlp_kernels.hip with operands rounded to bfloat16 and f32
// accumulation, on v_mfma_f32_32x32x16_bf16.  A capability beside the f32
// kernel, which is untouched.
//
// One kernel, k_cloud_mlp_bfloat<GATHER>: a workgroup of 1, 2, 4 or 8 waves
// owns a tile of 64 rows.  The tile's activations stay in LDS from the first
// layer to the last as bf16 ([row][channel], two buffers the layers alternate
// between); the waves share the rows and split a layer's output channels in
// chunks of 32, so a wave carries two accumulators (rows 0..31 and 32..63 of
// the tile) that share every weight fragment.  An MFMA operand fragment is 8
// consecutive k of one row: one 128-bit LDS read of the activations, one
// 128-bit global read of the weights (W is [c_out, ldw] bf16 with ldw a
// multiple of 8 and 16-byte aligned, so the weights need no staging).
//
// A hidden layer is computed transposed, D = W x^T: a lane then holds four
// consecutive channels of its own tile row in every four accumulator
// registers, which it rounds to bf16 (v_cvt_pk_bf16_f32) and writes to the
// other buffer as one 8-byte word.  The last layer is computed as D = x W^T,
// rows in the registers and the channel on the lane as in the f32 kernel, so
// the pooled maximum is taken in registers and `out` is written along the
// channels.  The bias is the initial accumulator in both.  A first layer
// wider than kBfKChunk is streamed through LDS in chunks of k with the
// accumulators kept.  A group longer than a tile is walked tile by tile by one
// workgroup with the running maximum in LDS.  No atomics, no scratch.
//
// LDS rows have a pitch of (a multiple of 32) + 8 bf16: 16 bytes times an odd
// number, so the 16 rows that a ds_read_b128 lane group reads at one column
// fall on 16 different 16-byte slots of the 256-byte bank row.
#include "ps_cloud_math.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kBfRows = 64;       // rows of a tile: two MFMA row blocks
constexpr int kBfChunk = 32;      // output channels of one wave's pass: the MFMA's N
constexpr int kBfMaxWaves = 8;
constexpr int kBfKChunk = 512;    // most input channels resident in LDS (= the hidden limit)
constexpr int kBfKStep = 16;      // k of one MFMA
constexpr int kBfPad = 8;         // bf16 past a row's channels
constexpr int kBfMaxHidden = PS_CLOUD_MLP_MAX_HIDDEN;
constexpr int kBfMaxLast = PS_CLOUD_MLP_MAX_LAST;
constexpr int kBfMaxC0 = PS_CLOUD_MAX_PROP_FEATURES + 3;
constexpr int64_t kBfMaxBlocks = 1 << 20;

struct BfNet {
    const uint16_t *W[PS_CLOUD_MLP_MAX_LAYERS];
    const float *b[PS_CLOUD_MLP_MAX_LAYERS];
    int c_out[PS_CLOUD_MLP_MAX_LAYERS];
    int relu[PS_CLOUD_MLP_MAX_LAYERS];
    int n_layers;
    int c0;
};

// Where the rows come from: `rows` [B, R, c0], or (GATHER) the rows of
// ps_cloud_group: feats[gidx] then xyz[gidx] - xyz[centre_idx], R = s * k.
struct BfRows {
    const float *rows;
    const float *xyz, *feats;
    const int32_t *centre_idx, *gidx;
    int n, d, s, k;
    int R;
};

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

// the row of the MFMA's result that register r of lane half h holds
PS_D int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// x clouds' units, grid stride.  Dynamic LDS: buf0 [64][pitch0] bf16, buf1
// [64][pitch1] bf16, the running maximum [pool_n] f32.
template <bool GATHER>
__global__ __launch_bounds__(kBfMaxWaves * 64) void k_cloud_mlp_bfloat(BfNet M, BfRows S, int G, float *out,
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
    const int c0 = M.c0, nkc = (c0 + kBfKChunk - 1) / kBfKChunk;
    const int tiles = G > kBfRows ? (G + kBfRows - 1) / kBfRows : 1;

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int64_t env = unit / units_per_cloud;
        const int u = (int)(unit - env * units_per_cloud);
        // the unit's groups g0 .. g0 + ngroups - 1 of its cloud
        int g0, ngroups;
        if (G > kBfRows) {
            g0 = u;
            ngroups = 1;
        } else {
            const int per = kBfRows / G;
            g0 = u * per;
            ngroups = groups - g0 < per ? groups - g0 : per;
        }
        for (int tt = 0; tt < tiles; tt++) {
            const int r0 = g0 * G + tt * kBfRows;  // the tile's first row of its cloud
            const int nrows = G > kBfRows ? (G - tt * kBfRows < kBfRows ? G - tt * kBfRows : kBfRows) : ngroups * G;
            if (GATHER && tid < kBfRows) {
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
                const uint16_t *W = nullptr;
                const float *bias = nullptr;
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
                const int ldw = (c_in + 7) & ~7;
                // layer l reads buf0 if l is even, buf1 if odd, and writes the other
                const uint16_t *xin = (l & 1) ? buf1 : buf0;
                uint16_t *xout = (l & 1) ? buf0 : buf1;
                const int pin = (l & 1) ? pitch1 : pitch0, pout = (l & 1) ? pitch0 : pitch1;
                const int nch = (c_out + kBfChunk - 1) / kBfChunk, npass = (nch + nw - 1) / nw;
                for (int pass = 0; pass < npass; pass++) {
                    const int oc = pass * nw + wave, o0 = oc * kBfChunk;
                    const bool active = oc < nch;
                    const int ch = o0 + j;
                    f32x16 acc[2];
                    if (last) {
                        const float b0 = (active && ch < c_out) ? bias[ch] : 0.0f;
#pragma unroll
                        for (int r = 0; r < 16; r++) acc[0][r] = acc[1][r] = b0;
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int o = o0 + acc_row(r, h);
                            acc[0][r] = acc[1][r] = (active && o < c_out) ? bias[o] : 0.0f;
                        }
                    }
                    if (l == 0) {
                        for (int kc = 0; kc < nkc; kc++) {
                            const int k0 = kc * kBfKChunk;
                            const int kw = c0 - k0 < kBfKChunk ? c0 - k0 : kBfKChunk;
                            const int kcp = (kw + kBfKStep - 1) & ~(kBfKStep - 1);
                            if (nkc > 1 || pass == 0) {
                                __syncthreads();  // the rows' indices are written, buf0 is read no more
                                // 2^lg lanes walk a row's pairs of columns, the others the next rows
                                const int kcp2 = kcp >> 1;
                                int lg = 32 - __clz(kcp2 - 1);
                                lg = lg > 6 ? 6 : lg;
                                const int lpr = 1 << lg;
                                for (int i = tid >> lg; i < kBfRows; i += nthreads >> lg) {
                                    const bool row_in = i < nrows;
                                    const float *src = nullptr, *pxyz = nullptr;
                                    if (row_in) {
                                        if (GATHER) {
                                            const int64_t p = env * S.n + s_gi[i];
                                            src = S.feats + p * S.d;
                                            pxyz = S.xyz + p * 3;
                                        } else {
                                            src = S.rows + (env * R + r0 + i) * c0;
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
                                    mma_chunk<false>(acc, buf0, pitch0, kcp, W, ldw, c_out, o0, k0);
                                else
                                    mma_chunk<true>(acc, buf0, pitch0, kcp, W, ldw, c_out, o0, k0);
                            }
                        }
                    } else if (active) {
                        const int kcp = (c_in + kBfKStep - 1) & ~(kBfKStep - 1);
                        if (last)
                            mma_chunk<false>(acc, xin, pin, kcp, W, ldw, c_out, o0, 0);
                        else
                            mma_chunk<true>(acc, xin, pin, kcp, W, ldw, c_out, o0, 0);
                    }
                    if (!active) continue;
                    if (relu) {
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            acc[0][r] = acc[0][r] > 0.0f ? acc[0][r] : 0.0f;
                            acc[1][r] = acc[1][r] > 0.0f ? acc[1][r] : 0.0f;
                        }
                    }
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
                            float *o = out + (env * R + r0) * out_stride + out_offset + ch;
#pragma unroll
                            for (int m = 0; m < 2; m++)
#pragma unroll
                                for (int r = 0; r < 16; r++) {
                                    const int row = 32 * m + acc_row(r, h);
                                    if (row < nrows) o[(int64_t)row * out_stride] = acc[m][r];
                                }
                        }
                    } else {
                        // G > 64: the one group's rows of this tile; else each whole group of the tile
                        const int span = G > kBfRows ? nrows : G;
                        for (int g = 0; g < ngroups; g++) {
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
                                    out[(env * groups + g0 + g) * out_stride + out_offset + ch] = mx;
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
inline int pitch_of(int width) { return ((width + kBfChunk - 1) / kBfChunk) * kBfChunk + kBfPad; }

constexpr size_t kBfMaxLds =
    sizeof(uint16_t) * kBfRows * 2 * (kBfMaxHidden + kBfPad) + sizeof(float) * kBfMaxLast;

inline const char *net_error(const ps_cloud_mlp_bfloat_layer *layers, int n_layers, int c0, int64_t out_stride,
                             int out_offset) {
    if (n_layers < 1 || n_layers > PS_CLOUD_MLP_MAX_LAYERS) return "n_layers outside 1..4";
    if (c0 < 1 || c0 > kBfMaxC0) return "C0 outside 1..2051";
    for (int l = 0; l < n_layers; l++) {
        if (!layers[l].W || !layers[l].b) return "a layer without W or b";
        if (((uintptr_t)layers[l].W & 15) != 0) return "a layer's W is not 16-byte aligned";
        const int most = l == n_layers - 1 ? kBfMaxLast : kBfMaxHidden;
        if (layers[l].c_out < 1 || layers[l].c_out > most) return "c_out outside 1..512 (the last: 1..1024)";
    }
    if (out_offset < 0 || out_stride < (int64_t)out_offset + layers[n_layers - 1].c_out)
        return "out_offset < 0 or out_stride < out_offset + the last c_out";
    return nullptr;
}

template <bool GATHER>
int launch_mlp(ps_ctx *c, const ps_cloud_mlp_bfloat_layer *layers, int n_layers, int c0, BfRows S, int G, float *out,
               int64_t out_stride, int out_offset, hipStream_t st) {
    BfNet M;
    memset(&M, 0, sizeof M);
    M.n_layers = n_layers;
    M.c0 = c0;
    int widest = 0, w0 = c0 < kBfKChunk ? c0 : kBfKChunk, w1 = 1;
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
    int nw = (widest + kBfChunk - 1) / kBfChunk;
    nw = nw >= 8 ? 8 : (nw >= 4 ? 4 : (nw >= 2 ? 2 : 1));
    const int pitch0 = pitch_of(w0), pitch1 = pitch_of(w1);
    const int pool_n = G > kBfRows ? layers[n_layers - 1].c_out : 0;
    const size_t lds = sizeof(uint16_t) * (size_t)kBfRows * (pitch0 + pitch1) + sizeof(float) * pool_n;
    const int groups = S.R / G;
    const int64_t upc = G > kBfRows ? groups : (groups + kBfRows / G - 1) / (kBfRows / G);
    const int64_t units = upc * c->num_envs;
    static_assert(kBfMaxLds + 2048 <= 160 * 1024, "the largest network must fit the 160 KiB of LDS");
    if (hipFuncSetAttribute((const void *)k_cloud_mlp_bfloat<GATHER>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kBfMaxLds) != hipSuccess)
        return fail(c, PS_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    const int64_t blocks = units < kBfMaxBlocks ? units : kBfMaxBlocks;
    hipLaunchKernelGGL(k_cloud_mlp_bfloat<GATHER>, dim3((unsigned)blocks), dim3(nw * 64), lds, st, M, S, G, out,
                       out_stride, out_offset, units, upc, pitch0, pitch1);
    return check_launch(c);
}

}  // namespace

extern "C" {

int ps_cloud_mlp_bfloat(ps_ctx *c, const float *rows, int R, int C0, const ps_cloud_mlp_bfloat_layer *layers,
                        int n_layers, int G, float *out, int64_t out_stride, int out_offset, void *stream) {
    if (!c || !rows || !layers || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = net_error(layers, n_layers, C0, out_stride, out_offset)) return fail(c, PS_ERR_ARG, e);
    if (R < 1 || G < 1 || R % G != 0) return fail(c, PS_ERR_ARG, "R < 1, G < 1 or R not a multiple of G");
    BfRows S;
    memset(&S, 0, sizeof S);
    S.rows = rows;
    S.R = R;
    return launch_mlp<false>(c, layers, n_layers, C0, S, G, out, out_stride, out_offset, (hipStream_t)stream);
}

int ps_cloud_group_mlp_bfloat(ps_ctx *c, const float *xyz, const float *feats, int N, int D, const int32_t *centre_idx,
                              int S, const int32_t *group_idx, int K, const ps_cloud_mlp_bfloat_layer *layers,
                              int n_layers, float *out, int64_t out_stride, int out_offset, void *stream) {
    if (!c || !xyz || !centre_idx || !group_idx || !layers || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (N < 1 || N > PS_CLOUD_MAX_POINTS) return fail(c, PS_ERR_ARG, "N outside 1..8192");
    if (S < 1 || S > N) return fail(c, PS_ERR_ARG, "S outside 1..N");
    if (K < 1 || (int64_t)S * K > 0x7fffffff) return fail(c, PS_ERR_ARG, "nsample < 1 (or S * nsample >= 2^31)");
    if (D < 0 || D > PS_CLOUD_MAX_PROP_FEATURES || (feats == nullptr) != (D == 0))
        return fail(c, PS_ERR_ARG, "D outside 0..2048, or D and feats disagree");
    if (const char *e = net_error(layers, n_layers, D + 3, out_stride, out_offset)) return fail(c, PS_ERR_ARG, e);
    BfRows Q;
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
