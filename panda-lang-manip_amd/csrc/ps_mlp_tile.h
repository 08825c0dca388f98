// ps_mlp_tile.h — what the two shared-MLP kernels (mlp_kernels.hip on the f32
// MFMA, mlp_bfloat_kernels.hip on the bf16 one) have in common: everything
// about a tile except its multiplications.
//
// A workgroup owns a tile of ROWS rows (32 in f32, 64 in bf16) of one cloud.
// The tile's activations stay in LDS from the first layer to the last
// ([row][channel], two buffers the layers alternate between: layer l reads
// buf0 if l is even, buf1 if odd, and writes the other); the waves share the
// rows and split a layer's output channels in chunks of 32.  Rows come from
// memory directly or, gathered, through group_idx as ps_cloud_group composes
// them, so the grouped tensor never exists.  The last layer leaves its result
// as rows in the accumulator registers and the channel on the lane (NACC = ROWS
// / 32 accumulators per wave); from there it goes to `out` (G = 1) or into the
// maximum of its group.  Groups no longer than a tile share it, ROWS / G to a
// tile; a group longer than a tile is walked tile by tile by one workgroup
// with the running maximum in LDS.  A kernel file keeps its LDS layout, its
// staging loop, its mma_chunk and its hidden-layer write-back.
#pragma once

#include <type_traits>

#include "ps_cloud_math.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMlpChunk = 32;    // output channels of one wave's pass: the MFMA's N
constexpr int kMlpKChunk = 512;  // most input channels resident in LDS (= the hidden limit)
constexpr int kMlpMaxHidden = PS_CLOUD_MLP_MAX_HIDDEN;
constexpr int kMlpMaxLast = PS_CLOUD_MLP_MAX_LAST;
constexpr int kMlpMaxC0 = PS_CLOUD_MAX_PROP_FEATURES + 3;
constexpr int64_t kMlpMaxBlocks = 1 << 20;

// WT: the weights' element, float or uint16_t (bf16 bits)
template <typename WT>
struct MlpNet {
    const WT *W[PS_CLOUD_MLP_MAX_LAYERS];
    const float *b[PS_CLOUD_MLP_MAX_LAYERS];
    int c_out[PS_CLOUD_MLP_MAX_LAYERS];
    int relu[PS_CLOUD_MLP_MAX_LAYERS];
    int n_layers;
    int c0;
};

// Where the rows come from: `rows` [B, R, c0], or (gathered) the rows of
// ps_cloud_group: feats[gidx] then xyz[gidx] - xyz[centre_idx], R = s * k.
struct MlpRows {
    const float *rows;
    const float *xyz, *feats;
    const int32_t *centre_idx, *gidx;
    int n, d, s, k;
    int R;
};

// the row of the MFMA's 32 x 32 result that register r of lane half h holds
PS_D int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Tile tt of a grid-stride unit: groups g0 .. g0 + ngroups - 1 of cloud env,
// rows r0 .. r0 + nrows - 1 of that cloud.
struct MlpTile {
    int64_t env;
    int g0, ngroups;
    int r0, nrows;
};

template <int ROWS>
PS_D int mlp_tiles(int G) { return G > ROWS ? (G + ROWS - 1) / ROWS : 1; }

// the unit's cloud and groups (once per unit: a 64-bit division), then mlp_tile for each of its tiles
template <int ROWS>
PS_D MlpTile mlp_unit(int64_t unit, int64_t units_per_cloud, int G, int groups) {
    MlpTile T;
    T.env = unit / units_per_cloud;
    const int u = (int)(unit - T.env * units_per_cloud);
    if (G > ROWS) {
        T.g0 = u;
        T.ngroups = 1;
    } else {
        const int per = ROWS / G;
        T.g0 = u * per;
        T.ngroups = groups - T.g0 < per ? groups - T.g0 : per;
    }
    T.r0 = T.nrows = 0;
    return T;
}

template <int ROWS>
PS_D MlpTile mlp_tile(MlpTile T, int tt, int G) {
    T.r0 = T.g0 * G + tt * ROWS;
    T.nrows = G > ROWS ? (G - tt * ROWS < ROWS ? G - tt * ROWS : ROWS) : T.ngroups * G;
    return T;
}

// The gathered tile's point indices (clamped) into s_gi[ROWS] and its rows'
// centres into s_centre[ROWS * 3]; rows past the tile's get index 0 and a zero
// centre.  A barrier stands between this and the first read.
template <int ROWS>
PS_D void mlp_gather_prologue(const MlpRows &S, const MlpTile &T, int32_t *s_gi, float *s_centre) {
    const int tid = threadIdx.x;
    if (tid >= ROWS) return;
    int gi = 0;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (tid < T.nrows) {
        const int r = T.r0 + tid;
        gi = clamp_index(S.gidx[T.env * S.R + r], S.n);
        const int ci = clamp_index(S.centre_idx[T.env * S.s + r / S.k], S.n);
        const float *c = S.xyz + (T.env * S.n + ci) * 3;
        cx = c[0], cy = c[1], cz = c[2];
    }
    s_gi[tid] = gi;
    s_centre[tid * 3 + 0] = cx;
    s_centre[tid * 3 + 1] = cy;
    s_centre[tid * 3 + 2] = cz;
}

// A layer's ReLU on a wave's accumulators: once per chunk, ahead of the branch
// between a hidden layer's write-back and the last layer's epilogue.
template <int NACC>
PS_D void mlp_relu(f32x16 (&acc)[NACC], int relu) {
    if (!relu) return;
#pragma unroll
    for (int m = 0; m < NACC; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[m][r] = acc[m][r] > 0.0f ? acc[m][r] : 0.0f;
}

// ------------------------------------------------------------- host side
// LAYER: ps_cloud_mlp_layer or ps_cloud_mlp_bfloat_layer
template <typename LAYER>
inline const char *net_error(const LAYER *layers, int n_layers, int c0, int64_t out_stride, int out_offset) {
    if (n_layers < 1 || n_layers > PS_CLOUD_MLP_MAX_LAYERS) return "n_layers outside 1..4";
    if (c0 < 1 || c0 > kMlpMaxC0) return "C0 outside 1..2051";
    for (int l = 0; l < n_layers; l++) {
        if (!layers[l].W || !layers[l].b) return "a layer without W or b";
        // the bf16 kernel reads the weights from global memory as 128-bit words
        if (std::is_same<LAYER, ps_cloud_mlp_bfloat_layer>::value && ((uintptr_t)layers[l].W & 15) != 0)
            return "a layer's W is not 16-byte aligned";
        const int most = l == n_layers - 1 ? kMlpMaxLast : kMlpMaxHidden;
        if (layers[l].c_out < 1 || layers[l].c_out > most) return "c_out outside 1..512 (the last: 1..1024)";
    }
    if (out_offset < 0 || out_stride < (int64_t)out_offset + layers[n_layers - 1].c_out)
        return "out_offset < 0 or out_stride < out_offset + the last c_out";
    return nullptr;
}

// The arguments of ps_cloud_mlp and its bfloat twin: PS_OK with S filled, or
// the refusal.
template <typename LAYER>
inline int mlp_args(ps_ctx *c, const float *rows, int R, int C0, const LAYER *layers, int n_layers, int G, float *out,
                    int64_t out_stride, int out_offset, MlpRows &S) {
    if (!c || !rows || !layers || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (const char *e = net_error(layers, n_layers, C0, out_stride, out_offset)) return fail(c, PS_ERR_ARG, e);
    if (R < 1 || G < 1 || R % G != 0) return fail(c, PS_ERR_ARG, "R < 1, G < 1 or R not a multiple of G");
    memset(&S, 0, sizeof S);
    S.rows = rows;
    S.R = R;
    return PS_OK;
}

// The arguments of ps_cloud_group_mlp and its bfloat twin, likewise.
template <typename LAYER>
inline int group_mlp_args(ps_ctx *c, const float *xyz, const float *feats, int N, int D, const int32_t *centre_idx,
                          int S, const int32_t *group_idx, int K, const LAYER *layers, int n_layers, float *out,
                          int64_t out_stride, int out_offset, MlpRows &Q) {
    if (!c || !xyz || !centre_idx || !group_idx || !layers || !out) return fail(c, PS_ERR_ARG, "null argument");
    if (N < 1 || N > PS_CLOUD_MAX_POINTS) return fail(c, PS_ERR_ARG, "N outside 1..8192");
    if (S < 1 || S > N) return fail(c, PS_ERR_ARG, "S outside 1..N");
    if (K < 1 || (int64_t)S * K > 0x7fffffff) return fail(c, PS_ERR_ARG, "nsample < 1 (or S * nsample >= 2^31)");
    if (D < 0 || D > PS_CLOUD_MAX_PROP_FEATURES || (feats == nullptr) != (D == 0))
        return fail(c, PS_ERR_ARG, "D outside 0..2048, or D and feats disagree");
    if (const char *e = net_error(layers, n_layers, D + 3, out_stride, out_offset)) return fail(c, PS_ERR_ARG, e);
    memset(&Q, 0, sizeof Q);
    Q.xyz = xyz;
    Q.feats = feats;
    Q.centre_idx = centre_idx;
    Q.gidx = group_idx;
    Q.n = N, Q.d = D, Q.s = S, Q.k = K;
    Q.R = S * K;
    return PS_OK;
}

// A launch: nw waves to a workgroup, the LDS pitches of the two activation
// buffers, pool_n running maxima, upc units to a cloud, `units` in all walked
// by `blocks` workgroups.
struct MlpPlan {
    int nw, pitch0, pitch1, pool_n;
    int64_t upc, units, blocks;
};

// Fills M from the (checked) layers and plans the launch for tiles of ROWS
// rows: as many waves as the widest layer has chunks of 32 channels, rounded
// down to a power of two, MAX_WAVES at most; pitch_of(width) is the file's LDS
// pitch of a buffer whose widest row has `width` channels.
template <int ROWS, int MAX_WAVES, typename LAYER, typename WT>
inline MlpPlan mlp_plan(const ps_ctx *c, const LAYER *layers, int n_layers, int c0, int R, int G, int (*pitch_of)(int),
                        MlpNet<WT> &M) {
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
    MlpPlan P;
    const int nch = (widest + kMlpChunk - 1) / kMlpChunk;
    for (P.nw = 1; 2 * P.nw <= nch && 2 * P.nw <= MAX_WAVES;) P.nw *= 2;
    P.pitch0 = pitch_of(w0), P.pitch1 = pitch_of(w1);
    P.pool_n = G > ROWS ? layers[n_layers - 1].c_out : 0;
    const int groups = R / G;
    P.upc = G > ROWS ? groups : (groups + ROWS / G - 1) / (ROWS / G);
    P.units = P.upc * c->num_envs;
    P.blocks = P.units < kMlpMaxBlocks ? P.units : kMlpMaxBlocks;
    return P;
}

// The kernels' common signature, and a launch of one with `lds` bytes of
// dynamic LDS (max_lds: the most any network takes).
template <typename WT>
using MlpKernel = void (*)(MlpNet<WT>, MlpRows, int, float *, int64_t, int, int64_t, int64_t, int, int);

template <typename WT>
inline int mlp_launch(ps_ctx *c, MlpKernel<WT> kernel, const MlpPlan &P, size_t lds, size_t max_lds,
                      const MlpNet<WT> &M, const MlpRows &S, int G, float *out, int64_t out_stride, int out_offset,
                      hipStream_t st) {
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds) !=
        hipSuccess)
        return fail(c, PS_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    hipLaunchKernelGGL(kernel, dim3((unsigned)P.blocks), dim3(P.nw * 64), lds, st, M, S, G, out, out_stride,
                       out_offset, P.units, P.upc, P.pitch0, P.pitch1);
    return check_launch(c);
}

}  // namespace
