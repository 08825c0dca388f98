// cloud_kernels.hip — the fused multi-view point-cloud observation
// (ps_point_cloud): the views' filtered point clouds of every env, merged
// view by view in pixel order, cropped, and sampled with replacement to a
// fixed number of points, without the per-pixel arrays in between.  Three
// kernels over the workspace (per env and (view, pixel tile): 256 validity
// bits, their count, the exclusive prefix of the counts):
//   k_cloud_mask    casts every pixel's ray, deprojects it and keeps one bit;
//   k_cloud_scan    prefix of an env's tile counts, and M_b;
//   k_cloud_gather  per sample: rank -> tile -> bit -> pixel, whose ray is
//                   cast again for the point and the colour.
// The per-pixel arithmetic is ps_render_pixel.h's, shared with k_render and
// k_deproject_image: the result equals their composition bit for bit.
#include "ps_ctx.h"
#include "ps_render.h"
#include "ps_render_pixel.h"

namespace {

constexpr int kCloudMaxViews = 8;
constexpr int kTileWords = kRenderTile / 64;  // wave64 ballot words of a tile
static_assert(kRenderBlock == 256 && kRenderPix == 1 && kTileWords == 4, "a tile is the four ballots of one block");

struct CloudArgs {
    RenderArgs r;  // the scene; r.cam is unused (cams[view])
    Cam cams[kCloudMaxViews];
    Tran tran[kCloudMaxViews];
    int n_views, has_crop;
    float lo[3], hi[3];
    int64_t tiles;  // pixel tiles of one view
};

// workspace of B envs with nt = n_views * tiles (view, tile) entries each
struct CloudSpace {
    uint64_t *bits;   // [B][nt][4]
    int32_t *count;   // [B][nt]
    int32_t *prefix;  // [B][nt]
};

inline CloudSpace space_of(void *ws, int64_t n_env, int64_t nt) {
    CloudSpace s;
    s.bits = (uint64_t *)ws;
    s.count = (int32_t *)(s.bits + n_env * nt * kTileWords);
    s.prefix = s.count + n_env * nt;
    return s;
}

PS_D bool in_crop(const CloudArgs &A, const double p[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && p[k] > (double)A.lo[k] && p[k] < (double)A.hi[k];
    return ok;
}

// the env's primitive table and the role colours, as k_render stages them
PS_D void stage_scene(const CloudArgs &A, const float *prims, int64_t env, float *pr, float *rgba) {
    for (int k = threadIdx.x; k < RENDER_PRIM_FLOATS; k += kRenderBlock) pr[k] = prims[env * RENDER_PRIM_FLOATS + k];
    if (threadIdx.x < 32) rgba[threadIdx.x] = A.r.vis.rgba[threadIdx.x >> 2][threadIdx.x & 3];
}

// One block per (env, pixel tile, view), the ray caster's own shape: x envs,
// y tiles (<= 65 535), z views.  (256, 4) as k_render: four waves per SIMD.
__global__ __launch_bounds__(kRenderBlock, 4) void k_cloud_mask(CloudArgs A, const float *prims, CloudSpace S) {
    __shared__ float pr[RENDER_PRIM_FLOATS];
    __shared__ float rgba[8 * 4];
    __shared__ unsigned arm_mask;
    __shared__ uint64_t words[kTileWords];
    const int64_t env = blockIdx.x;
    const int view = blockIdx.z;
    stage_scene(A, prims, env, pr, rgba);
    if (threadIdx.x == 0) arm_mask = 0u;
    __syncthreads();
    const Cam &cm = A.cams[view];
    const int width = A.r.width, height = A.r.height;
    const int64_t npix = (int64_t)width * height;
    if (threadIdx.x < RENDER_CAPSULES + PM_NUM_SPHERES &&
        arm_prim_meets_tile(pr, cm, width, height, npix, threadIdx.x, blockIdx.y))
        atomicOr(&arm_mask, 1u << threadIdx.x);
    __syncthreads();
    const unsigned mask = arm_mask;
    const int64_t pix = (int64_t)blockIdx.y * kRenderTile + threadIdx.x;
    bool ok = false;
    if (pix < npix) {
        int r = (int)(pix / width), c = (int)(pix - (int64_t)r * width);
        float dep, cr, cg, cb;
        render_pixel(cm, A.r, pr, rgba, mask, r, c, dep, cr, cg, cb);
        double x, y, p[3];
        ok = deproject_pixel(A.tran[view], width, height, r, c, dep, x, y, p);
        if (A.has_crop) ok = ok && in_crop(A, p);
    }
    const uint64_t w = __ballot(ok);
    if ((threadIdx.x & 63) == 0) words[threadIdx.x >> 6] = w;
    __syncthreads();
    const int64_t nt = A.tiles * A.n_views;
    const int64_t at = env * nt + (int64_t)view * A.tiles + blockIdx.y;
    if (threadIdx.x < kTileWords) S.bits[at * kTileWords + threadIdx.x] = words[threadIdx.x];
    if (threadIdx.x == 0) {
        int n = 0;
#pragma unroll
        for (int k = 0; k < kTileWords; k++) n += __popcll(words[k]);
        S.count[at] = n;
    }
}

// Exclusive prefix of one env's nt tile counts, 256 at a time: an inclusive
// Hillis-Steele scan in LDS plus the carry of the chunks before.
constexpr int kScanBlock = 256;

__global__ __launch_bounds__(kScanBlock) void k_cloud_scan(int64_t nt, CloudSpace S, int32_t *count) {
    __shared__ int32_t buf[2][kScanBlock];
    const int64_t env = blockIdx.x;
    const int32_t *cnt = S.count + env * nt;
    int32_t *pre = S.prefix + env * nt;
    int32_t carry = 0;
    for (int64_t base = 0; base < nt; base += kScanBlock) {
        const int64_t k = base + threadIdx.x;
        const int32_t mine = k < nt ? cnt[k] : 0;
        int cur = 0;
        buf[0][threadIdx.x] = mine;
        __syncthreads();
#pragma unroll
        for (int d = 1; d < kScanBlock; d <<= 1) {
            int32_t v = buf[cur][threadIdx.x];
            if ((int)threadIdx.x >= d) v += buf[cur][threadIdx.x - d];
            buf[cur ^ 1][threadIdx.x] = v;
            cur ^= 1;
            __syncthreads();
        }
        if (k < nt) pre[k] = carry + buf[cur][threadIdx.x] - mine;
        carry += buf[cur][kScanBlock - 1];
        __syncthreads();  // the next chunk overwrites buf
    }
    if (count && threadIdx.x == 0) count[env] = carry;
}

// position of the k-th (0-based) set bit of w, k < popcount(w): six halvings
PS_D int select_bit(uint64_t w, int k) {
    int pos = 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        int c = __popcll(w & ((1ull << s) - 1ull));
        if (k >= c) {
            k -= c;
            w >>= s;
            pos += s;
        }
    }
    return pos;
}

// splitmix64 of counter c under `seed` (the finaliser of ps_task.h's goal stream)
PS_D uint64_t cloud_draw(uint64_t seed, uint64_t c) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ULL * (c + 1ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// One lane per (env, sample): x envs, y blocks of 256 samples.
__global__ __launch_bounds__(kRenderBlock) void k_cloud_gather(CloudArgs A, const float *prims, CloudSpace S,
                                                               int n_points, uint64_t seed, float *points,
                                                               uint8_t *colors, int32_t *source) {
    __shared__ float pr[RENDER_PRIM_FLOATS];
    __shared__ float rgba[8 * 4];
    const int64_t env = blockIdx.x;
    stage_scene(A, prims, env, pr, rgba);
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.y * kRenderBlock + threadIdx.x;
    if (j >= n_points) return;
    const int64_t nt = A.tiles * A.n_views;
    const int32_t *pre = S.prefix + env * nt;
    const int32_t *cnt = S.count + env * nt;
    const int64_t M = (int64_t)pre[nt - 1] + cnt[nt - 1];
    const int64_t out = env * n_points + j;
    if (M == 0) {
        points[out * 3 + 0] = points[out * 3 + 1] = points[out * 3 + 2] = 0.0f;
        if (colors) colors[out * 3 + 0] = colors[out * 3 + 1] = colors[out * 3 + 2] = 0;
        if (source) source[out] = -1;
        return;
    }
    const int64_t rank = (int64_t)__umul64hi(cloud_draw(seed, (uint64_t)out), (uint64_t)M);
    // the last entry whose exclusive prefix is <= rank (empty tiles share the prefix of the next one)
    int64_t lo = 0, hi = nt;  // pre[lo] <= rank < pre[hi] (pre[nt] = M)
    while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (pre[mid] <= rank) lo = mid;
        else hi = mid;
    }
    int k = (int)(rank - pre[lo]);
    const uint64_t *w = S.bits + (env * nt + lo) * kTileWords;
    int word = 0;
    uint64_t bits = w[0];
#pragma unroll
    for (int q = 0; q < kTileWords - 1; q++) {
        int c = __popcll(bits);
        if (word == q && k >= c) {
            k -= c;
            word = q + 1;
            bits = w[q + 1];
        }
    }
    const int view = (int)(lo / A.tiles);
    const int64_t tile = lo - (int64_t)view * A.tiles;
    const int64_t pix = tile * kRenderTile + word * 64 + select_bit(bits, k);
    const int width = A.r.width, height = A.r.height;
    const int64_t npix = (int64_t)width * height;
    // the view differs from lane to lane: its camera is read in a uniform loop
    // (a lane-indexed kernarg array would go to scratch)
    float dep = 1.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    double p[3] = {0.0, 0.0, 0.0};
    const int r = (int)(pix / width), c = (int)(pix - (int64_t)r * width);
    for (int v = 0; v < A.n_views; v++) {
        if (v != view) continue;
        const Cam &cm = A.cams[v];
        unsigned mask = 0u;
        for (int q = 0; q < RENDER_CAPSULES + PM_NUM_SPHERES; q++)
            if (arm_prim_meets_tile(pr, cm, width, height, npix, q, tile)) mask |= 1u << q;
        render_pixel(cm, A.r, pr, rgba, mask, r, c, dep, cr, cg, cb);
        double x, y;
        deproject_pixel(A.tran[v], width, height, r, c, dep, x, y, p);
    }
    points[out * 3 + 0] = (float)p[0];
    points[out * 3 + 1] = (float)p[1];
    points[out * 3 + 2] = (float)p[2];
    if (colors) {
        colors[out * 3 + 0] = colour_u8(cr);
        colors[out * 3 + 1] = colour_u8(cg);
        colors[out * 3 + 2] = colour_u8(cb);
    }
    if (source) source[out] = (int32_t)((int64_t)view * npix + pix);
}

// tiles of one view, or a negative code for a shape ps_point_cloud refuses
inline int64_t cloud_tiles(int64_t num_envs, int n_views, int width, int height) {
    if (num_envs < 1 || num_envs > PS_MAX_ENVS || n_views < 1 || n_views > kCloudMaxViews || width <= 0 || height <= 0)
        return PS_ERR_ARG;
    const int64_t tiles = render_tiles(width, height);
    if (tiles > 65535 || (int64_t)n_views * width * height >= (1LL << 31)) return PS_ERR_ARG;
    return tiles;
}

}  // namespace

extern "C" {

int64_t ps_cloud_workspace_bytes(int64_t num_envs, int n_views, int width, int height) {
    const int64_t tiles = cloud_tiles(num_envs, n_views, width, height);
    if (tiles < 0) return tiles;
    return num_envs * n_views * tiles * (int64_t)(kTileWords * sizeof(uint64_t) + 2 * sizeof(int32_t));
}

int ps_point_cloud(ps_ctx *c, const void *state, const ps_cloud_view *views, int n_views, int width, int height,
                   const ps_visual *vis, const float *targets, const ps_cloud_crop *crop, int n_points, uint64_t seed,
                   float *points, uint8_t *colors, int32_t *source, int32_t *count, void *workspace, void *stream) {
    if (!c || !state || !views || !vis || !points || !workspace) return fail(c, PS_ERR_ARG, "null argument");
    if (n_views < 1 || n_views > kCloudMaxViews) return fail(c, PS_ERR_ARG, "n_views outside 1..8");
    if (n_points < 1) return fail(c, PS_ERR_ARG, "n_points < 1");
    if (width <= 0 || height <= 0) return fail(c, PS_ERR_ARG, "empty image");
    const int64_t tiles = cloud_tiles(c->num_envs, n_views, width, height);
    if (tiles < 0) return fail(c, PS_ERR_ARG, "image too large (more than 65 535 pixel tiles, or 2^31 merged pixels)");
    const int64_t sample_blocks = ((int64_t)n_points + kRenderBlock - 1) / kRenderBlock;
    if (sample_blocks > 65535) return fail(c, PS_ERR_ARG, "n_points too large (more than 65 535 blocks of samples)");
    hipStream_t st = (hipStream_t)stream;
    int rc = ps_launch_render_prep(c, state, targets, st);
    if (rc != PS_OK) return rc;
    CloudArgs A;
    memset(&A, 0, sizeof A);
    A.r = render_args_of(c, width, height, vis);
    for (int v = 0; v < n_views; v++) {
        A.cams[v] = cam_of(views[v].view, views[v].proj);
        memcpy(A.tran[v].m, views[v].tran_pix_world, sizeof A.tran[v].m);
    }
    A.n_views = n_views;
    A.has_crop = crop != nullptr;
    if (crop)
        for (int k = 0; k < 3; k++) {
            A.lo[k] = crop->lo[k];
            A.hi[k] = crop->hi[k];
        }
    A.tiles = tiles;
    const int64_t nt = tiles * n_views;
    CloudSpace S = space_of(workspace, c->num_envs, nt);
    hipLaunchKernelGGL(k_cloud_mask, dim3((unsigned)c->num_envs, (unsigned)tiles, (unsigned)n_views),
                       dim3(kRenderBlock), 0, st, A, c->render_prims, S);
    hipLaunchKernelGGL(k_cloud_scan, dim3((unsigned)c->num_envs), dim3(kScanBlock), 0, st, nt, S, count);
    hipLaunchKernelGGL(k_cloud_gather, dim3((unsigned)c->num_envs, (unsigned)sample_blocks), dim3(kRenderBlock), 0, st,
                       A, c->render_prims, S, n_points, seed, points, colors, source);
    return check_launch(c);
}

}  // extern "C"
