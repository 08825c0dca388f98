// keypoint_kernels.hip — the keypoint conditioning of the reference's
// take_rgbd (run_policy.py:202-285), fused (ps_cloud_keypoint_features): per
// 2-D keypoint of the keypoint view the pixels of a disc around it, their
// world points, and per cloud point whether its nearest such point lies under
// a threshold -- written as the feature rows the policy's network takes, the
// colours as floats and the conditioning value behind them.
//
// One kernel, k_cloud_keypoint, one block per (env, 256 cloud points).  A
// block first casts the rays of its env's n_kp * P patch pixels itself (at
// most 4 * 197: up to four per lane) and keeps their f64 world points in LDS
// (18.9 KB); no depth image and no per-pixel array exists.  The ray cast is
// ps_render_pixel.h's, shared with k_render, and the deprojection
// k_deproject_pixels' (deproject_at): a target equals ps_deproject_pixels of
// ps_render's depth bit for bit.  Then each lane takes one cloud point through
// the targets once: every lane reads the same LDS address (a broadcast), keeps
// the least squared distance per keypoint and takes one square root per
// keypoint.  No atomics, nothing shared between blocks; the blocks of an env
// recast the same few rays, which costs less than a second launch's latency
// (DESIGN.md §11.7).
#include "ps_ctx.h"
#include "ps_render.h"
#include "ps_render_pixel.h"

namespace {

constexpr int kKeypointBlock = kRenderBlock;
constexpr int kKeypointMaxSlots = 197;  // the disc of PS_CLOUD_KEYPOINT_MAX_RADIUS
static_assert(PS_CLOUD_KEYPOINT_MAX_RADIUS == 8, "kKeypointMaxSlots is the disc of radius 8");

struct KeypointArgs {
    RenderArgs r;  // the scene and, in r.cam, the keypoint view
    Tran tran;
    int n_kp, radius, slots;  // slots: P, the disc's pixels
    double threshold;
    float values[PS_CLOUD_KEYPOINT_MAX];
};

// largest h with h * h <= v, 0 <= v <= 64
PS_HD int isqrt_small(int v) {
    int h = 0;
    while ((h + 1) * (h + 1) <= v) h++;
    return h;
}

// P: the integer offsets (dx, dy) with dx^2 + dy^2 <= radius^2
inline int patch_slots(int radius) {
    int n = 0;
    for (int dx = -radius; dx <= radius; dx++) n += 2 * isqrt_small(radius * radius - dx * dx) + 1;
    return n;
}

// slot s (dx ascending, then dy ascending) of the disc -> its offset
PS_D void patch_offset(int radius, int s, int &dx, int &dy) {
    dx = dy = 0;
    for (int x = -radius; x <= radius; x++) {
        const int h = isqrt_small(radius * radius - x * x), n = 2 * h + 1;
        if (s < n) {
            dx = x;
            dy = s - h;
            return;
        }
        s -= n;
    }
}

__global__ __launch_bounds__(kKeypointBlock) void k_cloud_keypoint(KeypointArgs A, const float *prims,
                                                                   const int32_t *keypoints, const float *points,
                                                                   const uint8_t *colors, const int32_t *count,
                                                                   int n_points, float *feats, int ld, int offset,
                                                                   double *targets) {
#pragma clang fp contract(off)
    __shared__ float pr[RENDER_PRIM_FLOATS];
    __shared__ float rgba[8 * 4];
    __shared__ double tgt[PS_CLOUD_KEYPOINT_MAX * kKeypointMaxSlots * 3];
    const int64_t env = blockIdx.x;
    for (int k = threadIdx.x; k < RENDER_PRIM_FLOATS; k += kKeypointBlock) pr[k] = prims[env * RENDER_PRIM_FLOATS + k];
    if (threadIdx.x < 32) rgba[threadIdx.x] = A.r.vis.rgba[threadIdx.x >> 2][threadIdx.x & 3];
    __syncthreads();
    const int width = A.r.width, height = A.r.height;
    const int64_t npix = (int64_t)width * height;
    const int n_slots = A.n_kp * A.slots;
    for (int q = threadIdx.x; q < n_slots; q += kKeypointBlock) {
        const int k = q / A.slots;
        int dx, dy;
        patch_offset(A.radius, q - k * A.slots, dx, dy);
        const int32_t *kp = keypoints + (env * A.n_kp + k) * 2;
        const int64_t c = (int64_t)kp[0] + dx, r = (int64_t)kp[1] + dy;
        double p[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
        // a negative keypoint is the caller's "absent": none of its slots counts
        if (kp[0] >= 0 && kp[1] >= 0 && c >= 0 && c < width && r >= 0 && r < height) {
            // the arm primitives of the pixel's own tile, as k_cloud_gather takes them
            const int64_t tile = (r * width + c) / kRenderTile;
            unsigned mask = 0u;
            for (int a = 0; a < RENDER_CAPSULES + PM_NUM_SPHERES; a++)
                if (arm_prim_meets_tile(pr, A.r.cam, width, height, npix, a, tile)) mask |= 1u << a;
            float dep, cr, cg, cb;
            render_pixel(A.r.cam, A.r, pr, rgba, mask, (int)r, (int)c, dep, cr, cg, cb);
            deproject_at(A.tran, width, height, (int)c, (int)r, dep, p);
        }
        tgt[q * 3 + 0] = p[0];
        tgt[q * 3 + 1] = p[1];
        tgt[q * 3 + 2] = p[2];
        if (targets && blockIdx.y == 0) {
            double *o = targets + (env * n_slots + q) * 3;
            o[0] = p[0];
            o[1] = p[1];
            o[2] = p[2];
        }
    }
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.y * kKeypointBlock + threadIdx.x;
    if (j >= n_points) return;
    const int64_t at = env * n_points + j;
    float *row = feats + at * ld + offset;
    const bool empty = count && count[env] == 0;
    float value = 0.0f;
    if (!empty) {
        const double px = (double)points[at * 3 + 0], py = (double)points[at * 3 + 1], pz = (double)points[at * 3 + 2];
#pragma unroll
        for (int k = 0; k < PS_CLOUD_KEYPOINT_MAX; k++) {
            if (k >= A.n_kp) break;
            // a slot outside the image is NaN and never lowers the minimum
            double m = __builtin_inf();
            const double *t = tgt + k * A.slots * 3;
            for (int s = 0; s < A.slots; s++) {
                const double dx = px - t[s * 3 + 0], dy = py - t[s * 3 + 1], dz = pz - t[s * 3 + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                m = d2 < m ? d2 : m;
            }
            if (sqrt(m) < A.threshold) value = A.values[k];
        }
    }
    if (colors) {
        const uint8_t *col = colors + at * 3;
        row[0] = empty ? 0.0f : (float)col[0];
        row[1] = empty ? 0.0f : (float)col[1];
        row[2] = empty ? 0.0f : (float)col[2];
        row += 3;
    }
    row[0] = value;
}

}  // namespace

extern "C" {

int ps_cloud_keypoint_features(ps_ctx *c, const void *state, const ps_cloud_view *view, int width, int height,
                               const ps_visual *vis, const float *target_poses, const int32_t *keypoints, int n_kp,
                               int radius, double threshold, const float *values, const float *points,
                               const uint8_t *colors, const int32_t *count, int n_points, float *feats, int ld,
                               int out_offset, double *targets, void *stream) {
    if (!c || !state || !view || !vis || !keypoints || !values || !points || !feats)
        return fail(c, PS_ERR_ARG, "null argument");
    if (n_kp < 1 || n_kp > PS_CLOUD_KEYPOINT_MAX) return fail(c, PS_ERR_ARG, "n_kp outside 1..4");
    if (radius < 0 || radius > PS_CLOUD_KEYPOINT_MAX_RADIUS) return fail(c, PS_ERR_ARG, "radius outside 0..8");
    if (!(threshold > 0.0) || threshold == __builtin_inf())
        return fail(c, PS_ERR_ARG, "threshold must be positive and finite");
    if (width <= 0 || height <= 0 || (int64_t)width * height >= (1LL << 31))
        return fail(c, PS_ERR_ARG, "empty image, or 2^31 pixels or more");
    if (n_points < 1 || n_points > PS_CLOUD_MAX_DENSE_POINTS) return fail(c, PS_ERR_ARG, "K outside 1..2^20");
    const int cols = colors ? 4 : 1;
    if (out_offset < 0 || ld > PS_CLOUD_KEYPOINT_MAX_LD || (int64_t)out_offset + cols > ld)
        return fail(c, PS_ERR_ARG, "the feature columns do not fit ld (at most 4096)");
    hipStream_t st = (hipStream_t)stream;
    int rc = ps_launch_render_prep(c, state, target_poses, st);
    if (rc != PS_OK) return rc;
    KeypointArgs A;
    memset(&A, 0, sizeof A);
    A.r = render_args_of(c, width, height, vis);
    A.r.cam = cam_of(view->view, view->proj);
    memcpy(A.tran.m, view->tran_pix_world, sizeof A.tran.m);
    A.n_kp = n_kp;
    A.radius = radius;
    A.slots = patch_slots(radius);
    A.threshold = threshold;
    for (int k = 0; k < n_kp; k++) A.values[k] = values[k];
    const unsigned blocks = (unsigned)(((int64_t)n_points + kKeypointBlock - 1) / kKeypointBlock);
    hipLaunchKernelGGL(k_cloud_keypoint, dim3((unsigned)c->num_envs, blocks), dim3(kKeypointBlock), 0, st, A,
                       c->render_prims, keypoints, points, colors, count, n_points, feats, ld, out_offset, targets);
    return check_launch(c);
}

}  // extern "C"
