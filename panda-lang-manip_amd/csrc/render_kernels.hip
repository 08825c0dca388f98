// render_kernels.hip — the camera image of the batch, next to its ray-shape
// tests (ps_render.h) and the per-pixel work (ps_render_pixel.h): the per-env
// primitive table (k_render_prep), the ray caster (k_render) and render()'s
// deprojection of the depth buffer (k_deproject_image, k_deproject_pixels),
// with the C ABI entry points that launch them: ps_camera, ps_render,
// ps_deproject_image, ps_deproject_pixels.  Needs the state view and the
// link frames, nothing of the substep.
#include "ps_ctx.h"
#include "ps_kinematics.h"
#include "ps_render.h"
#include "ps_render_pixel.h"

namespace {

// Per-env primitives: the arm's capsules (joint frame to joint frame), the
// gripper spheres, object and target poses.  One lane per env.
__global__ __launch_bounds__(kBlock) void k_render_prep(KParams P, int n_objects, const float *targets, float *prims) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const StateView &s = P.s;
    float q[9], qd[9];
    load_robot(s, i, q, qd);
    Kin k;
    fk(q, k);
    float *o = prims + i * RENDER_PRIM_FLOATS;
    const V3 b = P.sc.base;
    auto put3 = [&](int at, V3 v) { o[at] = v.x; o[at + 1] = v.y; o[at + 2] = v.z; };
    // link0 column, upper arm, elbow offsets, forearm, wrist, flange, hand bar
    const V3 hand_a = k.f[8].o + mul(k.f[8].R, mk(0.0f, -0.09f, 0.03f));
    const V3 hand_b = k.f[8].o + mul(k.f[8].R, mk(0.0f, 0.09f, 0.03f));
    const V3 wrist = k.f[8].o + mul(k.f[8].R, mk(0.0f, 0.0f, 0.04f));  // flange -> palm (hand origin = flange)
    const V3 A[RENDER_CAPSULES] = {mk(0, 0, 0), k.f[1].o, k.f[2].o, k.f[3].o, k.f[5].o, k.f[6].o, k.f[7].o, hand_a};
    const V3 Bp[RENDER_CAPSULES] = {k.f[0].o, k.f[2].o, k.f[3].o, k.f[4].o, k.f[6].o, k.f[7].o, wrist, hand_b};
    const float R[RENDER_CAPSULES] = {0.07f, 0.065f, 0.06f, 0.06f, 0.055f, 0.05f, 0.045f, 0.03f};
#pragma unroll
    for (int c = 0; c < RENDER_CAPSULES; c++) {
        put3(RP_CAPS + c * 7, A[c] + b);
        put3(RP_CAPS + c * 7 + 3, Bp[c] + b);
        o[RP_CAPS + c * 7 + 6] = R[c];
    }
    static_for<0, PM_NUM_SPHERES>([&](auto SS) {
        constexpr int S = decltype(SS)::value;
        constexpr SphereDef d = sphere_def(S);
        V3 c = k.f[d.link].o + mul(k.f[d.link].R, mk((float)d.c[0], (float)d.c[1], (float)d.c[2])) + b;
        put3(RP_SPH + S * 4, c);
        o[RP_SPH + S * 4 + 3] = (float)d.r;
    });
    {
        // bounding sphere of the arm's primitives: k_render skips them for rays that miss it
        V3 lo = mk(3e38f, 3e38f, 3e38f), hi = mk(-3e38f, -3e38f, -3e38f);
        auto grow = [&](V3 p) {
            lo = mk(fminf(lo.x, p.x), fminf(lo.y, p.y), fminf(lo.z, p.z));
            hi = mk(fmaxf(hi.x, p.x), fmaxf(hi.y, p.y), fmaxf(hi.z, p.z));
        };
        float rmax = 0.0f;
        for (int c = 0; c < RENDER_CAPSULES; c++) {
            grow(mk(o[RP_CAPS + c * 7], o[RP_CAPS + c * 7 + 1], o[RP_CAPS + c * 7 + 2]));
            grow(mk(o[RP_CAPS + c * 7 + 3], o[RP_CAPS + c * 7 + 4], o[RP_CAPS + c * 7 + 5]));
            rmax = fmaxf(rmax, o[RP_CAPS + c * 7 + 6]);
        }
        for (int c = 0; c < PM_NUM_SPHERES; c++) {
            grow(mk(o[RP_SPH + c * 4], o[RP_SPH + c * 4 + 1], o[RP_SPH + c * 4 + 2]));
            rmax = fmaxf(rmax, o[RP_SPH + c * 4 + 3]);
        }
        V3 ctr = (lo + hi) * 0.5f, half = (hi - lo) * 0.5f;
        put3(RP_ARM_BOUND, ctr);
        o[RP_ARM_BOUND + 3] = sqrtf(dot(half, half)) * 1.0001f + rmax + 1e-4f;
    }
    for (int ob = 0; ob < 2; ob++) {
        Body bd;
        if (ob < n_objects) load_body(s, i, ob, bd);
        else bd = Body{mk(0, 0, -100.0f), Q4{0, 0, 0, 1}, mk(0, 0, 0), mk(0, 0, 0)};
        M3 Rm = quat_to_mat(bd.quat);
        put3(RP_OBJ + ob * 12, bd.pos);
        for (int e = 0; e < 9; e++) o[RP_OBJ + ob * 12 + 3 + e] = Rm.m[e];
        V3 tp = mk(0, 0, -100.0f);
        Q4 tq = Q4{0, 0, 0, 1};
        if (targets) {
            const float *t = targets + (i * 2 + ob) * 7;
            tp = mk(t[0], t[1], t[2]);
            tq = Q4{t[3], t[4], t[5], t[6]};
        }
        M3 Rt = quat_to_mat(tq);
        put3(RP_TGT + ob * 12, tp);
        for (int e = 0; e < 9; e++) o[RP_TGT + ob * 12 + 3 + e] = Rt.m[e];
    }
}

// getCameraImage (pybullet.py:186-192) by ray casting: one lane per pixel
// (render_pixel, ps_render_pixel.h), blockIdx.x = env.
// (256, 4): four waves per SIMD at <= 128 VGPRs -- a lone wave per SIMD leaves the
// ray tests' dependent chains exposed
__global__ __launch_bounds__(kRenderBlock, 4) void k_render(RenderArgs a, const float *prims, float *depth,
                                                            uint8_t *rgb) {
    __shared__ float pr[RENDER_PRIM_FLOATS];
    __shared__ float rgba[8 * 4];  // colours by role, indexed per pixel (a kernarg array would go to scratch)
    __shared__ unsigned arm_mask;
    const int64_t env = blockIdx.x;  // x: envs (up to 2^31), y: pixel tiles (<= 65 535)
    for (int k = threadIdx.x; k < RENDER_PRIM_FLOATS; k += kRenderBlock) pr[k] = prims[env * RENDER_PRIM_FLOATS + k];
    if (threadIdx.x < 32) rgba[threadIdx.x] = a.vis.rgba[threadIdx.x >> 2][threadIdx.x & 3];
    if (threadIdx.x == 0) arm_mask = 0u;
    __syncthreads();
    const Cam &cm = a.cam;
    const int64_t npix = (int64_t)a.width * a.height;
    // row culling of the arm primitives, one per lane (arm_prim_meets_tile)
    if (threadIdx.x < RENDER_CAPSULES + PM_NUM_SPHERES &&
        arm_prim_meets_tile(pr, cm, a.width, a.height, npix, threadIdx.x, blockIdx.y))
        atomicOr(&arm_mask, 1u << threadIdx.x);
    __syncthreads();
    const unsigned mask = arm_mask;
    const int64_t pix = (int64_t)blockIdx.y * kRenderTile + threadIdx.x;
    if (pix >= npix) return;
    int r = (int)(pix / a.width), c = (int)(pix - (int64_t)r * a.width);
    float dep, cr, cg, cb;
    render_pixel(cm, a, pr, rgba, mask, r, c, dep, cr, cg, cb);
    int64_t at = env * npix + pix;
    if (depth) depth[at] = dep;
    if (rgb) {
        rgb[at * 3 + 0] = colour_u8(cr);
        rgb[at * 3 + 1] = colour_u8(cg);
        rgb[at * 3 + 2] = colour_u8(cb);
    }
}

// render()'s post-processing of getCameraImage's depth (pybullet.py:203-262),
// per env and pixel: NDC of np.mgrid (left/top pixel edges, the reference's
// convention), valid = depth < 0.99 and the workspace box on the world point,
// the world point and pixels_2d.
constexpr int kDeprojBlock = 256;

__global__ __launch_bounds__(kDeprojBlock) void k_deproject_image(int64_t n_env, int width, int height, Tran T,
                                                                  const float *depth, double *points,
                                                                  uint8_t *valid, double *pix2d) {
#pragma clang fp contract(off)
    // the block's points / pixels_2d are staged in LDS and leave as
    // lane-contiguous 8-byte stores (a wave writes 512 contiguous bytes per
    // instruction) instead of 24- and 16-byte strided ones
    __shared__ double sp[kDeprojBlock * 3];
    __shared__ double sx[kDeprojBlock * 2];
    const int64_t npix = (int64_t)width * height, total = n_env * npix;
    const int64_t g0 = (int64_t)blockIdx.x * kDeprojBlock, g = g0 + threadIdx.x;
    if (g < total) {
        int64_t pix = g % npix;
        int r = (int)(pix / width), c = (int)(pix - (int64_t)r * width);
        double x, y, p[3];
        bool ok = deproject_pixel(T, width, height, r, c, depth[g], x, y, p);
        if (valid) valid[g] = ok;
        sp[threadIdx.x * 3 + 0] = p[0];
        sp[threadIdx.x * 3 + 1] = p[1];
        sp[threadIdx.x * 3 + 2] = p[2];
        // (xy + 1) / 2, x *= w, y *= h, y = h - y
        double px = opaque(x + 1.0) / 2.0, py = opaque(y + 1.0) / 2.0;
        sx[threadIdx.x * 2 + 0] = px * (double)width;
        sx[threadIdx.x * 2 + 1] = (double)height - opaque(py * (double)height);
    }
    __syncthreads();
    const int64_t n_here = total - g0 < kDeprojBlock ? total - g0 : kDeprojBlock;
    if (points)
        for (int k = threadIdx.x; k < n_here * 3; k += kDeprojBlock) points[g0 * 3 + k] = sp[k];
    if (pix2d)
        for (int k = threadIdx.x; k < n_here * 2; k += kDeprojBlock) pix2d[g0 * 2 + k] = sx[k];
}

// PyBullet.deproject(depth, pixels, tran_pix_world) (pybullet.py:109-146) for
// n pixels (col, row) per env
__global__ __launch_bounds__(256) void k_deproject_pixels(int64_t n_env, int n, int width, int height, Tran T,
                                                          const float *depth, const int32_t *pixels, double *points) {
#pragma clang fp contract(off)
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_env * n) return;
    int64_t env = g / n;
    int pc = pixels[g * 2 + 0], prow = pixels[g * 2 + 1];
    if (pc < 0 || pc >= width || prow < 0 || prow >= height) {
        // outside the image (numpy would raise; the host wrapper does): no read, NaN point
        points[g * 3 + 0] = points[g * 3 + 1] = points[g * 3 + 2] = __builtin_nan("");
        return;
    }
    double p[3];
    deproject_at(T, width, height, pc, prow, depth[env * (int64_t)width * height + (int64_t)prow * width + pc], p);
    points[g * 3 + 0] = p[0];
    points[g * 3 + 1] = p[1];
    points[g * 3 + 2] = p[2];
}

}  // namespace

// k_render_prep for every kernel that casts rays (declared in ps_render_pixel.h)
int ps_launch_render_prep(ps_ctx *c, const void *state, const float *targets, hipStream_t st) {
    if (!c->render_prims) {
        if (hipMalloc((void **)&c->render_prims, sizeof(float) * RENDER_PRIM_FLOATS * c->num_envs) != hipSuccess) {
            c->render_prims = nullptr;
            return fail(c, PS_ERR_HIP, "hipMalloc of the render scratch failed");
        }
    }
    KParams P = params_of(c, (void *)state);
    hipLaunchKernelGGL(k_render_prep, grid_of(P.n, kBlock), dim3(kBlock), 0, st, P, c->cfg.n_objects, targets,
                       c->render_prims);
    return PS_OK;
}

// ------------------------------------------------------------------- C ABI
extern "C" {

int ps_camera(const float target[3], float distance, float yaw, float pitch, float roll, int width, int height,
              float view[16], float proj[16], double tran_pix_world[16]) {
    if (!target || !view || !proj || width <= 0 || height <= 0) return PS_ERR_ARG;
    ps_camera_math::view_from_yaw_pitch_roll(target, distance, yaw, pitch, roll, view);
    ps_camera_math::projection_fov(60.0, (double)width / height, 0.1, 100.0, proj);
    if (tran_pix_world) {
        // np.linalg.inv(P @ V) of the reshape(order='F') matrices, in double
        double P[16], V[16], PV[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                P[r * 4 + c] = proj[c * 4 + r];
                V[r * 4 + c] = view[c * 4 + r];
            }
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                double acc = 0.0;
                for (int k = 0; k < 4; k++) acc += P[r * 4 + k] * V[k * 4 + c];
                PV[r * 4 + c] = acc;
            }
        if (!ps_camera_math::invert4(PV, tran_pix_world)) return PS_ERR_ARG;
    }
    return PS_OK;
}

int ps_render(ps_ctx *c, const void *state, const float view[16], const float proj[16], int width, int height,
              const ps_visual *vis, const float *targets, float *depth, uint8_t *rgb, void *stream) {
    if (!c || !state || !view || !proj || !vis || width <= 0 || height <= 0) return fail(c, PS_ERR_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    int rc = ps_launch_render_prep(c, state, targets, st);
    if (rc != PS_OK) return rc;
    RenderArgs a = render_args_of(c, width, height, vis);
    a.cam = cam_of(view, proj);
    int64_t tiles = render_tiles(width, height);
    if (tiles > 65535) return fail(c, PS_ERR_ARG, "image too large (more than 65 535 pixel tiles)");
    dim3 g((unsigned)c->num_envs, (unsigned)tiles);
    hipLaunchKernelGGL(k_render, g, dim3(kRenderBlock), 0, st, a, c->render_prims, depth, rgb);
    return check_launch(c);
}

int ps_deproject_image(ps_ctx *c, const float *depth, const double tran_pix_world[16], int width, int height,
                       double *points, uint8_t *valid, double *pixels_2d, void *stream) {
    if (!c || !depth || !tran_pix_world || width <= 0 || height <= 0) return fail(c, PS_ERR_ARG, "null argument");
    Tran T;
    memcpy(T.m, tran_pix_world, sizeof T.m);
    int64_t n = c->num_envs * (int64_t)width * height;
    hipLaunchKernelGGL(k_deproject_image, grid_of(n, kDeprojBlock), dim3(kDeprojBlock), 0, (hipStream_t)stream,
                       c->num_envs, width, height, T, depth, points, valid, pixels_2d);
    return check_launch(c);
}

int ps_deproject_pixels(ps_ctx *c, const float *depth, const int32_t *pixels, int n, const double tran_pix_world[16],
                        int width, int height, double *points, void *stream) {
    if (!c || !depth || !pixels || !points || !tran_pix_world || n < 0 || width <= 0 || height <= 0)
        return fail(c, PS_ERR_ARG, "null argument");
    if (n == 0) return PS_OK;
    Tran T;
    memcpy(T.m, tran_pix_world, sizeof T.m);
    int64_t tot = c->num_envs * (int64_t)n;
    hipLaunchKernelGGL(k_deproject_pixels, grid_of(tot, 256), dim3(256), 0, (hipStream_t)stream, c->num_envs, n,
                       width, height, T, depth, pixels, points);
    return check_launch(c);
}

}  // extern "C"
