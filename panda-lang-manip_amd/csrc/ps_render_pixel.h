// ps_render_pixel.h — the per-pixel work of the camera image, shared by the
// kernels that need one pixel's depth, colour or world point: the ray caster
// and the deprojection (render_kernels.hip) and the fused point-cloud
// observation (cloud_kernels.hip).  The camera of a view/projection pair
// (Cam, cam_of), the scene a ray is cast into (RenderArgs, render_args_of),
// the arm primitives' row culling (arm_prim_meets_tile), one pixel's ray cast
// (render_pixel), its 8-bit colour (colour_u8), render()'s deprojection of
// one depth sample (Tran, pix_to_world, deproject_pixel) and deproject()'s of
// one pixel of a list (deproject_at).
//
// Every kernel inlines the same bodies; the point-cloud tests hold the fused
// kernels to ps_render + ps_deproject_image of the same build bit for bit, so
// a change here changes all of them together.
#pragma once

#include "ps_ctx.h"
#include "ps_render.h"
#include "ps_task_rng.h"

namespace {

// ------------------------------------------------------------- rendering
// Camera of a view/projection pair (column-major float[16], as getCameraImage
// takes them): eye, the view axes (s, u, -f rows of the rotation) and the
// projection terms a pixel ray and the depth buffer need.
struct Cam {
    V3 eye, s, u, f;
    float p00, p11, p22, p23, nearv, farv;
    float light[3];
};

inline Cam cam_of(const float view[16], const float proj[16]) {
    Cam c;
    // V = [R | t] (row r, col k = view[k*4 + r]); eye = -R^T t
    c.s = mk(view[0], view[4], view[8]);
    c.u = mk(view[1], view[5], view[9]);
    c.f = mk(-view[2], -view[6], -view[10]);
    V3 t = mk(view[12], view[13], view[14]);
    c.eye = mk(-(c.s.x * t.x + c.u.x * t.y - c.f.x * t.z), -(c.s.y * t.x + c.u.y * t.y - c.f.y * t.z),
               -(c.s.z * t.x + c.u.z * t.y - c.f.z * t.z));
    c.p00 = proj[0];
    c.p11 = proj[5];
    c.p22 = proj[10];
    c.p23 = proj[14];
    // clip planes of the perspective matrix: z_ndc = -1 / +1
    c.nearv = proj[14] / (proj[10] - 1.0f);
    c.farv = proj[14] / (proj[10] + 1.0f);
    // a fixed key light from above and behind the camera
    V3 l = c.u * 0.6f - c.f * 0.3f + mk(0.0f, 0.0f, 0.7f);
    float ln = 1.0f / sqrtf(dot(l, l));
    c.light[0] = l.x * ln;
    c.light[1] = l.y * ln;
    c.light[2] = l.z * ln;
    return c;
}

struct RenderArgs {
    Cam cam;
    int width, height, n_objects, object_shape;
    V3 object_half, table_c, table_h;
    int has_table, has_plane;
    ps_visual vis;
};

// the scene of a context as the ray caster takes it; the camera is the caller's
inline RenderArgs render_args_of(const ps_ctx *c, int width, int height, const ps_visual *vis) {
    RenderArgs a;
    memset(&a.cam, 0, sizeof a.cam);
    a.width = width;
    a.height = height;
    a.n_objects = c->cfg.n_objects;
    a.object_shape = c->cfg.object_shape;
    a.object_half = mk(c->cfg.object_half[0], c->cfg.object_half[1], c->cfg.object_half[2]);
    // create_table: box of half extents (length, width, height) / 2 at (x_offset, 0, -height / 2)
    a.table_c = mk(c->cfg.table_cx, 0.0f, (float)PM_TABLE_TOP - 0.2f);
    a.table_h = mk(c->cfg.table_hx, c->cfg.table_hy, 0.2f);
    a.has_table = c->cfg.has_table;
    a.has_plane = c->cfg.has_plane;
    a.vis = *vis;
    return a;
}

PS_D M3 m3_at(const float *p) {
    M3 R;
#pragma unroll
    for (int e = 0; e < 9; e++) R.m[e] = p[e];
    return R;
}

// One lane per pixel; a block covers a tile of kRenderBlock consecutive pixels
// (row-major) of one env's image.
constexpr int kRenderBlock = 256;
constexpr int kRenderPix = 1;  // pixels per lane (strided by the block)
constexpr int kRenderTile = kRenderBlock * kRenderPix;

inline int64_t render_tiles(int width, int height) {
    return ((int64_t)width * height + kRenderTile - 1) / kRenderTile;
}

// Row culling of the arm primitives: pixel tile `tile` spans image rows
// [r0, r1]; primitive k (capsules, then spheres) of the LDS table `pr` is
// tested by the tile's rays when its bounding sphere's conservative projected
// row range meets them.
PS_D bool arm_prim_meets_tile(const float *pr, const Cam &cm, int width, int height, int64_t npix, int k,
                              int64_t tile) {
    V3 c;
    float rad;
    if (k < RENDER_CAPSULES) {
        const float *q = pr + RP_CAPS + k * 7;
        V3 pa = mk(q[0], q[1], q[2]), pb = mk(q[3], q[4], q[5]);
        c = (pa + pb) * 0.5f;
        rad = 0.5f * norm(pb - pa) + q[6];
    } else {
        const float *q = pr + RP_SPH + (k - RENDER_CAPSULES) * 4;
        c = mk(q[0], q[1], q[2]);
        rad = q[3];
    }
    rad = rad * 1.001f + 1e-4f;
    int64_t p0 = tile * kRenderTile;
    int64_t p1 = p0 + kRenderTile - 1;
    if (p1 >= npix) p1 = npix - 1;
    const float r0 = (float)(p0 / width), r1 = (float)(p1 / width);
    V3 v = c - cm.eye;
    float ze = dot(v, cm.f), yu = dot(v, cm.u);
    bool hit = true;
    if (ze - rad > cm.nearv) {
        float dmin = ze - rad, dmax = ze + rad;
        float nhi = yu + rad, nlo = yu - rad;
        float yhi = cm.p11 * (nhi >= 0.0f ? nhi / dmin : nhi / dmax);
        float ylo = cm.p11 * (nlo <= 0.0f ? nlo / dmin : nlo / dmax);
        // pixel-centre rows: y = 1 - (2 r + 1) / H
        float rlo = ((1.0f - yhi) * height - 1.0f) * 0.5f - 1.0f;
        float rhi = ((1.0f - ylo) * height - 1.0f) * 0.5f + 1.0f;
        hit = rlo <= r1 && rhi >= r0;
    }
    return hit;
}

// getCameraImage (pybullet.py:186-192) by ray casting, one pixel: pixel (row
// r, col c) is sampled at its centre, as a rasteriser does; dep is OpenGL
// window depth of the projection matrix (1 where nothing is hit), (cr, cg, cb)
// the shaded colour in [0, 1] with the ghost targets blended over it.  pr: the
// env's primitive table (k_render_prep) and rgba: ps_visual.rgba, both in LDS;
// mask: the arm primitives to test (arm_prim_meets_tile of the pixel's tile).
PS_D void render_pixel(const Cam &cm, const RenderArgs &a, const float *pr, const float *rgba, unsigned mask, int r,
                       int c, float &dep, float &cr, float &cg, float &cb) {
    const M3 I3 = M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    float xn = -1.0f + (2.0f * c + 1.0f) / a.width, yn = 1.0f - (2.0f * r + 1.0f) / a.height;
    // eye-space direction (xn / P00, yn / P11, -1): unit length along f, so t = -z_eye
    V3 d = cm.s * (xn / cm.p00) + cm.u * (yn / cm.p11) + cm.f;
    V3 o = cm.eye;
    Hit h{cm.farv, mk(0, 0, 1)};
    int role = VR_BACKGROUND;
    const float tmin = cm.nearv;
    if (a.has_plane && ray_box(o, d, mk(0, 0, (float)PM_PLANE_TOP - 0.01f), I3, mk(3.0f, 3.0f, 0.01f), tmin, h))
        role = VR_PLANE;
    if (a.has_table && ray_box(o, d, a.table_c, I3, a.table_h, tmin, h)) role = VR_TABLE;
    for (int ob = 0; ob < a.n_objects; ob++) {
        const float *q = pr + RP_OBJ + ob * 12;
        V3 c0 = mk(q[0], q[1], q[2]);
        M3 R = m3_at(q + 3);
        bool hit = a.object_shape == PS_SHAPE_CYLINDER
                       ? ray_cylinder(o, d, c0, R, a.object_half.x, a.object_half.z, tmin, h)
                       : ray_box(o, d, c0, R, a.object_half, tmin, h);
        if (hit) role = VR_OBJECT1 + ob;
    }
    if (mask && ray_meets_sphere(o, d, mk(pr[RP_ARM_BOUND], pr[RP_ARM_BOUND + 1], pr[RP_ARM_BOUND + 2]),
                                 pr[RP_ARM_BOUND + 3], h.t)) {
        for (int k = 0; k < RENDER_CAPSULES; k++) {
            if (!(mask & (1u << k))) continue;
            const float *q = pr + RP_CAPS + k * 7;
            if (ray_capsule(o, d, mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), q[6], tmin, h)) role = VR_ROBOT;
        }
        for (int k = 0; k < PM_NUM_SPHERES; k++) {
            if (!(mask & (1u << (RENDER_CAPSULES + k)))) continue;
            const float *q = pr + RP_SPH + k * 4;
            if (ray_sphere(o, d, mk(q[0], q[1], q[2]), q[3], tmin, h)) role = VR_ROBOT;
        }
    }
    dep = 1.0f;
    const float *col = rgba + role * 4;
    cr = col[0], cg = col[1], cb = col[2];
    if (role != VR_BACKGROUND) {
        float ze = -h.t;
        dep = 0.5f * ((cm.p22 * ze + cm.p23) / h.t) + 0.5f;
        float nl = fabsf(h.n.x * cm.light[0] + h.n.y * cm.light[1] + h.n.z * cm.light[2]);
        float sh = 0.35f + 0.65f * nl;
        cr *= sh;
        cg *= sh;
        cb *= sh;
    }
    // ghost targets: alpha-blended over whatever is behind, no depth write
    for (int g = 0; g < 2; g++) {
        int shape = a.vis.target_shape[g];
        if (shape < 0) continue;
        const float *q = pr + RP_TGT + g * 12;
        V3 c0 = mk(q[0], q[1], q[2]);
        M3 R = m3_at(q + 3);
        V3 hh = mk(a.vis.target_half[g][0], a.vis.target_half[g][1], a.vis.target_half[g][2]);
        Hit gh{h.t, mk(0, 0, 1)};
        bool hit = shape == PS_SHAPE_CYLINDER ? ray_cylinder(o, d, c0, R, hh.x, hh.z, tmin, gh)
                   : shape == PS_VISUAL_SPHERE ? ray_sphere(o, d, c0, hh.x, tmin, gh)
                                               : ray_box(o, d, c0, R, hh, tmin, gh);
        if (hit) {
            const float *tc = rgba + (VR_TARGET1 + g) * 4;
            float al = tc[3];
            cr = al * tc[0] + (1.0f - al) * cr;
            cg = al * tc[1] + (1.0f - al) * cg;
            cb = al * tc[2] + (1.0f - al) * cb;
        }
    }
}

// a colour channel in [0, 1] as the image's byte
PS_D uint8_t colour_u8(float v) { return (uint8_t)fminf(fmaxf(v * 255.0f + 0.5f, 0.0f), 255.0f); }

// ----------------------------------------------------------- deprojection
struct Tran {
    double m[16];  // row-major inv(P V)
};

// tran @ (x, y, z, 1) with the accumulation OpenBLAS's dgemm kernel uses for a
// 4-deep product (one fused multiply-add per term, k ascending), then the
// homogeneous divide (pybullet.py:140-143, 225-229)
PS_D void pix_to_world(const Tran &T, double x, double y, double z, double out[3]) {
    double w = fma(T.m[15], 1.0, fma(T.m[14], z, fma(T.m[13], y, T.m[12] * x)));
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double v = fma(T.m[r * 4 + 3], 1.0, fma(T.m[r * 4 + 2], z, fma(T.m[r * 4 + 1], y, T.m[r * 4 + 0] * x)));
        out[r] = v / w;
    }
}

// render()'s post-processing of one depth sample (pybullet.py:203-262): NDC of
// np.mgrid (left/top pixel edges, the reference's convention) in (x, y), the
// world point p, and valid = depth < 0.99 and the workspace box on p.
PS_D bool deproject_pixel(const Tran &T, int width, int height, int r, int c, float depth, double &x, double &y,
                          double p[3]) {
#pragma clang fp contract(off)
    // np.mgrid[-1:1:2/h, -1:1:2/w]: index * step + start; then y *= -1
    x = opaque(__dmul_rn((double)c, 2.0 / width)) + -1.0;
    y = -(opaque(__dmul_rn((double)r, 2.0 / height)) + -1.0);
    double z = (double)depth;
    double zn = opaque(__dmul_rn(2.0, z)) - 1.0;
    pix_to_world(T, x, y, zn, p);
    return z < 0.99 && p[2] > 0.0 && p[2] < 0.67 && p[0] > -0.5 && p[0] < 0.2;
}

// PyBullet.deproject of one pixel (pybullet.py:109-146): column pc, row prow
// inside the image and its window depth -> the world point.  x = px * 1 / w
// (integer numerator, true division), x *= 2, x -= 1; the same for (h - py);
// z = 2 depth - 1.  Pixel centres and no filter, unlike deproject_pixel.
PS_D void deproject_at(const Tran &T, int width, int height, int pc, int prow, float depth, double p[3]) {
#pragma clang fp contract(off)
    double x = opaque(opaque((double)pc / (double)width) * 2.0) - 1.0;
    double y = opaque(opaque((double)(height - prow) / (double)height) * 2.0) - 1.0;
    double z = opaque(2.0 * (double)depth) - 1.0;
    pix_to_world(T, x, y, z, p);
}

}  // namespace

// k_render_prep of every env into ctx->render_prims, allocated on first use
// (render_kernels.hip); every kernel that casts rays runs after it on `st`
int ps_launch_render_prep(ps_ctx *c, const void *state, const float *targets, hipStream_t st);
