// ps_collide.h — contact generation in fp32: the gripper's collision boxes
// against a cube, the cylinder and the ground (the oracle's gen_contacts), the
// two cubes' box-box contacts (Stack), and the wave-wide candidate work lists
// (robot_candidates).
#pragma once

#include "ps_scene.h"

namespace ps {

// ------------------------------------------------- gripper collision boxes
// The oracle's gen_contacts restated in fp32 (oracle/panda_oracle.c
// box_cube_cands / box_cyl_cands / box_ground_cands / pick_contacts, DESIGN.md
// §5): each (box, target) pair offers at most PM_BOX_CONTACTS points, picked
// from a fixed candidate stream -- the deepest within the margin, then the one
// farthest from it -- and ordered along the box's longest axis.  The stream is
// visited twice (once per pick) instead of being stored: its expensive part
// (separating axis, reference and incident faces) is computed once, the
// candidates themselves are a few FMAs each.
struct RCand {
    V3 pA, pB, n;  // robot point, object/ground point, normal from B to A
    float dist;
};
PS_D float comp(V3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }
PS_D V3 colsel(const M3 &R, int c) { return c == 0 ? col(R, 0) : (c == 1 ? col(R, 1) : col(R, 2)); }

template <int MAXN, class Visit>
PS_D int pick_two(Visit &&visit, V3 org, V3 w, RCand &c0, RCand &c1) {
    const float margin = (float)PM_CONTACT_MARGIN_ROBOT;
    const RCand none{mk(0, 0, 0), mk(0, 0, 0), mk(0, 0, 1), 1.0f};
    auto sel = [](bool t, const RCand &a, const RCand &b) {
        return RCand{t ? a.pA : b.pA, t ? a.pB : b.pB, t ? a.n : b.n, t ? a.dist : b.dist};
    };
    // one pass, branch-free, validity folded into the scores (see
    // BoxCube::pick): the first pick minimises depth + PM_PICK_SKEW_WEIGHT x
    // the skew coordinate; the candidates extreme along the skew are tracked
    // for the second
    RCand cmin = none, cmax = none;
    float s0 = 1e30f, vmin = 1e30f, vmax = -1e30f;
    c0 = none;
    c1 = none;  // written for MAXN < 2 too (the caller copies it)
    visit([&](bool ok, const RCand &c) {
        const bool valid = ok && c.dist < margin;
        const float sv = dot(c.pA - org, w);
        const float sc = valid ? fmaf((float)PM_PICK_SKEW_WEIGHT, sv, c.dist) : 1e30f;
        const bool take = sc < s0;
        s0 = take ? sc : s0;
        c0 = sel(take, c, c0);
        if constexpr (MAXN >= 2) {
            const bool tmin = valid && sv < vmin, tmax = valid && sv > vmax;
            vmin = tmin ? sv : vmin;
            vmax = tmax ? sv : vmax;
            cmin = sel(tmin, c, cmin);
            cmax = sel(tmax, c, cmax);
        }
    });
    const bool has0 = s0 < 1e29f;
    bool has1 = false;
    if constexpr (MAXN >= 2) {
        const float sf = dot(c0.pA - org, w);
        c1 = sel(vmax - sf >= sf - vmin, cmax, cmin);
        const V3 d = c1.pA - c0.pA;
        has1 = has0 && dot(d, d) > 1e-8f;  // (0.1 mm)^2: not the same point
        if (has1 && dot(c1.pA - org, w) < sf) {
            const RCand t = c0;
            c0 = c1;
            c1 = t;
        }
    }
    return has0 ? (has1 ? 2 : 1) : 0;
}

// robot box (centre xc, rotation xR, half extents xh) vs a cube (yc, yR, yh)
struct BoxCube {
    bool sep;
    V3 nref, t1, t2, cf;
    float hu, hv;
    bool robot_ref;
    float P[4][3];  // incident face vertices (u, v, depth below the reference face)
    PS_D BoxCube(V3 xc, const M3 &xR, V3 xh, V3 yc, const M3 &yR, V3 yh) {
        const V3 d = yc - xc;
        float best = 1e30f;
        int ref = 0, axn = 0;
        sep = false;
        nref = mk(0, 0, 0);
        // the separating-axis radii from |C| = |xR^T yR| (both rotations
        // orthonormal: a box's own axes project to its half extents), 9 dot
        // products instead of 36
        float C[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) C[i][k] = fabsf(dot(col(xR, i), col(yR, k)));
        const float xhv[3] = {xh.x, xh.y, xh.z}, yhv[3] = {yh.x, yh.y, yh.z};
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                const V3 L = col(b == 0 ? xR : yR, ax);
                const float ra = b == 0 ? xhv[ax] : xh.x * C[0][ax] + xh.y * C[1][ax] + xh.z * C[2][ax];
                const float rb = b == 1 ? yhv[ax] : yh.x * C[ax][0] + yh.y * C[ax][1] + yh.z * C[ax][2];
                const float c = dot(d, L);
                const float pen = ra + rb - fabsf(c);
                sep = sep || pen < -(float)PM_CONTACT_MARGIN_ROBOT;
                if (pen < best - (float)PM_PAIR_AXIS_TOL) {
                    best = pen;
                    ref = b;
                    axn = ax;
                    nref = L * ((b == 0 ? c : -c) >= 0.0f ? 1.0f : -1.0f);
                }
            }
        robot_ref = ref == 0;
        const int a1 = axn == 2 ? 0 : axn + 1, a2 = axn == 0 ? 2 : axn - 1;
        const V3 hr = robot_ref ? xh : yh, hi = robot_ref ? yh : xh;
        const V3 cr = robot_ref ? xc : yc, ci = robot_ref ? yc : xc;
        M3 Rr, Ri;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            Rr.m[k] = robot_ref ? xR.m[k] : yR.m[k];
            Ri.m[k] = robot_ref ? yR.m[k] : xR.m[k];
        }
        t1 = colsel(Rr, a1);
        t2 = colsel(Rr, a2);
        cf = cr + nref * comp(hr, axn);
        hu = comp(hr, a1);
        hv = comp(hr, a2);
        // incident face: the incident box's axis most anti-parallel to nref
        int ai = 0;
        float mostneg = 2.0f, si = 1.0f;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            const float dn = dot(col(Ri, ax), nref);
            if (-fabsf(dn) < mostneg) {
                mostneg = -fabsf(dn);
                ai = ax;
                si = dn > 0.0f ? -1.0f : 1.0f;
            }
        }
        const int b1 = ai == 2 ? 0 : ai + 1, b2 = ai == 0 ? 2 : ai - 1;
        const V3 ea = colsel(Ri, ai) * (si * comp(hi, ai)), eb = colsel(Ri, b1) * comp(hi, b1),
                 ec = colsel(Ri, b2) * comp(hi, b2);
        const V3 base = ci - cf;
        constexpr float cu[4] = {-1, 1, 1, -1}, cv[4] = {-1, -1, 1, 1};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const V3 rel = base + ea + eb * cu[q] + ec * cv[q];
            P[q][0] = dot(rel, t1);
            P[q][1] = dot(rel, t2);
            P[q][2] = dot(rel, nref);
        }
    }
    // the candidates in the reference face's frame: (ok, u, v, depth), from
    // the incident face P and the rectangle half extents hu, hv
    template <class F>
    PS_D static void visit(const float (&P)[4][3], float hu, float hv, F &&emit) {
        constexpr float cu[4] = {-1, 1, 1, -1}, cv[4] = {-1, -1, 1, 1};
        // 1. incident vertices inside the reference rectangle
#pragma unroll
        for (int q = 0; q < 4; q++) emit(fabsf(P[q][0]) <= hu && fabsf(P[q][1]) <= hv, P[q][0], P[q][1], P[q][2]);
        // 2. reference corners inside the incident quadrilateral, depth on its plane
        const float e1u = P[1][0] - P[0][0], e1v = P[1][1] - P[0][1], e1d = P[1][2] - P[0][2];
        const float e3u = P[3][0] - P[0][0], e3v = P[3][1] - P[0][1], e3d = P[3][2] - P[0][2];
        const float pnu = e1v * e3d - e1d * e3v, pnv = e1d * e3u - e1u * e3d, pnd = e1u * e3v - e1v * e3u;
        const bool okp = pnd != 0.0f;
        const float ipnd = okp ? __builtin_amdgcn_rcpf(pnd) : 0.0f;  // v_rcp_f32 (1 ulp): not an IEEE division
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float u = cu[q] * hu, v = cv[q] * hv;
            bool pos = true, neg = true;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int e2 = (e + 1) & 3;
                const float cr = (P[e2][0] - P[e][0]) * (v - P[e][1]) - (P[e2][1] - P[e][1]) * (u - P[e][0]);
                pos = pos && cr >= 0.0f;
                neg = neg && cr <= 0.0f;
            }
            const float depth = okp ? P[0][2] - (pnu * (u - P[0][0]) + pnv * (v - P[0][1])) * ipnd : 0.0f;
            emit((pos || neg) && okp, u, v, depth);
        }
        // 3. incident edges crossing the rectangle's edges (u = +-hu, v = +-hv)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int e2 = (e + 1) & 3;
            const float du = P[e2][0] - P[e][0], dv = P[e2][1] - P[e][1], dd = P[e2][2] - P[e][2];
            const float idu = du != 0.0f ? __builtin_amdgcn_rcpf(du) : 0.0f, idv = dv != 0.0f ? __builtin_amdgcn_rcpf(dv) : 0.0f;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const bool on_u = s < 2;
                const float lim = (s & 1) ? -(on_u ? hu : hv) : (on_u ? hu : hv);
                const float ca = on_u ? P[e][0] : P[e][1];
                const bool has = on_u ? du != 0.0f : dv != 0.0f;
                const float t = has ? (lim - ca) * (on_u ? idu : idv) : -1.0f;
                const float u = P[e][0] + t * du, v = P[e][1] + t * dv;
                const bool ok = t > 0.0f && t < 1.0f && (on_u ? fabsf(v) <= hv : fabsf(u) <= hu);
                emit(ok, on_u ? lim : u, on_u ? v : lim, P[e][2] + t * dd);
            }
        }
    }
    PS_D RCand to_world(float u, float v, float depth) const {
        const V3 pref = cf + t1 * u + t2 * v, pinc = pref + nref * depth;
        return RCand{robot_ref ? pref : pinc, robot_ref ? pinc : pref, robot_ref ? -nref : nref, depth};
    }
    // pick_two over the candidates, in the reference face's frame: the robot
    // point's offsets are (du, dv) when the box is the reference, (du, dv,
    // ddepth) when it is the incident one; only the two picks go to world
    PS_D int pick(V3 org, V3 w, RCand &c0, RCand &c1) const {
        const float margin = (float)PM_CONTACT_MARGIN_ROBOT;
        const float wd = robot_ref ? 0.0f : 1.0f;
        // the robot point's skew coordinate, affine in (u, v, depth)
        const float k0 = dot(cf - org, w), k1 = dot(t1, w), k2 = dot(t2, w), k3 = wd * dot(nref, w);
        const float lam = (float)PM_PICK_SKEW_WEIGHT;
        // One pass, branch-free selects, validity folded into the scores: as
        // lane masks, the 24 candidates' validity bits stayed live in SGPRs
        // and spilled ~900 of them to VGPR lanes per substep.
        float s0 = 1e30f, vmin = 1e30f, vmax = -1e30f;
        float u0 = 0.0f, v0 = 0.0f, d0 = 1.0f, un = 0.0f, vn = 0.0f, dn = 1.0f, ux = 0.0f, vx = 0.0f, dx = 1.0f;
        visit(P, hu, hv, [&](bool ok, float u, float v, float d) {
            const bool valid = ok && d < margin;
            const float sv = fmaf(k3, d, fmaf(k2, v, fmaf(k1, u, k0)));
            const float sc = valid ? fmaf(lam, sv, d) : 1e30f;
            const bool take = sc < s0, tmin = valid && sv < vmin, tmax = valid && sv > vmax;
            s0 = take ? sc : s0;
            u0 = take ? u : u0;
            v0 = take ? v : v0;
            d0 = take ? d : d0;
            vmin = tmin ? sv : vmin;
            un = tmin ? u : un;
            vn = tmin ? v : vn;
            dn = tmin ? d : dn;
            vmax = tmax ? sv : vmax;
            ux = tmax ? u : ux;
            vx = tmax ? v : vx;
            dx = tmax ? d : dx;
        });
        const bool has0 = s0 < 1e29f && !sep;
        const float sf = fmaf(k3, d0, fmaf(k2, v0, fmaf(k1, u0, k0)));
        const bool hi = vmax - sf >= sf - vmin;
        const float u1 = hi ? ux : un, v1 = hi ? vx : vn, d1 = hi ? dx : dn;
        c0 = to_world(u0, v0, d0);
        c1 = to_world(u1, v1, d1);
        const V3 dd = c1.pA - c0.pA;
        const bool has1 = has0 && dot(dd, dd) > 1e-8f;  // (0.1 mm)^2: not the same point
        if (has1 && (hi ? vmax : vmin) < sf) {
            const RCand t = c0;
            c0 = c1;
            c1 = t;
        }
        return has0 ? (has1 ? 2 : 1) : 0;
    }
};

// robot box vs the cylinder (Slide), in the cylinder's frame
struct BoxCyl {
    V3 bc, yc;
    M3 bR, yR;
    V3 xh;
    float r, hh;
    PS_D BoxCyl(const Scene &sc, V3 xc, const M3 &xR, V3 xh_, V3 yc_, const M3 &yR_) : yc(yc_), yR(yR_), xh(xh_) {
        r = sc.half.x;
        hh = sc.half.z;
        bc = tmul(yR, xc - yc);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const V3 lc = tmul(yR, col(xR, a));
            bR.m[a] = lc.x;
            bR.m[3 + a] = lc.y;
            bR.m[6 + a] = lc.z;
        }
    }
    // the candidate stream in the cylinder's frame: emit(ok, robot point,
    // cylinder point, normal, distance)
    template <class F>
    PS_D void visit(const Scene &sc, F &&emit) const {
        // 1. box vertices vs the solid (the loops stay rolled: unrolled, the
        // two visits of the 36 candidates spilled ~300 VGPRs in Slide's kernels)
#pragma unroll 1
        for (int v = 0; v < 8; v++) {
            const V3 lA = bc + mul(bR, mk((v & 1) ? xh.x : -xh.x, (v & 2) ? xh.y : -xh.y, (v & 4) ? xh.z : -xh.z));
            V3 cl, nl;
            const float dist = object_closest<SHAPE_CYL>(sc, lA, cl, nl);
            emit(true, lA, cl, nl, dist);
        }
        // 2. side faces of the box vs the generator line facing them (unrolled:
        // with a loop counter the face's axis selects -- colsel(bR, ax),
        // comp(xh, a1) -- became dynamic indices into the BoxCyl object, which
        // then lived in 120 B of scratch in every Slide kernel, round 4)
#pragma unroll
        for (int fc = 0; fc < 6; fc++) {
            const int ax = fc >> 1;
            const float sg = (fc & 1) ? -1.0f : 1.0f;
            const V3 nf = colsel(bR, ax) * sg;
            const int a1 = ax == 2 ? 0 : ax + 1, a2 = ax == 0 ? 2 : ax - 1;
            const V3 t1 = colsel(bR, a1), t2 = colsel(bR, a2);
            const float h1 = comp(xh, a1), h2 = comp(xh, a2);
            const V3 fcen = bc + nf * comp(xh, ax);
            const bool side = fabsf(nf.z) < 0.5f;
            const float nxy = fast_sqrt(nf.x * nf.x + nf.y * nf.y);
            const float inv = side ? r * fast_rcp(nxy) : 0.0f;
            const V3 s0 = mk(-nf.x * inv, -nf.y * inv, 0.0f), d0 = s0 - fcen;
            float lo = -hh, hi = hh;
            bool empty = false;
            const float K[5][3] = {{dot(d0, t1), t1.z, h1},
                                   {-dot(d0, t1), -t1.z, h1},
                                   {dot(d0, t2), t2.z, h2},
                                   {-dot(d0, t2), -t2.z, h2},
                                   {dot(nf, fcen), -nf.z, 0.0f}};
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const float k0 = K[k][0], k1 = K[k][1], lim = K[k][2];
                // (branch-free: z is read only where |k1| > 1e-12)
                const float z = (lim - k0) * fast_rcp(k1);
                hi = k1 > 1e-12f ? fminf(z, hi) : hi;
                lo = k1 < -1e-12f ? fmaxf(z, lo) : lo;
                empty = empty || (fabsf(k1) <= 1e-12f && k0 > lim);
            }
            const bool ok = side && !empty && lo <= hi;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const V3 lB = mk(s0.x, s0.y, e ? hi : lo);
                const float dist = dot(nf, lB - fcen);
                emit(ok, lB - nf * dist, lB, -nf, dist);
            }
        }
        // 3. rim points vs the box (support_point<SHAPE_CYL, V>'s order and
        // values) -- only for a box with a half extent beyond the radius (the
        // palm): a narrower box's face inside a cap is found by its vertices
        constexpr int order[PM_CYL_RIM_POINTS] = PM_CYL_RIM_ORDER;
        constexpr float c45 = 0.70710678118654752f;
        // A cap's rim points are skipped by the wave when no lane's box
        // reaches within the margin (+0.1 mm) of the cap's plane: such points
        // are farther than the margin from the box, invalid candidates that
        // cannot change the picks.  The bottom cap lies on the table, out of
        // the palm's reach, so its 8 points drop out in practically every
        // wave.  (The range is the wave's, so the loop counter stays scalar.)
        const bool wide = xh.x > r || xh.y > r || xh.z > r;
        const float reach = fabsf(bR.m[6]) * xh.x + fabsf(bR.m[7]) * xh.y + fabsf(bR.m[8]) * xh.z +
                            (float)PM_CONTACT_MARGIN_ROBOT + 1e-4f;
        const bool cap_lo = wide && fabsf(bc.z + hh) <= reach, cap_hi = wide && fabsf(bc.z - hh) <= reach;
        const bool any_lo = __builtin_amdgcn_ballot_w64(cap_lo) != 0, any_hi = __builtin_amdgcn_ballot_w64(cap_hi) != 0;
        const int vbeg = any_lo ? 0 : PM_CYL_RIM_POINTS, vend = any_hi ? 2 * PM_CYL_RIM_POINTS : PM_CYL_RIM_POINTS;
        static_assert(2 * PM_CYL_RIM_POINTS == num_support<SHAPE_CYL>(), "rim points: bottom cap, then top");
#pragma unroll 1
        for (int V = vbeg; V < vend; V++) {
            int j = 0;
#pragma unroll
            for (int k = 0; k < PM_CYL_RIM_POINTS; k++) j = (V % PM_CYL_RIM_POINTS) == k ? order[k] : j;
            const float cs = j == 0 ? 1.0f : j == 1 || j == 7 ? c45 : j == 2 || j == 6 ? 0.0f : j == 4 ? -1.0f : -c45;
            const float sn = j == 2 ? 1.0f : j == 1 || j == 3 ? c45 : j == 0 || j == 4 ? 0.0f : j == 6 ? -1.0f : -c45;
            const V3 p = mk(sc.half.x * cs, sc.half.x * sn, V >= PM_CYL_RIM_POINTS ? sc.half.z : -sc.half.z);
            const V3 lp = tmul(bR, p - bc);
            V3 cl = mk(fminf(fmaxf(lp.x, -xh.x), xh.x), fminf(fmaxf(lp.y, -xh.y), xh.y), fminf(fmaxf(lp.z, -xh.z), xh.z));
            const V3 dif = lp - cl;
            const float dn = fast_norm(dif);
            V3 nb;
            float dist;
            if (dn > 1e-9f) {
                nb = dif * fast_rcp(dn);
                dist = dn;
            } else {
                const float bx = xh.x - fabsf(lp.x), by = xh.y - fabsf(lp.y), bz = xh.z - fabsf(lp.z);
                int ax = 0;
                float bst = bx;
                if (by < bst) { bst = by; ax = 1; }
                if (bz < bst) { bst = bz; ax = 2; }
                const float s = comp(lp, ax) >= 0.0f ? 1.0f : -1.0f;
                nb = ax == 0 ? mk(s, 0, 0) : (ax == 1 ? mk(0, s, 0) : mk(0, 0, s));
                cl = ax == 0 ? mk(s * xh.x, cl.y, cl.z) : (ax == 1 ? mk(cl.x, s * xh.y, cl.z) : mk(cl.x, cl.y, s * xh.z));
                dist = -bst;
            }
            emit(wide, bc + mul(bR, cl), p, -mul(bR, nb), dist);
        }
    }
    PS_D RCand to_world(const RCand &l) const { return RCand{yc + mul(yR, l.pA), yc + mul(yR, l.pB), mul(yR, l.n), l.dist}; }
    // pick_two's selection in the cylinder's frame: the skew coordinate of a
    // robot point lA is dot(yc - org, w) + dot(lA, yR^T w), and only the two
    // picks go to world (per candidate, the world transform was 36 VALU of
    // the ~80 the generic pick_two spends)
    PS_D int pick(const Scene &sc, V3 org, V3 w, RCand &c0, RCand &c1) const {
        const float margin = (float)PM_CONTACT_MARGIN_ROBOT;
        const RCand none{mk(0, 0, 0), mk(0, 0, 0), mk(0, 0, 1), 1.0f};
        auto sel = [](bool t, const RCand &a, const RCand &b) {
            return RCand{t ? a.pA : b.pA, t ? a.pB : b.pB, t ? a.n : b.n, t ? a.dist : b.dist};
        };
        const V3 wl = tmul(yR, w);
        const float k0 = dot(yc - org, w);
        RCand l0 = none, lmin = none, lmax = none;
        float s0 = 1e30f, vmin = 1e30f, vmax = -1e30f;
        visit(sc, [&](bool ok, V3 lA, V3 lB, V3 ln, float dist) {
            const RCand c{lA, lB, ln, dist};
            const bool valid = ok && dist < margin;
            const float sv = k0 + dot(lA, wl);
            const float sc = valid ? fmaf((float)PM_PICK_SKEW_WEIGHT, sv, dist) : 1e30f;
            const bool take = sc < s0, tmin = valid && sv < vmin, tmax = valid && sv > vmax;
            s0 = take ? sc : s0;
            l0 = sel(take, c, l0);
            vmin = tmin ? sv : vmin;
            vmax = tmax ? sv : vmax;
            lmin = sel(tmin, c, lmin);
            lmax = sel(tmax, c, lmax);
        });
        const bool has0 = s0 < 1e29f;
        const float sf = k0 + dot(l0.pA, wl);
        const bool hi = vmax - sf >= sf - vmin;
        const RCand l1 = sel(hi, lmax, lmin);
        c0 = has0 ? to_world(l0) : none;
        c1 = has0 ? to_world(l1) : none;
        const V3 d = c1.pA - c0.pA;
        const bool has1 = has0 && dot(d, d) > 1e-8f;  // (0.1 mm)^2: not the same point
        if (has1 && (hi ? vmax : vmin) < sf) {
            const RCand t = c0;
            c0 = c1;
            c1 = t;
        }
        return has0 ? (has1 ? 2 : 1) : 0;
    }
};

// robot box vs the ground (table top or plane)
template <class F>
PS_D void box_ground_visit(const Scene &sc, V3 xc, const M3 &xR, V3 xh, F &&f) {
    const V3 ea = col(xR, 0) * xh.x, eb = col(xR, 1) * xh.y, ec = col(xR, 2) * xh.z;
#pragma unroll
    for (int v = 0; v < 8; v++) {
        const V3 p = xc + ((v & 1) ? ea : -ea) + ((v & 2) ? eb : -eb) + ((v & 4) ? ec : -ec);
        float top = 0.0f;
        const bool ok = ground_top(sc, p.x, p.y, top);
        f(ok, RCand{p, mk(p.x, p.y, top), mk(0, 0, 1), p.z - top});
    }
}

// Box-box contacts of the two cubes (Stack): the oracle's box_box_contacts
// (face-axis SAT, incident face clipped against the reference face) in fp32.
// Fills up to NP contact candidates: point on A (incident), point on B
// (reference), normal n (B -> A), distance.
struct PairCand {
    V3 pA, pB, n;
    float dist;
    bool a0;
};

// The clipped polygon in registers (round 5): a convex quad cut by four
// half-planes gains at most one vertex per cut, so 8 compile-time slots hold
// it, and a vertex goes to its runtime slot m by selects over the slots m can
// reach at that point.  With arrays indexed by m (the oracle's form) the
// polygons lived in 384 B of scratch per lane in every Stack kernel.
struct Poly8 {
    float u[8], v[8], d[8];
};

// write (u, v, d) to slot m when c; S = the slots m can address
template <int S>
PS_D void poly_put(Poly8 &p, int m, bool c, float u, float v, float d) {
#pragma unroll
    for (int s = 0; s < S; s++) {
        const bool w = c && m == s;
        p.u[s] = w ? u : p.u[s];
        p.v[s] = w ? v : p.v[s];
        p.d[s] = w ? d : p.d[s];
    }
}

// one Sutherland-Hodgman pass (oracle clip_half): keeps sign * coord <= lim,
// coord = u (AXIS 0) or v (AXIS 1); the input has n <= NI vertices.  Vertex i
// emits itself and/or the edge crossing, so before its writes m <= 2i and
// 2i + 1; a count past the NI + 1 slots (rounding at a degenerate edge) drops
// the extra vertices.
template <int NI, int AXIS>
PS_D int clip_half(const Poly8 &in, int n, float sign, float lim, Poly8 &out) {
    constexpr int NO = NI + 1 < 8 ? NI + 1 : 8;
    int m = 0;
    static_for<0, NI>([&](auto I) {
        constexpr int i = decltype(I)::value;
        constexpr int nx = i + 1 < NI ? i + 1 : 0;
        const bool act = i < n, wrap = i + 1 >= n;
        const float au = in.u[i], av = in.v[i], ad = in.d[i];
        const float bu = wrap ? in.u[0] : in.u[nx], bv = wrap ? in.v[0] : in.v[nx], bd = wrap ? in.d[0] : in.d[nx];
        const float ca = sign * (AXIS == 0 ? au : av) - lim, cb = sign * (AXIS == 0 ? bu : bv) - lim;
        const bool keep = act && ca <= 0.0f;
        poly_put<(2 * i + 1 < NO ? 2 * i + 1 : NO)>(out, m, keep, au, av, ad);
        m += keep ? 1 : 0;
        const bool cross = act && ((ca < 0.0f && cb > 0.0f) || (ca > 0.0f && cb < 0.0f));
        const float t = ca / (ca - cb);  // read only where the edge crosses
        poly_put<(2 * i + 2 < NO ? 2 * i + 2 : NO)>(out, m, cross, au + t * (bu - au), av + t * (bv - av),
                                                     ad + t * (bd - ad));
        m += cross ? 1 : 0;
    });
    return m < NO ? m : NO;
}

PS_D int box_box(const Scene &sc, const Body &b0, const Body &b1, const M3 &R0, const M3 &R1, PairCand out[NP]) {
    const V3 hv = sc.half;
    const float h[3] = {hv.x, hv.y, hv.z};  // constant indices only
    V3 d = b1.pos - b0.pos;
    float best = 1e30f;
    V3 nref = mk(0, 0, 0);
    int ref = 0, axn = 0;
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            V3 L = col(b == 0 ? R0 : R1, ax);
            float ra = 0.0f, rb = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                ra += h[k] * fabsf(dot(col(R0, k), L));
                rb += h[k] * fabsf(dot(col(R1, k), L));
            }
            float c = dot(d, L);
            float pen = ra + rb - fabsf(c);
            if (pen < -(float)PM_CONTACT_MARGIN_PAIR) return 0;
            if (pen < best - (float)PM_PAIR_AXIS_TOL) {
                best = pen;
                ref = b;
                axn = ax;
                float sg = (b == 0 ? c : -c) >= 0.0f ? 1.0f : -1.0f;
                nref = L * sg;
            }
        }
    // reference / incident bodies, selected per element (a select of the
    // matrices' addresses put them in memory)
    M3 Rr, Ri;
#pragma unroll
    for (int q = 0; q < 9; q++) {
        Rr.m[q] = ref == 0 ? R0.m[q] : R1.m[q];
        Ri.m[q] = ref == 0 ? R1.m[q] : R0.m[q];
    }
    V3 cr = ref == 0 ? b0.pos : b1.pos, ci = ref == 0 ? b1.pos : b0.pos;
    int a1 = axn + 1 == 3 ? 0 : axn + 1, a2 = axn + 2 >= 3 ? axn - 1 : axn + 2;
    V3 t1 = colsel(Rr, a1), t2 = colsel(Rr, a2);
    V3 cf = cr + nref * comp(hv, axn);
    int ai = 0;
    float mostneg = 2.0f, si = 1.0f;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        float dn = dot(col(Ri, ax), nref);
        if (-fabsf(dn) < mostneg) { mostneg = -fabsf(dn); ai = ax; si = dn > 0.0f ? -1.0f : 1.0f; }
    }
    int b1i = ai + 1 == 3 ? 0 : ai + 1;
    Poly8 P{}, T{};
    const float cu[4] = {-1, 1, 1, -1}, cv[4] = {-1, -1, 1, 1};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        // the incident face's corner k: axis ai at si h, b1i at cu h, b2i at cv h
        float loc[3];
#pragma unroll
        for (int c = 0; c < 3; c++) loc[c] = (c == ai ? si : c == b1i ? cu[k] : cv[k]) * h[c];
        V3 rel = mul(Ri, mk(loc[0], loc[1], loc[2])) + ci - cf;
        P.u[k] = dot(rel, t1);
        P.v[k] = dot(rel, t2);
        P.d[k] = dot(rel, nref);
    }
    int n = clip_half<4, 0>(P, 4, 1.0f, comp(hv, a1), T);
    n = clip_half<5, 0>(T, n, -1.0f, comp(hv, a1), P);
    n = clip_half<6, 1>(P, n, 1.0f, comp(hv, a2), T);
    n = clip_half<7, 1>(T, n, -1.0f, comp(hv, a2), P);
    // the vertices within the margin, in order
    Poly8 K{};
    int m = 0;
    static_for<0, 8>([&](auto I) {
        constexpr int k = decltype(I)::value;
        const bool keep = k < n && P.d[k] < (float)PM_CONTACT_MARGIN_PAIR;
        poly_put<k + 1>(K, m, keep, P.u[k], P.v[k], P.d[k]);
        m += keep ? 1 : 0;
    });
    int take = m < NP ? m : NP;
#pragma unroll
    for (int k = 0; k < NP; k++) {
        int idx = m <= NP ? k : (k * m) / NP;
        float u = K.u[0], v = K.v[0], dd = K.d[0];
#pragma unroll
        for (int s = 1; s < 8; s++) {
            u = idx == s ? K.u[s] : u;
            v = idx == s ? K.v[s] : v;
            dd = idx == s ? K.d[s] : dd;
        }
        PairCand c;
        c.pB = cf + t1 * u + t2 * v;
        c.pA = c.pB + nref * dd;
        c.n = nref;
        c.dist = dd;
        c.a0 = ref == 1;  // A = incident
        out[k] = c;
    }
    return take;
}

// Gripper contact candidates (oracle gen_contacts 3-4): per object, then the
// ground, the gripper boxes (PM_BOX_CONTACTS points each) and then the wrist
// sphere; the first NR fill the slots.  Cache ids 1 + (proxy * 3 + target) * 2
// + point.  Each slot's record (RobotCand, 14 floats) goes to LDS at the end of
// the M^-1 J^T area, which the row setup overwrites only after it has read the
// slot (slot s's rows are written to floats [27 s, 27 s + 27), its record sits
// at [52 + 14 s, 66 + 14 s)).  Returns the number of slots used.
struct RobotCand {
    V3 pA, pB, n;
    float dist, mu;
    int link;
    int obj;  // -1: ground
    int id;   // cache id: 1 + (proxy * 3 + target) * 2 + point (target 2: the ground)
    static constexpr int FLOATS = 14, OFFSET = NR * 27 - NR * 14;
    PS_D void store(const MJStore &L, int s) const {
        const float v[FLOATS] = {pA.x, pA.y, pA.z, pB.x, pB.y, pB.z, n.x, n.y, n.z, dist, mu,
                                 (float)link, (float)obj, (float)id};
#pragma unroll
        for (int k = 0; k < FLOATS; k++) L.base[(OFFSET + s * FLOATS + k) * L.stride] = v[k];
    }
    PS_D static RobotCand load(const MJStore &L, int s) {
        float v[FLOATS];
#pragma unroll
        for (int k = 0; k < FLOATS; k++) v[k] = L.base[(OFFSET + s * FLOATS + k) * L.stride];
        return RobotCand{mk(v[0], v[1], v[2]), mk(v[3], v[4], v[5]), mk(v[6], v[7], v[8]), v[9], v[10],
                         (int)v[11], (int)v[12], (int)v[13]};
    }
};
static_assert(RobotCand::OFFSET + NR * RobotCand::FLOATS <= NR * 27, "candidate records inside the M^-1 J^T area");

// position of the j-th (from 0) set bit of m (j < popcount(m)), branch-free
PS_D int nth_set_bit(uint64_t m, int j) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const uint64_t low = m & ((1ull << w) - 1ull);
        const int c = __builtin_popcountll(low);
        const bool up = j >= c;
        j = up ? j - c : j;
        pos += up ? w : 0;
        m = up ? (m >> w) : low;
    }
    return pos;
}

// Candidate work lists.  The bounding tests pass for few lanes of a wave (Push,
// 65 536 envs: 2.2 lanes of 64 per box-object test that passes anywhere, 14 per
// box-ground one; profiles/r04f_phase_push.log), and run per lane the pair's
// candidate block cost the whole wave a block per box.  Instead the (env, box)
// pairs that pass are numbered box-major across the wave (ballot + popcount),
// the owners park their geometry in their own LDS column, and active lane k
// evaluates pair k of the round -- one block per round for the wave, not one per
// box -- and leaves its picks in its column, which the owners read back in box
// order (the slot order of the per-lane version: the same values, bit for bit).
// Scratch: floats [0, 51) of each column, below the RobotCand records.
constexpr int CW_IN = 0;    // owner: hR (9), box centres (3 x 3), object position (3), rotation (9)
constexpr int CW_OUT = 30;  // worker: pick 0 (pA, pB, n, dist), pick 1, count
constexpr int CW_OUT_FLOATS = 21;
// the work lists' per-lane output rows are one wave wide: row q of worker lane
// c at cwo0[q * CW_LANES + c] (the step kernels' kBlock, asserted equal in
// ps_env.h: a workgroup of another width would overwrite other waves' rows)
constexpr int CW_LANES = 64;
static_assert(CW_OUT + CW_OUT_FLOATS <= RobotCand::OFFSET, "work-list scratch below the candidate records");

// The group kernels (G > 1) keep one LDS column per env, shared by the
// group's lanes: every lane of a group computes the same values, so the
// M^-1 J^T rows, candidate records, stash and cache are written with the same
// bits by each (round 5; round 3's attempt at this changed the bits, most
// likely through the FMA-contracted group sums of §12.8, since fixed).  The
// work lists' outputs, which differ per lane, keep a per-lane area.  LDS per
// workgroup 40.4 KB -> 7.9 KB (G = 16) / 10.4 KB (G = 8); C3 and C4 0.6 %
// faster.
template <int G>
constexpr bool shared_lds() { return G > 1; }

template <int NOBJ, int SHAPE, int G>
PS_D int robot_candidates(const Scene &sc, const Geo &geo, const Body *bd, const M3 *oR, const MJStore &lds PS_PROF_PARAM) {
    int nr = 0;
    auto offer = [&](const RobotCand &c) {
        c.store(lds, nr);
        nr++;
    };
    constexpr SphereDef ws = wrist_def();
    constexpr int NBX = PM_NUM_BOXES;
    const uint32_t lane = __lane_id();
    const uint64_t act = __ballot(true);  // G == 1: lanes past the batch end have returned
    const int nact = __builtin_popcountll(act);
    const int rank = __builtin_popcountll(act & ((1ull << lane) - 1ull));
    // G > 1: every lane of a group holds the same env; its first lane owns the pairs
    const uint32_t leader = lane & ~(uint32_t)(G - 1);
    const uint64_t below = (1ull << leader) - 1ull;
    constexpr bool SHARED = shared_lds<G>();
    // column 0 of the wave's LDS block; lane c's column (its env's when shared)
    lds_float *const col0 = lds.base - (SHARED ? lane / G : lane);
    auto at = [&](int k, int c) -> lds_float & { return col0[k * lds.stride + (SHARED ? c / G : c)]; };
    // worker lane c's output row q (stride CW_LANES = kBlock)
    lds_float *const cwo0 = lds.cwo - lane;
    auto wout = [&](int q, int c) -> lds_float & { return cwo0[q * CW_LANES + c]; };
    static_for<0, NOBJ + 1>([&](auto TT) {
        constexpr int TGT = decltype(TT)::value == NOBJ ? 2 : decltype(TT)::value;
        constexpr bool GROUND = TGT == 2;
        // a conservative bounding test per box first (no candidate of a pair
        // that fails it is within the margin, so the picks are unchanged)
        bool nearb[NBX];
        uint64_t m[NBX];
        int pre[NBX + 1];
        pre[0] = 0;
        static_for<0, NBX>([&](auto BB) {
            constexpr int B = decltype(BB)::value;
            constexpr BoxDef bx = box_def(B);
            const V3 xh = mk((float)bx.h[0], (float)bx.h[1], (float)bx.h[2]);
            const V3 xc = geo.bc[B];
            if constexpr (GROUND) {
                const V3 ea = col(geo.hR, 0) * xh.x, eb = col(geo.hR, 1) * xh.y, ec = col(geo.hR, 2) * xh.z;
                const float low = xc.z - (fabsf(ea.z) + fabsf(eb.z) + fabsf(ec.z));
                nearb[B] = low < (float)PM_TABLE_TOP + (float)PM_CONTACT_MARGIN_ROBOT;  // the highest ground
            } else {
                // the object's centre against the box: its distance to the box
                // beyond the object's bounding radius (+ margin) means no
                // candidate can be within the margin (a sphere around the
                // object: |half| bounds a box and, with half = (r, r, h), a
                // cylinder)
                const V3 l = tmul(geo.hR, bd[TGT].pos - xc);
                const V3 ex = mk(fmaxf(fabsf(l.x) - xh.x, 0.0f), fmaxf(fabsf(l.y) - xh.y, 0.0f), fmaxf(fabsf(l.z) - xh.z, 0.0f));
                const float robj = sqrtf(dot(sc.half, sc.half)) + (float)PM_CONTACT_MARGIN_ROBOT;
                nearb[B] = dot(ex, ex) < robj * robj;
            }
            m[B] = __ballot(nearb[B] && lane == leader);
            pre[B + 1] = pre[B] + __builtin_popcountll(m[B]);
#ifdef PS_PROFILE_PHASES
            pt.acc[GROUND ? 22 : 20] += __builtin_popcountll(m[B]);
            pt.acc[GROUND ? 23 : 21] += m[B] != 0;
#endif
        });
        const int total = pre[NBX];
        if (total > 0) {
            // the owner's geometry, in its own column
#pragma unroll
            for (int k = 0; k < 9; k++) lds.base[(CW_IN + k) * lds.stride] = geo.hR.m[k];
#pragma unroll
            for (int b = 0; b < NBX; b++) {
                lds.base[(CW_IN + 9 + 3 * b) * lds.stride] = geo.bc[b].x;
                lds.base[(CW_IN + 10 + 3 * b) * lds.stride] = geo.bc[b].y;
                lds.base[(CW_IN + 11 + 3 * b) * lds.stride] = geo.bc[b].z;
            }
            if constexpr (!GROUND) {
                lds.base[(CW_IN + 18) * lds.stride] = bd[TGT].pos.x;
                lds.base[(CW_IN + 19) * lds.stride] = bd[TGT].pos.y;
                lds.base[(CW_IN + 20) * lds.stride] = bd[TGT].pos.z;
#pragma unroll
                for (int k = 0; k < 9; k++) lds.base[(CW_IN + 21 + k) * lds.stride] = oR[TGT].m[k];
            }
            for (int r = 0; r < total; r += nact) {
                __syncthreads();
                const int k = r + rank;
                if (k < total) {
                    int B = 0;
#pragma unroll
                    for (int b = 1; b < NBX; b++) B = k >= pre[b] ? b : B;
                    uint64_t mb = m[0];
                    int pb = 0;
#pragma unroll
                    for (int b = 1; b < NBX; b++) {
                        mb = B == b ? m[b] : mb;
                        pb = B == b ? pre[b] : pb;
                    }
                    const int own = nth_set_bit(mb, k - pb);
                    M3 hR;
#pragma unroll
                    for (int q = 0; q < 9; q++) hR.m[q] = at(CW_IN + q, own);
                    // (selected per component: selects of whole vectors went
                    // through a stack array)
                    const int cb = CW_IN + 9 + 3 * B;
                    const V3 xc = mk(at(cb, own), at(cb + 1, own), at(cb + 2, own));
                    float hx = (float)box_def(0).h[0], hy = (float)box_def(0).h[1], hz = (float)box_def(0).h[2];
#pragma unroll
                    for (int b = 1; b < NBX; b++) {
                        hx = B == b ? (float)box_def(b).h[0] : hx;
                        hy = B == b ? (float)box_def(b).h[1] : hy;
                        hz = B == b ? (float)box_def(b).h[2] : hz;
                    }
                    const V3 xh = mk(hx, hy, hz);
                    // the pick's skew direction (PM_PICK_SKEW, box frame), world
                    const V3 w = mul(hR, mk((float)PM_PICK_SKEW_X, (float)PM_PICK_SKEW_Y, (float)PM_PICK_SKEW_Z));
                    RCand c0, c1;
                    int ns;
                    if constexpr (GROUND) {
                        ns = pick_two<PM_BOX_GROUND_CONTACTS>([&](auto &&f) { box_ground_visit(sc, xc, hR, xh, f); }, xc, w,
                                                              c0, c1);
                    } else {
                        const V3 yc = mk(at(CW_IN + 18, own), at(CW_IN + 19, own), at(CW_IN + 20, own));
                        M3 yR;
#pragma unroll
                        for (int q = 0; q < 9; q++) yR.m[q] = at(CW_IN + 21 + q, own);
                        if constexpr (SHAPE == SHAPE_CYL) {
                            const BoxCyl bcy(sc, xc, hR, xh, yc, yR);
                            ns = bcy.pick(sc, xc, w, c0, c1);
                        } else {
                            const BoxCube bcu(xc, hR, xh, yc, yR, sc.half);
                            ns = bcu.pick(xc, w, c0, c1);
                        }
                    }
                    const float out[21] = {c0.pA.x, c0.pA.y, c0.pA.z, c0.pB.x, c0.pB.y, c0.pB.z, c0.n.x, c0.n.y, c0.n.z,
                                           c0.dist, c1.pA.x, c1.pA.y, c1.pA.z, c1.pB.x, c1.pB.y, c1.pB.z, c1.n.x, c1.n.y,
                                           c1.n.z, c1.dist, (float)ns};
                    const int nout = GROUND && PM_BOX_GROUND_CONTACTS < 2 ? 10 : 20;
#pragma unroll
                    for (int q = 0; q < 20; q++)
                        if (q < nout) lds.cwo[q * CW_LANES] = out[q];
                    lds.cwo[20 * CW_LANES] = out[20];
                }
                __syncthreads();
                // the owners take their pairs of this round, in box order
                static_for<0, NBX>([&](auto BB) {
                    constexpr int B = decltype(BB)::value;
                    constexpr BoxDef bx = box_def(B);
                    const int idx = pre[B] + __builtin_popcountll(m[B] & below) - r;
                    if (nearb[B] && idx >= 0 && idx < nact) {
                        const int wl = nth_set_bit(act, idx);
                        const int ns = (int)wout(20, wl);
                        const float mu = (float)bx.mu * (GROUND ? (float)PM_DEFAULT_FRICTION : sc.fric);
                        const int obj = GROUND ? -1 : TGT;
#pragma unroll
                        for (int c = 0; c < 2; c++) {
                            if (nr < NR && ns > c) {
                                const int o = 10 * c;
                                offer(RobotCand{mk(wout(o, wl), wout(o + 1, wl), wout(o + 2, wl)),
                                                mk(wout(o + 3, wl), wout(o + 4, wl), wout(o + 5, wl)),
                                                mk(wout(o + 6, wl), wout(o + 7, wl), wout(o + 8, wl)), wout(o + 9, wl), mu,
                                                bx.link, obj, 1 + c + (B * 3 + TGT) * 2});
                            }
                        }
                    }
                });
            }
        }
        constexpr int WID = 1 + (PM_NUM_BOXES * 3 + TGT) * 2;
        if constexpr (GROUND) {
            float top;
            if (nr < NR && ground_top(sc, geo.wc.x, geo.wc.y, top)) {
                const float dist = geo.wc.z - (float)ws.r - top;
                if (dist < (float)PM_CONTACT_MARGIN_SPHERE) {
                    const V3 pA = geo.wc - mk(0, 0, (float)ws.r);
                    offer(RobotCand{pA, mk(pA.x, pA.y, top), mk(0, 0, 1), dist, (float)(ws.mu * PM_DEFAULT_FRICTION),
                                    ws.link, -1, WID});
                }
            }
        } else {
            const V3 loc = tmul(oR[TGT], geo.wc - bd[TGT].pos);
            V3 cl, nl;
            const float dist = object_closest<SHAPE>(sc, loc, cl, nl) - (float)ws.r;
            if (nr < NR && dist < (float)PM_CONTACT_MARGIN_SPHERE) {
                const V3 n = mul(oR[TGT], nl);
                offer(RobotCand{geo.wc - n * (float)ws.r, bd[TGT].pos + mul(oR[TGT], cl), n, dist,
                                (float)ws.mu * sc.fric, ws.link, TGT, WID});
            }
        }
    });
    return nr;
}

}  // namespace ps
