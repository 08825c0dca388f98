// ps_solver_group.h — the group solver: projected Gauss-Seidel with 16 or 8
// lanes per env (the small-batch step kernels), sibling of the one-lane
// solver in substep.
#pragma once

#include "ps_solver.h"

namespace ps {

// a row's impulse change into the diagnostic row dump; expands to locals of
// group_pgs (its recorder lambda `rec` and the flag `dump_on`, both defined
// under PS_DEBUG_ROW_DUMP only); undefined at the end of this header
#ifdef PS_DEBUG_ROW_DUMP
#define PS_REC(x) do { if (dump_on) rec(x); } while (0)
#else
#define PS_REC(x) do {} while (0)
#endif

// Projected Gauss-Seidel with G = 16 or 8 lanes per env (the small-batch
// step kernels): every lane of a group ran the same setup, and
// the 15 velocity DoFs (robot 0-8, then the object's omega 9-11 and v 12-14)
// are dealt to the lanes: lane e owns DoFs e + k G for k < 16 / G (G = 16: one
// DoF per lane; G = 8: two) with their slices of every row's J and M^-1 J^T.
// A row is then one product per owned DoF, a group sum (group_sum: the same
// bits in every lane, so every lane computes the same impulse), the clamp,
// and one FMA per owned DoF -- about 11 instructions for a row the one-lane
// solver spends 20-60 on.  Row order, gates, bounds and the stopping rule are
// the one-lane solver's.  Returns the full velocity change in every lane.
template <int G>
PS_D float group_sum(float x) {
    if constexpr (G == 16) return group16_sum(x);
    else return group8_sum(x);
}
template <int G, int K>
PS_D float group_bcast(float x) {
    if constexpr (G == 16) return group16_bcast<K>(x);
    else return group8_bcast<K>(x);
}
template <int NOBJ, int SHAPE, bool STD_MOTORS, int G>
PS_D void group_pgs(const Motors &mt, const float Mi[45], const MJStore &lds, unsigned gate_lim, unsigned lim_up,
                    unsigned lim_on, unsigned gate_gnd, unsigned gate_robot, const float dinvj[9],
                    const float lim_rhs[9], float lim_lam[9], const float mot_rhs[9], float mot_lam[9],
                    GroundContact gc[NG], RobotContact rc[NR], const BodyDyn<SHAPE> &od, float gmu, float dv[9],
                    V3 &dw, V3 &dvl PS_PROF_COUNT_PARAM PS_DUMP_PARAM) {
    static_assert((G == 16 || G == 8) && NOBJ <= 1, "groups of 16 or 8 lanes hold 9 robot + 6 object DoFs");
#ifdef PS_DEBUG_ROW_DUMP
    int dk = 0;
    auto rec = [&](float x) {
        if (dump && dk < PS_DUMP_ROWS) dump[dk] = x;
        dk++;
    };
#pragma unroll
    for (int d = 0; d < 9; d++) { rec(mot_rhs[d]); rec(dinvj[d]); rec(lim_rhs[d]); }
#pragma unroll
    for (int c = 0; c < NG; c++)
#pragma unroll
        for (int j = 0; j < 3; j++) { rec(gc[c].rhs[j]); rec(gc[c].dinv[j]); }
#pragma unroll
    for (int c = 0; c < NR; c++)
#pragma unroll
        for (int j = 0; j < 3; j++) { rec(rc[c].rhs[j]); rec(rc[c].dinv[j]); rec(rc[c].lam[j]); }
    rec(__builtin_bit_cast(float, gate_lim | (gate_gnd << 9) | (gate_robot << 13)));
    // wave-uniform (rec tests each lane's pointer): a per-lane flag put the
    // loop's scalar gates (regate) inside divergent branches, which this
    // compiler refuses ("illegal VGPR to SGPR copy")
    bool dump_on = __builtin_amdgcn_ballot_w64(dump != nullptr) != 0;
#endif
    constexpr int K = 16 / G;  // DoFs per lane
    const int e = (int)(__lane_id() & (unsigned)(G - 1));
    // lane e's slices: rows e + k G of M^-1 (joint rows), object-only rows, robot rows
    float mrow[K][9], midg[9];
#pragma unroll
    for (int d = 0; d < 9; d++) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            float v = 0.0f;
#pragma unroll
            for (int r = 0; r < 9; r++) v = e + k * G == r ? Mi[sidx(r, d)] : v;
            mrow[k][d] = v;
        }
        midg[d] = Mi[sidx(d, d)];
    }
    auto oslice = [&](int k, V3 a, V3 l) {
        const int dof = e + k * G;
        float v = 0.0f;
        v = dof == 9 ? a.x : v;
        v = dof == 10 ? a.y : v;
        v = dof == 11 ? a.z : v;
        v = dof == 12 ? l.x : v;
        v = dof == 13 ? l.y : v;
        v = dof == 14 ? l.z : v;
        return v;
    };
    float gJ[NG][3][K], gM[NG][3][K];
#pragma unroll
    for (int c = 0; c < NG; c++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int k = 0; k < K; k++) {
                gJ[c][j][k] = gM[c][j][k] = 0.0f;
                if constexpr (NOBJ > 0) {
                    V3 dir = j == 0 ? mk(0, 0, 1) : (j == 1 ? mk(0, -1, 0) : mk(1, 0, 0));
                    V3 rn = cross(gc[c].r, dir);
                    gJ[c][j][k] = oslice(k, rn, dir);
                    gM[c][j][k] = oslice(k, od.inv_inertia(rn), dir * od.inv_m);
                }
            }
    float rJ[NR][3][K], rM[NR][3][K];
    {
        const MJStore W = lds.opaque();
#pragma unroll
        for (int c = 0; c < NR; c++)
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const int dof = e + k * G;
                    float v = 0.0f;
#pragma unroll
                    for (int r = 0; r < 9; r++) v = dof == r ? rc[c].J[j][r] : v;
                    float m = (float)W.at(c, j, dof < 9 ? dof : 8);
                    m = dof < 9 ? m : 0.0f;
                    if constexpr (NOBJ > 0) {
                        // the object is body B: -rn, -dir
                        V3 rn = rc[c].rn[j], dir = rc[c].dir[j];
                        v += oslice(k, mk(-rn.x, -rn.y, -rn.z), mk(-dir.x, -dir.y, -dir.z));
                        m += oslice(k, od.inv_inertia(mk(-rn.x, -rn.y, -rn.z)), dir * -od.inv_m);
                    }
                    rJ[c][j][k] = v;
                    rM[c][j][k] = m;
                }
    }
    float dvm[K];  // this lane's velocity changes (DoFs e + k G)
#pragma unroll
    for (int k = 0; k < K; k++) dvm[k] = 0.0f;
    // KL: the first slot a row's J can be non-zero in.  The object's DoFs
    // (9-14) sit in slots k >= 9 / G, so an object-only row (ground contacts)
    // skips the slots below at compile time (IEEE 0 * x is not folded)
    constexpr int KOBJ = 9 / G;
    using KAll = std::integral_constant<int, 0>;
    using KObj = std::integral_constant<int, KOBJ>;
    auto prod = [&](auto KL, const float J[K]) {
        constexpr int k0 = decltype(KL)::value;
        float p = J[k0] * dvm[k0];
#pragma unroll
        for (int k = k0 + 1; k < K; k++) p = fmaf(J[k], dvm[k], p);
        return p;
    };
    // G = 8: a lane's two DoFs updated by one v_pk_fma_f32 (the same bits)
    auto apply2 = [&](float m0, float m1, float dl) {
        const f32x2 x = __builtin_elementwise_fma((f32x2){m0, m1}, (f32x2){dl, dl}, (f32x2){dvm[0], dvm[K - 1]});
        dvm[0] = x.x;
        dvm[K - 1] = x.y;
    };
    auto apply = [&](auto KL, const float M[K], float dl) {
        if constexpr (K == 2 && decltype(KL)::value == 0) {
            apply2(M[0], M[1], dl);
        } else {
#pragma unroll
            for (int k = decltype(KL)::value; k < K; k++) dvm[k] = fmaf(M[k], dl, dvm[k]);
        }
    };
    // warm start (see the one-lane solver)
#pragma unroll
    for (int c = 0; c < NG; c++)
        if (NOBJ > 0 && (gate_gnd & (1u << c))) apply(KObj{}, gM[c][0], gc[c].lam[0]);
#pragma unroll
    for (int c = 0; c < NR; c++)
        if (gate_robot & (1u << c)) apply(KAll{}, rM[c][0], rc[c].lam[0]);

    float res = 0.0f;
    // a joint row's J is e_d: its product is the velocity change of DoF d,
    // held by lane d % G in slot d / G: one broadcast instead of a sum
    auto jrow = [&](auto DD, float sgn, float rhs, float &lam, float lo, float hi) {
        constexpr int d = decltype(DD)::value;
        float s = group_bcast<G, d % G>(dvm[d / G]);
        float dl = rhs - dinvj[d] * (sgn * s);
        float nl = clamp_impulse(lam + dl, lo, hi);
        dl = nl - lam;
        lam = nl;
        PS_REC(dl);
        if constexpr (K == 2) {
            apply2(mrow[0][d], mrow[K - 1][d], sgn * dl);
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) dvm[k] = fmaf(mrow[k][d], sgn * dl, dvm[k]);
        }
        res = res_max(res, joint_viol(dl, midg[d]));
    };
    auto limit_row = [&](auto DD) {
        constexpr int d = decltype(DD)::value;
        if (gate_lim & (1u << d)) {
            float sgn = (lim_up >> d) & 1u ? -1.0f : 1.0f;
            float hi = (lim_on >> d) & 1u ? (float)PM_LIMIT_MAX_IMPULSE : 0.0f;
            jrow(DD, sgn, lim_rhs[d], lim_lam[d], 0.0f, hi);
        }
    };
    auto motor_row = [&](auto DD) {
        constexpr int d = decltype(DD)::value;
        float imp = STD_MOTORS ? (float)(joint_force(d) * PM_TIMESTEP) : mt.imp[d];
        jrow(DD, 1.0f, mot_rhs[d], mot_lam[d], -imp, imp);
    };
    // rows d = 8..0 and 0..8 with compile-time d
    auto down = [&](auto row) { static_for<0, 9>([&](auto I) { row(std::integral_constant<int, 8 - decltype(I)::value>{}); }); };
    auto up = [&](auto row) { static_for<0, 9>([&](auto I) { row(I); }); };
    auto normal = [&](auto KL, const float Jm[K], const float Mm[K], float rhs, float dinv, float &lam) {
        float s = group_sum<G>(prod(KL, Jm));
        float dl = rhs - dinv * s;
        float nl = clamp_impulse(lam + dl, 0.0f, (float)PM_CONTACT_UPPER);
        dl = nl - lam;
        lam = nl;
        PS_REC(dl);
        apply(KL, Mm, dl);
        res = res_max(res, row_viol(dl, dinv));
    };
    auto cone = [&](auto KL, const float J[3][K], const float M[3][K], const float rhs[3], const float dinv[3],
                    float lam[3], float mu) {
        // G = 8: the two rows side by side as f32x2 (v_pk_*) around their
        // group sums: the scalar rows' operations, fused where they were
        // fused, so the same bits (x = row 1, y = row 2).  G = 16 keeps the
        // scalar rows: fewer instructions with the pairs, but 0.8 % slower at
        // C2 (profiles/r05aa_ab.log)
        float dla, dlb;
        if constexpr (K == 1) {
            const float sa = group_sum<G>(prod(KL, J[1])), sb = group_sum<G>(prod(KL, J[2]));
            dla = rhs[1] - dinv[1] * sa;
            dlb = rhs[2] - dinv[2] * sb;
            float a = lam[1] + dla, b = lam[2] + dlb;
            const float lim = mu * lam[0];  // lam[0] >= 0: the normal row's clamp
            const float sc = cone_scale(a * a + b * b, lim);
            a *= sc;
            b *= sc;
            dla = a - lam[1];
            dlb = b - lam[2];
            lam[1] = a;
            lam[2] = b;
        } else {
#pragma clang fp contract(off)
            constexpr int k0 = decltype(KL)::value;
            f32x2 p = (f32x2){J[1][k0], J[2][k0]} * (f32x2){dvm[k0], dvm[k0]};
#pragma unroll
            for (int k = k0 + 1; k < K; k++)
                p = __builtin_elementwise_fma((f32x2){J[1][k], J[2][k]}, (f32x2){dvm[k], dvm[k]}, p);
            const f32x2 s2 = {group_sum<G>(p.x), group_sum<G>(p.y)};
            const f32x2 lam12 = {lam[1], lam[2]};
            const f32x2 ab = lam12 + __builtin_elementwise_fma(-(f32x2){dinv[1], dinv[2]}, s2, (f32x2){rhs[1], rhs[2]});
            const float lim = mu * lam[0];  // lam[0] >= 0: the normal row's clamp
            const float sc = cone_scale(fmaf(ab.x, ab.x, ab.y * ab.y), lim);
            const f32x2 dl2 = __builtin_elementwise_fma(ab, (f32x2){sc, sc}, -lam12);
            const f32x2 nl2 = ab * (f32x2){sc, sc};
            lam[1] = nl2.x;
            lam[2] = nl2.y;
            dla = dl2.x;
            dlb = dl2.y;
        }
        PS_REC(dla);
        PS_REC(dlb);
        if constexpr (K == 2 && decltype(KL)::value == 0) {
            apply2(M[1][0], M[1][1], dla);
            apply2(M[2][0], M[2][1], dlb);
        } else {
#pragma unroll
            for (int k = decltype(KL)::value; k < K; k++) dvm[k] = fmaf(M[2][k], dlb, fmaf(M[1][k], dla, dvm[k]));
        }
        res = res_max(res, res_max(row_viol(dla, dinv[1]), row_viol(dlb, dinv[2])));
    };
    // the object's ground normals touch only object DoFs: they commute with
    // the joint rows (robot DoFs only), so they run in the motor rows' block,
    // ungated (a slot a lane lacks is an all-zero no-op), where their
    // dependent chains interleave with the motor rows'
    auto ground_normals = [&]() {
        if constexpr (NOBJ > 0) {
#pragma unroll
            for (int c = 0; c < NG; c++) normal(KObj{}, gJ[c][0], gM[c][0], gc[c].rhs[0], gc[c].dinv[0], gc[c].lam[0]);
        }
    };
    auto contacts = [&]() {
#pragma unroll
        for (int c = 0; c < NR; c++)
            if (gate_robot & (1u << c)) normal(KAll{}, rJ[c][0], rM[c][0], rc[c].rhs[0], rc[c].dinv[0], rc[c].lam[0]);
#pragma unroll
        for (int c = 0; c < NG; c++)
            if (NOBJ > 0 && (gate_gnd & (1u << c))) cone(KObj{}, gJ[c], gM[c], gc[c].rhs, gc[c].dinv, gc[c].lam, gmu);
#pragma unroll
        for (int c = 0; c < NR; c++)
            if (gate_robot & (1u << c)) cone(KAll{}, rJ[c], rM[c], rc[c].rhs, rc[c].dinv, rc[c].lam, rc[c].mu);
    };
    // (the gates stay scalar tests inside the loop, as in the one-lane
    // solver's PS_REGATE)
    auto regate = [&]() { asm volatile("" : "+s"(gate_lim), "+s"(gate_gnd), "+s"(gate_robot)); };
    for (int it = 0; it < PM_SOLVER_ITERATIONS; it += 2) {
#ifdef PS_PROFILE_PHASES
        prof_it++;
#endif
        res = 0.0f;
        regate();
        down(motor_row);
        ground_normals();
        if (gate_lim != 0u) down(limit_row);
        contacts();
        if (res <= 0.0f) break;
#ifdef PS_PROFILE_PHASES
        prof_it++;
#endif
        res = 0.0f;
        regate();
        if (gate_lim != 0u) up(limit_row);
        up(motor_row);
        ground_normals();
        contacts();
#ifdef PS_DEBUG_ROW_DUMP
        rec(res);
        dump_on = false;
#endif
        if (res <= 0.0f) break;
    }
    // every lane of the group gets the whole velocity change
    static_for<0, 9>([&](auto DD) {
        constexpr int d = decltype(DD)::value;
        dv[d] = __shfl(dvm[d / G], d % G, G);
    });
    if constexpr (NOBJ > 0) {
        float o[6];
        static_for<0, 6>([&](auto JJ) {
            constexpr int dof = 9 + decltype(JJ)::value;
            o[dof - 9] = __shfl(dvm[dof / G], dof % G, G);
        });
        dw = mk(o[0], o[1], o[2]);
        dvl = mk(o[3], o[4], o[5]);
    }
}

#undef PS_REC

}  // namespace ps
