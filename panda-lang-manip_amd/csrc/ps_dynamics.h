// ps_dynamics.h — joint-space dynamics of the arm: mass matrix by composite
// rigid bodies, bias forces by a recursive Newton-Euler pass with prefix sums
// (gravity, gyroscopic, btMultiBody damping), the 9x9 Cholesky inverse, and
// the damped-least-squares inverse kinematics.
#pragma once

#include "ps_kinematics.h"

namespace ps {

// ------------------------------------------------------------------ dynamics
struct Comp {
    float m;
    V3 h;  // COM
    S3 I;  // about COM, base frame
};

template <int I>
PS_D Comp link_comp(const Kin &k) {
    constexpr LinkDef d = link_def(I);
    Comp c;
    c.m = (float)d.mass;
    c.h = com_pos<I>(k);
    c.I = rotate_diag(k.f[I].R, (float)link_inertia(I, 0), (float)link_inertia(I, 1), (float)link_inertia(I, 2));
    return c;
}

PS_D Comp combine(const Comp &a, const Comp &b) {
    Comp c;
    c.m = a.m + b.m;
    float inv = 1.0f / c.m;
    c.h = (a.h * a.m + b.h * b.m) * inv;
    // the two parallel-axis terms about the joint COM are one with the
    // reduced mass m_a m_b / (m_a + m_b) and d = h_a - h_b (masses are
    // compile-time constants, so is the factor)
    c.I = a.I + b.I + shift(a.m * b.m * inv, a.h - b.h);
    return c;
}

// Joint-space mass matrix (packed symmetric, 45 floats) by composite rigid
// bodies: for revolute b with composite C_b, the unit-rate momentum is
// P = m_b a_b x (h_b - o_b), L = I_b a_b; M_ab = a_a . (L + (h_b - o_a) x P).
PS_D void mass_matrix(const Kin &k, float M[45]) {
    V3 ax[9], org[9];
    static_for<0, 9>([&](auto D) {
        constexpr int d = decltype(D)::value;
        ax[d] = dof_axis<d>(k);
        org[d] = k.f[dof_def(d).link].o;
    });
    Comp f9 = link_comp<9>(k), f10 = link_comp<10>(k);
    // fingers (prismatic DoFs 7, 8)
    {
        V3 P9 = ax[7] * f9.m, P10 = ax[8] * f10.m;
        M[sidx(7, 7)] = f9.m;
        M[sidx(8, 8)] = f10.m;
        M[sidx(8, 7)] = 0.0f;
#pragma unroll
        for (int a = 0; a < 7; a++) {
            M[sidx(7, a)] = dot(ax[a], cross(f9.h - org[a], P9));
            M[sidx(8, a)] = dot(ax[a], cross(f10.h - org[a], P10));
        }
    }
    Comp c = combine(combine(link_comp<8>(k), f9), f10);
    static_for<0, 7>([&](auto BB) {
        constexpr int b = 6 - decltype(BB)::value;
        c = combine(link_comp<b>(k), c);
        V3 P = cross(ax[b], c.h - org[b]) * c.m;
        V3 L = mul(c.I, ax[b]);
#pragma unroll
        for (int a = 0; a <= b; a++) M[sidx(b, a)] = dot(ax[a], L + cross(c.h - org[a], P));
    });
}

// Bias forces h = C(q,qd) qd + g(q) + damping (RNEA with qdd = 0).  Forward
// pass over the chain; every link force/moment is folded into prefix sums so
// tau_i = a_i . ((N_tot - N_pre_i) - o_i x (F_tot - F_pre_i)) with moments
// about the base origin.
// Frames are produced on the fly (FK fused into the forward sweep) so no
// 12-frame kinematics array is held live next to the dynamics.
template <int I>
PS_D void link_wrench_f(const Frame &f, V3 w, V3 dw, V3 vo, V3 ao, V3 &F, V3 &N) {
    constexpr LinkDef d = link_def(I);
    constexpr float m = (float)d.mass;
    V3 c = f.o + com_offset<I>(f.R);
    V3 rc = c - f.o;
    V3 vc = vo + cross(w, rc);
    V3 ac = ao + cross(dw, rc) + cross(w, cross(w, rc));
    S3 Iw = rotate_diag(f.R, (float)link_inertia(I, 0), (float)link_inertia(I, 1), (float)link_inertia(I, 2));
    V3 Iww = mul(Iw, w);
    // (1-ulp square roots: the damping terms are ~1e-4 of the forces)
    float cl = (float)PM_LINEAR_DAMPING + (float)PM_LINEAR_DAMPING * fast_norm(vc);
    float ca = (float)PM_ANGULAR_DAMPING + (float)PM_ANGULAR_DAMPING * fast_norm(w);
    F = (ac + vc * cl) * m;
    V3 Nc = mul(Iw, dw) + cross(w, Iww) + Iww * ca;
    N = Nc + cross(c, F);  // about the base origin
}

PS_D void bias_forces(const float q[9], const float qd[9], float h[9]) {
    V3 w = mk(0, 0, 0), dw = mk(0, 0, 0), vo = mk(0, 0, 0), ao = mk(0, 0, -(float)PM_GRAVITY_Z);
    Frame f;
    f.R = M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    f.o = mk(0, 0, 0);
    V3 prev_o = f.o;
    V3 Fpre[7], Npre[7], ax[7], org[7];
    V3 Fs = mk(0, 0, 0), Ns = mk(0, 0, 0);
    static_for<0, 7>([&](auto II) {
        constexpr int I = decltype(II)::value;
        f = child_frame<I>(f, q[I]);
        V3 r = f.o - prev_o;
        vo = vo + cross(w, r);
        ao = ao + cross(dw, r) + cross(w, cross(w, r));
        V3 a = col(f.R, 2);
        ax[I] = a;
        org[I] = f.o;
        dw = dw + cross(w, a) * qd[I];
        w = w + a * qd[I];
        Fpre[I] = Fs;
        Npre[I] = Ns;
        V3 F, N;
        link_wrench_f<I>(f, w, dw, vo, ao, F, N);
        Fs = Fs + F;
        Ns = Ns + N;
        prev_o = f.o;
    });
    // link 7 (massless, fixed) and the hand (8): same origin as link 7
    f = child_frame<7>(f, 0.0f);
    f = child_frame<8>(f, 0.0f);
    {
        V3 r = f.o - prev_o;
        vo = vo + cross(w, r);
        ao = ao + cross(dw, r) + cross(w, cross(w, r));
        V3 F, N;
        link_wrench_f<8>(f, w, dw, vo, ao, F, N);
        Fs = Fs + F;
        Ns = Ns + N;
    }
    // fingers: prismatic children of the hand
    static_for<0, 2>([&](auto JJ) {
        constexpr int J = decltype(JJ)::value;
        constexpr int L = 9 + J;
        Frame ff = child_frame<L>(f, q[7 + J]);
        constexpr LinkDef ld = link_def(L);
        V3 a = mul(ff.R, mk((float)ld.axis[0], (float)ld.axis[1], (float)ld.axis[2]));
        float v = qd[7 + J];
        V3 r = ff.o - f.o;
        V3 vf = vo + cross(w, r) + a * v;
        V3 af = ao + cross(dw, r) + cross(w, cross(w, r)) + cross(w, a) * (2.0f * v);
        V3 F, N;
        link_wrench_f<L>(ff, w, dw, vf, af, F, N);
        h[7 + J] = dot(a, F);
        Fs = Fs + F;
        Ns = Ns + N;
    });
#pragma unroll
    for (int I = 0; I < 7; I++) {
        V3 Fsub = Fs - Fpre[I], Nsub = Ns - Npre[I];
        h[I] = dot(ax[I], Nsub - cross(org[I], Fsub));
    }
}

// M = L L^T, then M^-1 (packed symmetric) = L^-T L^-1
PS_D void spd_inverse(float M[45]) {
    // Cholesky with one reciprocal square root per column (v_rsq_f32, 1 ulp:
    // sqrtf and the IEEE division took ~22 VALU instructions per pivot): the
    // 36 off-diagonal divisions are products with it, and the inverse below
    // reads the pivots' reciprocals only
    float L[45], invd[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            float s = M[sidx(i, j)];
#pragma unroll
            for (int q = 0; q < j; q++) s -= L[sidx(i, q)] * L[sidx(j, q)];
            if (i == j) {
                invd[i] = __builtin_amdgcn_rsqf(s);  // M is SPD: s > 0
            } else {
                L[sidx(i, j)] = s * invd[j];
            }
        }
    }
    // invert L in place (lower triangular)
    float Li[45];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const float inv = invd[i];
        Li[sidx(i, i)] = inv;
#pragma unroll
        for (int j = 0; j < i; j++) {
            float s = 0.0f;
#pragma unroll
            for (int q = j; q < i; q++) s += L[sidx(i, q)] * Li[sidx(q, j)];
            Li[sidx(i, j)] = -s * inv;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            float s = 0.0f;
#pragma unroll
            for (int q = i; q < 9; q++) s += Li[sidx(q, i)] * Li[sidx(q, j)];
            M[sidx(i, j)] = s;
        }
}

// --------------------------------------------------------------------- IK
// calculateInverseKinematics (restated in DESIGN.md §5, IK): <= 20 DLS steps
// dq = (J^T J + 0.5 I)^-1 J^T [dp; dr], pivot-frame Jacobian, 45 deg clamp.
template <int LINK>
PS_D void inverse_kinematics(const float q_start[9], V3 target, Q4 orn, float q_out[9]) {
    constexpr int NA = LINK <= 6 ? LINK + 1 : 7;  // arm DoFs that move LINK
    constexpr bool FINGER = (LINK == 9 || LINK == 10);
    constexpr int N = NA + (FINGER ? 1 : 0);
    constexpr int FD = LINK == 9 ? 7 : 8;
    float on = sqrtf(orn.x * orn.x + orn.y * orn.y + orn.z * orn.z + orn.w * orn.w);
    Q4 ot = Q4{orn.x / on, orn.y / on, orn.z / on, orn.w / on};
    float q[9];
#pragma unroll
    for (int d = 0; d < 9; d++) q[d] = q_start[d];
    float diff = 1e30f;
    for (int it = 0; it < PM_IK_MAX_ITERS && diff > (float)PM_IK_RESIDUAL; it++) {
        Kin k;
        fk(q, k);
        V3 p = k.f[LINK].o;
        V3 dS = target - p;
        diff = norm(dS);
        Q4 qe = mat_to_quat(k.f[LINK].R);
        float n2 = qe.x * qe.x + qe.y * qe.y + qe.z * qe.z + qe.w * qe.w;
        const float in2 = 1.0f / n2;
        Q4 qinv = Q4{-qe.x * in2, -qe.y * in2, -qe.z * in2, qe.w * in2};
        Q4 dq = qmul(ot, qinv);
        // btQuaternion::getAngle()/getAxis() evaluate 2 acos(w) and
        // v / sqrt(1 - w^2); for a unit quaternion these equal 2 atan2(|v|, w)
        // and v / |v|, which stay accurate in fp32 when w -> 1 (acos would
        // quantise small orientation errors to ~7e-4 rad).
        float s2 = dq.x * dq.x + dq.y * dq.y + dq.z * dq.z;
        float vn = sqrtf(s2);
        float angle = 2.0f * atan2f(vn, dq.w);
        V3 axv = s2 < 10.0f * 2.2204460492503131e-16f ? mk(1, 0, 0) : mk(dq.x, dq.y, dq.z) * (1.0f / vn);
        if (angle > 3.14159265358979323846f) angle -= 6.28318530717958647692f;
        else if (angle < -3.14159265358979323846f) angle += 6.28318530717958647692f;
        V3 dR = axv * (angle / norm(axv));
        // Jacobian columns (6 x N)
        V3 Jv[N], Jw[N];
#pragma unroll
        for (int c = 0; c < NA; c++) {
            V3 a = col(k.f[c].R, 2);
            Jv[c] = cross(a, p - k.f[c].o);
            Jw[c] = a;
        }
        if constexpr (FINGER) {
            Jv[NA] = mul(k.f[LINK].R, mk(0.0f, LINK == 9 ? 1.0f : -1.0f, 0.0f));
            Jw[NA] = mk(0, 0, 0);
        }
        float U[N * (N + 1) / 2], g[N];
#pragma unroll
        for (int a = 0; a < N; a++) {
            g[a] = dot(Jv[a], dS) + dot(Jw[a], dR);
#pragma unroll
            for (int b = 0; b <= a; b++)
                U[a * (a + 1) / 2 + b] = dot(Jv[a], Jv[b]) + dot(Jw[a], Jw[b]) + (a == b ? (float)PM_IK_DAMPING : 0.0f);
        }
        // Cholesky solve, one reciprocal per pivot (the divisions by it are
        // products: an IEEE division is ~10 VALU instructions).  A v_rsq_f32
        // pivot (1 ulp) measured 0.3 % faster per step but, together with the
        // damping norms' v_sqrt in bias_forces, moved one in-contact Push
        // sample past the parity bound: not kept.
        float Lc[N * (N + 1) / 2], il[N];
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                float s = U[i * (i + 1) / 2 + j];
#pragma unroll
                for (int t = 0; t < j; t++) s -= Lc[i * (i + 1) / 2 + t] * Lc[j * (j + 1) / 2 + t];
                if (i == j) {
                    Lc[i * (i + 1) / 2 + i] = sqrtf(s);
                    il[i] = 1.0f / Lc[i * (i + 1) / 2 + i];
                } else {
                    Lc[i * (i + 1) / 2 + j] = s * il[j];
                }
            }
        float y[N], x[N];
#pragma unroll
        for (int i = 0; i < N; i++) {
            float s = g[i];
#pragma unroll
            for (int t = 0; t < i; t++) s -= Lc[i * (i + 1) / 2 + t] * y[t];
            y[i] = s * il[i];
        }
#pragma unroll
        for (int i = N - 1; i >= 0; i--) {
            float s = y[i];
#pragma unroll
            for (int t = i + 1; t < N; t++) s -= Lc[t * (t + 1) / 2 + i] * x[t];
            x[i] = s * il[i];
        }
        float mx = 0.0f;
#pragma unroll
        for (int i = 0; i < N; i++) mx = fmaxf(mx, fabsf(x[i]));
        float sc = mx > (float)PM_IK_MAX_ANGLE ? (float)PM_IK_MAX_ANGLE / mx : 1.0f;
#pragma unroll
        for (int i = 0; i < NA; i++) q[i] += x[i] * sc;
        if constexpr (FINGER) q[FD] += x[NA] * sc;
    }
#pragma unroll
    for (int d = 0; d < 9; d++) q_out[d] = q[d];
}

}  // namespace ps
