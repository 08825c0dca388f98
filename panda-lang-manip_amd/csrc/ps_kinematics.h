// ps_kinematics.h — the Panda's link frames: forward kinematics with exact
// URDF origin rotations (12 links), DoF axes and link COM positions.
#pragma once

#include "ps_common.h"

namespace ps {

struct Frame {
    M3 R;
    V3 o;
};

struct Kin {
    Frame f[PM_NUM_LINKS];
};

// frame of link I given its parent frame and its joint coordinate
template <int I>
PS_D Frame child_frame(const Frame &P, float q) {
    constexpr LinkDef d = link_def(I);
    Frame F;
    M3 Rj;
    // P.R times the constant joint-origin rotation and offset with the zero
    // terms dropped at compile time (IEEE x * 0 is not folded, and the
    // origins are axis permutations or identities: 18 of the 27 products
    // were zeros, in every one of the ~60 frames an env-step builds)
    static_for<0, 3>([&](auto RR) {
        constexpr int r = decltype(RR)::value;
        static_for<0, 3>([&](auto CC) {
            constexpr int c = decltype(CC)::value;
            float acc = 0.0f;
            bool any = false;
            static_for<0, 3>([&](auto KK) {
                constexpr int k = decltype(KK)::value;
                constexpr double w = origin_rot(I).m[k * 3 + c];
                if constexpr (w != 0.0) {
                    const float t = w == 1.0 ? P.R.m[r * 3 + k] : (w == -1.0 ? -P.R.m[r * 3 + k] : P.R.m[r * 3 + k] * (float)w);
                    acc = any ? acc + t : t;
                    any = true;
                }
            });
            Rj.m[r * 3 + c] = acc;
        });
    });
    V3 off = mk(0.0f, 0.0f, 0.0f);
    bool anyo = false;
    static_for<0, 3>([&](auto KK) {
        constexpr int k = decltype(KK)::value;
        if constexpr (d.o[k] != 0.0) {
            const V3 t = col(P.R, k) * (float)d.o[k];
            off = anyo ? off + t : t;
            anyo = true;
        }
    });
    V3 oj = P.o + off;
    if constexpr (d.type == PM_JOINT_REVOLUTE) {
        // libm sincosf (its range-reduction branch doubles as a scheduling
        // fence; __sinf/__cosf measured 12% slower on Push through spills)
        float s, c;
        sincosf(q, &s, &c);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            float a = Rj.m[r * 3 + 0], b = Rj.m[r * 3 + 1];
            F.R.m[r * 3 + 0] = a * c + b * s;
            F.R.m[r * 3 + 1] = b * c - a * s;
            F.R.m[r * 3 + 2] = Rj.m[r * 3 + 2];
        }
        F.o = oj;
    } else if constexpr (d.type == PM_JOINT_PRISMATIC) {
        F.R = Rj;
        V3 ax = mul(Rj, mk((float)d.axis[0], (float)d.axis[1], (float)d.axis[2]));
        F.o = oj + ax * q;
    } else {
        F.R = Rj;
        F.o = oj;
    }
    return F;
}

// R times link I's constant COM offset, zero terms dropped at compile time
template <int I>
PS_D V3 com_offset(const M3 &R) {
    constexpr LinkDef d = link_def(I);
    V3 off = mk(0.0f, 0.0f, 0.0f);
    bool any = false;
    static_for<0, 3>([&](auto KK) {
        constexpr int k = decltype(KK)::value;
        if constexpr (d.com[k] != 0.0) {
            const V3 t = col(R, k) * (float)d.com[k];
            off = any ? off + t : t;
            any = true;
        }
    });
    return off;
}

// all link frames, base-relative (robot base at the origin, identity rotation)
PS_D void fk(const float q[9], Kin &k) {
    Frame base;
    base.R = M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    base.o = mk(0, 0, 0);
    k.f[0] = child_frame<0>(base, q[0]);
    k.f[1] = child_frame<1>(k.f[0], q[1]);
    k.f[2] = child_frame<2>(k.f[1], q[2]);
    k.f[3] = child_frame<3>(k.f[2], q[3]);
    k.f[4] = child_frame<4>(k.f[3], q[4]);
    k.f[5] = child_frame<5>(k.f[4], q[5]);
    k.f[6] = child_frame<6>(k.f[5], q[6]);
    k.f[7] = child_frame<7>(k.f[6], 0.0f);
    k.f[8] = child_frame<8>(k.f[7], 0.0f);
    k.f[9] = child_frame<9>(k.f[8], q[7]);
    k.f[10] = child_frame<10>(k.f[8], q[8]);
    k.f[11] = child_frame<11>(k.f[8], 0.0f);
}

// world axis of DoF d (revolute: frame z; prismatic: frame * axis)
template <int D>
PS_D V3 dof_axis(const Kin &k) {
    constexpr int L = dof_def(D).link;
    constexpr LinkDef d = link_def(L);
    if constexpr (d.type == PM_JOINT_REVOLUTE) return col(k.f[L].R, 2);
    else return mul(k.f[L].R, mk((float)d.axis[0], (float)d.axis[1], (float)d.axis[2]));
}

template <int I>
PS_D V3 com_pos(const Kin &k) {
    constexpr LinkDef d = link_def(I);
    return k.f[I].o + com_offset<I>(k.f[I].R);
}

}  // namespace ps
