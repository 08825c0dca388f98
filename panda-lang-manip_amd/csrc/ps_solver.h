// ps_solver.h — projected Gauss-Seidel in btMultiBodyConstraintSolver order:
// what the row setup and both solvers share: the rows' rhs and 1/den helpers,
// the residual and clamps, the warm start's contact cache, the friction cone.
// The one-lane solver is the G == 1 block of substep (ps_substep.h), the
// group solver (16 or 8 lanes per env) ps_solver_group.h.
#pragma once

#include "ps_scene.h"

namespace ps {

// row rhs of a contact normal (btSequentialImpulseConstraintSolver setup:
// speculative margin when separated, ERP/split-impulse when penetrating)
// (1/dt = 500 is exact in fp32: products with it instead of IEEE divisions
// by the rounded dt, and closer to the fp64 oracle's pen / dt)
constexpr float PS_INV_DT = (float)(1.0 / PM_TIMESTEP);
PS_D float normal_rhs(float dist, float rel, float dinv) {
    float pen = dist + (float)PM_LINEAR_SLOP;
    float velerr = -rel, poserr = 0.0f;
    if (pen > 0.0f) velerr -= pen * PS_INV_DT;
    else poserr = -pen * (float)PM_ERP * PS_INV_DT;
    bool combined = pen > (float)PM_SPLIT_PENETRATION_THRESHOLD;
    return (combined ? poserr + velerr : velerr) * dinv;
}

// 1/den of a row (v_rcp_f32, 1 ulp: an IEEE division is ~10 VALU
// instructions, and the substep takes ~35 of these)
PS_D float safe_inv(float den) { return den > 2.2204460492503131e-16f ? __builtin_amdgcn_rcpf(den) : 0.0f; }

// Stack: 1/den of a cube's ground row j (normal +z, then (0,-1,0), (1,0,0))
// from its contact offset r: den = |r x dir|^2 iI + 1/m (isotropic inertia);
// the row setup and the solver both use this, so LDS holds r and rhs only
PS_D float cube_ground_dinv(V3 r, int j, float iI, float inv_m) {
    V3 rn = j == 0 ? mk(r.y, -r.x, 0.0f) : j == 1 ? mk(r.z, 0.0f, -r.x) : mk(0.0f, r.z, -r.y);
    return __builtin_amdgcn_rcpf(dot(rn, rn * iI) + inv_m);  // den >= 1/m > 0
}

// ---------------------------------------------------------- residual, clamps
// PGS residual of a row is dl / dinv (the impulse change in velocity units).
// v_rcp_f32 replaces the IEEE division.  A lane without the row has dinv = 0
// and dl = 0: dinv is clamped to FLT_MIN so that the residual is 0 * 2^126 = 0
// there (the reference skips such rows), never 0 * inf = NaN -- a NaN in the
// residual max would depend on fmaxf's NaN rule, which a build that assumes
// no NaNs is free to change.
// PGS stopping rule: Bullet stops once max over rows of (dl / dinv)^2 <= 1e-7
// (the residual is the impulse change times the row's effective mass).  The
// loop tracks it as a violation that is <= 0 once every row has
// |dl| / dinv <= sqrt(1e-7), so no row takes a reciprocal:
//   contact rows  |dl| - sqrt(1e-7) dinv
//   joint rows    |dl| den - sqrt(1e-7)      (den = M^-1_dd, in registers)
constexpr float kResidualAbs = 3.16227766e-4f;

// A row-family gate with a layout hint of how often it is open (the cube's
// ground rows and gripper slots 0-1: open; slots 2-3 and joint limits:
// closed).  A lone wave pays ~20 cycles for a taken branch (the instruction
// stream is refetched: profiles/r03a_issue_probe.jsonl, 8- vs 128-instruction
// loop bodies); laying the open blocks out as fall-through took Push from
// 3.18 to 3.14 ms and Reach from 1.47 to 1.44 ms per step at 65 536 envs.
#define PS_GATE(cond, likely) __builtin_expect(!!(cond), (likely))
PS_D float row_viol(float dl, float dinv) { return fmaf(-kResidualAbs, dinv, fabsf(dl)); }
// The solver's running residual max: llvm.maximum (v_maximum3_f32).  With
// fmaxf (llvm.maxnum) the IEEE-mode lowering re-canonicalised the running max
// (v_max x, x, x) at every row: ~30 VALU instructions per Push iteration.  The
// values are finite (the residual's 1/den is clamped, see kResidualAbs), where
// both give the same bits.  The impulse clamps stay fminf(fmaxf()): as
// v_med3_f32 (the same bits too) they made Push 0.25 % slower
// (profiles/r05v_ab.log).
// A NaN row violation (an env whose state is already non-finite) keeps res at
// NaN, so that lane never meets `res <= 0` and runs the 50-iteration cap; it is
// masked like any other lane, so no other env's rows or bits change, and the
// NaN/Inf guard flags (and optionally resets) the env after the step
// (test_gpu_contacts.py::test_nonfinite_guard_flags_and_resets: every other
// env equal bit for bit to a run without the corrupted one).
PS_D float res_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
PS_D float clamp_impulse(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
PS_D float joint_viol(float dl, float den) { return fmaf(fabsf(dl), den, -kResidualAbs); }

// The warm start's contact cache (state rows PS_F_WG0.. of this env, see
// include/pandasim.h): read at contact generation, written after the solve.
// Addresses are re-derived at each access from wave-uniform values (row base,
// stride, the wave's first env) and the lane id (v_mbcnt), so no per-lane
// pointer or index stays live through the solve.  The step kernels run one
// 64-lane wave per workgroup with G lanes per env, so env = (step_block * 64
// + lane) / G.  With G > 1 every lane of a group computes the same values;
// lanes of a group past the batch end (live = false) compute a copy of the
// last env and store nothing.
// Scenes with at most one object (IN_LDS) use rows WG0..WG0ID and WR..WRID
// only, held in LDS slots 0-4 and 5-9 over the substeps (cache_to_lds,
// cache_from_lds); Stack reads and writes the state rows directly.
template <int G, int NOBJ>
struct WarmCache {
    static constexpr bool IN_LDS = NOBJ <= 1;
    float *base;  // &f[PS_F_WG0 * stride]
    int64_t stride;
    bool live;
    MJStore lds;
    PS_D static int slot(int row) { return row < PS_F_WG1 ? row - PS_F_WG0 : 5 + (row - PS_F_WR); }
    PS_D float &at(int row) const {
        // a 32-bit byte offset from a wave-uniform row base (ps_create caps
        // the batch at PS_MAX_ENVS), as StateView
        const uint32_t e = (uint32_t)(((uint64_t)step_block<G>() * 64 + __lane_id()) / G) * 4u;
        return *(float *)((char *)(base + (int64_t)(row - PS_F_WG0) * stride) + e);
    }
    PS_D float load(int row) const {
        if constexpr (IN_LDS) return lds.cache(slot(row));
        else return at(row);
    }
    PS_D void store(int row, float v) const {
        if constexpr (IN_LDS) lds.cache(slot(row)) = v;
        else if (G == 1 || live) at(row) = v;
    }
    // once per control step, around the substep loop
    PS_D void to_lds() const {
        if constexpr (IN_LDS) {
#pragma unroll
            for (int k = 0; k < 5; k++) {
                lds.cache(k) = at(PS_F_WG0 + k);
                lds.cache(5 + k) = at(PS_F_WR + k);
            }
        }
    }
    PS_D void from_lds() const {
        if constexpr (IN_LDS) {
            if (G == 1 || live) {
#pragma unroll
                for (int k = 0; k < 5; k++) {
                    at(PS_F_WG0 + k) = lds.cache(k);
                    at(PS_F_WR + k) = lds.cache(5 + k);
                }
            }
        }
    }
};
// slot k's id (1 + feature, 0 = empty) of a packed id row
PS_D unsigned cache_id(unsigned pack, int k) { return (pack >> (5 * k)) & 31u; }
// normal impulse cached for `id` among the 4 slots (0 when absent)
PS_D float cache_lookup(const float lam[4], unsigned pack, unsigned id) {
    float l = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) l = cache_id(pack, k) == id ? lam[k] : l;
    return l;
}

// Friction-cone projection factor (resolveConeFrictionConstraintRows): lim/|f|
// when |f|^2 = m2 exceeds lim^2, else 1.  Raw v_rsq_f32: rsqrtf's denormal
// rescaling costs three instructions per cone row; m2 is clamped to FLT_MIN
// instead, so a denormal m2 cannot produce inf (and 0 * inf) there.
// lim = mu * lam_n takes the normal impulse as it is: every normal row clamps
// it to [0, upper] (and warm starts are 0.85 x a clamped impulse), so the
// oracle's max(lam_n, 0) is the identity here and only cost a v_max (plus a
// canonicalising one) per cone.
PS_D float cone_scale(float m2, float lim) {
    return m2 > lim * lim ? lim * __builtin_amdgcn_rsqf(fmaxf(m2, 1.17549435e-38f)) : 1.0f;
}

}  // namespace ps
