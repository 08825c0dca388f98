// state_kernels.hip — the small kernels on the state and the C ABI entry
// points (include/pandasim.h) that launch them: state init and reset
// (ps_init_state, ps_reset), link / base / IK queries (ps_link_state,
// ps_inverse_kinematics, ps_base_state), the per-env rng (ps_rng_*), HER's
// reward (ps_compute_reward) and the Euler / quaternion conversions.  One
// env (or one row) per lane; every kernel reads/writes the
// structure-of-arrays state with coalesced row accesses.  No substep here.
#include "ps_ctx.h"
#include "ps_reward.h"
#include "ps_task.h"

namespace {

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__(kBlock) void k_init_state(KParams P) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const StateView &s = P.s;
    for (int r = 0; r < PS_NUM_FLOAT_ROWS; r++) s.F(r, i) = 0.0f;
    s.F(PS_F_CQUAT + 3, i) = 1.0f;
    s.F(PS_F_C2QUAT + 3, i) = 1.0f;
    for (int d = 0; d < 9; d++) {
        s.F(PS_F_MKD + d, i) = 1.0f;
        s.F(PS_F_MIMP + d, i) = (float)PM_DEFAULT_MOTOR_MAX_IMPULSE;
    }
    for (int d = 0; d < PS_MAX_GOAL_DIM; d++) s.G(d, i) = 0.0;
    store_rng(s, i, pcg_seed(0));
    aux_rng(s, i) = aux_seed(0);
    s.E(i) = 0;
}

template <int TASK>
__global__ __launch_bounds__(kBlock) void k_reset(KParams P, const uint8_t *mask, const uint64_t *seeds, float *obs,
                                                  float *ag, float *dg) {
    using T = TaskTraits<TASK>;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    if (mask && !mask[i]) return;
    const StateView &s = P.s;
    Pcg r = seeds ? pcg_seed(seeds[i]) : load_rng(s, i);
    uint64_t aux = seeds ? aux_seed(seeds[i]) : aux_rng(s, i);
    float q[9], qd[9];
    Body bd[T::NOBJ > 0 ? T::NOBJ : 1];
#pragma unroll
    for (int b = 0; b < T::NOBJ; b++) load_body(s, i, b, bd[b]);
    double g[6] = {0, 0, 0, 0, 0, 0};
    reset_env<TASK>(q, qd, bd, g, r, aux);
    store_robot(s, i, q, qd);
#pragma unroll
    for (int b = 0; b < T::NOBJ; b++) store_body(s, i, b, bd[b]);
    for (int d = 0; d < T::GOAL; d++) s.G(d, i) = g[d];
    store_rng(s, i, r);
    aux_rng(s, i) = aux;
    s.E(i) = 0;
    clear_contact_cache(s, i);
    // RecordEpisodeStatistics (ps_set_episode_stats) zeroes the running
    // return on reset(): an abandoned episode's partial return does not carry
    // into the next one
    if (P.epstats) P.epstats[i] = 0.0f;
    write_obs<TASK>(P, i, q, qd, bd, g, obs, ag, dg);
}


__global__ __launch_bounds__(kBlock) void k_link_state(KParams P, int link, float *pos, float *quat, float *lv,
                                                       float *av) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    float q[9], qd[9];
    load_robot(P.s, i, q, qd);
    Kin k;
    fk(q, k);
    // COM frame of `link` (getLinkState [0], [1], [6], [7])
    M3 R = k.f[0].R;
    V3 c = mk(0, 0, 0);
    static_for<0, PM_NUM_LINKS>([&](auto L) {
        constexpr int l = decltype(L)::value;
        if (l == link) {
            R = k.f[l].R;
            c = com_pos<l>(k);
        }
    });
    V3 v = mk(0, 0, 0), w = mk(0, 0, 0);
    static_for<0, 9>([&](auto D) {
        constexpr int d = decltype(D)::value;
        constexpr int jl = dof_def(d).link;
        // ancestor-or-self test on the fixed tree: arm joints precede every
        // later link; finger joints only move their own finger
        bool anc = (jl <= 6) ? (jl <= link) : (jl == link);
        if (anc) {
            V3 a = dof_axis<d>(k);
            if (link_def(jl).type == PM_JOINT_REVOLUTE) {
                v = v + cross(a, c - k.f[jl].o) * qd[d];
                w = w + a * qd[d];
            } else {
                v = v + a * qd[d];
            }
        }
    });
    if (pos) { V3 p = c + P.sc.base; pos[i * 3] = p.x; pos[i * 3 + 1] = p.y; pos[i * 3 + 2] = p.z; }
    if (quat) { Q4 qq = mat_to_quat(R); quat[i * 4] = qq.x; quat[i * 4 + 1] = qq.y; quat[i * 4 + 2] = qq.z; quat[i * 4 + 3] = qq.w; }
    if (lv) { lv[i * 3] = v.x; lv[i * 3 + 1] = v.y; lv[i * 3 + 2] = v.z; }
    if (av) { av[i * 3] = w.x; av[i * 3 + 1] = w.y; av[i * 3 + 2] = w.z; }
}

template <int LINK>
__global__ __launch_bounds__(kBlock) void k_ik(KParams P, const float *pos, const float *orn, float *q_out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    float q[9], qd[9];
    load_robot(P.s, i, q, qd);
    V3 t = mk(pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]) - P.sc.base;
    Q4 o = Q4{orn[i * 4], orn[i * 4 + 1], orn[i * 4 + 2], orn[i * 4 + 3]};
    float out[9];
    inverse_kinematics<LINK>(q, t, o, out);
    for (int d = 0; d < 9; d++) q_out[i * 9 + d] = out[d];
}

// gymnasium.utils.seeding.np_random(seed) per env (core.py:244): the env's
// generator becomes Generator(PCG64(SeedSequence(seeds[i]))), and Flip's goal
// stream restarts from the same seed
__global__ __launch_bounds__(kBlock) void k_rng_seed(KParams P, const uint8_t *mask, const uint64_t *seeds) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n || (mask && !mask[i])) return;
    store_rng(P.s, i, pcg_seed(seeds[i]));
    aux_rng(P.s, i) = aux_seed(seeds[i]);
}

// Generator.uniform(low[n], high[n]) per env: n consecutive draws from the
// env's own stream (push.py:75-80 draws a 3-vector in one call)
struct UniformArgs {
    int n;
    double lo[PS_MAX_UNIFORM], hi[PS_MAX_UNIFORM];
};
__global__ __launch_bounds__(kBlock) void k_rng_uniform(KParams P, const uint8_t *mask, UniformArgs u, double *out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n || (mask && !mask[i])) return;
    Pcg r = load_rng(P.s, i);
    for (int k = 0; k < u.n; k++) out[i * u.n + k] = uniform(r, u.lo[k], u.hi[k]);
    store_rng(P.s, i, r);
}

// Flip's goal (Rotation.random(), flip.py:70-72) from each env's goal stream
__global__ __launch_bounds__(kBlock) void k_rng_rotation(KParams P, const uint8_t *mask, double *out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n || (mask && !mask[i])) return;
    uint64_t st = aux_rng(P.s, i);
    double q[4];
    random_rotation(st, q);
    aux_rng(P.s, i) = st;
    for (int k = 0; k < 4; k++) out[i * 4 + k] = q[k];
}

// getBasePositionAndOrientation + getEulerFromQuaternion + getBaseVelocity of
// object `b` (pybullet.py:284-349)
__global__ __launch_bounds__(kBlock) void k_base_state(KParams P, int b, float *pos, float *quat, float *euler,
                                                       float *vel, float *avel) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    Body c;
    load_body(P.s, i, b, c);
    if (pos) { pos[i * 3] = c.pos.x; pos[i * 3 + 1] = c.pos.y; pos[i * 3 + 2] = c.pos.z; }
    if (quat) { quat[i * 4] = c.quat.x; quat[i * 4 + 1] = c.quat.y; quat[i * 4 + 2] = c.quat.z; quat[i * 4 + 3] = c.quat.w; }
    if (euler) { V3 e = euler_from_quat(c.quat); euler[i * 3] = e.x; euler[i * 3 + 1] = e.y; euler[i * 3 + 2] = e.z; }
    if (vel) { vel[i * 3] = c.vel.x; vel[i * 3 + 1] = c.vel.y; vel[i * 3 + 2] = c.vel.z; }
    if (avel) { avel[i * 3] = c.omg.x; avel[i * 3 + 1] = c.omg.y; avel[i * 3 + 2] = c.omg.z; }
}

// compute_reward / is_success for HER (core.py:226): goal pairs of `gd`
// values; f64 arithmetic when either side is f64 (numpy promotion), f32
// otherwise (threshold rounded to f32): ps_reward.h, shared with the replay
// sampler
__global__ __launch_bounds__(256) void k_compute_reward(int task, int reward_type, const void *ag, int ag_dbl,
                                                        const void *dg, int dg_dbl, float *reward, uint8_t *success,
                                                        int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int gd = goal_pair_dim(task);
    float r;
    bool ok;
    if (ag_dbl || dg_dbl) {
        const void *a = ag_dbl ? (const void *)((const double *)ag + i * gd) : (const void *)((const float *)ag + i * gd);
        const void *g = dg_dbl ? (const void *)((const double *)dg + i * gd) : (const void *)((const float *)dg + i * gd);
        goal_pair_reward_f64(task, reward_type, a, ag_dbl, g, dg_dbl, r, ok);
    } else {
        goal_pair_reward_f32(task, reward_type, (const float *)ag + i * gd, (const float *)dg + i * gd, r, ok);
    }
    if (reward) reward[i] = r;
    if (success) success[i] = ok;
}


// scipy's Rotation.from_euler('xyz', e, degrees=True).as_quat() (panda_ori.py:91):
// extrinsic rotations about x, then y, then z, q = qz qy qx as (x, y, z, w).
// One lane per row, fp64 arithmetic, rounded once to f32 on store.
__global__ __launch_bounds__(256) void k_euler_xyz_to_quat(const float *euler_deg, float *quat, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr double half_rad = 3.14159265358979323846 / 180.0 * 0.5;
    double sa, ca, sb, cb, sc, cc;
    sincos((double)euler_deg[i * 3] * half_rad, &sa, &ca);
    sincos((double)euler_deg[i * 3 + 1] * half_rad, &sb, &cb);
    sincos((double)euler_deg[i * 3 + 2] * half_rad, &sc, &cc);
    quat[i * 4] = (float)(sa * cb * cc - ca * sb * sc);
    quat[i * 4 + 1] = (float)(ca * sb * cc + sa * cb * sc);
    quat[i * 4 + 2] = (float)(ca * cb * sc - sa * sb * cc);
    quat[i * 4 + 3] = (float)(ca * cb * cc + sa * sb * sc);
}

// Rotation.from_quat(q).as_euler('xyz', degrees=True) (panda_cartesian.py:222-225):
// q is normalised first; angles about x and z in [-180, 180], about y in
// [-90, 90].  Within 1e-3 deg of pitch +-90 (gimbal lock: the x and z angles
// are not separately determined) the result is unspecified.
__global__ __launch_bounds__(256) void k_quat_to_euler_xyz(const float *quat, float *euler_deg, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = quat[i * 4], y = quat[i * 4 + 1], z = quat[i * 4 + 2], w = quat[i * 4 + 3];
    const double inv = 1.0 / sqrt(x * x + y * y + z * z + w * w);
    x *= inv; y *= inv; z *= inv; w *= inv;
    // R = Rz(c) Ry(b) Rx(a): R20 = -sin b, R21 = cos b sin a, R22 = cos b cos a,
    // R10 = cos b sin c, R00 = cos b cos c; b from atan2(sin b, |cos b|), which
    // keeps its precision near +-90 where asin loses it
    const double r21 = 2.0 * (y * z + w * x), r22 = 1.0 - 2.0 * (x * x + y * y);
    const double r10 = 2.0 * (x * y + w * z), r00 = 1.0 - 2.0 * (y * y + z * z);
    const double sb = 2.0 * (w * y - x * z);
    constexpr double deg = 180.0 / 3.14159265358979323846;
    euler_deg[i * 3] = (float)(atan2(r21, r22) * deg);
    euler_deg[i * 3 + 1] = (float)(atan2(sb, sqrt(r21 * r21 + r22 * r22)) * deg);
    euler_deg[i * 3 + 2] = (float)(atan2(r10, r00) * deg);
}

}  // namespace

// ------------------------------------------------------------------- C ABI
extern "C" {

int ps_init_state(ps_ctx *c, void *state, void *stream) {
    if (!c || !state) return fail(c, PS_ERR_ARG, "null argument");
    KParams P = params_of(c, state);
    hipLaunchKernelGGL(k_init_state, grid_of(P.n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, P);
    c->gains_dirty = 1;
    return check_launch(c);
}

int ps_reset(ps_ctx *c, void *state, const uint8_t *mask, const uint64_t *seeds, float *obs, float *ag, float *dg,
             void *stream) {
    if (!c || !state) return fail(c, PS_ERR_ARG, "null argument");
    if (!scene_matches_task(c->cfg)) return fail(c, PS_ERR_UNSUPPORTED, "scene does not match the task");
    KParams P = params_of(c, state);
    dim3 g = grid_of(P.n, kBlock), b(kBlock);
    hipStream_t st = (hipStream_t)stream;
    // the next step rewrites the gain rows: a reset is where a caller starts
    // with a fresh or swapped-in buffer, whose address a caching allocator may
    // have handed out before (so the pointer test of the step launcher alone
    // would not see it)
    c->gains_dirty = 1;
#define PS_RESET_CASE(T) \
    case T: hipLaunchKernelGGL(k_reset<T>, g, b, 0, st, P, mask, seeds, obs, ag, dg); break;
    switch (c->cfg.task) {
        PS_FOR_EACH_TASK(PS_RESET_CASE)
        default: return fail(c, PS_ERR_ARG, "bad task");  // (ps_create admits none)
    }
#undef PS_RESET_CASE
    return check_launch(c);
}

int ps_link_state(ps_ctx *c, const void *state, int link, float *pos, float *quat, float *lin_vel, float *ang_vel,
                  void *stream) {
    if (!c || !state || link < 0 || link >= PM_NUM_LINKS) return fail(c, PS_ERR_ARG, "bad argument");
    KParams P = params_of(c, (void *)state);
    hipLaunchKernelGGL(k_link_state, grid_of(P.n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, P, link, pos, quat,
                       lin_vel, ang_vel);
    return check_launch(c);
}

int ps_inverse_kinematics(ps_ctx *c, const void *state, int link, const float *pos, const float *orn, float *q_out,
                          void *stream) {
    if (!c || !state || !pos || !orn || !q_out || link < 0 || link >= PM_NUM_LINKS)
        return fail(c, PS_ERR_ARG, "bad argument");
    KParams P = params_of(c, (void *)state);
    dim3 g = grid_of(P.n, kBlock), b(kBlock);
    hipStream_t st = (hipStream_t)stream;
    switch (link) {
#define PS_IK_CASE(L) \
    case L: hipLaunchKernelGGL(k_ik<L>, g, b, 0, st, P, pos, orn, q_out); break;
        PS_IK_CASE(0) PS_IK_CASE(1) PS_IK_CASE(2) PS_IK_CASE(3) PS_IK_CASE(4) PS_IK_CASE(5)
        PS_IK_CASE(6) PS_IK_CASE(7) PS_IK_CASE(8) PS_IK_CASE(9) PS_IK_CASE(10) PS_IK_CASE(11)
#undef PS_IK_CASE
    }
    return check_launch(c);
}

int ps_rng_seed(ps_ctx *c, void *state, const uint8_t *mask, const uint64_t *seeds, void *stream) {
    if (!c || !state || !seeds) return fail(c, PS_ERR_ARG, "null argument");
    KParams P = params_of(c, state);
    hipLaunchKernelGGL(k_rng_seed, grid_of(P.n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, P, mask, seeds);
    return check_launch(c);
}

int ps_rng_uniform(ps_ctx *c, void *state, const uint8_t *mask, int n, const double *low, const double *high,
                   double *out, void *stream) {
    if (!c || !state || !out || !low || !high || n < 1 || n > PS_MAX_UNIFORM)
        return fail(c, PS_ERR_ARG, "bad argument");
    KParams P = params_of(c, state);
    UniformArgs u;
    u.n = n;
    for (int k = 0; k < PS_MAX_UNIFORM; k++) {
        u.lo[k] = k < n ? low[k] : 0.0;
        u.hi[k] = k < n ? high[k] : 0.0;
    }
    hipLaunchKernelGGL(k_rng_uniform, grid_of(P.n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, P, mask, u, out);
    return check_launch(c);
}

int ps_rng_rotation(ps_ctx *c, void *state, const uint8_t *mask, double *out, void *stream) {
    if (!c || !state || !out) return fail(c, PS_ERR_ARG, "null argument");
    KParams P = params_of(c, state);
    hipLaunchKernelGGL(k_rng_rotation, grid_of(P.n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, P, mask, out);
    return check_launch(c);
}

int ps_base_state(ps_ctx *c, const void *state, int object, float *pos, float *quat, float *euler, float *lin_vel,
                  float *ang_vel, void *stream) {
    if (!c || !state) return fail(c, PS_ERR_ARG, "null argument");
    if (object < 0 || object >= c->cfg.n_objects) return fail(c, PS_ERR_UNSUPPORTED, "scene has no such object");
    KParams P = params_of(c, (void *)state);
    hipLaunchKernelGGL(k_base_state, grid_of(P.n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, P, object, pos,
                       quat, euler, lin_vel, ang_vel);
    return check_launch(c);
}

int ps_compute_reward(int task, int reward_type, const void *ag, int ag_is_double, const void *dg, int dg_is_double,
                      float *reward, uint8_t *success, int64_t n, void *stream) {
    if (!ag || !dg || n < 0 || task < 0 || task >= PS_NUM_TASKS || reward_type < 0 || reward_type > 1)
        return PS_ERR_ARG;
    if (n == 0) return PS_OK;
    hipLaunchKernelGGL(k_compute_reward, grid_of(n, 256), dim3(256), 0, (hipStream_t)stream, task, reward_type, ag,
                       ag_is_double, dg, dg_is_double, reward, success, n);
    return hipGetLastError() == hipSuccess ? PS_OK : PS_ERR_HIP;
}

int ps_euler_xyz_to_quat(ps_ctx *c, const float *euler_deg, float *quat, int64_t n, void *stream) {
    if (!c || !euler_deg || !quat || n < 0) return fail(c, PS_ERR_ARG, "bad argument");
    if (n == 0) return PS_OK;
    hipLaunchKernelGGL(k_euler_xyz_to_quat, grid_of(n, 256), dim3(256), 0, (hipStream_t)stream, euler_deg, quat, n);
    return check_launch(c);
}

int ps_quat_to_euler_xyz(ps_ctx *c, const float *quat, float *euler_deg, int64_t n, void *stream) {
    if (!c || !quat || !euler_deg || n < 0) return fail(c, PS_ERR_ARG, "bad argument");
    if (n == 0) return PS_OK;
    hipLaunchKernelGGL(k_quat_to_euler_xyz, grid_of(n, 256), dim3(256), 0, (hipStream_t)stream, quat, euler_deg, n);
    return check_launch(c);
}

}  // extern "C"
