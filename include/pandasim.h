/*
 * pandasim.h — C ABI of the MI355X-native batched Panda simulator
 * (libpandasim.so, built from panda-lang-manip_amd/csrc: pandasim.hip and the
 * kernel units).
 *
 * Drop-in boundary for the reference's step()/reset() path.  Each entry point
 * replaces one call site of /root/reference (cited per function); see
 * INTEGRATION.md for the host-side binding (ctypes) a maintainer adds.
 *
 * Conventions
 *   - Every buffer argument is a DEVICE pointer owned by the caller (PyTorch
 *     tensors in panda-lang-manip_amd/pandasim); the library never allocates
 *     per call and holds no host-language objects.  Two context-owned
 *     scratch buffers are allocated on first use and freed by ps_destroy: the
 *     ray-casting calls' render_prims (ps_render, ps_point_cloud,
 *     ps_cloud_keypoint_features) and Stack's stash (ps_step, ps_step_oriented,
 *     ps_sim_step, ps_motion_run); each is initialised on the stream of the
 *     call that creates it.
 *   - Calls are asynchronous on the given HIP stream (hipStream_t passed as
 *     void*; NULL = default stream).  One ps_ctx per (process, device); a
 *     context is not re-entrant.
 *   - Every call returns PS_OK (0) or a negative PS_ERR_* code; no C++
 *     exception crosses the ABI.  ps_last_error() gives the message.
 *   - Batched state lives in one caller-owned device buffer of
 *     ps_layout.total_bytes bytes, structure-of-arrays, described by ps_layout.
 *     save_state/restore_state (core.py:252-278) are copies of that buffer.
 */
#ifndef PANDASIM_H
#define PANDASIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_ABI_VERSION 6

/* the six registered tasks (panda_gym/__init__.py:8-54) */
enum {
    PS_TASK_REACH = 0,
    PS_TASK_PUSH = 1,
    PS_TASK_PICK_AND_PLACE = 2,
    PS_TASK_SLIDE = 3,
    PS_TASK_STACK = 4,
    PS_TASK_FLIP = 5,
    PS_NUM_TASKS = 6
};
enum { PS_CONTROL_EE = 0, PS_CONTROL_JOINTS = 1 };
enum { PS_REWARD_SPARSE = 0, PS_REWARD_DENSE = 1 };
enum { PS_SHAPE_BOX = 0, PS_SHAPE_CYLINDER = 1 };
#define PS_VISUAL_SPHERE 2 /* ps_visual.target_shape only: create_sphere ghost (reach.py:31-38) */
enum { PS_OK = 0, PS_ERR_ARG = -1, PS_ERR_HIP = -2, PS_ERR_UNSUPPORTED = -3 };

/* Largest batch one context holds (2^28 envs, ~260 GB of state): the kernels
 * address an env's state rows by a 32-bit byte offset.  ps_state_layout and
 * ps_create return PS_ERR_ARG above it. */
#define PS_MAX_ENVS (1LL << 28)

/* Scene/env configuration.  ps_default_config() fills the registered env
 * (panda_gym/__init__.py:8-54 + envs/panda_tasks.py:14-113 + the task's
 * _create_scene); the scene fields let tests build the reference's
 * engine-level KAT scenes (test/pybullet_test.py).
 *   n_objects      dynamic objects: 0 (Reach), 1, or 2 (Stack)
 *   object_shape   PS_SHAPE_BOX (half extents object_half) or
 *                  PS_SHAPE_CYLINDER (radius object_half[0], half height
 *                  object_half[2], axis z; slide.py:33-42)
 *   object_mass    mass of object 1; object2_mass of object 2 (stack.py:33-55)
 *   object_friction lateral friction of the objects (default 0.5; Slide 0.04)
 *   table_cx/hx/hy table centre x and half extents (top at z = 0;
 *                  pybullet.py:741-771) */
typedef struct {
    int32_t task, control, reward, block_gripper;
    int32_t has_table, has_plane, n_objects, object_shape;
    float base[3];
    float object_half[3];
    float object_mass, object2_mass, object_friction;
    float table_cx, table_hx, table_hy;
} ps_config;

/* State layout: byte offsets from the state pointer.  Float fields are rows
 * of `stride` floats (env i at [row*stride + i]); goal is PS_MAX_GOAL_DIM
 * rows of doubles, rng is 5 rows of uint64 (PCG64 state hi, lo, inc hi, lo of
 * the task's np_random, then the splitmix64 state of Flip's goal stream),
 * elapsed one row of int32 (TimeLimit counter). */
#define PS_MAX_GOAL_DIM 6
enum {
    PS_F_Q = 0,        /* 9 joint positions (DoF order: joints 0..6, 9, 10) */
    PS_F_QD = 9,       /* 9 joint velocities */
    PS_F_MTARGET = 18, /* 9 motor target positions */
    PS_F_MKP = 27,     /* 9 motor position gains */
    PS_F_MKD = 36,     /* 9 motor velocity gains */
    PS_F_MVEL = 45,    /* 9 motor target velocities */
    PS_F_MIMP = 54,    /* 9 motor max impulses (force * 1/500 s) */
    PS_F_CPOS = 63,    /* 3 object position (world) */
    PS_F_CQUAT = 66,   /* 4 object orientation quaternion x,y,z,w */
    PS_F_CVEL = 70,    /* 3 object linear velocity */
    PS_F_COMG = 73,    /* 3 object angular velocity */
    PS_F_C2POS = 76,   /* object 2 (Stack): position, */
    PS_F_C2QUAT = 79,  /*   orientation, */
    PS_F_C2VEL = 83,   /*   linear velocity, */
    PS_F_C2OMG = 86,   /*   angular velocity */
    /* contact cache of the warm-started solver (Bullet's persistent contact
     * manifolds): the previous substep's contacts per group,
     * slot by slot, with their final normal impulses.  Id rows pack the four
     * slots' ids as sum_k id_k * 32^k (exact in f32), id = 1 + feature, 0 =
     * empty: ground slots 1 + support point, gripper slots 1 + sphere +
     * 8 * (0 object 1, 1 object 2, 2 ground). */
    PS_F_WG0 = 89,     /* 4 ground-contact normal impulses of object 1 */
    PS_F_WG0ID = 93,   /*   their packed ids */
    PS_F_WG1 = 94,     /* object 2 (Stack) */
    PS_F_WG1ID = 98,
    PS_F_WR = 99,      /* 4 gripper-contact normal impulses */
    PS_F_WRID = 103,   /*   their packed ids */
    PS_F_WP = 104,     /* 4 object-object (Stack) normal impulses, */
    PS_F_WPPT = 108,   /*   their points in object 1's frame (x, y, z per slot), */
    PS_F_WPN = 120,    /*   and how many slots are in use */
    PS_NUM_FLOAT_ROWS = 121,
    PS_NUM_RNG_ROWS = 5
};

typedef struct {
    int64_t num_envs, stride;
    int64_t float_offset, goal_offset, rng_offset, elapsed_offset;
    int64_t total_bytes;
} ps_layout;

typedef struct ps_ctx ps_ctx;

int ps_abi_version(void);
int ps_default_config(int task, int control, int reward, ps_config *out);
int ps_state_layout(int64_t num_envs, ps_layout *out);

/* gym.make(id) -> RobotTaskEnv.__init__ (core.py:209-227), minus the initial
 * reset, which the caller issues with ps_reset. */
int ps_create(const ps_config *cfg, int64_t num_envs, int device, ps_ctx **out);
void ps_destroy(ps_ctx *ctx);
const char *ps_last_error(const ps_ctx *ctx);
int ps_obs_dim(const ps_ctx *ctx);
int ps_action_dim(const ps_ctx *ctx);
int ps_goal_dim(const ps_ctx *ctx);        /* 3, 4 (Flip quaternion) or 6 (Stack) */
int ps_max_episode_steps(const ps_ctx *ctx); /* TimeLimit: 50, Stack 100 (__init__.py:18-46) */

/* Zero state, identity object orientation and PyBullet's default joint
 * velocity motors (loadURDF, core.py:40-52). */
int ps_init_state(ps_ctx *ctx, void *state, void *stream);

/* RobotTaskEnv.reset(seed) (core.py:240-250) for every env with mask[i] != 0
 * (mask == NULL: all).  seeds != NULL: env i is re-seeded with
 * Generator(PCG64(SeedSequence(seeds[i]))) (core.py:244); seeds == NULL: the
 * env's current generator continues.  obs/ag/dg may be NULL. */
int ps_reset(ps_ctx *ctx, void *state, const uint8_t *mask, const uint64_t *seeds, float *obs, float *ag,
             float *dg, void *stream);

/* RobotTaskEnv.step(action) (core.py:280-289) + TimeLimit(50), fused:
 * Panda.set_action (panda.py:52-107, incl. calculateInverseKinematics) ->
 * PyBullet.step (pybullet.py:52-55, 20 substeps) -> _get_obs -> is_success /
 * compute_reward.  actions: [B, action_dim] f32.  obs [B, obs_dim], ag/dg
 * [B, goal_dim], reward [B] f32, terminated/truncated [B] u8.  autoreset != 0:
 * finished envs are reset in-kernel (generator continues) and obs/ag/dg hold
 * the reset observation; final_obs/final_ag (may be NULL) receive the
 * pre-reset observation of every env. */
int ps_step(ps_ctx *ctx, void *state, const float *actions, float *obs, float *ag, float *dg, float *reward,
            uint8_t *terminated, uint8_t *truncated, int autoreset, float *final_obs, float *final_ag,
            void *stream);

/* ps_step with a target orientation of the end effector per env: the fused
 * step of Panda.set_action(action, euler_xyz) (panda_ori.py:52-99).  orn:
 * device [B, 4] f32 quaternions (x, y, z, w), which calculateInverseKinematics
 * receives in place of panda.py:89's standard (1, 0, 0, 0) and normalises;
 * every other argument, the 20 substeps, observation, reward, TimeLimit,
 * auto-reset, the non-finite guard, the episode statistics, the lanes-per-env
 * choice (ps_set_lanes_per_env, ps_step_lanes) and the motor-row bookkeeping
 * are ps_step's.  orn == NULL: PS_ERR_ARG.  A joints-control context:
 * PS_ERR_UNSUPPORTED (the reference ignores euler_xyz there: call ps_step). */
int ps_step_oriented(ps_ctx *ctx, void *state, const float *actions, const float *orn, float *obs, float *ag,
                     float *dg, float *reward, uint8_t *terminated, uint8_t *truncated, int autoreset,
                     float *final_obs, float *final_ag, void *stream);

/* scipy's Rotation.from_euler('xyz', e, degrees=True).as_quat() (panda_ori.py:91:
 * extrinsic rotations about x, y, then z) for n rows: euler_deg device [n, 3]
 * f32 degrees -> quat device [n, 4] f32 (x, y, z, w; the sign is not
 * canonicalised).  fp64 arithmetic, rounded once to f32. */
int ps_euler_xyz_to_quat(ps_ctx *ctx, const float *euler_deg, float *quat, int64_t n, void *stream);

/* Rotation.from_quat(q).as_euler('xyz', degrees=True) (panda_cartesian.py:222-225)
 * for n rows: quat device [n, 4] f32 (x, y, z, w; normalised first) ->
 * euler_deg device [n, 3] f32 degrees, x and z angles in [-180, 180], y angle
 * in [-90, 90].  fp64 arithmetic, rounded once to f32.  Within 1e-3 degrees of
 * pitch +-90 (gimbal lock) the result is unspecified. */
int ps_quat_to_euler_xyz(ps_ctx *ctx, const float *quat, float *euler_deg, int64_t n, void *stream);

/* Lanes per env of ps_step's kernel: 1 (one env per lane, the large-batch
 * kernel), 16 or 8 (a group of 16 or 8 lanes shares each env's constraint
 * solve -- the small-batch kernels, one object at most: not Stack); 0
 * (default) picks 16 for batches of at most PS_GROUP16_AUTO_MAX_ENVS envs, 8
 * up to PS_GROUP8_AUTO_MAX_ENVS and 1 above.  The kernels sum in different
 * orders, so their results agree to fp32 rounding, not bit for bit: fix the
 * value to compare runs of different batch sizes bit for bit. */
#define PS_GROUP16_AUTO_MAX_ENVS 4096
#define PS_GROUP8_AUTO_MAX_ENVS 8192
int ps_set_lanes_per_env(ps_ctx *ctx, int lanes);
int ps_step_lanes(const ps_ctx *ctx); /* the value ps_step uses */

/* gymnasium's RecordEpisodeStatistics, fused into ps_step (no reference
 * counterpart: the training loop's wrapper around gym.make).  stats != NULL:
 * device [4, B] f32, caller-owned, must outlive the steps: row 0 the running
 * return of each env's current episode, row 1 the return of its last finished
 * episode, row 2 that episode's success (terminated: 1, truncated: 0), row 3
 * the number of finished episodes.  Every following ps_step adds its reward
 * to row 0 and, when the episode ends, moves it to row 1 and clears it.
 * stats == NULL turns it off. */
int ps_set_episode_stats(ps_ctx *ctx, float *stats);

/* NaN/Inf guard of ps_step (no reference counterpart; SURVEY.md §5 failure
 * detection): with flags != NULL (device [B] u8, caller-owned, must outlive
 * the steps) every following ps_step writes flags[i] = 1 when env i's joint
 * or object state is not finite after the step, else 0; with
 * reset_nonfinite != 0 such an env is also reset in-kernel (its generator
 * continues, as in auto-reset) and reported truncated, even when ps_step's
 * autoreset is 0.  flags == NULL and reset_nonfinite == 0 turn it off. */
int ps_set_nonfinite_guard(ps_ctx *ctx, uint8_t *flags, int reset_nonfinite);

/* The fused step sets POSITION_CONTROL on all nine joints (panda.py:52-107 ->
 * control_joints, pybullet.py:462-477), as env.step does.  It stores the
 * motor targets and max impulses every step but the gain rows (kp, kd,
 * target velocity) only when they may differ from its own: on the first
 * ps_step after ps_create, ps_init_state or ps_reset, and after this call
 * (a step of a buffer at another address than the last step's also writes
 * them, but a caching allocator can hand a new buffer the old address, so
 * callers must not rely on that).  A caller that swaps buffers without a
 * ps_reset, or writes motor rows itself (the plugin path's control_joints,
 * a raw write into the state, a snapshot copied into it), calls it first. */
int ps_mark_motor_rows_dirty(ps_ctx *ctx);

/* Engine level: PyBullet.step() (pybullet.py:52-55) with the motors already in
 * the state (n_substeps of 1/500 s). */
int ps_sim_step(ps_ctx *ctx, void *state, int n_substeps, void *stream);

/* getLinkState(computeLinkVelocity=1) (pybullet.py:351-400) for all envs:
 * pos/lin_vel/ang_vel [B,3], quat [B,4]; any output may be NULL. */
int ps_link_state(ps_ctx *ctx, const void *state, int link, float *pos, float *quat, float *lin_vel,
                  float *ang_vel, void *stream);

/* calculateInverseKinematics (pybullet.py:479-497) from the current joint
 * positions: pos [B,3] world, orn [B,4] (x,y,z,w), q_out [B,9]. */
int ps_inverse_kinematics(ps_ctx *ctx, const void *state, int link, const float *pos, const float *orn,
                          float *q_out, void *stream);

/* --- Cartesian motion primitives (panda_cartesian.py:53-145), fused ---
 *
 * move / grasp / release of the language-manipulation pipeline's robot, per
 * env: a plan call fills a plan from the state, ps_motion_run executes its
 * control steps (Cartesian set_action + PyBullet.step each).  They touch no
 * goal, generator, TimeLimit counter, observation or reward.
 *
 * The plan is a caller-owned device buffer of ps_motion_plan_bytes(num_envs)
 * bytes, structure-of-arrays with the state's stride (ps_layout.stride):
 * PS_PLAN_NUM_F64_ROWS rows of `stride` doubles, then PS_PLAN_NUM_I32_ROWS
 * rows of `stride` int32 (env i at [row*stride + i]).  A zeroed buffer is a
 * valid plan with nothing to do. */
enum {
    PS_PLAN_START = 0,  /* 3 f64: move: ee position when the plan was made */
    PS_PLAN_DELTA = 3,  /* 3 f64: move: (goal - start) / num_steps */
    PS_PLAN_WIDTH = 6,  /* 1 f64: action[3]: move: finger width at plan time; grasp 1; release `width` */
    PS_PLAN_Q0 = 7,     /* 4 f64: ee link quaternion at plan time (x, y, z, w), unit */
    PS_PLAN_ROTVEC = 11, /* 3 f64: move: rotation vector of R_start^-1 R_goal (angle <= pi) */
    PS_PLAN_NUM_F64_ROWS = 14
};
enum {
    PS_PLAN_NUM_STEPS = 0, /* control steps of the plan */
    PS_PLAN_DONE = 1,      /* control steps executed so far */
    PS_PLAN_BLOCKED = 2,   /* gripper blocked (finger targets 0): set by grasp, cleared by release, kept by move */
    PS_PLAN_KIND = 3,      /* PS_PLAN_KIND_MOVE or PS_PLAN_KIND_HOLD */
    PS_PLAN_NUM_I32_ROWS = 4
};
enum { PS_PLAN_KIND_MOVE = 0, PS_PLAN_KIND_HOLD = 1 };
#define PS_PLAN_HOLD_STEPS 30 /* control steps of grasp and release (panda_cartesian.py:127, 142) */

/* Bytes of a plan buffer for num_envs envs (PS_ERR_ARG, negative, for a batch
 * ps_state_layout rejects). */
int64_t ps_motion_plan_bytes(int64_t num_envs);

/* Panda.move(goal_pos, goal_euler) up to its loop (panda_cartesian.py:98-114)
 * for every env with mask[i] != 0 (mask == NULL: all): start = ee position,
 * start orientation = ee link quaternion, finger_width = q9 + q10, d = |goal -
 * start|, num_steps = 20 when d < 0.03, else d // 0.015 (+ 1 when d % 0.015 >
 * 1e-3), delta = (goal - start) / num_steps; fp64 arithmetic on the f32 state.
 * goal_pos: device [B, 3] f32 world; goal_quat: device [B, 4] f32 (x, y, z, w;
 * normalised; ps_euler_xyz_to_quat of goal_euler).  The orientation is
 * interpolated as scipy's Slerp([1, num_steps], [start, goal]) does, along the
 * shortest arc.  Sets done = 0 and keeps the plan's blocked row (the caller
 * writes it: the reference's block_gripper).  Envs with mask[i] == 0 get
 * num_steps = done = 0. */
int ps_plan_move(ps_ctx *ctx, const void *state, void *plan, const float *goal_pos, const float *goal_quat,
                 const uint8_t *mask, void *stream);

/* Panda.grasp() (panda_cartesian.py:124-130): blocked := 1 and 30 control
 * steps of action (0, 0, 0, 1) with the ee link's orientation of that step.
 * Envs with mask[i] == 0 get num_steps = done = 0 and keep blocked. */
int ps_plan_grasp(ps_ctx *ctx, const void *state, void *plan, const uint8_t *mask, void *stream);

/* Panda.release(width) (panda_cartesian.py:139-145): blocked := 0 and 30
 * control steps of action (0, 0, 0, width[i]); width: device [B] f32, NULL = 1. */
int ps_plan_release(ps_ctx *ctx, const void *state, void *plan, const float *width, const uint8_t *mask,
                    void *stream);

/* The loops of move / grasp / release (panda_cartesian.py:116-122, 127-130,
 * 142-145), fused: every env executes min(max_steps, num_steps - done) control
 * steps -- the step's waypoint and orientation, Cartesian Panda.set_action
 * (:53-72, 147-176: action clipped to [-1, 1], target = ee position +
 * action[:3] unscaled, z >= 0, calculateInverseKinematics on link 11, finger
 * targets 0 when blocked else (width + action[3]) / 2, POSITION_CONTROL as
 * ps_step), PyBullet.step (20 substeps) -- and advances done.  An env with no
 * steps left keeps its state bits; an env's result does not depend on how
 * many steps the other envs run, nor on how the steps are split over calls.
 * The motor gain rows are written with ps_step's values.  Any context (any
 * task, either control type).  PS_ERR_ARG: a NULL buffer or max_steps < 1. */
int ps_motion_run(ps_ctx *ctx, void *state, void *plan, int max_steps, void *stream);

/* --- Motion programs: a sequence of primitives in one launch ---
 *
 * A program is num_segments segments, 1 to PS_PROGRAM_MAX_SEGMENTS; every env
 * runs its own segments one after the other to the end, planning each from
 * the state it has reached, without waiting for any other env. */
enum {
    PS_SEG_MOVE = 0,    /* Panda.move to goal_pos[s], goal_quat[s] */
    PS_SEG_GRASP = 1,   /* Panda.grasp */
    PS_SEG_RELEASE = 2, /* Panda.release of width[s] */
    PS_SEG_WAIT = 3     /* wait_steps[s] times PyBullet.step (20 substeps), the motors as they stand */
};
#define PS_PROGRAM_MAX_SEGMENTS 32
#define PS_PROGRAM_MAX_WAIT 1000 /* control steps of one wait segment, at least 1 */

/* Runs the program in one launch; env i ends where the calls ps_plan_move /
 * ps_plan_grasp / ps_plan_release + ps_motion_run to the plan's end, made
 * segment by segment with the segments' masks, leave it, bit for bit.
 *
 * Host arrays, read before the call returns: kinds [S] (PS_SEG_*), wait_steps
 * [S] (read for PS_SEG_WAIT only; may be NULL without one).  blocked0: the
 * gripper's blocked flag before the first segment (the reference's
 * block_gripper, which ps_plan_move's caller writes into the plan); a grasp
 * sets it and a release clears it for the segments after it, in every env,
 * whatever the masks are.
 * Device arrays: goal_pos [S, B, 3] f32 world and goal_quat [S, B, 4] f32
 * (x, y, z, w), row s read for a move; width [S, B] f32, row s read for a
 * release, NULL = 1 for every release; mask [S, B] u8, NULL = all: env i runs
 * segment s when mask[s, i] != 0.
 *
 * A wait uses the motor targets of the last control step this launch executed
 * in that env, or the state's target rows when it is the env's first segment,
 * with ps_step's gains and no inverse kinematics.  A move whose goal position
 * or quaternion is not finite, or whose quaternion is zero, is not started:
 * the env stops there and runs none of its later segments.  An env whose
 * segments are all masked out, or which stops before its first control step,
 * keeps its state and plan bits.
 *
 * completed [B] i32 (may be NULL): the index of the first segment not run, S
 * when all ran (a masked-out segment counts as run); steps [B] i32 (may be
 * NULL): the control steps executed.  On return the plan holds each env's
 * last move, grasp or release that ran, with done == num_steps (a wait writes
 * no plan row).  The motor gain rows are written as ps_motion_run writes them.
 *
 * PS_ERR_ARG, nothing launched or written: a NULL ctx, state, plan or kinds;
 * num_segments out of range; an unknown kind; a wait without wait_steps or
 * with a count outside 1 to PS_PROGRAM_MAX_WAIT; a move with a NULL goal_pos
 * or goal_quat. */
int ps_motion_program(ps_ctx *ctx, void *state, void *plan, int num_segments, const int32_t *kinds,
                      const int32_t *wait_steps, int blocked0, const float *goal_pos, const float *goal_quat,
                      const float *width, const uint8_t *mask, int32_t *completed, int32_t *steps, void *stream);

/* --- pieces of the unfused (Robot/Task plugin) path, pandasim/core.py --- */

#define PS_MAX_UNIFORM 8

/* gymnasium.utils.seeding.np_random(seed) (core.py:244) for every env with
 * mask[i] != 0 (mask == NULL: all): env i's generator becomes
 * Generator(PCG64(SeedSequence(seeds[i]))).  seeds: device [B] uint64. */
int ps_rng_seed(ps_ctx *ctx, void *state, const uint8_t *mask, const uint64_t *seeds, void *stream);

/* np_random.uniform(low, high) with n = len(low) <= PS_MAX_UNIFORM
 * (reach.py:52, push.py:78,85, pick_and_place.py:75-76; random() is
 * uniform(0, 1)): n consecutive draws from each masked env's stream into
 * out [B, n] f64 (device).  low/high are HOST arrays of n doubles. */
int ps_rng_uniform(ps_ctx *ctx, void *state, const uint8_t *mask, int n, const double *low, const double *high,
                   double *out, void *stream);

/* Flip's goal, scipy Rotation.random().as_quat() (flip.py:70-72): the
 * reference draws it from numpy's unseeded global RandomState; here from each
 * masked env's splitmix64 goal stream (seeded with the env seed by ps_reset /
 * ps_rng_seed), four Box-Muller normals normalised, into out [B, 4] f64. */
int ps_rng_rotation(ps_ctx *ctx, void *state, const uint8_t *mask, double *out, void *stream);

/* getBasePositionAndOrientation / getEulerFromQuaternion / getBaseVelocity of
 * object `object` (0 or 1) (pybullet.py:284-349): pos, euler, lin_vel, ang_vel
 * [B,3], quat [B,4] (x,y,z,w); any output may be NULL.  PS_ERR_UNSUPPORTED if
 * the scene has no such object. */
int ps_base_state(ps_ctx *ctx, const void *state, int object, float *pos, float *quat, float *euler,
                  float *lin_vel, float *ang_vel, void *stream);

/* Task.compute_reward / is_success of `task` (reach.py:56-65, push.py:89-98,
 * stack.py:118-131, flip.py:80-91), vectorised for HER (core.py:226): n goal
 * pairs [n, goal_dim(task)], each f64 when its *_is_double flag is set, else
 * f32.  Goal-distance tasks use utils.distance (threshold 0.05, Stack 0.1),
 * Flip uses utils.angle_distance = 1 - <a, b>^2 (threshold 0.2).  As numpy
 * does, the arithmetic is f64 when either side is f64 and f32 (threshold
 * rounded to f32) when both are f32.  reward and success may be NULL. */
int ps_compute_reward(int task, int reward_type, const void *ag, int ag_is_double, const void *dg,
                      int dg_is_double, float *reward, uint8_t *success, int64_t n, void *stream);


/* --- camera images (pybullet.py:69-264; §8(f) rank 4) --- */

/* Visual description of the scene for ps_render: flat colours (r, g, b, a in
 * [0, 1]) by role -- 0 plane, 1 table, 2 object 1, 3 object 2, 4 target 1,
 * 5 target 2, 6 robot, 7 background -- and the ghost targets' shapes
 * (PS_SHAPE_BOX, PS_SHAPE_CYLINDER, PS_VISUAL_SPHERE; -1 = none) with box half
 * extents / cylinder (radius, radius, half height) / sphere (radius, ...). */
typedef struct {
    float rgba[8][4];
    int32_t target_shape[2];
    float target_half[2][3];
} ps_visual;

/* computeViewMatrixFromYawPitchRoll(target, distance, yaw, pitch, roll,
 * upAxisIndex=2) and computeProjectionMatrixFOV(fov=60, aspect=width/height,
 * near=0.1, far=100) as column-major float[16] (pybullet.py:69-107), and
 * tran_pix_world = inv(P V) of the order='F' matrices, row-major double[16]
 * (may be NULL).  Host arithmetic only: no context, no GPU. */
int ps_camera(const float target[3], float distance, float yaw, float pitch, float roll, int width, int height,
              float view[16], float proj[16], double tran_pix_world[16]);

/* getCameraImage(width, height, view, proj) of every env (pybullet.py:186-192):
 * depth [B, height, width] f32 (OpenGL window depth, 1 = nothing hit) and rgb
 * [B, height, width, 3] u8, either may be NULL.  targets: device [B, 2, 7] f32
 * ghost-target poses (position, quaternion x,y,z,w), NULL = no targets.  The
 * arm is drawn as capsules between its joint frames plus the gripper spheres
 * (the URDF meshes are not available); the rest of the scene is exact. */
int ps_render(ps_ctx *ctx, const void *state, const float view[16], const float proj[16], int width, int height,
              const ps_visual *vis, const float *targets, float *depth, uint8_t *rgb, void *stream);

/* render()'s deprojection (pybullet.py:203-262) of depth [B, h, w]: per pixel
 * the world point [B, h*w, 3] f64, valid [B, h*w] u8 (depth < 0.99 and
 * 0 < z < 0.67 and -0.5 < x < 0.2) and pixels_2d [B, h*w, 2] f64; outputs may
 * be NULL.  tran_pix_world: HOST row-major double[16]. */
int ps_deproject_image(ps_ctx *ctx, const float *depth, const double tran_pix_world[16], int width, int height,
                       double *points, uint8_t *valid, double *pixels_2d, void *stream);

/* PyBullet.deproject(depth, pixels, tran_pix_world) (pybullet.py:109-146):
 * n pixels (column, row) int32 per env [B, n, 2] -> points [B, n, 3] f64;
 * a pixel outside the image reads nothing and yields a NaN point. */
int ps_deproject_pixels(ps_ctx *ctx, const float *depth, const int32_t *pixels, int n,
                        const double tran_pix_world[16], int width, int height, double *points, void *stream);

/* --- fused multi-view point-cloud observation --- */

/* One view of the observation: what ps_camera returns for it. */
typedef struct {
    float view[16], proj[16];
    double tran_pix_world[16];
} ps_cloud_view;

/* An extra open box lo < p < hi on the world point (the reference's
 * filter_outliers; lo z just above the table top drops the table). */
typedef struct {
    float lo[3], hi[3];
} ps_cloud_crop;

/* Bytes of the device workspace of ps_point_cloud: per env and (view, tile of
 * 256 pixels) 32 B of validity bits, a 4 B count and a 4 B prefix; it does not
 * grow with n_points.  Host arithmetic only.  PS_ERR_ARG (negative) for
 * num_envs outside 1..PS_MAX_ENVS, n_views outside 1..8, an empty image, more
 * than 65 535 pixel tiles or n_views * width * height >= 2^31. */
int64_t ps_cloud_workspace_bytes(int64_t num_envs, int n_views, int width, int height);

/* The observation the reference's policies start from (grasp.py:122-137,
 * generate_dset.py:148-195, 334): render n_views views, keep the points
 * render() keeps, merge, crop, draw n_points with replacement -- in one call,
 * without the per-pixel arrays.
 *
 * The merged cloud of env b is, view 0 first and in row-major pixel order
 * inside a view, every pixel that ps_deproject_image of that view's ps_render
 * depth marks valid and whose world point lies strictly inside crop (NULL =
 * no crop); M_b is its length.  Sample j of env b takes the merged cloud's
 * entry of rank (z * M_b) >> 64, z the splitmix64 output of counter
 * c = b * n_points + j:  z = seed + 0x9E3779B97F4A7C15 * (c + 1);
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
 * 0x94D049BB133111EB; z ^= z >> 31 (mod 2^64).
 *
 * points [B, n_points, 3] f32: ps_deproject_image's f64 world point rounded
 * once; colors [B, n_points, 3] u8: ps_render's rgb of the pixel; source
 * [B, n_points] i32: view * width * height + pixel; count [B] i32: M_b.
 * colors, source and count may be NULL.  An env with M_b = 0 gets points 0,
 * colors 0 and source -1.  views and crop are HOST memory, the outputs,
 * targets (as ps_render's) and workspace (ps_cloud_workspace_bytes) device
 * memory.  Every value is bit-identical to the composition of ps_render and
 * ps_deproject_image of the same library.
 * PS_ERR_ARG: a NULL ctx, state, views, vis, points or workspace, n_views
 * outside 1..8, n_points < 1 (or above 65 535 * 256), an empty image, more
 * than 65 535 pixel tiles, n_views * width * height >= 2^31. */
int ps_point_cloud(ps_ctx *ctx, const void *state, const ps_cloud_view *views, int n_views, int width, int height,
                   const ps_visual *vis, const float *targets, const ps_cloud_crop *crop, int n_points,
                   uint64_t seed, float *points, uint8_t *colors, int32_t *source, int32_t *count, void *workspace,
                   void *stream);

/* --- PointNet++ front end of the point-cloud observation --- */

/* What the reference's policies do to every cloud before a learned weight is
 * touched (envs/inference/models/pointnet2_utils.py): pc_normalize,
 * farthest_point_sample, query_ball_point, and the index_points gathers with
 * the centring of PointNetSetAbstractionMsg.forward.  Every call works on the
 * context's B = num_envs clouds of N points; all pointers are device memory
 * unless said otherwise, every call is ordered on `stream`.
 *
 * The squared distance of two points is, everywhere below,
 *   d = a - b;  d2 = (d.x * d.x + d.y * d.y) + d.z * d.z
 * in f32 with every product and sum rounded (no fused multiply-add).
 *
 * Limits (PS_ERR_ARG, nothing launched, outputs untouched): a NULL required
 * pointer, N outside 1..PS_CLOUD_MAX_POINTS, S outside 1..N, nsample < 1, a
 * radius that is not positive and finite, D outside 0..PS_CLOUD_MAX_FEATURES
 * or D != 0 without feats (and the reverse), n_scales outside
 * 1..PS_CLOUD_MAX_SCALES.  Indices read from device memory (start, centre_idx,
 * group_idx) cannot be refused by a stream-ordered call: a value outside
 * 0..N-1 is clamped into it, so nothing is read out of bounds; the Python
 * layer refuses such a start before the call. */
#define PS_CLOUD_MAX_POINTS 8192  /* 12 B of LDS per point in one workgroup */
#define PS_CLOUD_MAX_SCALES 4
#define PS_CLOUD_MAX_FEATURES 16

/* pc_normalize of points [B, N, 3]: centroid [B, 3] = the mean of the N rows,
 * accumulated in f64 in a fixed order (partial sum t of 256 takes rows t,
 * t + 256, ...; the partials are added by halving) and rounded once to f32;
 * scale [B] = the largest sqrt(d2(p, centroid)); xyz_out [B, N, 3] =
 * (p - centroid) / scale.  A cloud of scale 0 yields zeros, not NaN. */
int ps_cloud_normalize(ps_ctx *ctx, const float *points, int N, float *xyz_out, float *centroid, float *scale,
                       void *stream);

/* farthest_point_sample of xyz [B, N, 3] from start [B] i32 (the reference
 * draws it) into idx [B, S] i32:  dist = 1e10 for every point, far = start;
 * S times: emit far; dist = min(dist, d2(x, x[far])); far = the arg-max of
 * dist, the lowest index among equal values. */
int ps_cloud_fps(ps_ctx *ctx, const float *xyz, int N, const int32_t *start, int S, int32_t *idx, void *stream);

/* query_ball_point: group_idx [B, S, nsample] i32 = per centre
 * xyz[centre_idx[b, s]] the first nsample indices, in ascending order, whose
 * d2 to the centre is not > (float)(radius * radius) (the product in f64, as
 * the reference compares with radius ** 2); fewer than nsample are padded with
 * the first.  No sort and no distance matrix. */
int ps_cloud_ball_query(ps_ctx *ctx, const float *xyz, int N, const int32_t *centre_idx, int S, double radius,
                        int nsample, int32_t *group_idx, void *stream);

/* The gathers and the centring, in the layout and channel order of
 * PointNetSetAbstractionMsg.forward before its permute:
 * out [B, S, nsample, D + 3] = feats[group_idx] (feats [B, N, D] f32, NULL
 * with D = 0) followed by xyz[group_idx] - xyz[centre_idx];
 * new_xyz [B, S, 3] = xyz[centre_idx], may be NULL. */
int ps_cloud_group(ps_ctx *ctx, const float *xyz, const float *feats, int N, int D, const int32_t *centre_idx, int S,
                   const int32_t *group_idx, int nsample, float *out, float *new_xyz, void *stream);

/* One radius of ps_cloud_set_abstraction: group_idx [B, S, nsample] i32 and
 * grouped [B, S, nsample, D + 3] f32 (may be NULL: indices only). */
typedef struct {
    double radius;
    int32_t nsample;
    int32_t *group_idx;
    float *grouped;
} ps_cloud_scale;

/* The first set-abstraction layer's sampling and grouping in one call:
 * normalise (if `normalize`: xyz, centroid, scale as ps_cloud_normalize; else
 * the cloud is `points` itself and the three may be NULL), ps_cloud_fps into
 * fps_idx [B, S], then for each of n_scales scales (HOST array) the ball query
 * around the sampled points and the group, the scales sharing one walk over
 * the points; new_xyz [B, S, 3] may be NULL.  Every value equals the
 * composition of the four calls above bit for bit.  No workspace. */
int ps_cloud_set_abstraction(ps_ctx *ctx, const float *points, const float *feats, int N, int D, const int32_t *start,
                             int S, const ps_cloud_scale *scales, int n_scales, int normalize, float *xyz,
                             float *centroid, float *scale, int32_t *fps_idx, float *new_xyz, void *stream);

/* --- PointNet++ feature propagation: 3-NN interpolation --- */

/* The interpolation inside PointNetFeaturePropagation.forward
 * (pointnet2_utils.py:276-310), the step between the learned layers of every
 * segmentation and keypoint model (fp3, fp2, fp1), for the context's B clouds:
 * xyz1 [B, N, 3] f32 the dense points, xyz2 [B, S, 3] f32 the coarse points,
 * points2 [B, S, D2] f32 the coarse features, points1 [B, N, D1] f32 the dense
 * features (NULL with D1 = 0).  No distance matrix and no sort.
 *
 * Per dense point n, in f32 with every product, sum and quotient rounded (no
 * fused multiply-add, correctly rounded division):
 *   d2_j      = the squared distance above of xyz1[n] and xyz2[j], every j;
 *   i_0..i_2  = the three smallest d2 in ascending order, the lowest index
 *               first among equal values;
 *   w_k       = 1.0f / (d2_k + 1e-8f);   norm = (w_0 + w_1) + w_2;
 *   weight_k  = w_k / norm;
 *   interp[c] = (points2[i_0][c] * weight_0 + points2[i_1][c] * weight_1)
 *               + points2[i_2][c] * weight_2.
 * S = 1 is the reference's repeat: idx = (0, 0, 0), weight = (1, 0, 0) and
 * interp = points2[b, 0] itself.  S = 2 is refused, as the reference raises
 * there.  The three indices of a cloud whose distances are all finite are
 * distinct; a distance that is not finite never displaces an index, so every
 * index written is inside 0..S-1 whatever the input.
 *
 * Limits (PS_ERR_ARG, nothing launched, outputs untouched): a NULL required
 * pointer, N outside 1..PS_CLOUD_MAX_DENSE_POINTS, S outside
 * 1..PS_CLOUD_MAX_POINTS or S = 2, D2 outside 1..PS_CLOUD_MAX_PROP_FEATURES,
 * D1 outside 0..PS_CLOUD_MAX_PROP_FEATURES, D1 != 0 without points1 (and the
 * reverse).  Outputs are addressed with 64-bit offsets. */
#define PS_CLOUD_MAX_PROP_FEATURES 2048
#define PS_CLOUD_MAX_DENSE_POINTS 1048576 /* 2^20 */

/* idx [B, N, 3] i32 and weight [B, N, 3] f32 of every dense point. */
int ps_cloud_three_nn(ps_ctx *ctx, const float *xyz1, int N, const float *xyz2, int S, int32_t *idx, float *weight,
                      void *stream);

/* out [B, N, D1 + D2] = points1 followed by interp, from idx and weight as
 * ps_cloud_three_nn writes them: the layout and channel order of forward
 * before its final permute.  An idx read from device memory is clamped into
 * 0..S-1, as the group entry points clamp theirs.  With S = 1 idx and weight
 * are not read. */
int ps_cloud_interpolate(ps_ctx *ctx, const float *points1, int D1, const float *points2, int D2, int N, int S,
                         const int32_t *idx, const float *weight, float *out, void *stream);

/* Both in one launch: a workgroup finds the 3-NN of its dense points, keeps
 * idx and weight on chip and writes those points' rows of out.  idx and
 * weight may be NULL (not written).  Every value equals the composition of
 * the two calls above bit for bit.  No workspace. */
int ps_cloud_feature_propagation(ps_ctx *ctx, const float *xyz1, int N, const float *xyz2, int S,
                                 const float *points1, int D1, const float *points2, int D2, float *out,
                                 int32_t *idx, float *weight, void *stream);

/* --- PointNet++ shared MLP with max-pool, on the f32 matrix cores --- */

/* What every model of envs/inference/models/ does to the tensors above: the
 * loop F.relu(bn(conv(x))) over 1x1 convolutions followed by torch.max over
 * the neighbourhood (pointnet2_utils.py:196-200 and :253-257), the same loop
 * without the max (:312-314), and the head's conv1 / conv2 -- at inference,
 * with the batch norm folded into the weights by the caller
 * (pandasim.fold_batchnorm).  Weights, checkpoints, training, dropout and
 * log_softmax are not part of the library.
 *
 * A layer is W [c_out, c_in] f32 row-major (a conv weight with its trailing 1s
 * dropped), b [c_out] f32, and a relu flag; W and b are device memory, shared
 * by all clouds; the array of layers is HOST memory.  c_in of the first layer
 * is C0, of every other the c_out before it.
 *
 * Per row x [C0] and layer, in f32:
 *   y[o] = b[o];  for k = 0 .. c_in-1 ascending:  y[o] = fmaf(x[k], W[o][k], y[o]);
 *   if relu:  y[o] = y[o] > 0 ? y[o] : 0;
 * the next layer reads y.  One rounding per step, nothing wider in between:
 * the f32-input MFMA of gfx950 computes exactly this chain from its C operand,
 * so the accumulators start as the bias and k is never split.
 * With group size G, output row g is the element-wise maximum over rows
 * g G .. g G + G - 1 of the last layer's y; G = 1 is no pooling.
 * Comparisons are by value (-0 equals +0: which zero is written is
 * unspecified).  The result for an input, weight or bias that is not finite
 * is unspecified.
 *
 * Limits (PS_ERR_ARG, nothing launched, outputs untouched): a NULL required
 * pointer (a layer's W or b included), n_layers outside
 * 1..PS_CLOUD_MLP_MAX_LAYERS, C0 outside 1..PS_CLOUD_MAX_PROP_FEATURES + 3, a
 * c_out outside 1..PS_CLOUD_MLP_MAX_HIDDEN (the last layer's:
 * 1..PS_CLOUD_MLP_MAX_LAST), R < 1, G < 1, R not a multiple of G, out_offset
 * < 0, out_stride < out_offset + the last c_out.  Outputs are addressed with
 * 64-bit offsets. */
#define PS_CLOUD_MLP_MAX_LAYERS 4
#define PS_CLOUD_MLP_MAX_HIDDEN 512 /* a 32-row tile's two live activations stay in LDS */
#define PS_CLOUD_MLP_MAX_LAST 1024

typedef struct {
    const float *W; /* [c_out, c_in] */
    const float *b; /* [c_out] */
    int32_t c_out;
    int32_t relu;
} ps_cloud_mlp_layer;

/* rows [B, R, C0] f32 -> out[b, g, out_offset + c] for g in 0..R/G-1 and c in
 * 0..C_n-1 (C_n the last c_out); the pitch of an out row is out_stride floats,
 * columns outside out_offset .. out_offset + C_n - 1 are not written. */
int ps_cloud_mlp(ps_ctx *ctx, const float *rows, int R, int C0, const ps_cloud_mlp_layer *layers, int n_layers, int G,
                 float *out, int64_t out_stride, int out_offset, void *stream);

/* The same on the rows of ps_cloud_group, gathered inside the kernel (the
 * grouped tensor never exists): row (s, k) is feats[group_idx[b, s, k]]
 * followed by xyz[group_idx[b, s, k]] - xyz[centre_idx[b, s]] (the subtraction
 * in f32, as there), so C0 = D + 3, R = S * K and G = K:
 * out[b, s, out_offset + c].  N and S as ps_cloud_group's, D in
 * 0..PS_CLOUD_MAX_PROP_FEATURES (feats NULL with D = 0), K >= 1; indices are
 * clamped as there.  Every value equals ps_cloud_group followed by
 * ps_cloud_mlp bit for bit.  The column offset is how the scales of
 * PointNetSetAbstractionMsg land in one [B, S, sum C_n] tensor. */
int ps_cloud_group_mlp(ps_ctx *ctx, const float *xyz, const float *feats, int N, int D, const int32_t *centre_idx,
                       int S, const int32_t *group_idx, int K, const ps_cloud_mlp_layer *layers, int n_layers,
                       float *out, int64_t out_stride, int out_offset, void *stream);

/* --- PointNet++ shared MLP with max-pool, bfloat16 on the matrix cores --- */

/* The same layers at reduced precision: operands rounded to bfloat16, products
 * and sums in f32 on the bf16 matrix cores (16 times the f32 MFMA's rate).  A
 * capability beside ps_cloud_mlp / ps_cloud_group_mlp, which are unchanged.
 *
 * Per row x [C0] and layer:
 *   xh[k] = bf16(x[k])                     round to nearest even from f32 (layer 0: the caller's f32
 *                                          rows; later layers: the previous layer's f32 y after its ReLU)
 *   Wh    = the layer's weights, bf16, rounded once on the host at upload
 *   y[o]  = b[o] + sum_k xh[k] * Wh[o][k]  b f32; products exact; accumulated in f32 on the matrix
 *                                          core, the order of the additions unspecified
 *   if relu:  y[o] = y[o] > 0 ? y[o] : 0
 * The last layer's y is written as f32 and is not rounded to bf16.  Pooling
 * over G rows, out_stride / out_offset, the -inf start of the maximum and the
 * clamping of the gather's indices are exactly ps_cloud_mlp's and
 * ps_cloud_group_mlp's.  In the gather variant the row is feats[group_idx]
 * then xyz[group_idx] - xyz[centre_idx]: the subtraction in f32 first, its
 * result then rounded to bf16.
 *
 * Unspecified: the result for an input, weight or bias that is not finite, and
 * wherever a nonzero operand's bf16 value is subnormal (whether the matrix core
 * or the conversion flushes it is not promised either way).
 * Guaranteed: the result is deterministic (the same bits on a repeated call),
 * and a cloud's bits do not depend on its position in the batch or on the
 * other clouds.
 *
 * A layer's W is [c_out, ldw] bf16 bit patterns (uint16), row-major, with
 * ldw = c_in rounded up to a multiple of 8 and columns c_in .. ldw-1 zero, at a
 * 16-byte aligned device address; b is [c_out] f32.  The array of layers is
 * HOST memory.  Limits and refusals (PS_ERR_ARG, nothing launched, outputs
 * untouched) are those of the f32 calls, and a W that is not 16-byte aligned. */
typedef struct {
    const uint16_t *W; /* [c_out, ldw] bf16 bits, row-major; ldw = c_in rounded up to a multiple of 8,
                          columns c_in..ldw-1 zero; 16-byte aligned */
    const float *b;    /* [c_out] f32 */
    int32_t c_out;
    int32_t relu;
} ps_cloud_mlp_bfloat_layer;

int ps_cloud_mlp_bfloat(ps_ctx *ctx, const float *rows, int R, int C0, const ps_cloud_mlp_bfloat_layer *layers,
                        int n_layers, int G, float *out, int64_t out_stride, int out_offset, void *stream);
int ps_cloud_group_mlp_bfloat(ps_ctx *ctx, const float *xyz, const float *feats, int N, int D,
                              const int32_t *centre_idx, int S, const int32_t *group_idx, int K,
                              const ps_cloud_mlp_bfloat_layer *layers, int n_layers, float *out, int64_t out_stride,
                              int out_offset, void *stream);

/* --- Point-cloud policy: waypoint decoding --- */

/* What envs/inference/inference_cls_off_rot.py: Inference.predict does after
 * the classifier (lines 68-107), for the context's B clouds in one launch, one
 * workgroup per cloud, every head row read once.
 *
 * head [B, N, ld] f32 is the network's last layer, one row per point: columns
 * 0 .. nc-1 the class logits, then the start offset (3), the end offset (3),
 * the start quaternion xyzw (4) and the end quaternion xyzw (4); columns from
 * nc + 14 on are not read.  xyz [B, N, 3] f32 are the normalised points,
 * centroid [B, 3] and scale [B] f32 the cloud's normalisation (both NULL: no
 * un-normalisation, the same values as centroid 0 and scale 1).  Bit c of
 * start_mask / end_mask set means class c belongs to the start / end set; the
 * reference's sets (classes 1 and 3, classes 2 and 3) are 0b1010 and 0b1100.
 * Set 0 below is the start set, set 1 the end set.
 *
 *   Label.      best = logit[0], label = 0; for c = 1 .. nc-1 ascending:
 *               if logit[c] > best, best = logit[c] and label = c.  The lowest
 *               index wins a tie; a NaN logit never wins.  (The one deviation:
 *               the reference takes the max of softmax(log_softmax(logits)),
 *               whose roundings can merge two close logits into a tie.)
 *   Waypoint.   (the mean over the set's points of (xyz - offset)) * scale +
 *               centroid.  Each difference is taken in f64 from the f32
 *               operands, the sums are f64 in a fixed order (thread t of the
 *               T = 1024 of a workgroup takes points t, t + T, ... ascending;
 *               the T partial sums are added by halving in LDS: partial t takes
 *               partial t + h for h = T/2, T/4, ... 1), the mean, the product
 *               and the sum with the centroid are f64, and the result is
 *               rounded to f32 once.  No atomics: the bits of cloud b depend
 *               on nothing but cloud b's inputs.
 *   Quaternion. The head's quaternion of the set at the lowest point index in
 *               the set (the reference's np.union1d(...)[0]), each component
 *               divided in f32 by the norm, the norm being the f64 square root
 *               of the f64 sum of squares rounded to f32.  A zero quaternion
 *               gives NaN, as in the reference.
 *   Euler.      scipy's 'xyz' (extrinsic) in degrees of that normalised
 *               quaternion, evaluated in f64 and rounded to f32:
 *               roll  = atan2(2 (w x + y z), 1 - 2 (x x + y y)),
 *               pitch = asin(clamp(2 (w y - z x), -1, 1)),
 *               yaw   = atan2(2 (w z + x y), 1 - 2 (y y + z z)).
 *   Empty set.  The reference raises.  Here counts = 0, first_idx = -1 and that
 *               set's waypoint, quaternion and Euler angles are NaN; nothing is
 *               left unwritten.
 *
 * Outputs: waypoints [B, 2, 3] f32, quats [B, 2, 4] f32 (normalised xyzw),
 * euler_deg [B, 2, 3] f32, counts [B, 2] i32 (the sets' sizes), labels [B, N]
 * i32 (may be NULL), first_idx [B, 2] i32 (the lowest point index of each set
 * or -1; may be NULL).
 *
 * Limits (PS_ERR_ARG, nothing launched, outputs untouched): a NULL required
 * pointer, N outside 1..PS_CLOUD_MAX_DENSE_POINTS, nc outside
 * 2..PS_CLOUD_DECODE_MAX_CLASSES, ld outside nc + 14 .. PS_CLOUD_DECODE_MAX_LD,
 * a mask that is zero or has a bit at or above nc, centroid and scale not both
 * present or both NULL.  Inputs are addressed with 64-bit offsets. */
#define PS_CLOUD_DECODE_MAX_CLASSES 16
#define PS_CLOUD_DECODE_MAX_LD 4096

int ps_cloud_decode_waypoints(ps_ctx *ctx, const float *head, int N, int ld, int nc, const float *xyz,
                              const float *centroid, const float *scale, uint32_t start_mask, uint32_t end_mask,
                              float *waypoints, float *quats, float *euler_deg, int32_t *counts, int32_t *labels,
                              int32_t *first_idx, void *stream);

/* --- Point-cloud policy: demonstration labels and losses --- */

/* The ground-truth side of the policy, forward only: the per-point targets a
 * demonstration gives (task_classes/generate_combined_dset.py:422-484, record,
 * with the normalisation of data_utils/PourDataLoader_cls_off.py:43-45) and the
 * value of the reference's losses on them (models/model_cls_off_rot.py:63-79).
 * Both work on the context's B clouds of N points, ordered on `stream`; all
 * pointers are device memory, addressed with 64-bit offsets.  No atomics on
 * floating-point values and nothing shared between clouds: the bits of cloud
 * b depend on nothing but cloud b's inputs.
 *
 * ps_cloud_waypoint_labels is the inverse of ps_cloud_decode_waypoints: its
 * 14 target columns are the columns the head carries behind its logits.
 *
 * Inputs.  points [B, N, 3] f32 the world points, xyz [B, N, 3] f32 the
 * normalised ones, centroid [B, 3] and scale [B] f32 as ps_cloud_normalize
 * wrote them, waypoints [B, 2, 3] f32 in the world (start, then end), quats
 * [B, 2, 4] f32 xyzw (written through unchanged), radius (the reference's is
 * 0.125), count [B] i32 or NULL (ps_point_cloud's M_b).  Set 0 below is the
 * start set, set 1 the end set.
 *
 *   Distance.   d2(p, w), the f32 squared distance above, of the world point
 *               and the world waypoint.  r2 = (float)radius * (float)radius,
 *               one rounded f32 product, computed on the host.  The point is
 *               in set k iff d2(p, w_k) <= r2: not strictly, as sklearn's
 *               radius_neighbors; a NaN distance is in no set.
 *   Class.      0 in neither set, 1 in the start set only, 2 in the end set
 *               only, 3 in both.
 *   Waypoint.   wn_k = (w_k - centroid) / scale per component in f32, both
 *               operations rounded: ps_cloud_normalize's expression, so a
 *               waypoint equal to a cloud point normalises to that point's xyz
 *               bit for bit.
 *   Targets.    The offset of set k is xyz - wn_k (f32) where the point is in
 *               set k, else 0; the quaternion of set k is quats[b, k] where
 *               the point is in set k, else 0.  A point of class 3 carries
 *               both offsets, which is what Inference.predict's union1d reads
 *               back.  (The one deviation: record()'s own three-column offsets
 *               array, which predates the six-column head, leaves the points
 *               of class 3 at zero.)
 *   Zero scale. A cloud whose scale is not > 0 gets zero offsets, not NaN;
 *               classes and quaternions as above.
 *   Empty.      With count given, a cloud whose count is 0 gets cls -1 at
 *               every point and zeros in its target columns.
 *
 * Outputs.  cls [B, N] i32; target [B, N, ld] f32, of which the columns
 * out_offset .. out_offset + 13 are written (start offset 3, end offset 3,
 * start quaternion 4, end quaternion 4) and the others left.
 *
 * Limits (PS_ERR_ARG, nothing launched, outputs untouched): a NULL required
 * pointer, N outside 1..PS_CLOUD_MAX_DENSE_POINTS, a radius that is not
 * positive and finite, out_offset < 0 or out_offset + 14 > ld, ld above
 * PS_CLOUD_LABEL_MAX_LD. */
#define PS_CLOUD_LABEL_MAX_LD 4096
#define PS_CLOUD_LABEL_COLUMNS 14

int ps_cloud_waypoint_labels(ps_ctx *ctx, const float *points, const float *xyz, const float *centroid,
                             const float *scale, const float *waypoints, const float *quats, double radius,
                             const int32_t *count, int N, int32_t *cls, float *target, int ld, int out_offset,
                             void *stream);

/* The forward value of the reference's losses (F.nll_loss on the class
 * log-softmax, nn.L1Loss on the offsets and quaternions) as per-cloud sums,
 * with the counts that turn them into means, and the accuracy's.
 *
 * Inputs.  head [B, N, ld] f32 with nc classes, as ps_cloud_decode_waypoints
 * takes it; cls [B, N] i32 the true classes; target [B, N, ld_t] f32 whose
 * columns target_offset .. target_offset + 13 are ps_cloud_waypoint_labels';
 * start_mask / end_mask as ps_cloud_decode_waypoints takes them, here applied
 * to the TRUE class.
 *
 *   Skipped.    A point whose cls is outside 0..nc-1 is skipped everywhere:
 *               that is how -1 means "ignore".
 *   NLL.        Of a point: the logits widened to f64; m = x[0], and for
 *               c = 1 .. nc-1 ascending m = x[c] if x[c] > m;
 *               nll = (m + log(sum over c ascending of exp(x[c] - m))) - x[cls].
 *               A NaN logit makes that cloud's NLL sum NaN and nothing else.
 *   L1.         |head - target| in f64 from the f32 operands (exact), summed
 *               over the 3 (4) offset (quaternion) columns of set k at each
 *               point whose true class is in set k.
 *   Prediction. ps_cloud_decode_waypoints' Label rule.
 *   Sums.       Every f64 sum in ps_cloud_decode_waypoints' fixed order: thread
 *               t of T = 1024 takes points t, t + T, ... ascending (a point's
 *               columns ascending), the T partial sums are added by halving.
 *
 * Outputs.  sums [B, 5] f64: the NLL, |d| of the start offsets, of the end
 * offsets, of the start quaternions, of the end quaternions.  counts [B, 4]
 * i32: the labelled (not skipped) points, those whose true class is in the
 * start set, in the end set, and those whose predicted class equals cls.
 * confusion [B, nc, nc] i32 or NULL: true class x predicted class.
 *
 * Limits (PS_ERR_ARG, nothing launched, outputs untouched): a NULL required
 * pointer, N outside 1..PS_CLOUD_MAX_DENSE_POINTS, nc outside
 * 2..PS_CLOUD_DECODE_MAX_CLASSES, ld outside nc + 14 .. PS_CLOUD_DECODE_MAX_LD,
 * target_offset < 0 or target_offset + 14 > ld_t, ld_t above
 * PS_CLOUD_LABEL_MAX_LD, a mask that is zero or has a bit at or above nc. */
int ps_cloud_policy_loss(ps_ctx *ctx, const float *head, int N, int ld, int nc, const int32_t *cls,
                         const float *target, int ld_t, int target_offset, uint32_t start_mask, uint32_t end_mask,
                         double *sums, int32_t *counts, int32_t *confusion, void *stream);

/* --- Point-cloud policy: keypoint conditioning --- */

/* The fourth feature channel of the reference's inp_dim = 7 policies
 * (run_policy.py:202-285, take_rgbd: pix2pix_neighborhood, deproject,
 * point2point_neighborhood), with the colours, as the feature rows the network
 * takes -- for the context's B clouds in one launch, without a depth image or
 * any per-pixel array.
 *
 * Inputs.  state, vis and target_poses (device [B, 2, 7] f32 or NULL) as
 * ps_point_cloud takes them; view: HOST, the keypoint view; keypoints
 * [B, n_kp, 2] i32 device, (column, row) in that view; radius in pixels;
 * threshold in metres; values [n_kp] f32 HOST; points [B, K, 3] f32 device;
 * colors [B, K, 3] u8 device or NULL; count [B] i32 device or NULL.
 *
 *   Patch.     The integer offsets (dx, dy) with dx^2 + dy^2 <= radius^2, slot
 *              order dx ascending, then dy ascending; P is their number (1, 29
 *              and 197 for radius 0, 3 and 8).  Slot s of keypoint k is pixel
 *              (column + dx, row + dy).  A slot whose pixel lies outside the
 *              image is skipped, so a keypoint whose whole disc lies outside
 *              marks nothing; and every slot of a keypoint with a negative
 *              coordinate is skipped, whatever the radius: that is how a
 *              caller says "absent" without a host synchronisation.
 *   Target.    The world point of an in-image slot: ps_deproject_pixels of that
 *              pixel on ps_render's depth of the view, bit for bit (the pixel's
 *              ray is cast inside the kernel), f64.  No depth or workspace
 *              filter, as PyBullet.deproject has none: a background pixel
 *              gives its point on the far plane.
 *   Distance.  With p the f32 point widened to f64 and t a target,
 *              d2 = (dx*dx + dy*dy) + dz*dz of the f64 differences, every
 *              operation rounded (no fused multiply-add).  m_k is the least d2
 *              over keypoint k's in-image slots (a d2 that is NaN never lowers
 *              it; +inf with no slot).  Keypoint k marks the point iff
 *              sqrt(m_k) < threshold, strictly and in f64.
 *   Value.     values[k] of the highest-index keypoint that marks the point,
 *              else 0.0f: a later keypoint overwrites an earlier one.
 *   Empty.     With count given, an env whose count is 0 (ps_point_cloud's
 *              empty cloud) gets all-zero feature rows.
 *
 * Outputs.  feats [B, K, ld] f32: with colors, columns out_offset ..
 * out_offset + 2 take the colour bytes as floats (0..255, exact) and column
 * out_offset + 3 the value; without, column out_offset takes the value.  Other
 * columns are left.  targets [B, n_kp, P, 3] f64 or NULL: every slot's target,
 * NaN for a slot outside the image.
 *
 * Limits (PS_ERR_ARG, nothing launched, outputs untouched): a NULL ctx, state,
 * view, vis, keypoints, values, points or feats, n_kp outside
 * 1..PS_CLOUD_KEYPOINT_MAX, radius outside 0..PS_CLOUD_KEYPOINT_MAX_RADIUS, a
 * threshold that is not positive and finite, an empty image or one of 2^31
 * pixels or more, K outside 1..PS_CLOUD_MAX_DENSE_POINTS, out_offset < 0, the
 * written columns beyond ld, ld above PS_CLOUD_KEYPOINT_MAX_LD. */
#define PS_CLOUD_KEYPOINT_MAX 4
#define PS_CLOUD_KEYPOINT_MAX_RADIUS 8 /* 4 * 197 targets of 24 B in LDS */
#define PS_CLOUD_KEYPOINT_MAX_LD 4096

int ps_cloud_keypoint_features(ps_ctx *ctx, const void *state, const ps_cloud_view *view, int width, int height,
                               const ps_visual *vis, const float *target_poses, const int32_t *keypoints, int n_kp,
                               int radius, double threshold, const float *values, const float *points,
                               const uint8_t *colors, const int32_t *count, int K, float *feats, int ld,
                               int out_offset, double *targets, void *stream);

/* --- Device-resident HER replay --- */

/* stable-baselines3's HerReplayBuffer for the context's B envs
 * (examples/train_push.py: DDPG(..., replay_buffer_class=HerReplayBuffer); the
 * env's compute_reward, core.py:226, is what it relabels with), in one
 * caller-owned device buffer: one launch stores a step of all envs, one call
 * samples a batch with the `future` or `final` hindsight goals and their
 * rewards recomputed, without a host synchronisation.  The host counts the
 * stores (n_stores) and passes scalars; no device counter is read back.
 *
 *   Ring.      capacity = T time slots of B envs.  A store writes slot
 *              pos = n_stores mod T of every env; stored = min(n_stores, T).
 *              A transition is one row of row_floats 32-bit words, padded to a
 *              multiple of 16 bytes, rows laid out [T][B][row]: obs[O], ag[G],
 *              dg[G], action[A], next_obs[O], next_ag[G], reward (f32),
 *              terminated (0 / 1 in a 32-bit word) and ep_end (i32: the slot of
 *              the last transition of the row's episode, -1 while it runs), at
 *              the word offsets ps_replay_layout names.  Beside the ring, per
 *              env: cur_len (i32; slots of the running episode, saturating at
 *              T) and the pending obs / ag / dg of the transition that the next
 *              store completes (rows of pending_floats words, [B][pending]).
 *   begin.     After a reset: records the pending observation of the masked
 *              envs (all with mask NULL).  A masked env with cur_len > 0 (a
 *              reset in mid-episode) has its running episode closed at its last
 *              stored slot, (pos_next - 1) mod T, as an episode's end below;
 *              then cur_len = 0.
 *   store.     Per env b: (1) slot pos takes the pending obs / ag / dg, the
 *              action, next_obs = final_obs[b], next_ag = final_ag[b] (obs[b] and
 *              ag[b] with final_obs NULL: auto-reset off), reward, terminated and
 *              ep_end = -1; (2) cur_len = min(cur_len + 1, T); (3) with
 *              terminated | truncated, ep_end of the last cur_len slots (from
 *              pos backwards, mod T) becomes pos, then cur_len = 0; (4) pending
 *              becomes obs / ag / dg.  ps_step leaves the pre-reset observation
 *              of every env in final_obs, so the last transition of an episode
 *              never holds the next episode's first observation.  An episode
 *              longer than T overwrites its own oldest slots; cur_len
 *              saturates, so the back-fill never walks more than T slots and
 *              every T >= 1 is legal.
 *   Valid.     Env b has v_b = stored - cur_len[b] valid transitions: the v_b
 *              oldest slots from oldest = (pos_next - stored) mod T, the j-th
 *              at slot (oldest + j) mod T; each has ep_end >= 0.  V is the sum
 *              of v_b and P the inclusive prefix sum of v over the envs.
 *   sample.    For sample i of M, in integers only (u64, wrapping):
 *                mix(z): z += 0x9E3779B97F4A7C15;
 *                        z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                        z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
 *                h = mix(mix(seed) ^ draw); w_k = mix(h ^ (4 i + k)), k = 0, 1, 2
 *                r = mulhi64(w_0, V)                the rank among the valid
 *                b = the least env with P[b] > r; j = r - (P[b] - v_b)
 *                t = (oldest + j) mod T
 *                relabel = (w_1 >> 32) < her_threshold
 *                n = ((ep_end[t, b] - t) mod T) + 1
 *                future: g = (t + mulhi64(w_2, n)) mod T;  final: g = ep_end[t, b]
 *              obs, ag, action, next_obs, next_ag and terminated are those of
 *              slot (t, b).  Not relabelled, dg and reward are the stored ones
 *              and goal_slot = -1; relabelled, dg = next_ag[g, b], goal_slot = g
 *              and reward is the task's compute_reward of (next_ag[t, b], dg) in
 *              ps_compute_reward's f32 / f32 arithmetic.  success is is_success
 *              of (next_ag[t, b], dg) of every sample, in that arithmetic.
 *              mulhi64's bias is below V / 2^64; there is no rejection.  With
 *              V = 0 every output is zero, except env_idx = slot = goal_slot =
 *              -1.  n_valid[0] = V.  The same (seed, draw, buffer) gives the
 *              same batch; a caller counts draw up per call.
 *
 * The caller's buffer is ps_replay_layout.bytes long and 16-byte aligned (rows
 * and pending rows are moved by 128-bit words; every section of the layout
 * starts at a multiple of 256 bytes).  pos, pos_next and stored must be those
 * of the buffer's own history of stores: the range checks below cannot tell a
 * consistent pair that belongs to another history, and with such scalars a
 * sample's indices are unspecified -- the kernel keeps them inside the ring
 * (a slot index is clamped to 0..T-1, an ep_end outside 0..T-1 counts as the
 * slot itself), so nothing is read out of bounds, and nothing else is promised.
 *
 * The buffer holds the prefix sum's workspace too, so ps_replay_sample writes
 * that part of an otherwise read buffer, and two samples of one buffer must
 * not run concurrently.  Every call is ordered on the caller's stream: no
 * synchronisation, no default-stream work.  Limits (PS_ERR_ARG before anything
 * is enqueued, the buffer untouched): NULL ctx, replay or required pointer; a
 * replay pointer that is not 16-byte aligned;
 * capacity outside 1..PS_REPLAY_MAX_CAPACITY or more than PS_REPLAY_MAX_ENVS
 * envs; pos or pos_next outside 0..capacity-1; stored outside 0..capacity (and
 * pos_next != stored while stored < capacity); stored = 0 on sample; M outside
 * 1..PS_REPLAY_MAX_BATCH; an unknown strategy; her_threshold > 2^32. */
#define PS_REPLAY_MAX_CAPACITY (1 << 20)
#define PS_REPLAY_MAX_ENVS (1 << 20) /* one second-level scan block of 1 024 first-level blocks */
#define PS_REPLAY_MAX_BATCH (1LL << 27)
enum { PS_REPLAY_FUTURE = 0, PS_REPLAY_FINAL = 1 };

/* Byte offsets from the replay pointer and word offsets within a row. */
typedef struct ps_replay_layout {
    int64_t bytes; /* of the whole buffer */
    int64_t ring_offset, cur_len_offset, pending_offset, prefix_offset, block_sum_offset;
    int32_t capacity, num_envs, row_floats, pending_floats;
    int32_t obs_dim, goal_dim, action_dim;
    int32_t off_obs, off_ag, off_dg, off_action, off_next_obs, off_next_ag, off_reward, off_terminated, off_ep_end;
} ps_replay_layout;

/* Outputs of a sample, device pointers: obs [M, O], ag / dg / next_ag [M, G],
 * action [M, A], next_obs [M, O], reward [M] f32, terminated / success /
 * relabelled [M] u8, env_idx / slot / goal_slot [M] i32, n_valid [1] i64.  Any
 * may be NULL except obs, action and dg. */
typedef struct ps_replay_batch {
    float *obs, *ag, *dg, *action, *next_obs, *next_ag, *reward;
    uint8_t *terminated, *success, *relabelled;
    int32_t *env_idx, *slot, *goal_slot;
    int64_t *n_valid;
} ps_replay_batch;

/* needs no GPU */
int ps_replay_layout_of(const ps_ctx *ctx, int capacity, ps_replay_layout *out);
/* the whole buffer zero, every ep_end = -1 */
int ps_replay_init(ps_ctx *ctx, void *replay, int capacity, void *stream);
int ps_replay_begin(ps_ctx *ctx, void *replay, int capacity, int pos_next, int stored, const float *obs,
                    const float *ag, const float *dg, const uint8_t *mask, void *stream);
int ps_replay_store(ps_ctx *ctx, void *replay, int capacity, int pos, const float *actions, const float *obs,
                    const float *ag, const float *dg, const float *final_obs, const float *final_ag,
                    const float *reward, const uint8_t *terminated, const uint8_t *truncated, void *stream);
int ps_replay_sample(ps_ctx *ctx, const void *replay, int capacity, int pos_next, int stored, int strategy,
                     uint64_t seed, uint64_t draw, uint64_t her_threshold, int64_t M, const ps_replay_batch *out,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif
