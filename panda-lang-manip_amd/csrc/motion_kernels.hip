// motion_kernels.hip — the fused motion-primitive kernel (k_motion,
// ps_motion.h) of one scene: built once per (objects, shape) with
// -DPS_MOTION_NOBJ=n -DPS_MOTION_SHAPE=s (pandasim/build.py), as
// sim_kernels.hip is.  ps_motion_run (pandasim.hip) calls it.
#include "ps_motion.h"

#if !defined(PS_MOTION_NOBJ) || !defined(PS_MOTION_SHAPE)
#error "build with -DPS_MOTION_NOBJ=<objects> -DPS_MOTION_SHAPE=<shape>"
#endif

int PS_MOTION_LAUNCHER_NAME(PS_MOTION_NOBJ, PS_MOTION_SHAPE)(ps_ctx *c, void *state, void *plan, int max_steps,
                                                            hipStream_t st) {
    KParams P = params_of(c, state);
    hipLaunchKernelGGL((k_motion<PS_MOTION_NOBJ, PS_MOTION_SHAPE>), grid_of(P.n, kBlock), dim3(kBlock), 0, st, P,
                       plan_view(c, plan), max_steps);
    return check_launch(c);
}
