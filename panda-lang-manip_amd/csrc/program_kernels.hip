// program_kernels.hip — the motion-program kernel (k_motion_program,
// ps_motion_program.h) of one scene: built once per (objects, shape) with
// -DPS_PROGRAM_NOBJ=n -DPS_PROGRAM_SHAPE=s (pandasim/build.py), as
// motion_kernels.hip is.  ps_motion_program (pandasim.hip) calls it.
#include "ps_motion_program.h"

#if !defined(PS_PROGRAM_NOBJ) || !defined(PS_PROGRAM_SHAPE)
#error "build with -DPS_PROGRAM_NOBJ=<objects> -DPS_PROGRAM_SHAPE=<shape>"
#endif

int PS_PROGRAM_LAUNCHER_NAME(PS_PROGRAM_NOBJ, PS_PROGRAM_SHAPE)(ps_ctx *c, void *state, void *plan,
                                                               const ps_program_args &prog, hipStream_t st) {
    KParams P = params_of(c, state);
    hipLaunchKernelGGL((k_motion_program<PS_PROGRAM_NOBJ, PS_PROGRAM_SHAPE>), grid_of(P.n, kBlock), dim3(kBlock), 0, st,
                       P, plan_view(c, plan), prog);
    return check_launch(c);
}
