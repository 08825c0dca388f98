// ps_cloud_math.h — the arithmetic the point-cloud units share
// (group_kernels.hip, propagate_kernels.hip): the squared distance that
// include/pandasim.h fixes, the opaque copy that keeps its products rounded,
// and the clamp of an index read from device memory.
#pragma once

#include "ps_ctx.h"

namespace {

// an opaque copy: hipcc contracts a*b+c across inlined calls even under
// `fp contract(off)` (ps_task_rng.h); a product that went through here stays a
// rounded value of its own
PS_D float rounded(float x) {
    asm("" : "+v"(x));
    return x;
}

PS_D float dist2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (rounded(dx * dx) + rounded(dy * dy)) + rounded(dz * dz);
}

PS_D int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

}  // namespace
