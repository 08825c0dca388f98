// ps_cloud_math.h — the arithmetic the point-cloud units share
// (group_kernels.hip, propagate_kernels.hip, decode_kernels.hip,
// label_kernels.hip): the squared distance that include/pandasim.h fixes, the
// opaque copy that keeps its products rounded, the clamp of an index read from
// device memory, and the arg-max rule of the policy's class logits.
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

// the Label rule of include/pandasim.h (decode_kernels.hip, label_kernels.hip):
// the class of the largest logit, the lowest index among equal ones; a NaN
// logit never wins
PS_D int cloud_argmax(const float *row, int nc) {
    float best = row[0];
    int label = 0;
    for (int c = 1; c < nc; c++) {
        const float v = row[c];
        if (v > best) {
            best = v;
            label = c;
        }
    }
    return label;
}

}  // namespace
