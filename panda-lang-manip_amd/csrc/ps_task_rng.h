// ps_task_rng.h — the per-env random stream under the task layer (ps_task.h):
//   numpy SeedSequence + PCG64 + Generator.uniform (gymnasium seeding,
//   panda_gym/envs/core.py:244), the opaque() rounding barriers of the fp64
//   task arithmetic, and getEulerFromQuaternion.  Needs ps_common.h only.
// Integer work is exact; the fp64 arithmetic uses explicit round-to-nearest
// intrinsics (no FMA contraction) so results are bit-identical to numpy.
#pragma once

#include "ps_common.h"

namespace ps {

struct Pcg {
    uint64_t sh, sl, ih, il;  // state hi/lo, increment hi/lo
};

PS_D void pcg_step(Pcg &r) {
    const uint64_t MH = 0x2360ED051FC65DA4ULL, ML = 0x4385DF649FCCF645ULL;
    uint64_t lo = r.sl * ML;
    uint64_t hi = __umul64hi(r.sl, ML) + r.sl * MH + r.sh * ML;
    uint64_t nl = lo + r.il;
    uint64_t carry = nl < lo ? 1ULL : 0ULL;
    r.sh = hi + r.ih + carry;
    r.sl = nl;
}

PS_D uint64_t pcg_next(Pcg &r) {
    pcg_step(r);
    uint64_t x = r.sh ^ r.sl;
    unsigned rot = (unsigned)(r.sh >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

// Opaque barriers: hipcc contracts a*b+c into an FMA across inlined helper
// calls even under `#pragma clang fp contract(off)`; numpy rounds the product
// first.  An empty asm on the product keeps it a separate, rounded value.
PS_D double opaque(double x) {
    asm volatile("" : "+v"(x));
    return x;
}
PS_D float opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

PS_D double pcg_double(Pcg &r) { return __dmul_rn((double)(pcg_next(r) >> 11), 1.0 / 9007199254740992.0); }

// Generator.uniform: low + (high - low) * next_double
PS_D double uniform(Pcg &r, double lo, double hi) {
#pragma clang fp contract(off)
    double range = __dsub_rn(hi, lo);
    double u = pcg_double(r);
    return __dadd_rn(lo, opaque(__dmul_rn(range, u)));
}

// SeedSequence(seed).generate_state(4, uint64) -> pcg64_set_seed
PS_D Pcg pcg_seed(uint64_t seed) {
    const uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu;
    const uint32_t MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
    uint32_t e0 = (uint32_t)seed, e1 = (uint32_t)(seed >> 32);
    int nent = (seed >> 32) ? 2 : 1;
    uint32_t pool[4], hc = INIT_A;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t v = (i == 0 ? e0 : (i == 1 && nent == 2 ? e1 : 0u)) ^ hc;
        hc *= MULT_A;
        v *= hc;
        v ^= v >> 16;
        pool[i] = v;
    }
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
        for (int d = 0; d < 4; d++)
            if (s != d) {
                uint32_t v = pool[s] ^ hc;
                hc *= MULT_A;
                v *= hc;
                v ^= v >> 16;
                uint32_t r = MIX_L * pool[d] - MIX_R * v;
                r ^= r >> 16;
                pool[d] = r;
            }
    uint32_t w[8], hb = INIT_B;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t v = pool[i & 3] ^ hb;
        hb *= MULT_B;
        v *= hb;
        v ^= v >> 16;
        w[i] = v;
    }
    uint64_t v0 = (uint64_t)w[0] | ((uint64_t)w[1] << 32), v1 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    uint64_t v2 = (uint64_t)w[4] | ((uint64_t)w[5] << 32), v3 = (uint64_t)w[6] | ((uint64_t)w[7] << 32);
    Pcg r;
    // inc = (initseq << 1) | 1 with initseq = v2:v3
    r.ih = (v2 << 1) | (v3 >> 63);
    r.il = (v3 << 1) | 1ULL;
    r.sh = 0;
    r.sl = 0;
    pcg_step(r);
    // state += initstate (v0:v1)
    uint64_t nl = r.sl + v1;
    r.sh = r.sh + v0 + (nl < r.sl ? 1ULL : 0ULL);
    r.sl = nl;
    pcg_step(r);
    return r;
}

// getEulerFromQuaternion (fp32)
PS_D V3 euler_from_quat(Q4 q) {
    float sqx = q.x * q.x, sqy = q.y * q.y, sqz = q.z * q.z, squ = q.w * q.w;
    float sarg = -2.0f * (q.x * q.z - q.w * q.y);
    if (sarg <= -0.99999f) return mk(0.0f, -0.5f * 3.14159265358979323846f, 2.0f * atan2f(q.x, -q.y));
    if (sarg >= 0.99999f) return mk(0.0f, 0.5f * 3.14159265358979323846f, 2.0f * atan2f(-q.x, q.y));
    return mk(atan2f(2.0f * (q.y * q.z + q.w * q.x), squ - sqx - sqy + sqz), asinf(sarg),
              atan2f(2.0f * (q.x * q.y + q.w * q.z), squ + sqx - sqy - sqz));
}

}  // namespace ps
