// ps_scene.h — what a substep works on: the scene and its objects (inertia,
// support points, closest points), the per-lane LDS / global-stash layout
// (MJStore), the contact row records and the solver's velocity-change types.
#pragma once

#include "ps_common.h"

namespace ps {

// ------------------------------------------------------------- the scene
// Objects: NOBJ dynamic bodies (0 Reach; 1 Push/PickAndPlace/Flip/Slide; 2
// Stack) of one SHAPE (SHAPE_BOX: cubes, isotropic inertia; SHAPE_CYL: the
// upright cylinder of Slide, anisotropic inertia).
constexpr int SHAPE_BOX = PS_SHAPE_BOX;
constexpr int SHAPE_CYL = PS_SHAPE_CYLINDER;

struct Scene {
    V3 base;
    V3 half;                 // box half extents; cylinder (radius, radius, half height)
    float mass, mass2, fric;  // object 1 / object 2 mass, lateral friction of the objects
    float table_cx, table_hx, table_hy;
    int has_table, has_plane;
};

struct Motors {
    float target[9], kp[9], kd[9], vel[9], imp[9];
};

struct Body {
    V3 pos;
    Q4 quat;
    V3 vel, omg;
};
typedef Body Cube;

// btBoxShape / btCylinderShapeZ::calculateLocalInertia (oracle object_inertia)
template <int SHAPE>
PS_D V3 local_inertia(const Scene &sc, float m) {
    if constexpr (SHAPE == SHAPE_CYL) {
        float r = sc.half.x, hh = sc.half.z;
        float t1 = m / 12.0f * (4.0f * hh * hh) + m / 4.0f * (r * r), t2 = m / 2.0f * (r * r);
        return mk(t1, t1, t2);
    } else {
        float lx = 2.0f * sc.half.x, ly = 2.0f * sc.half.y, lz = 2.0f * sc.half.z;
        return mk(m / 12.0f * (ly * ly + lz * lz), m / 12.0f * (lx * lx + lz * lz), m / 12.0f * (lx * lx + ly * ly));
    }
}

// per-substep body quantities: the world inverse inertia is a scalar for the
// isotropic cubes and a symmetric 3x3 for the cylinder
// two fp32 lanes of a v_pk_*_f32 instruction (the solver packs pairs of
// independent scalar operations into them)
typedef float f32x2 __attribute__((ext_vector_type(2)));

// mul(S3, V3) with rows x and y as v_pk_* pairs, for the solver loop's
// velocity updates: each lane computes what the scalar row compiles to there,
// fma(I_xz, v_z, fma(I_xx, v_x, I_xy v_y)) for row x, so the same bits
PS_D V3 mul_pk(const S3 &I, V3 v) {
#pragma clang fp contract(off)
    f32x2 xy = (f32x2){I.xy, I.yy} * (f32x2){v.y, v.y};
    xy = __builtin_elementwise_fma((f32x2){I.xx, I.xy}, (f32x2){v.x, v.x}, xy);
    xy = __builtin_elementwise_fma((f32x2){I.xz, I.yz}, (f32x2){v.z, v.z}, xy);
    return mk(xy.x, xy.y, fmaf(I.zz, v.z, fmaf(I.xz, v.x, I.yz * v.y)));
}
// the same product inside a `fp contract(off)` block: three products and two
// sums per row
PS_D V3 mul_pk_unfused(const S3 &I, V3 v) {
#pragma clang fp contract(off)
    const f32x2 xy = ((f32x2){I.xx, I.xy} * (f32x2){v.x, v.x} + (f32x2){I.xy, I.yy} * (f32x2){v.y, v.y}) +
                     (f32x2){I.xz, I.yz} * (f32x2){v.z, v.z};
    return mk(xy.x, xy.y, (I.xz * v.x + I.yz * v.y) + I.zz * v.z);
}

template <int SHAPE>
struct BodyDyn {
    M3 R;
    float inv_m, iI;
    S3 Ii;
    PS_D V3 inv_inertia(V3 v) const {
        if constexpr (SHAPE == SHAPE_CYL) return mul(Ii, v);
        else return v * iI;
    }
    // the solver loop's: rows x and y packed (mul_pk, mul_pk_unfused)
    PS_D V3 inv_inertia_pk(V3 v) const {
        if constexpr (SHAPE == SHAPE_CYL) return mul_pk(Ii, v);
        else return v * iI;
    }
    PS_D V3 inv_inertia_pk_unfused(V3 v) const {
        if constexpr (SHAPE == SHAPE_CYL) return mul_pk_unfused(Ii, v);
        else return v * iI;
    }
};

template <int SHAPE>
PS_D BodyDyn<SHAPE> body_dyn(const Scene &sc, const Body &b, float m) {
    BodyDyn<SHAPE> o;
    o.R = quat_to_mat(b.quat);
    o.inv_m = 1.0f / m;
    V3 I = local_inertia<SHAPE>(sc, m);
    o.iI = 1.0f / I.x;
    if constexpr (SHAPE == SHAPE_CYL) o.Ii = rotate_diag(o.R, 1.0f / I.x, 1.0f / I.y, 1.0f / I.z);
    return o;
}

PS_D bool ground_top(const Scene &sc, float x, float y, float &top) {
    if (sc.has_table && fabsf(x - sc.table_cx) <= sc.table_hx && fabsf(y) <= sc.table_hy) {
        top = (float)PM_TABLE_TOP;
        return true;
    }
    if (sc.has_plane) {
        top = (float)PM_PLANE_TOP;
        return true;
    }
    return false;
}

// support point v of the shape (object frame): box vertices, or cylinder rim
// points (bottom cap then top cap, PM_CYL_RIM_ORDER)
template <int SHAPE>
constexpr int num_support() { return SHAPE == SHAPE_CYL ? 2 * PM_CYL_RIM_POINTS : 8; }

template <int SHAPE, int V>
PS_D V3 support_point(const Scene &sc) {
    if constexpr (SHAPE == SHAPE_CYL) {
        constexpr int order[PM_CYL_RIM_POINTS] = PM_CYL_RIM_ORDER;
        constexpr int cap = V / PM_CYL_RIM_POINTS;
        constexpr int j = order[V % PM_CYL_RIM_POINTS];
        // cos/sin of multiples of 45 degrees, exact to float
        constexpr float cs[8] = {1.0f, 0.70710678118654752f, 0.0f, -0.70710678118654752f,
                                 -1.0f, -0.70710678118654752f, 0.0f, 0.70710678118654752f};
        constexpr float sn[8] = {0.0f, 0.70710678118654752f, 1.0f, 0.70710678118654752f,
                                 0.0f, -0.70710678118654752f, -1.0f, -0.70710678118654752f};
        return mk(sc.half.x * cs[j], sc.half.x * sn[j], cap ? sc.half.z : -sc.half.z);
    } else {
        return mk((V & 1) ? sc.half.x : -sc.half.x, (V & 2) ? sc.half.y : -sc.half.y,
                  (V & 4) ? sc.half.z : -sc.half.z);
    }
}

// closest point of the solid to `loc` (object frame): surface point cl,
// outward normal nl; returns the signed distance (negative inside)
template <int SHAPE>
PS_D float object_closest(const Scene &sc, V3 loc, V3 &cl, V3 &nl) {
    const V3 h = sc.half;
    if constexpr (SHAPE == SHAPE_CYL) {
        float r = h.x, hh = h.z;
        float rho = fast_sqrt(loc.x * loc.x + loc.y * loc.y);
        float zc = fminf(fmaxf(loc.z, -hh), hh);
        float irho = fast_rcp(rho);  // used only where rho > 1e-12
        float s = rho > r ? r * irho : 1.0f;
        cl = mk(loc.x * s, loc.y * s, zc);
        V3 dif = loc - cl;
        float dn = fast_norm(dif);
        if (dn > 1e-9f) {
            nl = dif * fast_rcp(dn);
            return dn;
        }
        float side = r - rho, cap = hh - fabsf(loc.z);
        if (side < cap) {
            nl = rho > 1e-12f ? mk(loc.x * irho, loc.y * irho, 0.0f) : mk(1.0f, 0.0f, 0.0f);
            cl = mk(nl.x * r, nl.y * r, cl.z);
            return -side;
        }
        nl = mk(0.0f, 0.0f, loc.z >= 0.0f ? 1.0f : -1.0f);
        cl.z = nl.z * hh;
        return -cap;
    } else {
        cl = mk(fminf(fmaxf(loc.x, -h.x), h.x), fminf(fmaxf(loc.y, -h.y), h.y), fminf(fmaxf(loc.z, -h.z), h.z));
        V3 dif = loc - cl;
        float dn = norm(dif);
        if (dn > 1e-9f) {
            nl = dif * (1.0f / dn);
            return dn;
        }
        float bx = h.x - fabsf(loc.x), by = h.y - fabsf(loc.y), bz = h.z - fabsf(loc.z);
        int ax = 0;
        float best = bx;
        if (by < best) { best = by; ax = 1; }
        if (bz < best) { best = bz; ax = 2; }
        float sg;
        if (ax == 0) { sg = loc.x >= 0.0f ? 1.0f : -1.0f; nl = mk(sg, 0, 0); cl.x = sg * h.x; }
        else if (ax == 1) { sg = loc.y >= 0.0f ? 1.0f : -1.0f; nl = mk(0, sg, 0); cl.y = sg * h.y; }
        else { sg = loc.z >= 0.0f ? 1.0f : -1.0f; nl = mk(0, 0, sg); cl.z = sg * h.z; }
        return -best;
    }
}

// btPlaneSpace1
PS_D void plane_space(V3 n, V3 &p, V3 &q) {
    if (fabsf(n.z) > 0.70710678118654752f) {
        float a = n.y * n.y + n.z * n.z, k = rsqrtf(a);
        p = mk(0.0f, -n.z * k, n.y * k);
        q = mk(a * k, -n.x * p.z, n.x * p.y);
    } else {
        float a = n.x * n.x + n.y * n.y, k = rsqrtf(a);
        p = mk(-n.y * k, n.x * k, 0.0f);
        q = mk(-n.z * p.y, n.z * p.x, a * k);
    }
}

constexpr int NG = PM_MAX_GROUND_CONTACTS;
constexpr int NR = PM_MAX_ROBOT_CONTACTS;
constexpr int NP = PM_MAX_PAIR_CONTACTS;
// LDS floats per lane: M^-1 J^T of the 3 rows of every gripper contact
// (108 floats x 256 lanes per CU = 108 KiB of the 160 KiB LDS at one wave per
// SIMD).
// Then 40 floats of per-substep values the PGS loop never reads (q, v1, the
// split-impulse position correction, object 1's pre-solve velocities and
// pose): they wait in LDS across the solve instead of holding registers.
constexpr int LDS_STASH_OFFSET = NR * 27;
constexpr int LDS_STASH_FLOATS = 40;
// Then the scenes with at most one object hold their contact cache (the
// object's ground rows and the gripper rows, 10 floats) in LDS across the
// control step's substeps: loaded from the state once per step and written
// back once (run_substeps), not read and written through L2 every substep.
constexpr int LDS_CACHE_OFFSET = LDS_STASH_OFFSET + LDS_STASH_FLOATS;
constexpr int LDS_CACHE_FLOATS = 10;
constexpr int LDS_FLOATS = LDS_CACHE_OFFSET + LDS_CACHE_FLOATS;
static_assert(LDS_FLOATS * 4 * 64 * 4 <= 160 * 1024, "four workgroups per CU");
// The one-lane kernels of these scenes (G == 1, at most one object) lay the
// M^-1 J^T rows out in 16-byte chunks, [chunk][lane][4] (MJStore::chunk), so
// the sweep fetches them with ds_read_b128: a slot's 27 floats padded to 28 =
// 7 chunks.  Lane l's chunk c is floats [256 c + 4 l, 256 c + 4 l + 4) of the
// workgroup's LDS, i.e. rows 4 c .. 4 c + 3 of the float-major grid, in other
// lanes' columns: rows [0, 112).  Their stash follows at row 112 without the
// split-impulse rows (31 floats: split_of rebuilds them from q, as for Stack),
// and the contact cache stays where it is.
constexpr int LDS_CHUNK_FLOATS = 28;
constexpr int LDS_CHUNKS = LDS_CHUNK_FLOATS / 4;
constexpr int LDS1_STASH_OFFSET = NR * LDS_CHUNK_FLOATS;
constexpr int LDS1_STASH_FLOATS = LDS_STASH_FLOATS - 9;
static_assert(LDS1_STASH_OFFSET + LDS1_STASH_FLOATS <= LDS_CACHE_OFFSET, "the one-lane stash below the contact cache");
// the one-lane solver of which scenes reads its gripper rows as chunks
template <int NOBJ, int G>
constexpr bool chunked_lds() {
    return G == 1 && NOBJ <= 1;
}
// Stack (two cubes) keeps in LDS the gripper rows' J (the slots the other
// scenes use for M^-1 J^T; the loop forms M^-1 J^T from the M^-1 registers)
// and both cubes' ground rows (r, rhs: 6 per contact; 1/den is rebuilt from r,
// cube_ground_dinv) instead of registers, where they spilled to scratch.  Its
// 40-float stash, object 1's pre-solve state and the box-box pair rows
// (dir[3], rA, rB, rhs, dinv: 21 per contact, read only while some lane of
// the wave has a pair contact; r x dir is rebuilt in the loop) sit in a global
// per-env buffer (GSTASH_FLOATS: the stash rows env-minor, the pair rows
// env-major so one lane pointer with immediate offsets reads them).  That is 156 LDS floats per lane = 39 KB per
// 64-lane workgroup: four workgroups per CU, one wave per SIMD, as the
// one-object scenes.
constexpr int LDS_GND_OFFSET = NR * 27;
constexpr int LDS_GND_FLOATS = 6;
constexpr int LDS_FLOATS_STACK = LDS_GND_OFFSET + 2 * NG * LDS_GND_FLOATS;
static_assert(LDS_FLOATS_STACK * 4 * 64 * 4 <= 160 * 1024, "four Stack workgroups per CU");
constexpr int PAIR_FLOATS = 21;
// Stack's global stash rows (env-minor): the stash without the split-impulse
// corrections (recomputed from q after the solve, split_of: 9 rows fewer) and
// object 1's pre-solve state.
constexpr int GSTASH_ROWS = LDS_STASH_FLOATS + 13 - 9;
constexpr int GSTASH_PAIR_OFFSET = GSTASH_ROWS;
// The pair and gripper rows of a slot an env does not use are never written:
// the solver, which runs a slot's rows while any lane of the wave has it,
// points the lanes without it at one all-zero block (GSTASH_ZERO_FLOATS, after
// the stash, zeroed at allocation: ensure_stash) -- exact no-op rows, one
// cache line for the whole wave.  Before, every env rewrote its unused slots
// as zeros every substep and the wave read 64 env-major rows per slot: most of
// Stack's HBM traffic (2.03 GB per launch at 65 536 envs, VERDICT r05 weak 3;
// ~2 % of envs have a box-box contact at a time).
constexpr int GSTASH_ZERO_FLOATS = 32;
// Stack: M^-1 J^T of the gripper slots' normal rows, env-major after the
// pair rows (9 floats per slot), computed with J at contact setup and loaded
// at the top of each sweep (object_normals), so a gripper normal updates dv
// with 9 FMAs instead of the 81 of M^-1 (J^T dl): 7.89 -> 7.60 ms per step at
// 65 536 envs.  The friction rows' 18 floats per slot the same way spilled
// 40-81 VGPRs and ran slower (8.12 ms for 2 slots, 8.76 for 4:
// profiles/r03j_variants_stack_grip_mj.log), so those keep the M^-1 product.
constexpr int GRIP_MJ_SLOTS = NR;
constexpr int GSTASH_GRIP_OFFSET = GSTASH_PAIR_OFFSET + NP * PAIR_FLOATS;
constexpr int GRIP_FLOATS = GRIP_MJ_SLOTS * 9;
constexpr int GSTASH_FLOATS = GSTASH_GRIP_OFFSET + GRIP_FLOATS;
template <int NOBJ>
constexpr int lds_floats() {
    return NOBJ == 2 ? LDS_FLOATS_STACK : LDS_FLOATS;
}

// object-ground contact: object-only rows; normal +z, friction dirs of
// planeSpace(+z) = (0,-1,0), (1,0,0).  The cylinder's I^-1 (r x dir) is rebuilt
// in the solver from its 3x3 inverse inertia rather than held per row.
struct GroundContact {
    V3 r;  // contact point - object COM
    float rhs[3], lam[3], dinv[3];
    int id;  // contact cache id: 1 + support point (0: no contact)
};

// object-object contact (Stack): A = incident body (+n), B = reference (-n)
struct PairContact {
    V3 dir[3], rA, rB;  // contact point - COM of object 0 (rA) and of object 1 (rB)
    float rhs[3], lam[3], dinv[3];
    bool a0;  // body A is object 0
};

// gripper contact: robot rows with explicit Jacobians (M^-1 J^T lives in LDS)
struct RobotContact {
    float J[3][9];
    V3 dir[3];
    V3 rn[3];  // object side: (pB - x_obj) x dir (zero when the contact is with the ground)
    float rhs[3], lam[3], dinv[3], mu;
    bool o1;   // the object is object 1 (Stack)
};

// per-lane view of the LDS rows: element (slot, row, k) at base[((slot*3 + row)*9 + k) * stride]
typedef __attribute__((address_space(3))) float lds_float;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
struct MJStore {
    lds_float *base;
    int stride;
    // the work lists' per-lane output rows (robot_candidates), stride kBlock:
    // in this lane's column (base + CW_OUT rows) unless the env's column is
    // shared by its group's lanes (shared_lds<G>)
    lds_float *cwo = nullptr;
    PS_D lds_float &at(int slot, int row, int k) const { return base[((slot * 3 + row) * 9 + k) * stride]; }
    PS_D lds_float &cache(int k) const { return base[(LDS_CACHE_OFFSET + k) * stride]; }
    PS_D lds_float &stash(int k) const { return base[(LDS_STASH_OFFSET + k) * stride]; }
    // The chunked mode (chunked_lds: one lane per env, one 64-lane wave per
    // workgroup, base = the workgroup's LDS + lane).  Chunk c of gripper slot
    // `slot` is 16 bytes per lane, contiguous over the lanes: a ds_read_b128
    // whose 16-lane groups each cover the 64 banks once (no conflicts).
    // A slot's chunks: 0-1 row 0's DoFs 0..7, 2-3 row 1's, 4-5 row 2's (the
    // pairs VelChange::apply takes, on even registers), 6 the rows' DoF 8
    // (x, y, z) and a pad.
    PS_D lds_f32x4 &chunk(int slot, int c) const {
        return ((lds_f32x4 *)(base + 3 * (int)threadIdx.x))[(slot * LDS_CHUNKS + c) * 64];
    }
    // row 0 of a slot (the normal's M^-1 J^T): chunks 0, 1 and 6
    PS_D void chunk_row(int slot, int, float m[9]) const {
        const f32x4 a = chunk(slot, 0), b = chunk(slot, 1), z = chunk(slot, 6);
        m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
        m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
        m[8] = z.x;
    }
    // rows 1 and 2 (the friction rows'): chunks 2..6
    PS_D void chunk_rows12(int slot, float m1[9], float m2[9]) const {
        const f32x4 a = chunk(slot, 2), b = chunk(slot, 3), c = chunk(slot, 4), d = chunk(slot, 5), z = chunk(slot, 6);
        m1[0] = a.x; m1[1] = a.y; m1[2] = a.z; m1[3] = a.w;
        m1[4] = b.x; m1[5] = b.y; m1[6] = b.z; m1[7] = b.w;
        m2[0] = c.x; m2[1] = c.y; m2[2] = c.z; m2[3] = c.w;
        m2[4] = d.x; m2[5] = d.y; m2[6] = d.z; m2[7] = d.w;
        m1[8] = z.y;
        m2[8] = z.z;
    }
    PS_D lds_float &stash1(int k) const { return base[(LDS1_STASH_OFFSET + k) * stride]; }
    // Stack: the stash in global memory ([GSTASH_PAIR_OFFSET][stride] floats, this env's column)
    // (wave-uniform base and stride, the lane's byte offset: global_* v_off, s[base])
    float *gst = nullptr;
    int64_t gst_stride = 0;
    uint32_t goff = 0;
    // Stack: this env's pair rows, env-major after the stash rows
    // ([stride][NP * PAIR_FLOATS]): one lane pointer plus immediate offsets
    __attribute__((address_space(1))) float *gpair = nullptr;
    PS_D float &gstash(int k) const {
        float *row = gst + k * gst_stride;
        asm("" : "+s"(row));  // no reassociation into a per-lane pointer (StateView::at)
        return *(float *)((char *)row + goff);
    }
    // Stack only: ground row c of cube c / NG, field k (r.xyz, rhs[3])
    PS_D lds_float &gnd(int c, int k) const { return base[(LDS_GND_OFFSET + c * LDS_GND_FLOATS + k) * stride]; }
    // Stack only (global stash): pair row c, field k (dir[3].xyz, r0.xyz, r1.xyz, rhs[3], dinv[3]);
    // dir is body A's (+n), r0 / r1 are the offsets from object 0 / 1
    PS_D float &pair(int c, int k) const { return *(float *)&gpair[c * PAIR_FLOATS + k]; }
    // Stack only (global stash): M^-1 J^T of gripper slot c's normal row, element k
    __attribute__((address_space(1))) float *ggrip = nullptr;
    PS_D float &grip(int c, int k) const { return *(float *)&ggrip[c * 9 + k]; }
    // Stack: the solver's source of pair slot c / gripper slot c: this env's
    // rows if it has the slot (c < n), else the shared zero block
    __attribute__((address_space(1))) float *gzero = nullptr;
    PS_D __attribute__((address_space(1))) float *pair_rows(int c, int n) const {
        return c < n ? gpair + c * PAIR_FLOATS : gzero;
    }
    PS_D __attribute__((address_space(1))) float *grip_rows(int c, int n) const {
        return c < n ? ggrip + c * 9 : gzero;
    }
    // a copy whose address the compiler cannot see through: loads from it are
    // not loop-invariant, so they stay in the PGS loop as ds_reads instead of
    // being hoisted into (spilled) registers
    PS_D MJStore opaque() const {
        MJStore r = *this;
        asm volatile("" : "+v"(r.base));
        asm volatile("" : "+v"(r.goff));
        asm volatile("" : "+v"(r.gpair));
        asm volatile("" : "+v"(r.ggrip));
        return r;
    }
};

// The one-lane solver's robot velocity change, DoFs (2k, 2k + 1) as f32x2
// values and DoF 8 alone: the pairs stay vectors through the solver loop's
// phis, so a DoF's broadcast into a packed operand selects its half of the
// register pair (op_sel) instead of copying it out first.
struct VelChange {
    f32x2 p[4];
    float z;
    PS_D float g(int a) const { return a == 8 ? z : p[a >> 1][a & 1]; }
    PS_D void s(int a, float v) {
        if (a == 8) z = v;
        else p[a >> 1][a & 1] = v;
    }
    // (dv_a, dv_a): the broadcast of one DoF
    PS_D f32x2 bc(int a) const {
        if (a == 8) return (f32x2){z, z};
        return (a & 1) ? __builtin_shufflevector(p[a >> 1], p[a >> 1], 1, 1)
                       : __builtin_shufflevector(p[a >> 1], p[a >> 1], 0, 0);
    }
    // dv += m s as four v_pk_fma_f32 and one v_fma_f32: the same fused
    // products, element for element, as nine v_fma_f32 (the gripper rows'
    // M^-1 J^T come from LDS as ds_read2 pairs, already in register pairs)
    PS_D void apply(const float m[9], float sc) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            p[k] = __builtin_elementwise_fma((f32x2){m[2 * k], m[2 * k + 1]}, (f32x2){sc, sc}, p[k]);
        z = fmaf(m[8], sc, z);
    }
    // J . dv as the scalar chain fma(J_a, dv_a, s) from s = 0 (jrow_dot)
    PS_D float dot(const float J[9]) const {
        float acc = 0.0f;
#pragma unroll
        for (int a = 0; a < 9; a++) acc = fmaf(J[a], g(a), acc);
        return acc;
    }
};

// fma3 with x and y as one v_pk_fma_f32 (the same bits)
PS_D V3 pk_fma3(V3 a, float s, V3 c) {
    const f32x2 xy = __builtin_elementwise_fma((f32x2){a.x, a.y}, (f32x2){s, s}, (f32x2){c.x, c.y});
    return mk(xy.x, xy.y, fmaf(a.z, s, c.z));
}

PS_D float jrow_dot(const float J[9], const float v[9]) {
    float s = 0.0f;
#pragma unroll
    for (int d = 0; d < 9; d++) s += J[d] * v[d];
    return s;
}

// Geometry that outlives the kinematics: DoF axes/origins (gripper-contact
// Jacobians), the hand's rotation (every gripper box's: the finger frames are
// the hand's, translated), the world box centres and the wrist sphere centre.
struct Geo {
    V3 ax[9], org[7], bc[PM_NUM_BOXES], wc;
    M3 hR;
};

}  // namespace ps
