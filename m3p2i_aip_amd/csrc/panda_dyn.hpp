// panda_dyn.hpp -- device-side "Panda world spec" (currently v3.1) and the panda_env task costs.
//
// Replaces, for the panda_env scene, what the reference delegates to Isaac Gym / PhysX
// (IsaacGymWrapper.step(), isaacgym_wrapper.py:354-360) with:
//   * a velocity-servoed 9-dof chain (drive damping 600, isaacgym_wrapper.py:341-344; effort /
//     velocity / position limits of franka_panda.urdf:34..240), the servos in closed form,
//   * forward kinematics from the URDF joint origins (franka_panda.urdf:27-242),
//   * cubeA and cubeB as free rigid cubes and the dyn-obs plate as a free body that does not rotate; table and
//     shelf_stand static; sleeping cubes,
//   * a velocity-level contact solver: one contact per gripper collision sphere, four-point face-to-face manifolds of the
//     cubes against table / shelf_stand / each other, rows in generalized coordinates with fixed summation trees
//     (spec v3), effective masses by spec_rcp (v3.1), friction rows first, warm-started normal rows last,
//   * the grasp as a latch (pad channel: grasp region inside the pads' region inside the capture volume),
//   * the net contact forces on table / shelf_stand / cubeB from the solver's impulses (what get_motion_cost reads).
// Costs follow the reference (pinned by golden group G6b):
//   get_panda_reach_cost :91-114, get_panda_pick_cost :116-125, get_panda_place_cost :127-136,
//   get_pick_tilt_cost :138-156, get_motion_cost :158-169 (cost_functions.py);
//   quaternion_rotation_matrix / get_general_ori_* skill_utils.py:140-180, 224-290.
//
// One, eight or sixteen lanes per sample (LPS); a sample's environment (9+9 joint values, the bodies' poses, grasp state)
// sits in VGPRs, the solver's per-substep store in LDS.  Trigonometry uses the spec's own Cody-Waite + polynomial sin/cos
// (plain f32 ops) so that the CPU oracle agrees bit-for-bit.
//
// Every function that reads the scene is a template on its type: PandaScene (the reference's workspace compiled in) or
// PandaSceneRT (the workspace of m3_set_panda_scene as kernel-argument members of the same names).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "spec_fma.hpp"

namespace m3 {

// Kernel argument: only what depends on dt / substeps (per-dof servo and drive-row constants, the free bodies' inverse
// inertias, computed once on the host in f32 in the oracle's order).  Everything the URDF / yaml files fix is a
// compile-time constant and folds into the (fully unrolled) per-dof code.
struct PandaScene {
    float h, inv_h;  // substep
    int substeps, iters;
    float a[9], rden[9], dv[9];      // servo in closed form: a = hD/I, 1/(1+a), h*effort/I
    float invI[9], pmax[9], hD;      // the drives as rows of the contact passes
    float invm_cube, invI_cube, invm_obs, sleep_v2, sleep_w2;
    static constexpr float g = 9.8f;
    static constexpr float drive_damping = 600.0f;                       // isaacgym_wrapper.py:344
    static constexpr float base[3] = {-0.45f, 0.0f, 1.125f};             // panda.yaml:8
    static constexpr float effort[9] = {87, 87, 87, 87, 12, 12, 12, 20, 20};  // urdf :34..240
    static constexpr float vlim[9] = {2.175f, 2.175f, 2.175f, 2.175f, 2.61f, 2.61f, 2.61f, 0.2f, 0.2f};
    static constexpr float qlo[9] = {-2.8973f, -1.7628f, -2.8973f, -3.0718f, -2.8973f, -0.0175f, -2.8973f, 0.0f, 0.0f};
    static constexpr float qhi[9] = {2.8973f, 1.7628f, 2.8973f, -0.0698f, 2.8973f, 3.7525f, 2.8973f, 0.04f, 0.04f};
    static constexpr float table[6] = {0.0f, 0.0f, 1.0f, 0.6f, 0.6f, 0.025f};    // 1_table.yaml
    static constexpr float shelf[6] = {0.5f, 0.0f, 1.175f, 0.1f, 0.1f, 0.15f};   // 3_shelf_stand.yaml
    static constexpr float obs_half[3] = {0.1f, 0.1f, 0.01f};                    // 4_obs.yaml
    static constexpr float cube_half = 0.025f, cube_m = 0.125f;                  // 5_cubeA.yaml, 6_cubeB.yaml
    static constexpr float grasp_z = 0.1034f, grasp_dx = 0.025f, grasp_dz = 0.025f;   // spec v1.1: pad centre on the cube's face
    static constexpr float finger_max = 0.04f;                                          // franka_panda.urdf:226-242
    static constexpr float grasp_align = 0.95f, grasp_tol = 0.002f;
    static constexpr float tip_z = 0.045f, tip_r = 0.012f, hand_z = 0.03f, hand_r = 0.04f;
    // spec v2: the contact solver (isaacgym_wrapper.py:26-31)
    static constexpr float contact_offset = 0.01f, slop = 0.001f, baumgarte = 0.2f, max_bias = 2.0f, act_margin = 0.002f;
    static constexpr float mu = 1.0f;                                                   // actor_utils.py:27
    static constexpr float rest_gap = 0.002f, cube_rad = 0.0434f;
};

// the run-time part of the scene (host side: m3_create, and the host build in tests/native/), in f32, in the oracle's order.
// Joint inertias: the diagonal of the joint-space mass matrix at the initial pose, from the collision meshes at the
// default density (tools/panda_inertia.py).
// cube_m, obs_m: the masses of cubeA / cubeB and of the plate (m3_set_panda_scene; the defaults are the reference's).
inline void make_panda_scene(PandaScene& s, float dt, int substeps, int iters = 6, float cube_m = PandaScene::cube_m,
                             float obs_m = 0.8f) {
    const float h = dt / (float)substeps;
    s.h = h; s.inv_h = 1.0f / h; s.substeps = substeps; s.iters = iters;
    const float inertia[9] = {1.32f, 2.12f, 1.30f, 0.918f, 0.0271f, 0.0366f, 0.0030f, 0.022f, 0.022f};
    const float effort[9] = {87, 87, 87, 87, 12, 12, 12, 20, 20};
    s.hD = h * 600.0f;
    for (int i = 0; i < 9; ++i) {
        s.a[i] = s.hD / inertia[i];
        s.rden[i] = 1.0f / (1.0f + s.a[i]);
        s.invI[i] = 1.0f / inertia[i];
        s.pmax[i] = h * effort[i];
        s.dv[i] = s.pmax[i] * s.invI[i];
    }
    const float cube_half = 0.025f;
    s.invm_cube = 1.0f / cube_m;      // (the oracle's order: panda_chain.c, m3o_panda_step)
    s.invI_cube = 1.0f / ((cube_m * ((2.0f * cube_half) * (2.0f * cube_half))) / 6.0f);
    s.invm_obs = 1.0f / obs_m;
    s.sleep_v2 = 0.02f * 0.02f; s.sleep_w2 = 0.4f * 0.4f;
}

// The scene with the workspace of m3_set_panda_scene as run-time members: the five names below hide PandaScene's
// constants of the same names, everything else (the run-time part above, the robot, the grasp geometry, the solver
// constants) is PandaScene's.  Formed on the host by make_panda_scene_rt (panda_scene.hpp).
struct PandaSceneRT : PandaScene {
    float base[3];
    float table[6];
    float shelf[6];
    float obs_half[3];
    float mu;
};

struct Body {
    float p[3], q[4], v[3], w[3];   // pos, quaternion xyzw, linear / angular velocity
};

struct PandaWorld {
    float q[9], qd[9];
    Body A, B;                       // cubeA, cubeB: free rigid cubes
    float obs_p[3], obs_v[3];        // the dyn-obs plate: a free body that does not rotate (no gravity: 4_obs.yaml)
    float held;
    float rel_p[3], rel_q[4];
    float awake[2];                  // cubeA, cubeB
    float f_table[3], f_shelf[3], f_cubeB[3];
    float warm_t[4], warm_l[4];      // per collision sphere: 1 + target of the last substep's contact, its normal impulse
};

struct Frame {
    float x[3], y[3], z[3], p[3];
};

__device__ __forceinline__ void spec_sincos(float x, float& s, float& c) {
    const float k = rintf(x * 0.63661977236758134308f);
    // (spec v1.2: the Cody-Waite steps, the Horner steps and the final sums are fused multiply-adds)
    float r = mad(-k, 1.5703125f, x);
    r = mad(-k, 4.837512969970703125e-4f, r);
    r = mad(-k, 7.54978995489188e-8f, r);
    const float z = r * r;
    float ps = -1.9515295891e-4f;
    ps = mad(ps, z, 8.3321608736e-3f);
    ps = mad(ps, z, -1.6666654611e-1f);
    const float sn = mad(r, z * ps, r);
    float pc = 2.443315711809948e-5f;
    pc = mad(pc, z, -1.388731625493765e-3f);
    pc = mad(pc, z, 4.166664568298827e-2f);
    const float cs = mad(z * z, pc, mad(-0.5f, z, 1.0f));
    // quadrant q = k mod 4: (s, c) = (sn, cs), (cs, -sn), (-sn, -cs), (-cs, sn).  One swap select and
    // two sign-bit XORs instead of a chain of compares and selects (same values bit for bit).
    const unsigned q = (unsigned)((int)k) & 3u;
    const bool swap = (q & 1u) != 0u;
    const float s0 = swap ? cs : sn, c0 = swap ? sn : cs;
    s = __uint_as_float(__float_as_uint(s0) ^ ((q & 2u) << 30));
    c = __uint_as_float(__float_as_uint(c0) ^ (((q + 1u) & 2u) << 30));
}

__device__ __forceinline__ void rot_xp(Frame& f) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float y = f.y[i]; f.y[i] = f.z[i]; f.z[i] = -y; }
}
__device__ __forceinline__ void rot_xm(Frame& f) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float y = f.y[i]; f.y[i] = -f.z[i]; f.z[i] = y; }
}
__device__ __forceinline__ void rot_z(Frame& f, float s, float c) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float x = f.x[i], y = f.y[i];
        f.x[i] = mad(c, x, s * y);
        f.y[i] = mad(c, y, -(s * x));
    }
}
// p <- mad(tz, z, mad(ty, y, mad(tx, x, p))) (spec v1.2: the offset accumulated into p by fused multiply-adds, x then
// y then z).  The offsets are URDF literals, mostly with one or two zero components; under IEEE rules the compiler
// must keep `0 * x + p` (NaN / signed-zero semantics).  The zero terms are dropped here by hand (the tests fold at
// compile time after inlining); the value can differ from the spec's full expression only in the sign of a zero,
// which no later operation of the chain can observe.
__device__ __forceinline__ void trans(Frame& f, float tx, float ty, float tz) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float p = f.p[i];
        if (tx != 0.0f) p = mad(tx, f.x[i], p);
        if (ty != 0.0f) p = mad(ty, f.y[i], p);
        if (tz != 0.0f) p = mad(tz, f.z[i], p);
        f.p[i] = p;
    }
}

__device__ __forceinline__ void mat2quat(const Frame& f, float* q) {
    const float r00 = f.x[0], r10 = f.x[1], r20 = f.x[2];
    const float r01 = f.y[0], r11 = f.y[1], r21 = f.y[2];
    const float r02 = f.z[0], r12 = f.z[1], r22 = f.z[2];
    const float tr = (r00 + r11) + r22;
    if (tr > 0.0f) {
        const float s = sqrtf(tr + 1.0f) * 2.0f;
        q[3] = 0.25f * s; q[0] = (r21 - r12) / s; q[1] = (r02 - r20) / s; q[2] = (r10 - r01) / s;
    } else if (r00 > r11 && r00 > r22) {
        const float s = sqrtf(((1.0f + r00) - r11) - r22) * 2.0f;
        q[3] = (r21 - r12) / s; q[0] = 0.25f * s; q[1] = (r01 + r10) / s; q[2] = (r02 + r20) / s;
    } else if (r11 > r22) {
        const float s = sqrtf(((1.0f + r11) - r00) - r22) * 2.0f;
        q[3] = (r02 - r20) / s; q[0] = (r01 + r10) / s; q[1] = 0.25f * s; q[2] = (r12 + r21) / s;
    } else {
        const float s = sqrtf(((1.0f + r22) - r00) - r11) * 2.0f;
        q[3] = (r10 - r01) / s; q[0] = (r02 + r20) / s; q[1] = (r12 + r21) / s; q[2] = 0.25f * s;
    }
}

// skill_utils.py:140-180 (xyzw -> row-major 3x3)
__device__ __forceinline__ void quat2mat(const float* Q, float* R) {
    const float q0 = Q[3], q1 = Q[0], q2 = Q[1], q3 = Q[2];
    R[0] = 2 * (q0 * q0 + q1 * q1) - 1; R[1] = 2 * (q1 * q2 - q0 * q3); R[2] = 2 * (q1 * q3 + q0 * q2);
    R[3] = 2 * (q1 * q2 + q0 * q3); R[4] = 2 * (q0 * q0 + q2 * q2) - 1; R[5] = 2 * (q2 * q3 - q0 * q1);
    R[6] = 2 * (q1 * q3 - q0 * q2); R[7] = 2 * (q2 * q3 + q0 * q1); R[8] = 2 * (q0 * q0 + q3 * q3) - 1;
}

__device__ __forceinline__ float dot3(const float* a, const float* b) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// ---- world spec v3: generalized coordinates (the oracle's comment above sum16 is the definition) ---------------------------
// A sample's generalized vector has 16 entries: joints 0-8 | linear (9-11) and angular (12-14) velocity of the free body a
// gripper row touches | 0.  LPS = lanes per sample: with LPS = 1 a lane holds all sixteen (step mode, the host build of the
// tests, launches with more wavefronts than SIMDs), with LPS = 16 the sixteen lanes of a DPP row hold one each -- a joint-space
// row is then ONE register, its velocity one multiply + a four-step butterfly across the row, an impulse one fused
// multiply-add (tools/ubench/coop_panda_rows.hip: 2.3x per pass against nine serial fused multiply-adds fed from LDS).
// Everything that is not a generalized vector is replicated in the sixteen lanes (same values, same control flow).
template <int LPS> struct Gen {
    static_assert(LPS == 1 || LPS == 8 || LPS == 16, "lanes per sample");
    static constexpr int N = 16 / LPS;      // entries per lane: element e of lane l (of the sample's LPS) is coordinate e * LPS + l
    float a[N];
};
template <int LPS> __device__ __forceinline__ int gen_lane() { return (LPS == 1) ? 0 : (int)(threadIdx.x & (unsigned)(LPS - 1)); }
// the coordinate element e of this lane's Gen holds
template <int LPS> __device__ __forceinline__ int gen_coord(int e) { return e * LPS + gen_lane<LPS>(); }
// what the sixteen lanes of a sample share instead of repeating (experiment builds switch them off: tools/flag_variants.sh)
#ifdef M3_PABL_NO_DETECT_SHARE
constexpr bool DETECT_BY_QUADS = false;     // the gripper's four spheres / a manifold's four corners: one per quad of the DPP row
#else
constexpr bool DETECT_BY_QUADS = true;
#endif
#ifdef M3_PABL_NO_FK_SHARE
constexpr bool SINCOS_BY_LANES = false;     // the seven joints' sines and cosines: lane j forms joint j's
#else
constexpr bool SINCOS_BY_LANES = true;
#endif
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// SUM16: the fixed pairwise tree ((x0+x1)+(x2+x3)) + ... ; across lanes: quad_perm xor 1, xor 2, row_half_mirror (, row_mirror) --
// every step pairs lanes symmetrically, so all lanes of the sample end with the same bits; a lane's elements (eight lanes per
// sample: the sums of coordinates 0-7 and 8-15) are added last: the tree's top level
template <int LPS> __device__ __forceinline__ float gen_sum(const Gen<LPS>& x) {
    if constexpr (LPS == 1) {
        float a[8], b[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = x.a[2 * i] + x.a[2 * i + 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = a[2 * i] + a[2 * i + 1];
        return (b[0] + b[1]) + (b[2] + b[3]);
    } else {
        float v[Gen<LPS>::N];
#pragma unroll
        for (int e = 0; e < Gen<LPS>::N; ++e) {
            v[e] = x.a[e];
            v[e] = v[e] + dpp_f<0xB1>(v[e]);
            v[e] = v[e] + dpp_f<0x4E>(v[e]);
            v[e] = v[e] + dpp_f<0x141>(v[e]);
            if constexpr (LPS == 16) v[e] = v[e] + dpp_f<0x140>(v[e]);
        }
        if constexpr (LPS == 16) return v[0];
        else return v[0] + v[1];
    }
}
// the generalized vector whose coordinate c is f(c) (f: replicated values, c a compile-time constant after unrolling).  The
// selects run from the highest coordinate down so that runs of equal constants (the zeros of coordinates 9-15) fold away.
template <int LPS, class F> __device__ __forceinline__ Gen<LPS> gen_make(F f) {
    Gen<LPS> g;
    const int l = gen_lane<LPS>();
#pragma unroll
    for (int e = 0; e < Gen<LPS>::N; ++e) {
        if constexpr (LPS == 1) g.a[e] = f(e);
        else {
            float a = f(e * LPS + LPS - 1);
#pragma unroll
            for (int j = LPS - 2; j >= 0; --j) a = (l == j) ? f(e * LPS + j) : a;
            g.a[e] = a;
        }
    }
    return g;
}
// coordinates [lo, hi) <- f(c), the others kept
template <int LPS, class F> __device__ __forceinline__ void gen_update(Gen<LPS>& g, int lo, int hi, F f) {
    const int l = gen_lane<LPS>();
#pragma unroll
    for (int e = 0; e < Gen<LPS>::N; ++e) {
#pragma unroll
        for (int j = 0; j < LPS; ++j) {
            const int c = e * LPS + j;
            if (c >= lo && c < hi) g.a[e] = (LPS == 1 || l == j) ? f(c) : g.a[e];
        }
    }
}
// entries 0-8 <- nine replicated values, 9-15 <- +0
template <int LPS> __device__ __forceinline__ Gen<LPS> gen_from9(const float* x) {
    return gen_make<LPS>([&](int c) __attribute__((always_inline)) { return (c < 9) ? x[c < 9 ? c : 0] : 0.0f; });
}
// coordinate c of the sample's vector -> replicated
template <int LPS> __device__ __forceinline__ float gen_entry(const Gen<LPS>& g, int c) {
    if constexpr (LPS == 1) return g.a[c];
    else return __int_as_float(__builtin_amdgcn_ds_bpermute((int)((threadIdx.x & ~(unsigned)(LPS - 1)) + (unsigned)(c % LPS)) << 2,
                                                            __float_as_int(g.a[c / LPS])));
}
// entries 9-11 <- v, 12-14 <- w (a free body's velocities; replicated inputs)
template <int LPS> __device__ __forceinline__ void gen_set_body(Gen<LPS>& g, const float* v, const float* w) {
    gen_update<LPS>(g, 9, 15, [&](int c) __attribute__((always_inline)) { return (c < 12) ? v[c < 12 ? c - 9 : 0] : w[c >= 12 ? c - 12 : 0]; });
}
template <int LPS> __device__ __forceinline__ void gen_clear_body(Gen<LPS>& g) {      // entries 9-15 <- +0
    gen_update<LPS>(g, 9, 16, [](int) __attribute__((always_inline)) { return 0.0f; });
}

// ---- the cubes' manifold rows (world spec v3; the oracle's comment above sum8_6 is the definition) -------------------------
// Body coordinates: c = 8 b + i, b = 0 cubeA, 1 cubeB; i = 0-2 linear, 3-5 angular velocity, 6-7 pads (+0).  With sixteen lanes
// per sample that is lanes 0-7 | 8-15 of ONE register, with eight lanes one register per cube, with one lane an array.
enum { BK_A = 0, BK_AB = 1, BK_B = 2 };         // whose coordinates a manifold's rows touch (= the manifold's index)
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// SUM8 over cube h's coordinates: ((x0+x1)+(x2+x3)) + ((x4+x5)+(x6+x7)), x6 = x7 = +0; replicated result
template <int LPS> __device__ __forceinline__ float body_half_sum(const Gen<LPS>& x, int h) {
    if constexpr (LPS == 1) {
        return ((x.a[8 * h] + x.a[8 * h + 1]) + (x.a[8 * h + 2] + x.a[8 * h + 3])) + ((x.a[8 * h + 4] + x.a[8 * h + 5]) + 0.0f);
    } else {
        float v = x.a[(LPS == 8) ? h : 0];
        v = v + dpp_f<0xB1>(v);
        v = v + dpp_f<0x4E>(v);
        v = v + dpp_f<0x141>(v);
        if constexpr (LPS == 16) {
            const float t = dpp_mov<0x140>(v);        // the other half's sum (row_mirror)
            v = ((int)((threadIdx.x >> 3) & 1u) == h) ? v : t;
        }
        return v;
    }
}
template <int LPS> __device__ __forceinline__ float body_sum(const Gen<LPS>& x, int kind) {
    if (kind == BK_A) return body_half_sum<LPS>(x, 0);
    if (kind == BK_B) return body_half_sum<LPS>(x, 1);
    if constexpr (LPS == 16) {
        float v = x.a[0];
        v = v + dpp_f<0xB1>(v);
        v = v + dpp_f<0x4E>(v);
        v = v + dpp_f<0x141>(v);
        return v + dpp_f<0x140>(v);                  // SUM8(A) + SUM8(B) (either order: the same bits)
    } else {
        return body_half_sum<LPS>(x, 0) + body_half_sum<LPS>(x, 1);
    }
}
// is coordinate (element e of this lane) one of a row of `kind`?  (compile-time for LPS = 1, 8)
template <int LPS> __device__ __forceinline__ bool body_in_kind(int e, int kind) {
    if (kind == BK_AB) return true;
    const int h = (LPS == 16) ? (int)((threadIdx.x >> 3) & 1u) : (LPS == 8) ? e : e / 8;
    return h == ((kind == BK_B) ? 1 : 0);
}
// the row (d | aa | 0 0) on the mover's coordinates and, for a cubeA-against-cubeB row, (-d | -ab | 0 0) on cubeB's
template <int LPS> __device__ __forceinline__ Gen<LPS> body_row(int kind, const float* d, const float* aa, const float* ab) {
    return gen_make<LPS>([&](int c) __attribute__((always_inline)) {
        const int b = c / 8, i = c % 8;
        const bool mover = (b == ((kind == BK_B) ? 1 : 0));
        const float vm = (i < 3) ? d[i < 3 ? i : 0] : (i < 6) ? aa[(i >= 3 && i < 6) ? i - 3 : 0] : 0.0f;
        const float vt = (i < 3) ? -d[i < 3 ? i : 0] : (i < 6) ? -ab[(i >= 3 && i < 6) ? i - 3 : 0] : 0.0f;
        return mover ? vm : (kind == BK_AB) ? vt : 0.0f;
    });
}
// the two cubes' velocities as a generalized vector, and back (replicated <-> coordinates)
template <int LPS> __device__ __forceinline__ Gen<LPS> body_vel_load(const Body& A, const Body& B) {
    return gen_make<LPS>([&](int c) __attribute__((always_inline)) {
        const int b = c / 8, i = c % 8;
        const float va = (i < 3) ? A.v[i < 3 ? i : 0] : (i < 6) ? A.w[(i >= 3 && i < 6) ? i - 3 : 0] : 0.0f;
        const float vb = (i < 3) ? B.v[i < 3 ? i : 0] : (i < 6) ? B.w[(i >= 3 && i < 6) ? i - 3 : 0] : 0.0f;
        return (b == 0) ? va : vb;
    });
}
template <int LPS> __device__ __forceinline__ void body_vel_store(const Gen<LPS>& VB, int b, Body& M) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { M.v[i] = gen_entry<LPS>(VB, 8 * b + i); M.w[i] = gen_entry<LPS>(VB, 8 * b + 3 + i); }
}
// a gripper row's free target cube: its six velocities between the cubes' vector (coordinates 8 tb + 0..5) and the joints'
// vector (coordinates 9..14) -- a row shift inside the sample's lanes
template <int LPS> __device__ __forceinline__ void body_to_joint_vec(Gen<LPS>& V, const Gen<LPS>& VB, int tb) {
    if constexpr (LPS == 1) {
#pragma unroll
        for (int i = 0; i < 6; ++i) V.a[9 + i] = (tb == 0) ? VB.a[i] : VB.a[8 + i];
    } else if constexpr (LPS == 8) {
        const float t = dpp_mov<0x111>((tb == 0) ? VB.a[0] : VB.a[1]);          // row_shr:1 -- lanes 1-6 <- 0-5
        const int l = gen_lane<LPS>();
        V.a[1] = (l >= 1 && l <= 6) ? t : V.a[1];
    } else {
        const float tA = dpp_mov<0x119>(VB.a[0]), tB = dpp_mov<0x111>(VB.a[0]);  // row_shr:9 / :1 -- lanes 9-14 <- 0-5 / 8-13
        const int l = gen_lane<LPS>();
        V.a[0] = (l >= 9 && l <= 14) ? ((tb == 0) ? tA : tB) : V.a[0];
    }
}
template <int LPS> __device__ __forceinline__ void joint_vec_to_body(const Gen<LPS>& V, Gen<LPS>& VB, int tb) {
    if constexpr (LPS == 1) {
#pragma unroll
        for (int i = 0; i < 6; ++i) { VB.a[i] = (tb == 0) ? V.a[9 + i] : VB.a[i]; VB.a[8 + i] = (tb == 1) ? V.a[9 + i] : VB.a[8 + i]; }
    } else if constexpr (LPS == 8) {
        const float t = dpp_mov<0x101>(V.a[1]);                                  // row_shl:1 -- lanes 0-5 <- 1-6
        const int l = gen_lane<LPS>();
        VB.a[0] = (tb == 0 && l < 6) ? t : VB.a[0];
        VB.a[1] = (tb == 1 && l < 6) ? t : VB.a[1];
    } else {
        const float tA = dpp_mov<0x109>(V.a[0]), tB = dpp_mov<0x101>(V.a[0]);    // row_shl:9 / :1
        const int l = gen_lane<LPS>();
        VB.a[0] = (tb == 0 && l < 6) ? tA : (tb == 1 && l >= 8 && l < 14) ? tB : VB.a[0];
    }
}

// FK.  STORE: write every link pose (pos3 + quat4) to out[11][7] (step mode views).  JAC: also the arm's Jacobian
// columns at the hand origin (joint axis z_i: angular part; z_i x (p_hand - p_i): linear part) into `gj` -- all seven
// (LPS = 1) or the one of the lane's own joint (LPS = 8, 16: lane l < 7 of the sample owns joint l; the other lanes: zeros).
// gripper geometry of one configuration: hand frame, the arm's Jacobian columns at the hand origin, the spheres
template <int LPS> struct GripperT {
    static constexpr int NJ = (LPS == 1) ? 7 : 1;
    Frame hand;
    float Jv[NJ][3], Jw[NJ][3];
    float c[4][3];       // tip left, tip right, hand, held cube
};
__device__ __forceinline__ void fk_cross(const float* a, const float* b, float* c) {   // (cross3 of the contact code, same order)
    c[0] = mad(a[1], b[2], -(a[2] * b[1]));
    c[1] = mad(a[2], b[0], -(a[0] * b[2]));
    c[2] = mad(a[0], b[1], -(a[1] * b[0]));
}
template <bool STORE, bool JAC = false, int LPS = 1, class SC>
__device__ __forceinline__ void panda_fk(const SC& sc, const float* q, Frame& hand,
                                         float* pl, float* pr, float* out, GripperT<LPS>* gj = nullptr) {
    constexpr int NJ = GripperT<LPS>::NJ;
    float jz[NJ][3], jp[NJ][3];
    if constexpr (JAC && LPS != 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { jz[0][i] = 0.0f; jp[0][i] = 0.0f; }
    }
    Frame f;
    f.x[0] = 1; f.x[1] = 0; f.x[2] = 0; f.y[0] = 0; f.y[1] = 1; f.y[2] = 0;
    f.z[0] = 0; f.z[1] = 0; f.z[2] = 1;
    f.p[0] = sc.base[0]; f.p[1] = sc.base[1]; f.p[2] = sc.base[2];
    int li = 0;
    auto store = [&](const Frame& g) {
        if constexpr (STORE) {
            float* o = out + li * 7;
            o[0] = g.p[0]; o[1] = g.p[1]; o[2] = g.p[2];
            mat2quat(g, o + 3);
        }
        ++li;
    };
    store(f);
    auto rec = [&](int j) {
        if constexpr (JAC) {
            if constexpr (LPS == 1) {
#pragma unroll
                for (int i = 0; i < 3; ++i) { jz[j][i] = f.z[i]; jp[j][i] = f.p[i]; }
            } else {
                const bool mine = gen_lane<LPS>() == j;
#pragma unroll
                for (int i = 0; i < 3; ++i) { jz[0][i] = mine ? f.z[i] : jz[0][i]; jp[0][i] = mine ? f.p[i] : jp[0][i]; }
            }
        }
    };
    // the seven joints' sines and cosines.  Sixteen lanes per sample: q is replicated over the sample's DPP row, so lane j
    // (j < 7) forms joint j's pair alone and the row reads the seven pairs with row broadcasts -- one spec_sincos (~28 VALU)
    // + 14 v_mov_dpp per lane instead of seven; the same function of the same argument: the same bits.  (Every caller is
    // under a wave-uniform condition, and a sample's sixteen lanes are active together.)
    float sj[7], cj[7];
    if constexpr (LPS == 16 && SINCOS_BY_LANES) {
        const int l = gen_lane<16>();
        // (the operands pass through an identity quad_perm: a select between elements of the world's array would be compiled
        // into ONE load through a selected offset -- with the whole world in scratch memory for it)
        const float a0 = dpp_f<0xE4>(q[0]), a1 = dpp_f<0xE4>(q[1]), a2 = dpp_f<0xE4>(q[2]), a3 = dpp_f<0xE4>(q[3]),
                    a4 = dpp_f<0xE4>(q[4]), a5 = dpp_f<0xE4>(q[5]), a6 = dpp_f<0xE4>(q[6]);
        const float q01 = (l & 1) ? a1 : a0, q23 = (l & 1) ? a3 : a2, q45 = (l & 1) ? a5 : a4;
        const float q03 = (l & 2) ? q23 : q01, q47 = (l & 2) ? a6 : q45;
        const float ql = (l & 4) ? q47 : q03;          // lane l: q[l] (l < 7; lanes 7-15 form a pair nobody reads)
        float s1, c1;
        spec_sincos(ql, s1, c1);
        sj[0] = dpp_f<0x150>(s1); cj[0] = dpp_f<0x150>(c1);      // (row_newbcast:j)
        sj[1] = dpp_f<0x151>(s1); cj[1] = dpp_f<0x151>(c1);
        sj[2] = dpp_f<0x152>(s1); cj[2] = dpp_f<0x152>(c1);
        sj[3] = dpp_f<0x153>(s1); cj[3] = dpp_f<0x153>(c1);
        sj[4] = dpp_f<0x154>(s1); cj[4] = dpp_f<0x154>(c1);
        sj[5] = dpp_f<0x155>(s1); cj[5] = dpp_f<0x155>(c1);
        sj[6] = dpp_f<0x156>(s1); cj[6] = dpp_f<0x156>(c1);
    } else {
#pragma unroll
        for (int j = 0; j < 7; ++j) spec_sincos(q[j], sj[j], cj[j]);
    }
    trans(f, 0, 0, 0.333f); rot_z(f, sj[0], cj[0]); store(f); rec(0);
    rot_xm(f); rot_z(f, sj[1], cj[1]); store(f); rec(1);
    trans(f, 0, -0.316f, 0); rot_xp(f); rot_z(f, sj[2], cj[2]); store(f); rec(2);
    trans(f, 0.0825f, 0, 0); rot_xp(f); rot_z(f, sj[3], cj[3]); store(f); rec(3);
    trans(f, -0.0825f, 0.384f, 0); rot_xm(f); rot_z(f, sj[4], cj[4]); store(f); rec(4);
    rot_xp(f); rot_z(f, sj[5], cj[5]); store(f); rec(5);
    trans(f, 0.088f, 0, 0); rot_xp(f); rot_z(f, sj[6], cj[6]); store(f); rec(6);
    trans(f, 0, 0, 0.107f); rot_z(f, -0.70710678118654752f, 0.70710678118654752f); store(f);
    hand = f;
    if constexpr (JAC) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float lever[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { gj->Jw[j][i] = jz[j][i]; lever[i] = f.p[i] - jp[j][i]; }
            fk_cross(gj->Jw[j], lever, gj->Jv[j]);
        }
    }
    trans(f, 0, 0, 0.0584f);
#pragma unroll
    for (int i = 0; i < 3; ++i) { pl[i] = mad(q[7], f.y[i], f.p[i]); pr[i] = mad(-q[8], f.y[i], f.p[i]); }
    if constexpr (STORE) {
        Frame g = f;
        g.p[0] = pl[0]; g.p[1] = pl[1]; g.p[2] = pl[2]; store(g);
        g.p[0] = pr[0]; g.p[1] = pr[1]; g.p[2] = pr[2]; store(g);
    }
}

// ======================================================================================================
// spec v2: contact response.  Written with STATIC slots -- four gripper contacts (one per collision sphere) in
// registers, three face-to-face manifolds (cubeA / its static box, cubeA / cubeB, cubeB / its static box) of four
// contact points whose per-point data sit in a per-lane store (LDS in the kernels) -- where the oracle keeps dynamic
// row lists; the arithmetic of every row is the oracle's, operation for operation.
// ======================================================================================================
__device__ __forceinline__ float spec_rsqrt_p(float a) {      // (as the planar spec: seed + three Newton steps)
    float y = __uint_as_float(0x5f3759dfu - (__float_as_uint(a) >> 1));
    const float hlf = 0.5f * a;
    y = y * mad(-hlf, y * y, 1.5f);
    y = y * mad(-hlf, y * y, 1.5f);
    y = y * mad(-hlf, y * y, 1.5f);
    return y;
}
__device__ __forceinline__ void cross3(const float* a, const float* b, float* c) {
    c[0] = mad(a[1], b[2], -(a[2] * b[1]));
    c[1] = mad(a[2], b[0], -(a[0] * b[2]));
    c[2] = mad(a[0], b[1], -(a[1] * b[0]));
}
__device__ __forceinline__ float dotm(const float* a, const float* b) { return mad(a[0], b[0], mad(a[1], b[1], a[2] * b[2])); }
// value select.  (`k == 0 ? x[0] : x[1]` on lvalues is an lvalue in C++: the compiler selects the ADDRESS and loads
// through it, which pins the whole struct / array in scratch memory; passing the candidates by value avoids that.)
__device__ __forceinline__ float pick3(int k, float a, float b, float c) { return (k == 0) ? a : (k == 1) ? b : c; }

__device__ __forceinline__ void body_rot(const float* q, float* R) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = mad(-2.0f, yy + zz, 1.0f); R[1] = 2.0f * (xy - wz);          R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz);          R[4] = mad(-2.0f, xx + zz, 1.0f); R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy);          R[7] = 2.0f * (yz + wx);          R[8] = mad(-2.0f, xx + yy, 1.0f);
}

// a box: centre, half extents, rotation (ORIENTED: a cube; else axis-aligned: table, shelf_stand, the plate)
template <bool ORIENTED>
struct BoxT {
    float p[3], e[3];
    const float* R;
    __device__ __forceinline__ void local(const float* c, float* l) const {
        const float dl[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) l[i] = ORIENTED ? mad(dl[0], R[0 * 3 + i], mad(dl[1], R[1 * 3 + i], dl[2] * R[2 * 3 + i])) : dl[i];
    }
    __device__ __forceinline__ void world(const float* v, float* o) const {
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = ORIENTED ? mad(R[j * 3 + 0], v[0], mad(R[j * 3 + 1], v[1], R[j * 3 + 2] * v[2])) : v[j];
    }
    __device__ __forceinline__ void dir_local(const float* v, float* o) const {   // rotation only
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = ORIENTED ? mad(v[0], R[0 * 3 + i], mad(v[1], R[1 * 3 + i], v[2] * R[2 * 3 + i])) : v[i];
    }
};
__device__ __forceinline__ BoxT<false> box_static(const float* b6) {
    BoxT<false> o;
#pragma unroll
    for (int i = 0; i < 3; ++i) { o.p[i] = b6[i]; o.e[i] = b6[3 + i]; }
    o.R = nullptr;
    return o;
}
template <class SC>
__device__ __forceinline__ BoxT<true> box_cube(const SC& sc, const float* p, const float* R) {
    BoxT<true> o;
#pragma unroll
    for (int i = 0; i < 3; ++i) { o.p[i] = p[i]; o.e[i] = sc.cube_half; }
    o.R = R;
    return o;
}

// sphere (centre c, radius r) against a box: the gap, the unit normal from the box to the sphere (world), the contact
// point on the sphere's surface.  Centre inside (or on the surface): the face of least penetration, lowest axis first.
template <bool ORIENTED>
__device__ __forceinline__ float pt_box(const BoxT<ORIENTED>& b, const float* c, float r, float* n, float* x) {
    float l[3], d[3], nl[3], gap;
    b.local(c, l);
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = l[i] - fminf(fmaxf(l[i], -b.e[i]), b.e[i]);
    const float d2 = mad(d[0], d[0], mad(d[1], d[1], d[2] * d[2]));
    if (d2 > 1.0e-12f) {
        const float rs = spec_rsqrt_p(d2);
#pragma unroll
        for (int i = 0; i < 3; ++i) nl[i] = d[i] * rs;
        gap = d2 * rs - r;
    } else {
        const float p0 = b.e[0] - fabsf(l[0]), p1 = b.e[1] - fabsf(l[1]), p2 = b.e[2] - fabsf(l[2]);
        int f = 0;
        float pen = p0;
        if (p1 < pen) { pen = p1; f = 1; }
        if (p2 < pen) { pen = p2; f = 2; }
        const float lf = pick3(f, l[0], l[1], l[2]);
        const float sg = (lf >= 0.0f) ? 1.0f : -1.0f;
        nl[0] = (f == 0) ? sg : 0.0f; nl[1] = (f == 1) ? sg : 0.0f; nl[2] = (f == 2) ? sg : 0.0f;
        gap = -pen - r;
    }
    b.world(nl, n);
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = mad(-r, n[j], c[j]);
    return gap;
}

// unit tangents: the coordinate axis least aligned with n, crossed with n and normalised; t2 = n x t1
__device__ __forceinline__ void tangents(const float* n, float* t1, float* t2) {
    const float ax = fabsf(n[0]), ay = fabsf(n[1]), az = fabsf(n[2]);
    float c[3];
    if (ax <= ay && ax <= az) { c[0] = 0.0f; c[1] = -n[2]; c[2] = n[1]; }
    else if (ay <= az) { c[0] = n[2]; c[1] = 0.0f; c[2] = -n[0]; }
    else { c[0] = -n[1]; c[1] = n[0]; c[2] = 0.0f; }
    const float rs = spec_rsqrt_p(mad(c[0], c[0], mad(c[1], c[1], c[2] * c[2])));
#pragma unroll
    for (int i = 0; i < 3; ++i) t1[i] = c[i] * rs;
    cross3(n, t1, t2);
}

enum { T_TABLE = 0, T_SHELF = 1, T_CUBEA = 2, T_CUBEB = 3, T_OBS = 4 };

// a gripper contact (one per collision sphere): the rows are re-formed from these whenever they are needed
struct RSlot {
    bool on;
    int target;          // T_*
    float d[3][3];       // n, t1, t2
    float rho[3];        // contact point - hand origin
    float rt[3];         // contact point - target body's centre
    float meff[3], bias, lam[3];
};

// the row of direction d at the point ph + rho of the gripper (sphere s: the finger columns) in generalized coordinates:
// (J_0..J_8 | -d | -(r_t x d) | 0), the body entries +0 for a static target (tb < 0), the angular ones for the plate (tb = 2)
template <int LPS>
__device__ __forceinline__ Gen<LPS> gen_robot_row(const GripperT<LPS>& g, int s, bool held, const float* rho, const float* d,
                                                  int tb, const float* rt) {
    float m[3];
    cross3(rho, d, m);
    const float dy = dotm(d, g.hand.y);
    const float f7 = (s == 0 && !held) ? dy : 0.0f, f8 = (s == 1 && !held) ? -dy : 0.0f;
    Gen<LPS> r;
    if constexpr (LPS == 1) {
#pragma unroll
        for (int j = 0; j < 7; ++j) r.a[j] = dotm(d, g.Jv[j]) + dotm(m, g.Jw[j]);
        r.a[7] = f7; r.a[8] = f8;
#pragma unroll
        for (int e = 9; e < 16; ++e) r.a[e] = 0.0f;
        if (tb >= 0) {
            float ab[3];
            cross3(rt, d, ab);
#pragma unroll
            for (int i = 0; i < 3; ++i) { r.a[9 + i] = -d[i]; r.a[12 + i] = (tb < 2) ? -ab[i] : 0.0f; }
        }
    } else {
        const float arm = dotm(d, g.Jv[0]) + dotm(m, g.Jw[0]);       // (the lane's own joint column; lanes >= 7: not used)
        r = gen_make<LPS>([&](int c) __attribute__((always_inline)) { return (c == 7) ? f7 : (c == 8) ? f8 : 0.0f; });
        r.a[0] = (gen_lane<LPS>() < 7) ? arm : r.a[0];
        if (tb >= 0) {
            float ab[3];
            cross3(rt, d, ab);
            gen_update<LPS>(r, 9, 12, [&](int c) __attribute__((always_inline)) { return -d[(c >= 9 && c < 12) ? c - 9 : 0]; });
            if (tb < 2) gen_update<LPS>(r, 12, 15, [&](int c) __attribute__((always_inline)) { return -ab[(c >= 12 && c < 15) ? c - 12 : 0]; });
        }
    }
    return r;
}

// the free bodies as the rows see them
struct BodyVel { float v[3], w[3]; };
__device__ __forceinline__ void body_get(const PandaWorld& W, int b, BodyVel& o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.v[i] = pick3(b, W.A.v[i], W.B.v[i], W.obs_v[i]);
        o.w[i] = pick3(b, W.A.w[i], W.B.w[i], 0.0f);
    }
}
__device__ __forceinline__ void body_put(PandaWorld& W, int b, const BodyVel& o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {     // (unconditional value selects: stores in the arms of an if / else chain are merged
        W.A.v[i] = (b == 0) ? o.v[i] : +W.A.v[i];   //  into ONE store through a selected address -- scratch memory again)
        W.A.w[i] = (b == 0) ? o.w[i] : +W.A.w[i];
        W.B.v[i] = (b == 1) ? o.v[i] : +W.B.v[i];
        W.B.w[i] = (b == 1) ? o.w[i] : +W.B.w[i];
        W.obs_v[i] = (b == 2) ? o.v[i] : +W.obs_v[i];
    }
}
template <class SC>
__device__ __forceinline__ float body_k(const SC& sc, int b, const float* a) {
    return (b < 2) ? mad(sc.invI_cube, dotm(a, a), sc.invm_cube) : sc.invm_obs;
}
__device__ __forceinline__ float bodyvel_along(int b, const BodyVel& o, const float* d, const float* a) {
    const float lin = dotm(d, o.v);
    return (b < 2) ? lin + dotm(a, o.w) : lin;
}
template <class SC>
__device__ __forceinline__ void bodyvel_apply(const SC& sc, int b, BodyVel& o, const float* d, const float* a, float dl) {
    const float im = ((b < 2) ? sc.invm_cube : sc.invm_obs) * dl;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.v[i] = mad(im, d[i], o.v[i]);
    if (b < 2) {
        const float ia = sc.invI_cube * dl;
#pragma unroll
        for (int i = 0; i < 3; ++i) o.w[i] = mad(ia, a[i], o.w[i]);
    }
}
template <class SC>
__device__ __forceinline__ float contact_bias(const SC& sc, float gap) {
    if (gap > 0.0f) return gap * sc.inv_h;
    const float pen = fmaxf(-gap - sc.slop, 0.0f);
    const float push = fminf((sc.baumgarte * pen) * sc.inv_h, sc.max_bias);
    return -push;
}

// ---- face-to-face manifold of a cube against a box (the oracle's cube_manifold) ----------------------------------
// per-lane store of the manifolds' contact points: slot = manifold * 4 + corner, 10 floats each
// (x3 | meff3 | bias | lam3); in the kernels it is LDS (stride 64 floats between a lane's consecutive values)
// ... followed, with one lane per sample (LPS = 1), by the gripper contacts' generalized rows: 4 slots x 3 rows x 16 floats
// (formed once per substep); with sixteen lanes per sample those rows are registers
// (LPS > 1: a manifold slot holds its three rows' entries of the lane -- 3 x Gen::N floats -- in place of the point: 3 N + 7)
constexpr int panda_slot_floats(int lps) { return lps == 1 ? 10 : 3 * (16 / lps) + 7; }
constexpr int panda_store_floats(int lps) { return 12 * panda_slot_floats(lps) + (lps == 1 ? 4 * 3 * 16 : 0); }
constexpr int PANDA_STORE_FLOATS = panda_store_floats(1);
struct CornerStore {
    float* base;
    int stride;
    __device__ __forceinline__ float& at(int slot, int field) const { return base[(slot * 10 + field) * stride]; }
    __device__ __forceinline__ float& row(int s, int r3, int j) const { return base[(120 + (s * 3 + r3) * 16 + j) * stride]; }   // (LPS = 1)
};
// the manifold slots of one substep.  LPS = 1: point x3 | meff3 | bias | lam3, the rows re-formed from the point on every visit
// (36 rows x 16 entries do not fit a lane's share of LDS); LPS > 1: the lane's entries of the three rows | meff3 | bias | lam3
template <int LPS> struct ManStore {
    static constexpr int NE = (LPS == 1) ? 1 : Gen<LPS>::N, SF = panda_slot_floats(LPS), RO = (LPS == 1) ? 3 : 3 * NE;
    const CornerStore& cs;
    __device__ __forceinline__ explicit ManStore(const CornerStore& c) : cs(c) {}
    __device__ __forceinline__ float& f(int slot, int k) const { return cs.base[(slot * SF + k) * cs.stride]; }
    __device__ __forceinline__ float& x(int slot, int i) const { return f(slot, i); }                    // LPS = 1 only
    __device__ __forceinline__ float& rowf(int slot, int r3, int e) const { return f(slot, r3 * NE + e); }  // LPS > 1 only
    __device__ __forceinline__ float& meff(int slot, int r3) const { return f(slot, RO + r3); }
    __device__ __forceinline__ float& bias(int slot) const { return f(slot, RO + 3); }
    __device__ __forceinline__ float& lam(int slot, int r3) const { return f(slot, RO + 4 + r3); }
};
// the gripper contacts' rows of one substep
template <int LPS> struct GripRows;
template <> struct GripRows<1> {
    const CornerStore& cs;
    __device__ __forceinline__ explicit GripRows(const CornerStore& c) : cs(c) {}
    __device__ __forceinline__ Gen<1> get(int s, int r3) const {
        Gen<1> g;
#pragma unroll
        for (int l = 0; l < 16; ++l) g.a[l] = cs.row(s, r3, l);
        return g;
    }
    __device__ __forceinline__ void set(int s, int r3, const Gen<1>& g) {
#pragma unroll
        for (int l = 0; l < 16; ++l) cs.row(s, r3, l) = g.a[l];
    }
};
template <int LPS> struct GripRows {       // LPS = 8, 16: registers
    float J[12][Gen<LPS>::N];
    __device__ __forceinline__ explicit GripRows(const CornerStore&) {
#pragma unroll
        for (int i = 0; i < 12; ++i)
#pragma unroll
            for (int e = 0; e < Gen<LPS>::N; ++e) J[i][e] = 0.0f;
    }
    __device__ __forceinline__ Gen<LPS> get(int s, int r3) const {
        Gen<LPS> g;
#pragma unroll
        for (int e = 0; e < Gen<LPS>::N; ++e) g.a[e] = J[s * 3 + r3][e];
        return g;
    }
    __device__ __forceinline__ void set(int s, int r3, const Gen<LPS>& g) {
#pragma unroll
        for (int e = 0; e < Gen<LPS>::N; ++e) J[s * 3 + r3][e] = g.a[e];
    }
};
// per-coordinate constants of the solver (replicated scene values -> generalized vectors, once per kernel)
template <int LPS> struct GenConst {
    Gen<LPS> invM_cube, invM_obs;    // inverse masses: joints | the touched body's 1/m x 3, 1/I x 3 | 0 (cube / plate)
    Gen<LPS> rden, pmax;             // the drive rows (entries 9-15: 0, so they are no-ops there)
};
template <int LPS, class SC> __device__ __forceinline__ GenConst<LPS> gen_consts(const SC& sc) {
    GenConst<LPS> k;
    k.invM_cube = gen_make<LPS>([&](int c) __attribute__((always_inline)) {
        return (c < 9) ? sc.invI[c < 9 ? c : 0] : (c < 12) ? sc.invm_cube : (c < 15) ? sc.invI_cube : 0.0f; });
    k.invM_obs = gen_make<LPS>([&](int c) __attribute__((always_inline)) {
        return (c < 9) ? sc.invI[c < 9 ? c : 0] : (c < 12) ? sc.invm_obs : 0.0f; });
    k.rden = gen_from9<LPS>(sc.rden);
    k.pmax = gen_from9<LPS>(sc.pmax);
    return k;
}
struct Manifold {
    bool any;            // the cube is near the box
    float n[3], t1[3], t2[3];
    unsigned on;         // bit j: contact point j is a row
    int made, up, down;  // contacts made; of them carrying the cube (n_z >= 0.99, gap < rest_gap) / carried by it
    bool centre_over;
};
template <bool ORIENTED, int LPS = 1, class SC>
__device__ __forceinline__ void manifold_detect(const SC& sc, const float* pb, const float* Rb, const BoxT<ORIENTED>& tgt,
                                                Manifold& m, float (*X)[3], float* gap) {
    m.any = false; m.on = 0u; m.made = 0; m.up = 0; m.down = 0; m.centre_over = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) { m.n[i] = 0.0f; m.t1[i] = 0.0f; m.t2[i] = 0.0f; }   // (defined for the masked lanes of a wave)
    float l[3], dd[3], dw[3], dlc[3];
    tgt.local(pb, l);
#pragma unroll
    for (int i = 0; i < 3; ++i) dd[i] = fminf(fmaxf(l[i], -tgt.e[i]), tgt.e[i]) - l[i];
    const float d2 = mad(dd[0], dd[0], mad(dd[1], dd[1], dd[2] * dd[2]));
    const float lim = sc.cube_rad + sc.contact_offset;
    if (!(d2 > 1.0e-12f) || d2 > lim * lim) return;
    m.any = true;
    int pref = 0;
    if (fabsf(dd[1]) > fabsf(dd[0])) pref = 1;
    if (fabsf(dd[2]) > fabsf(pick3(pref, dd[0], dd[1], 0.0f))) pref = 2;
    auto sel = [](const float* v, int i) __attribute__((always_inline)) { return pick3(i, v[0], v[1], v[2]); };
    const int a1 = (pref == 2) ? 0 : pref + 1, a2 = (pref == 0) ? 2 : pref - 1;     // (pref + 1) % 3, (pref + 2) % 3
    const float side = (sel(dd, pref) <= 0.0f) ? 1.0f : -1.0f;
    m.centre_over = (sel(dd, a1) == 0.0f && sel(dd, a2) == 0.0f);
    tgt.world(dd, dw);
#pragma unroll
    for (int i = 0; i < 3; ++i) dlc[i] = mad(dw[0], Rb[0 * 3 + i], mad(dw[1], Rb[1 * 3 + i], dw[2] * Rb[2 * 3 + i]));
    int f = 0;
    if (fabsf(dlc[1]) > fabsf(dlc[0])) f = 1;
    if (fabsf(dlc[2]) > fabsf(pick3(f, dlc[0], dlc[1], 0.0f))) f = 2;
    const float e = sc.cube_half;
    const float sgn = (sel(dlc, f) >= 0.0f) ? 1.0f : -1.0f;
    float nmw[3], nml[3], nl[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nmw[k] = sgn * pick3(f, Rb[k * 3 + 0], Rb[k * 3 + 1], Rb[k * 3 + 2]);
    tgt.dir_local(nmw, nml);
    const float mz = side * sel(nml, pref);
    const bool clip = (mz <= -0.7f);
    const float rz = clip ? 1.0f / mz : 0.0f;
    nl[0] = (pref == 0) ? side : 0.0f; nl[1] = (pref == 1) ? side : 0.0f; nl[2] = (pref == 2) ? side : 0.0f;
    tgt.world(nl, m.n);
    tangents(m.n, m.t1, m.t2);
    const float e_p = sel(tgt.e, pref), e_1 = sel(tgt.e, a1), e_2 = sel(tgt.e, a2);
    const float m1 = sel(nml, a1), m2 = sel(nml, a2);
    const float sf = sgn * e;
    auto corner = [&](float s1, float s2, float& gp, float* Xo) __attribute__((always_inline)) {
        // cl[f] = sf, cl[(f + 1) % 3] = s1, cl[(f + 2) % 3] = s2
        const float cl[3] = {pick3(f, sf, s2, s1), pick3(f, s1, sf, s2), pick3(f, s2, s1, sf)};
        float xw[3], lc[3], lq[3], qw[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) xw[k] = pb[k] + mad(Rb[k * 3 + 0], cl[0], mad(Rb[k * 3 + 1], cl[1], Rb[k * 3 + 2] * cl[2]));
        tgt.local(xw, lc);
        const float lcp = sel(lc, pref), lc1 = sel(lc, a1), lc2 = sel(lc, a2);
        const float hgt = side * lcp - e_p;
        const float q1 = fminf(fmaxf(lc1, -e_1), e_1);
        const float q2 = fminf(fmaxf(lc2, -e_2), e_2);
        const float d1 = q1 - lc1, d2_ = q2 - lc2;
        const bool moved = (d1 != 0.0f) || (d2_ != 0.0f);
        if (moved && !clip) gp = 1.0f;
        else if (moved) gp = hgt - mad(m1, d1, m2 * d2_) * rz;
        else gp = hgt;
        const float fp = side * e_p;
        // lq[a1] = q1, lq[a2] = q2, lq[pref] = fp
        lq[0] = (pref == 0) ? fp : (a1 == 0) ? q1 : q2;
        lq[1] = (pref == 1) ? fp : (a1 == 1) ? q1 : q2;
        lq[2] = (pref == 2) ? fp : (a1 == 2) ? q1 : q2;
        tgt.world(lq, qw);
#pragma unroll
        for (int k = 0; k < 3; ++k) Xo[k] = tgt.p[k] + qw[k];
    };
    if constexpr (LPS == 16 && DETECT_BY_QUADS) {
        // sixteen lanes per sample: quad j of the sample's DPP row forms corner j, the row reads the four (gap, point)
        // with row broadcasts of lanes 0 / 4 / 8 / 12 (every caller's condition is the same in a sample's sixteen lanes)
        const int jq = gen_lane<16>() >> 2;
        float gq, Xq[3];
        corner((jq & 1) ? e : -e, (jq & 2) ? e : -e, gq, Xq);
        gap[0] = dpp_f<0x150>(gq); X[0][0] = dpp_f<0x150>(Xq[0]); X[0][1] = dpp_f<0x150>(Xq[1]); X[0][2] = dpp_f<0x150>(Xq[2]);
        gap[1] = dpp_f<0x154>(gq); X[1][0] = dpp_f<0x154>(Xq[0]); X[1][1] = dpp_f<0x154>(Xq[1]); X[1][2] = dpp_f<0x154>(Xq[2]);
        gap[2] = dpp_f<0x158>(gq); X[2][0] = dpp_f<0x158>(Xq[0]); X[2][1] = dpp_f<0x158>(Xq[1]); X[2][2] = dpp_f<0x158>(Xq[2]);
        gap[3] = dpp_f<0x15C>(gq); X[3][0] = dpp_f<0x15C>(Xq[0]); X[3][1] = dpp_f<0x15C>(Xq[1]); X[3][2] = dpp_f<0x15C>(Xq[2]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) corner((j & 1) ? e : -e, (j & 2) ? e : -e, gap[j], X[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float gp = gap[j];
        if (gp < sc.contact_offset) {
            m.on |= 1u << j;
            ++m.made;
            if (m.n[2] >= 0.99f && gp < sc.rest_gap) ++m.up;
            if (m.n[2] <= -0.99f && gp < sc.rest_gap) ++m.down;
        }
    }
}

// the static box a cube makes contact with: the nearer to its centre (the table on a tie)
template <class SC>
__device__ __forceinline__ bool nearer_is_table(const SC& sc, const float* pb) {
    float d2[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float* b = s ? sc.shelf : sc.table;
        float dd[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float l = pb[i] - b[i];
            dd[i] = fminf(fmaxf(l, -b[3 + i]), b[3 + i]) - l;
        }
        d2[s] = mad(dd[0], dd[0], mad(dd[1], dd[1], dd[2] * dd[2]));
    }
    return d2[0] <= d2[1];
}
template <class SC>
__device__ __forceinline__ bool cube_on_static(const SC& sc, const Body& c) {
    float R[9], X[4][3], gap[4];
    body_rot(c.q, R);
    Manifold m;
    const BoxT<false> b = box_static(nearer_is_table(sc, c.p) ? sc.table : sc.shelf);
    manifold_detect<false>(sc, c.p, R, b, m, X, gap);
    if (!m.any) return false;
    bool ok = m.n[2] >= 0.99f;
#pragma unroll
    for (int j = 0; j < 4; ++j) ok = ok && (gap[j] < sc.rest_gap);
    return ok;
}
template <class SC>
__device__ __forceinline__ bool cube_on_cube(const SC& sc, const Body& up, const Body& lo) {
    float Ru[9], Rl[9], X[4][3], gap[4];
    body_rot(up.q, Ru);
    body_rot(lo.q, Rl);
    Manifold m;
    const BoxT<true> b = box_cube(sc, lo.p, Rl);
    manifold_detect<true>(sc, up.p, Ru, b, m, X, gap);
    if (!m.any || !m.centre_over || !(m.n[2] >= 0.99f)) return false;
    int n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (gap[j] < sc.rest_gap) ++n;
    return n >= 3;
}

// cube pose relative to the hand + alignment test shared by the grasp rule and infer_held
struct GraspGeom {
    float cx, cy, cz;
    float Rc[9];
    bool in_region;
    bool in_capture;   // spec v2.1: the volume in which the tips' spheres do not act on cubeA (the oracle's comment)
    bool in_pads;      // spec v2.1: the pads meet the cube's side faces (they cannot enter it, closing pads sweep it)
};
constexpr float PADS_DX = 0.035f, PADS_DZ = 0.03f;
template <class SC>
__device__ __forceinline__ void grasp_geom(const SC& sc, const PandaWorld& w, const Frame& hand,
                                           GraspGeom& g) {
    const float d[3] = {w.A.p[0] - hand.p[0], w.A.p[1] - hand.p[1], w.A.p[2] - hand.p[2]};
    g.cx = dot3(d, hand.x); g.cy = dot3(d, hand.y); g.cz = dot3(d, hand.z);
    quat2mat(w.A.q, g.Rc);
    float ay = 0.0f, az = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float col[3] = {g.Rc[j], g.Rc[3 + j], g.Rc[6 + j]};
        ay = fmaxf(ay, fabsf(dot3(hand.y, col)));
        az = fmaxf(az, fabsf(dot3(hand.z, col)));
    }
    // spec v1.1: footprint of the pads along the hand's x and z + alignment; the callers add their y condition
    // (step: centre between the two pad faces; infer_held: centred between closed pads)
    g.in_region = fabsf(g.cx) <= sc.grasp_dx && fabsf(g.cz - sc.grasp_z) <= sc.grasp_dz &&
                  ay >= sc.grasp_align && az >= sc.grasp_align;
    g.in_capture = fabsf(g.cx) <= 0.045f && (g.cz - sc.grasp_z) <= 0.08f && (g.cz - sc.grasp_z) >= -0.03f && az >= 0.9f;
    g.in_pads = fabsf(g.cx) <= PADS_DX && fabsf(g.cz - sc.grasp_z) <= PADS_DZ && az >= 0.9f;
}
__device__ __forceinline__ void set_rel_rot(PandaWorld& w, const Frame& hand, const float* Rc) {
    Frame r;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float col[3] = {Rc[j], Rc[3 + j], Rc[6 + j]};
        float* dstc = (j == 0) ? r.x : (j == 1) ? r.y : r.z;
        dstc[0] = dot3(hand.x, col); dstc[1] = dot3(hand.y, col); dstc[2] = dot3(hand.z, col);
    }
    mat2quat(r, w.rel_q);
}

// A world is loaded from the wrapper's tensors, which carry neither a "held" bit nor the cubes' sleep state: both are
// inferred from geometry (the oracle's m3o_panda_infer_held).
template <class SC>
__device__ __forceinline__ void panda_infer_held(const SC& sc, PandaWorld& w, float* hand_p = nullptr) {
    Frame hand;
    float pl[3], pr[3];
    panda_fk<false>(sc, w.q, hand, pl, pr, nullptr);
    if (hand_p) { hand_p[0] = hand.p[0]; hand_p[1] = hand.p[1]; hand_p[2] = hand.p[2]; }
    GraspGeom g;
    grasp_geom(sc, w, hand, g);
    const float gap = w.q[7] + w.q[8];
    const float mid = 0.5f * (w.q[7] - w.q[8]);
    w.held = 0.0f;
    if (g.in_region && fabsf(g.cy - mid) <= sc.grasp_tol && gap <= 2.0f * sc.cube_half + sc.grasp_tol) {
        w.held = 1.0f;
        w.rel_p[0] = g.cx; w.rel_p[1] = g.cy; w.rel_p[2] = g.cz;
        set_rel_rot(w, hand, g.Rc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { w.warm_t[i] = 0.0f; w.warm_l[i] = 0.0f; }      // nothing is carried over from before the load
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.f_table[i] = 0.0f; w.f_shelf[i] = 0.0f; w.f_cubeB[i] = 0.0f; }
    auto still = [](const Body& b) __attribute__((always_inline)) {
        return b.v[0] == 0.0f && b.v[1] == 0.0f && b.v[2] == 0.0f && b.w[0] == 0.0f && b.w[1] == 0.0f && b.w[2] == 0.0f;
    };
    const bool stA = still(w.A), stB = still(w.B);
    const bool onA = cube_on_static(sc, w.A), onB = cube_on_static(sc, w.B);
    const bool freeA = (w.held == 0.0f);
    const bool stackA = freeA && !onA && onB && stA && stB && cube_on_cube(sc, w.A, w.B);
    const bool stackB = freeA && !onB && onA && stA && stB && cube_on_cube(sc, w.B, w.A);
    w.awake[0] = (stA && (onA || stackA)) ? 0.0f : 1.0f;
    w.awake[1] = (stB && (onB || stackB)) ? 0.0f : 1.0f;
}

// what the costs read after a step
struct PandaObs {
    float left[3], left_q[4], right[3];
};

__device__ __forceinline__ void integrate_quat(float* q, const float* w, float h) {
    if (w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f) return;
    const float hh = 0.5f * h;
    const float tx = mad(w[0], q[3], mad(w[1], q[2], -(w[2] * q[1])));
    const float ty = mad(w[1], q[3], mad(w[2], q[0], -(w[0] * q[2])));
    const float tz = mad(w[2], q[3], mad(w[0], q[1], -(w[1] * q[0])));
    const float tw = -mad(w[0], q[0], mad(w[1], q[1], w[2] * q[2]));
    const float n0 = mad(hh, tx, q[0]), n1 = mad(hh, ty, q[1]), n2 = mad(hh, tz, q[2]), n3 = mad(hh, tw, q[3]);
    const float rs = spec_rsqrt_p(mad(n0, n0, mad(n1, n1, mad(n2, n2, n3 * n3))));
    q[0] = n0 * rs; q[1] = n1 * rs; q[2] = n2 * rs; q[3] = n3 * rs;
}

// FORCES: whether the net contact forces on table / shelf_stand / cubeB are formed (a rollout: only the pick cost reads
// them, get_motion_cost, cost_functions.py:116-125,158-169; step mode: always).
//
// LAZY (rollout): kinematics are evaluated only where something can depend on them.  (a) The contact detection of a
// substep needs the gripper's geometry only if a collision sphere can be within the contact offset of a box: all
// four spheres lie within GRIP_R0 of the hand's origin, the hand's origin cannot have moved farther than `trav` =
// LEVER * sum_i |dq_i| from where the last evaluated kinematics had it (`hp`); a wave in which no lane passes that test
// for any box skips it.  (b) The kinematics AFTER the integration feed the grasp rule of a free cube, the pose of a held
// one and, in a step's last substep, the finger poses the costs read: as in spec v1 (a held cube is re-attached in the
// last substep only -- nothing reads its pose in between except the contact detection, which then uses the held
// sphere at the pose of the last attachment: so a wave with a held cube in a lane that is NEAR a box re-attaches in
// every substep).  Identical results: the oracle evaluates everything every substep.
constexpr float PANDA_LEVER = 1.2f;
constexpr float GRIP_R0 = 0.17f;
struct HeldYes { static constexpr bool value = true; };
struct HeldNo { static constexpr bool value = false; };
// The kinematics of a configuration, kept from where a substep evaluates them AFTER its integration to where the next substep's
// contact detection needs them BEFORE its own (same joint values: the grasp rule in between moves the fingers only, which
// the hand frame and the arm's Jacobian columns at the hand origin do not depend on).  Rollouts only (LAZY).  With several
// lanes per sample the lane's own Jacobian column travels along (6 registers); with one lane per sample only the hand frame
// does (the 42 registers of seven columns would spill) and the columns are formed -- by a pass over the chain of their own --
// in the substeps in which some lane of the wavefront has a contact candidate: never, in a reach rollout that touches nothing.
template <int LPS> struct FkCarry {
    bool valid;
    Frame hand;
    float Jv[3], Jw[3];
    int near_lane_substeps; // sum over the substeps so far of the lanes whose gripper was within reach of a box or whose cubes were awake (wave-uniform)
};
// the friction rows' clamp to +-mx (mx >= 0, no NaN): one v_med3_f32 or a max / min pair -- the same value; which one is the
// faster instruction stream was measured per kernel form (pick, K = 4000: one lane 1.67 -> 1.59 ms and eight lanes 0.833 ->
// 0.825 with v_med3, sixteen lanes 0.764 -> 0.784: there the pair schedules better between the DPP steps)
template <int LPS> __device__ __forceinline__ float friction_clamp(float l, float mx) {
    if constexpr (LPS == 16) return fminf(fmaxf(l, -mx), mx);
    else return __builtin_amdgcn_fmed3f(l, -mx, mx);
}
#ifdef M3_PABL_PROF      // (profiling build, tools/panda_wave_profile.py: shader clocks and substep counts per sample)
struct PandaProf { long long solve_clk, near_clk, detect_clk, post_clk, pre_clk, mid_clk, wake_clk; int n_robot, n_body, n_near, n_act, n_fk; };
#define M3_PROF_ARG , PandaProf* prof = nullptr
#else
#define M3_PROF_ARG
#endif
template <bool FORCES = true, bool LAZY = false, int LPS = 1, class SC>
__device__ __forceinline__ void panda_step(const SC& sc, PandaWorld& w, const float* u, PandaObs& obs,
                                           const CornerStore& cs, float* hp = nullptr, float* trav = nullptr,
                                           FkCarry<LPS>* fkc = nullptr M3_PROF_ARG) {
    constexpr bool CARRY = LAZY, CARRY_JAC = LAZY && LPS != 1;
    const float h = sc.h;
    const GenConst<LPS> gk = gen_consts<LPS>(sc);
    const Gen<LPS> uG = gen_from9<LPS>(u);
    for (int sub = 0; sub < sc.substeps; ++sub) {
#ifdef M3_PABL_PROF
        const long long prof_ts = __builtin_readcyclecounter();
#endif
        const bool last = (sub == sc.substeps - 1);
        // 0. release
        if (w.held != 0.0f && (u[7] >= 0.0f || u[8] >= 0.0f)) {
            w.held = 0.0f;
#pragma unroll
            for (int i = 0; i < 3; ++i) { w.A.v[i] = 0.0f; w.A.w[i] = 0.0f; }
            w.awake[0] = 1.0f;
        }
        const bool held = (w.held != 0.0f);
        // 1. the joint servos in closed form
        float qd1[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            if (held && i >= 7) { qd1[i] = 0.0f; continue; }
            float v = mad(sc.a[i], u[i], w.qd[i]) * sc.rden[i];
            const float tau = sc.drive_damping * (u[i] - v);
            if (tau > sc.effort[i]) v = w.qd[i] + sc.dv[i];
            if (tau < -sc.effort[i]) v = w.qd[i] - sc.dv[i];
            qd1[i] = fminf(fmaxf(v, -sc.vlim[i]), sc.vlim[i]);
        }
        // 2. gripper contacts
        RSlot rs[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {   // (all fields defined: the passes run branch-free over a wave's slots, masked by `on`)
            rs[s].on = false; rs[s].target = -1; rs[s].bias = 0.0f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                rs[s].d[0][i] = rs[s].d[1][i] = rs[s].d[2][i] = 0.0f;
                rs[s].rho[i] = rs[s].rt[i] = rs[s].meff[i] = rs[s].lam[i] = 0.0f;
            }
        }
        bool robot_rows = false;
        bool touched[3] = {false, false, false};
        GripperT<LPS> g;
        GripRows<LPS> rows(cs);
        float RA[9], RB[9];
        bool near = true;
        if constexpr (LAZY) {
            const float reach = GRIP_R0 + *trav + sc.contact_offset;
            auto box_d2 = [&](const float* b, const float* e) __attribute__((always_inline)) {
                float d2 = 0.0f;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float l = hp[i] - b[i];
                    const float d = l - fminf(fmaxf(l, -e[i]), e[i]);
                    d2 = mad(d, d, d2);
                }
                return d2;
            };
            const float rc = reach + sc.cube_rad;
            const float ce[3] = {0.0f, 0.0f, 0.0f};
            const bool nr = box_d2(sc.table, sc.table + 3) < reach * reach || box_d2(sc.shelf, sc.shelf + 3) < reach * reach ||
                            (!held && box_d2(w.A.p, ce) < rc * rc) || box_d2(w.B.p, ce) < rc * rc ||
                            box_d2(w.obs_p, sc.obs_half) < reach * reach;
            const unsigned long long nrm = __builtin_amdgcn_ballot_w64(nr);
            near = nrm != 0ull;
            // (what the choice of the next reach command's kernel form reads, rollout_panda.hip: lanes with the gripper within reach
            // of a box or with an awake cube -- the substeps that have rows to solve or detection to run)
            if constexpr (CARRY)
                fkc->near_lane_substeps += __builtin_popcountll(__builtin_amdgcn_ballot_w64(nr || (!held && w.awake[0] != 0.0f) || w.awake[1] != 0.0f));
        }
#ifdef M3_PABL_NO_NEAR      // (ablations for tools/time_variants_bench.sh: they change results)
        near = false;
#endif
#ifdef M3_PABL_NO_BODIES
        w.awake[0] = 0.0f; w.awake[1] = 0.0f;
#endif
        const bool bodies_awake_wave = __builtin_amdgcn_ballot_w64((!held && w.awake[0] != 0.0f) || w.awake[1] != 0.0f) != 0ull;
        if (near || bodies_awake_wave) { body_rot(w.A.q, RA); body_rot(w.B.q, RB); }
#ifdef M3_PABL_PROF
        const long long prof_t0 = __builtin_readcyclecounter();
        if (prof) prof->pre_clk += prof_t0 - prof_ts;
#endif
        if (near) {
            float pl[3], pr[3];
            // (with the arm's Jacobian columns: keeping the joint axes and origins costs ~60 instructions on top of the
            // chain's ~400; a second pass over the chain for the lanes that turn out to have a candidate cost all 400)
            bool carried = false;
            if constexpr (CARRY) carried = __builtin_amdgcn_readfirstlane((int)fkc->valid) != 0;
            if (carried) {
                if constexpr (CARRY) {
                    g.hand = fkc->hand;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        if constexpr (CARRY_JAC) { g.Jv[0][i] = fkc->Jv[i]; g.Jw[0][i] = fkc->Jw[i]; }
                        const float fo = mad(0.0584f, g.hand.z[i], g.hand.p[i]);     // (panda_fk's last translation)
                        pl[i] = mad(w.q[7], g.hand.y[i], fo);
                        pr[i] = mad(-w.q[8], g.hand.y[i], fo);
                    }
                }
            } else if constexpr (CARRY && !CARRY_JAC) panda_fk<false, false, LPS>(sc, w.q, g.hand, pl, pr, nullptr);
            else panda_fk<false, true, LPS>(sc, w.q, g.hand, pl, pr, nullptr, &g);
            if constexpr (LAZY) { hp[0] = g.hand.p[0]; hp[1] = g.hand.p[1]; hp[2] = g.hand.p[2]; *trav = 0.0f; }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                g.c[0][i] = mad(sc.tip_z, g.hand.z[i], pl[i]);
                g.c[1][i] = mad(sc.tip_z, g.hand.z[i], pr[i]);
                g.c[2][i] = mad(sc.hand_z, g.hand.z[i], g.hand.p[i]);
                g.c[3][i] = w.A.p[i];
            }
            // Broad phase per box, once per WAVE (it cannot change a result): all four spheres lie inside the ball of
            // radius GRIP_R around the hand sphere's centre -- the finger tips 0.0734 z + q7 y (q7 <= 0.04) + 0.012 =
            // 0.096 from it, the held cube's centre at most |(0.025, 0.04, 0.1034 + 0.025 - 0.03)| = 0.109 (the pad
            // channel bounds rel_p) + its radius 0.025 = 0.134 -- so a box farther than GRIP_R + contact_offset from that
            // centre in every lane has no candidate: its tests (each ~40 instructions) are skipped.
            constexpr float GRIP_R = 0.15f;
            auto near_box = [&](const float* b, const float* e, float extra) __attribute__((always_inline)) {
                float d2 = 0.0f;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float l = g.c[2][i] - b[i];
                    const float d = l - fminf(fmaxf(l, -e[i]), e[i]);
                    d2 = mad(d, d, d2);
                }
                const float lim = GRIP_R + sc.contact_offset + extra;
                return __builtin_amdgcn_ballot_w64(!(d2 > lim * lim)) != 0ull;
            };
            const float zero3[3] = {0.0f, 0.0f, 0.0f};
            const bool nt = near_box(sc.table, sc.table + 3, 0.0f), ns = near_box(sc.shelf, sc.shelf + 3, 0.0f);
            const bool nA = near_box(w.A.p, zero3, sc.cube_rad), nB = near_box(w.B.p, zero3, sc.cube_rad);
            const bool no = near_box(w.obs_p, sc.obs_half, 0.0f);
            // the capture volume (spec v2.1: the space between and under the open fingers): there the pads, not the tip
            // spheres, act on cubeA
            bool in_channel = false;
            if (nA && !held) {
                GraspGeom gg;
                grasp_geom(sc, w, g.hand, gg);
                in_channel = gg.in_capture && gg.cy < w.q[7] && gg.cy > -w.q[8];
            }
            const BoxT<false> bt = box_static(sc.table), bs = box_static(sc.shelf);
            const BoxT<true> bA = box_cube(sc, w.A.p, RA), bB = box_cube(sc, w.B.p, RB);
            BoxT<false> bo;
#pragma unroll
            for (int i = 0; i < 3; ++i) { bo.p[i] = w.obs_p[i]; bo.e[i] = sc.obs_half[i]; }
            bo.R = nullptr;
            float bgap[4];
            if constexpr (LPS == 16 && DETECT_BY_QUADS) {
                // Sixteen lanes per sample: the four collision spheres are tested by the four quads of the sample's DPP row
                // (quad s = sphere s: one sphere against the near boxes instead of four) and every lane reads the four
                // results -- target, gap, normal, contact point -- with row broadcasts of lanes 0, 4, 8, 12.  The same tests
                // in the same order on the same values: the same bits.  (The centres pass through an identity quad_perm: see
                // panda_fk.)
                const int sq = gen_lane<16>() >> 2;
                float ctr[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float c0 = dpp_f<0xE4>(g.c[0][i]), c1 = dpp_f<0xE4>(g.c[1][i]), c2 = dpp_f<0xE4>(g.c[2][i]), c3 = dpp_f<0xE4>(g.c[3][i]);
                    const float c01 = (sq & 1) ? c1 : c0, c23 = (sq & 1) ? c3 : c2;
                    ctr[i] = (sq & 2) ? c23 : c01;
                }
                const float r = (sq < 2) ? sc.tip_r : (sq == 2) ? sc.hand_r : sc.cube_half;
                float mgap = sc.contact_offset;
                int mt = -1;
                float bn[3] = {0.0f, 0.0f, 0.0f}, bx[3] = {0.0f, 0.0f, 0.0f};
                if (!(sq == 3 && !held)) {
                    auto take = [&](float gap, const float* n, const float* x, int t) __attribute__((always_inline)) {
                        if (gap < mgap) { mgap = gap; mt = t; bn[0] = n[0]; bn[1] = n[1]; bn[2] = n[2]; bx[0] = x[0]; bx[1] = x[1]; bx[2] = x[2]; }
                    };
                    float n[3], x[3];
                    if (nt) take(pt_box<false>(bt, ctr, r, n, x), n, x, T_TABLE);
                    if (ns) take(pt_box<false>(bs, ctr, r, n, x), n, x, T_SHELF);
                    if (nA && !(held || (sq < 2 && in_channel))) take(pt_box<true>(bA, ctr, r, n, x), n, x, T_CUBEA);
                    if (nB) take(pt_box<true>(bB, ctr, r, n, x), n, x, T_CUBEB);
                    if (no) take(pt_box<false>(bo, ctr, r, n, x), n, x, T_OBS);
                }
                auto fetch = [&](auto ctrl, int s) __attribute__((always_inline)) {
                    constexpr int C = decltype(ctrl)::value;
                    RSlot& c = rs[s];
                    c.target = __builtin_amdgcn_update_dpp(0, mt, C, 0xF, 0xF, false);
                    bgap[s] = dpp_f<C>(mgap);
                    const float n0 = dpp_f<C>(bn[0]), n1 = dpp_f<C>(bn[1]), n2 = dpp_f<C>(bn[2]);
                    const float x0 = dpp_f<C>(bx[0]), x1 = dpp_f<C>(bx[1]), x2 = dpp_f<C>(bx[2]);
                    if (s != 3 || held) {      // (a slot that is not tested keeps its zeros)
                        c.d[0][0] = n0; c.d[0][1] = n1; c.d[0][2] = n2;
                        c.rho[0] = x0 - g.hand.p[0]; c.rho[1] = x1 - g.hand.p[1]; c.rho[2] = x2 - g.hand.p[2];
                        c.rt[0] = x0; c.rt[1] = x1; c.rt[2] = x2;
                    }
                };
                fetch(std::integral_constant<int, 0x150>{}, 0);
                fetch(std::integral_constant<int, 0x154>{}, 1);
                fetch(std::integral_constant<int, 0x158>{}, 2);
                fetch(std::integral_constant<int, 0x15C>{}, 3);
            } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                RSlot& c = rs[s];
                c.target = -1;
                bgap[s] = sc.contact_offset;
                if (s == 3 && !held) continue;
                const float r = (s < 2) ? sc.tip_r : (s == 2) ? sc.hand_r : sc.cube_half;
                float bn[3] = {0.0f, 0.0f, 0.0f}, bx[3] = {0.0f, 0.0f, 0.0f};
                auto take = [&](float gap, const float* n, const float* x, int t) __attribute__((always_inline)) {
                    if (gap < bgap[s]) { bgap[s] = gap; c.target = t; bn[0] = n[0]; bn[1] = n[1]; bn[2] = n[2]; bx[0] = x[0]; bx[1] = x[1]; bx[2] = x[2]; }
                };
                float n[3], x[3];
                if (nt) take(pt_box<false>(bt, g.c[s], r, n, x), n, x, T_TABLE);
                if (ns) take(pt_box<false>(bs, g.c[s], r, n, x), n, x, T_SHELF);
                if (nA && !(held || (s < 2 && in_channel))) take(pt_box<true>(bA, g.c[s], r, n, x), n, x, T_CUBEA);
                if (nB) take(pt_box<true>(bB, g.c[s], r, n, x), n, x, T_CUBEB);
                if (no) take(pt_box<false>(bo, g.c[s], r, n, x), n, x, T_OBS);
#pragma unroll
                for (int i = 0; i < 3; ++i) { c.d[0][i] = bn[i]; c.rho[i] = bx[i] - g.hand.p[i]; c.rt[i] = bx[i]; }
            }
            }
            const bool cand = rs[0].target >= 0 || rs[1].target >= 0 || rs[2].target >= 0 || rs[3].target >= 0;
            if (__builtin_amdgcn_ballot_w64(cand) != 0ull) {
                // some lane has a candidate: culling, rows, effective masses
                if constexpr (CARRY && !CARRY_JAC) {     // (one lane per sample: the Jacobian columns only now, see FkCarry)
                    Frame h2;
                    float a2[3], b2[3];
                    panda_fk<false, true, LPS>(sc, w.q, h2, a2, b2, nullptr, &g);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    RSlot& c = rs[s];
                    if (c.target < 0) continue;
                    const int tb = c.target - T_CUBEA;
                    tangents(c.d[0], c.d[1], c.d[2]);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float tp = pick3(tb, w.A.p[i], w.B.p[i], w.obs_p[i]);
                        c.rt[i] = (tb >= 0) ? c.rt[i] - tp : 0.0f;
                    }
                    // culling: the gap predicted for the end of the substep from the servo's velocities
                    const Gen<LPS> invMs = (tb == 2) ? gk.invM_obs : gk.invM_cube;
                    Gen<LPS> row = gen_robot_row<LPS>(g, s, held, c.rho, c.d[0], tb, c.rt);
                    {
                        Gen<LPS> u1 = gen_from9<LPS>(qd1), x;
                        if (tb >= 0) { BodyVel bv; body_get(w, tb, bv); gen_set_body<LPS>(u1, bv.v, bv.w); }
#pragma unroll
                        for (int e = 0; e < Gen<LPS>::N; ++e) x.a[e] = row.a[e] * u1.a[e];
                        const float vn0 = gen_sum<LPS>(x);
                        if (!(mad(h, vn0, bgap[s]) < sc.act_margin)) continue;
                    }
                    // the rows (LPS = 1: kept in the per-lane store; LPS = 16: one register each), effective masses, bias
#pragma unroll
                    for (int r3 = 0; r3 < 3; ++r3) {
                        if (r3 > 0) row = gen_robot_row<LPS>(g, s, held, c.rho, c.d[r3], tb, c.rt);
                        Gen<LPS> x;
#pragma unroll
                        for (int e = 0; e < Gen<LPS>::N; ++e) x.a[e] = (row.a[e] * invMs.a[e]) * row.a[e];
                        rows.set(s, r3, row);
                        c.meff[r3] = spec_rcp(gen_sum<LPS>(x));          // world spec v3.1
                        c.lam[r3] = 0.0f;
                    }
                    c.bias = contact_bias(sc, bgap[s]);
                    if (w.warm_t[s] == (float)(c.target + 1)) c.lam[0] = w.warm_l[s];
                    c.on = true;
                    robot_rows = true;
                    touched[0] = touched[0] || tb == 0; touched[1] = touched[1] || tb == 1; touched[2] = touched[2] || tb == 2;
                    w.awake[0] = (tb == 0) ? 1.0f : +w.awake[0];
                    w.awake[1] = (tb == 1) ? 1.0f : +w.awake[1];
                }
            }
        }
#ifdef M3_PABL_PROF
        const long long prof_tn = __builtin_readcyclecounter();
        if (prof) { prof->near_clk += prof_tn - prof_t0; prof->n_near += near ? 1 : 0; }
#endif
        // 3. an awake cube wakes the other one when they are close
        const bool freeA = !held;
        if (freeA && (w.awake[0] != 0.0f) != (w.awake[1] != 0.0f)) {
            const float dx = w.A.p[0] - w.B.p[0], dy = w.A.p[1] - w.B.p[1], dz = w.A.p[2] - w.B.p[2];
            const float lim = 2.0f * sc.cube_rad + sc.contact_offset;
            if (mad(dx, dx, mad(dy, dy, dz * dz)) < lim * lim) { w.awake[0] = 1.0f; w.awake[1] = 1.0f; }
        }
        const bool actA = freeA && w.awake[0] != 0.0f, actB = w.awake[1] != 0.0f;
        // 4. gravity, then the cubes' face-to-face contacts
        if (actA) w.A.v[2] = mad(-sc.g, h, w.A.v[2]);
        if (actB) w.B.v[2] = mad(-sc.g, h, w.B.v[2]);
        const ManStore<LPS> ms(cs);
        const Gen<LPS> invMB = gen_make<LPS>([&](int c) __attribute__((always_inline)) {     // the cubes' inverse masses
            return (c % 8 < 3) ? sc.invm_cube : (c % 8 < 6) ? sc.invI_cube : 0.0f; });
        Manifold mA, mAB, mB;
        mA.any = mAB.any = mB.any = false; mA.on = mAB.on = mB.on = 0u;
        mA.made = mAB.made = mB.made = 0; mA.up = mAB.up = mB.up = 0; mA.down = mAB.down = mB.down = 0;
        mA.centre_over = mAB.centre_over = mB.centre_over = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            mA.n[i] = mA.t1[i] = mA.t2[i] = 0.0f; mAB.n[i] = mAB.t1[i] = mAB.t2[i] = 0.0f; mB.n[i] = mB.t1[i] = mB.t2[i] = 0.0f;
        }
        bool tA = true, tB = true;      // the cube's static box is the table
        const bool any_act = __builtin_amdgcn_ballot_w64(actA || actB) != 0ull;
#ifdef M3_PABL_PROF
        const long long prof_t2 = __builtin_readcyclecounter();
        if (prof) prof->wake_clk += prof_t2 - prof_tn;
#endif
        if (any_act) {
            if (near == false && !bodies_awake_wave) { body_rot(w.A.q, RA); body_rot(w.B.q, RB); }   // (woken just now: cannot happen without `near`)
            auto prepare = [&](int m_id, const Manifold& m, const float (*X)[3], const float* gap, const float* pm, const float* pt)
                               __attribute__((always_inline)) {     // (m_id must be a constant in the body: it indexes a lane's elements)
                // (LPS > 1) the lane's components of the manifold's three directions: d[k], d[(k + 1) % 3], d[(k + 2) % 3], k = (lane & 7) % 3
                const int li = (LPS == 1) ? 0 : (int)(threadIdx.x & 7u);
                const bool lane_lin = li < 3, lane_pad = li >= 6, lane_hi = (LPS == 16) && ((threadIdx.x >> 3) & 1u) != 0u;
                const int lk = (li >= 3) ? li - 3 : li;
                const bool k_is0 = lk == 0, k_is1 = lk == 1;
                float dk0[3], dk1[3], dk2[3];
                if constexpr (LPS != 1) {
#pragma unroll
                    for (int r3 = 0; r3 < 3; ++r3) {
                        const float* d = (r3 == 0) ? m.n : (r3 == 1) ? m.t1 : m.t2;
                        dk0[r3] = k_is0 ? d[0] : k_is1 ? d[1] : d[2];
                        dk1[r3] = k_is0 ? d[1] : k_is1 ? d[2] : d[0];
                        dk2[r3] = k_is0 ? d[2] : k_is1 ? d[0] : d[1];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!((m.on >> j) & 1u)) continue;
                    const int slot = m_id * 4 + j;
                    float r[3], rt[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) { r[i] = X[j][i] - pm[i]; rt[i] = (m_id == BK_AB) ? X[j][i] - pt[i] : 0.0f; }
                    if constexpr (LPS == 1) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) ms.x(slot, i) = X[j][i];
                    }
                    // LPS > 1: the lane's entries are formed in "lane space" -- coordinate i = lane & 7 of a cube is d[i] (i < 3) or
                    // (r x d)[i - 3]: the lane picks ITS components of r once per point (and of the three directions once per
                    // manifold, above), then every row is one multiply + one fused multiply-add, the arithmetic of cross3
                    float rk1[Gen<LPS>::N], rk2[Gen<LPS>::N];
                    if constexpr (LPS != 1) {
#pragma unroll
                        for (int e = 0; e < Gen<LPS>::N; ++e) {
                            const bool tgt = (m_id == BK_AB) && ((LPS == 8) ? (e == 1) : lane_hi);
                            const float q0 = tgt ? rt[0] : r[0], q1 = tgt ? rt[1] : r[1], q2 = tgt ? rt[2] : r[2];
                            rk1[e] = k_is0 ? q1 : k_is1 ? q2 : q0;       // r[(k + 1) % 3]
                            rk2[e] = k_is0 ? q2 : k_is1 ? q0 : q1;       // r[(k + 2) % 3]
                        }
                    }
#pragma unroll
                    for (int r3 = 0; r3 < 3; ++r3) {
                        const float* d = (r3 == 0) ? m.n : (r3 == 1) ? m.t1 : m.t2;
                        Gen<LPS> row;
                        if constexpr (LPS == 1) {
                            float aa[3], ab[3] = {0.0f, 0.0f, 0.0f};
                            cross3(r, d, aa);
                            if (m_id == BK_AB) cross3(rt, d, ab);
                            row = body_row<LPS>(m_id, d, aa, ab);
                        } else {
#pragma unroll
                            for (int e = 0; e < Gen<LPS>::N; ++e) {
                                const float ang = mad(rk1[e], dk2[r3], -(rk2[e] * dk1[r3]));
                                float ent = lane_lin ? dk0[r3] : ang;
                                ent = lane_pad ? 0.0f : ent;
                                const bool hi = (LPS == 8) ? (e == 1) : lane_hi;            // the element's cube: B
                                const bool mover = hi == (m_id == BK_B), tgt = (m_id == BK_AB) && hi;
                                row.a[e] = mover ? ent : tgt ? -ent : 0.0f;
                            }
                        }
                        Gen<LPS> x;
#pragma unroll
                        for (int e = 0; e < Gen<LPS>::N; ++e) {
                            x.a[e] = (row.a[e] * invMB.a[e]) * row.a[e];
                            if constexpr (LPS != 1) ms.rowf(slot, r3, e) = row.a[e];
                        }
                        ms.meff(slot, r3) = spec_rcp(body_sum<LPS>(x, m_id));   // world spec v3.1
                        ms.lam(slot, r3) = 0.0f;
                    }
                    ms.bias(slot) = contact_bias(sc, gap[j]);
                }
            };
            float X[4][3], gap[4];
            if (actA) {
                tA = nearer_is_table(sc, w.A.p);
                manifold_detect<false, LPS>(sc, w.A.p, RA, box_static(tA ? sc.table : sc.shelf), mA, X, gap);
                prepare(BK_A, mA, X, gap, w.A.p, nullptr);
            }
            if (actA && actB) {
                manifold_detect<true, LPS>(sc, w.A.p, RA, box_cube(sc, w.B.p, RB), mAB, X, gap);
                prepare(BK_AB, mAB, X, gap, w.A.p, w.B.p);
            }
            if (actB) {
                tB = nearer_is_table(sc, w.B.p);
                manifold_detect<false, LPS>(sc, w.B.p, RB, box_static(tB ? sc.table : sc.shelf), mB, X, gap);
                prepare(BK_B, mB, X, gap, w.B.p, nullptr);
            }
        }
        // 5. velocity passes.  (Tried: wave-uniform control flow with the inactive lanes masked by value selects instead
        // of per-lane branches -- 15-20 % slower, the selects cost more than the exec-mask regions: docs/NOTEBOOK.md.)
        const bool body_rows = (mA.on | mAB.on | mB.on) != 0u;
        Gen<LPS> V, P;         // generalized velocity (joints; entries 9-15 are +0 outside a slot with a free target) and drive impulses
#pragma unroll
        for (int e = 0; e < Gen<LPS>::N; ++e) { V.a[e] = 0.0f; P.a[e] = 0.0f; }
        if (robot_rows) {
            float qds0[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) qds0[i] = (held && i >= 7) ? 0.0f : w.qd[i];
            V = gen_from9<LPS>(qds0);
        }
        // the cubes' velocities as a generalized vector while rows act on them (manifold rows, gripper rows on a cube)
        const bool use_vb = body_rows || touched[0] || touched[1];
        Gen<LPS> VB;
#pragma unroll
        for (int e = 0; e < Gen<LPS>::N; ++e) VB.a[e] = 0.0f;
        if (use_vb) VB = body_vel_load<LPS>(w.A, w.B);
        auto robot_solve = [&](int s, RSlot& c, bool only_warm) __attribute__((always_inline)) {
            const int tb = c.target - T_CUBEA;
            const Gen<LPS> invMs = (tb == 2) ? gk.invM_obs : gk.invM_cube;
            if (only_warm && c.lam[0] == 0.0f) return;        // the warm-start impulse acts before the first pass
            if (tb == 2) { const float z3[3] = {0.0f, 0.0f, 0.0f}; gen_set_body<LPS>(V, w.obs_v, z3); }
            else if (tb >= 0) body_to_joint_vec<LPS>(V, VB, tb);
            auto apply = [&](const Gen<LPS>& row, float dl) __attribute__((always_inline)) {
#pragma unroll
                for (int e = 0; e < Gen<LPS>::N; ++e) V.a[e] = mad(row.a[e] * invMs.a[e], dl, V.a[e]);
            };
            if (only_warm) apply(rows.get(s, 0), c.lam[0]);
            else {
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) {
                    const int r3 = (rr + 1) % 3;      // friction rows first, the normal row last
#ifdef M3_PABL_NO_ROBOT_FRICTION
                    if (r3 != 0) continue;            // (ablation: what the gripper contacts' friction rows cost)
#endif
                    const Gen<LPS> row = rows.get(s, r3);
                    Gen<LPS> x;
#pragma unroll
                    for (int e = 0; e < Gen<LPS>::N; ++e) x.a[e] = row.a[e] * V.a[e];
                    const float v = gen_sum<LPS>(x);
                    float dl = -c.meff[r3] * ((r3 == 0) ? v + c.bias : v);
                    const float l0 = c.lam[r3];
                    float l1 = l0 + dl;
                    if (r3 == 0) l1 = fmaxf(l1, 0.0f);
                    else { const float mx = sc.mu * c.lam[0]; l1 = friction_clamp<LPS>(l1, mx); }
                    c.lam[r3] = l1;
                    dl = l1 - l0;
                    apply(row, dl);
                }
            }
            if (tb == 2) {
#pragma unroll
                for (int i = 0; i < 3; ++i) w.obs_v[i] = gen_entry<LPS>(V, 9 + i);
            } else if (tb >= 0) joint_vec_to_body<LPS>(V, VB, tb);
            if (tb >= 0) gen_clear_body<LPS>(V);
        };
        auto manifold_solve = [&](int m_id, const Manifold& m, const float* pm, const float* pt) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((m.on >> j) & 1u)) continue;
                const int slot = m_id * 4 + j;
                float r[3] = {0.0f, 0.0f, 0.0f}, rt[3] = {0.0f, 0.0f, 0.0f};
                if constexpr (LPS == 1) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) { const float x = ms.x(slot, i); r[i] = x - pm[i]; rt[i] = (m_id == BK_AB) ? x - pt[i] : 0.0f; }
                }
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) {
                    const int r3 = (rr + 1) % 3;
#ifdef M3_PABL_NO_BODY_FRICTION
                    if (r3 != 0) continue;        // (ablation: what the manifolds' friction rows cost)
#endif
                    Gen<LPS> row;
                    if constexpr (LPS == 1) {
                        const float* d = (r3 == 0) ? m.n : (r3 == 1) ? m.t1 : m.t2;
                        float aa[3], ab[3] = {0.0f, 0.0f, 0.0f};
                        cross3(r, d, aa);
                        if (m_id == BK_AB) cross3(rt, d, ab);
                        row = body_row<LPS>(m_id, d, aa, ab);
                    } else {
#pragma unroll
                        for (int e = 0; e < Gen<LPS>::N; ++e) row.a[e] = ms.rowf(slot, r3, e);
                    }
                    Gen<LPS> x;
#pragma unroll
                    for (int e = 0; e < Gen<LPS>::N; ++e) x.a[e] = row.a[e] * VB.a[e];
                    const float v = body_sum<LPS>(x, m_id);
                    float dl = -ms.meff(slot, r3) * ((r3 == 0) ? v + ms.bias(slot) : v);
                    const float l0 = ms.lam(slot, r3);
                    float l1 = l0 + dl;
                    if (r3 == 0) l1 = fmaxf(l1, 0.0f);
                    else { const float mx = sc.mu * ms.lam(slot, 0); l1 = friction_clamp<LPS>(l1, mx); }
                    ms.lam(slot, r3) = l1;
                    dl = l1 - l0;
#pragma unroll
                    for (int e = 0; e < Gen<LPS>::N; ++e) {
                        if (LPS == 1 && (e % 8 >= 6 || !body_in_kind<LPS>(e, m_id))) continue;      // (pads and the other cube: untouched)
                        if (LPS == 8 && !body_in_kind<LPS>(e, m_id)) continue;
                        const float nv = mad(row.a[e] * invMB.a[e], dl, VB.a[e]);
                        VB.a[e] = (LPS == 16 && !body_in_kind<LPS>(e, m_id)) ? VB.a[e] : nv;
                    }
                }
            }
        };
#ifdef M3_PABL_PROF
        const long long prof_t1 = __builtin_readcyclecounter();
        if (prof) { prof->n_robot += robot_rows ? 1 : 0; prof->n_body += body_rows ? 1 : 0; prof->n_act += any_act ? 1 : 0; prof->detect_clk += prof_t1 - prof_t2; }
#endif
        bool any_rows = __builtin_amdgcn_ballot_w64(robot_rows || body_rows) != 0ull;
#ifdef M3_PABL_NO_SOLVE
        any_rows = false;
#endif
        if (any_rows) {
            if (robot_rows) {
#pragma unroll
                for (int s = 0; s < 4; ++s) if (rs[s].on) robot_solve(s, rs[s], true);
            }
#ifdef M3_PABL_ITERS
            const int n_iters = M3_PABL_ITERS;
#else
            const int n_iters = sc.iters;
#endif
            for (int pass = 0; pass <= n_iters; ++pass) {      // the last sweep: the contacts alone (isaacgym_wrapper.py:29)
                if (robot_rows && pass < n_iters) {       // the nine drive rows (one lane-parallel row with LPS = 16)
#pragma unroll
                    for (int e = 0; e < ((LPS == 1) ? 9 : Gen<LPS>::N); ++e) {
                        const int l = gen_coord<LPS>(e);
                        const bool skip = held && l >= 7 && l < 9;
                        const float er = mad(sc.hD, uG.a[e] - V.a[e], -P.a[e]);
                        float dp = er * gk.rden.a[e];
                        const float p1 = fminf(fmaxf(P.a[e] + dp, -gk.pmax.a[e]), gk.pmax.a[e]);
                        dp = p1 - P.a[e];
                        P.a[e] = skip ? P.a[e] : p1;
                        V.a[e] = skip ? V.a[e] : mad(gk.invM_cube.a[e], dp, V.a[e]);
                    }
                }
                if (robot_rows) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) if (rs[s].on) robot_solve(s, rs[s], false);
                }
                if (mA.on) manifold_solve(BK_A, mA, w.A.p, nullptr);
                if (mAB.on) manifold_solve(BK_AB, mAB, w.A.p, w.B.p);
                if (mB.on) manifold_solve(BK_B, mB, w.B.p, nullptr);
            }
        }
#ifdef M3_PABL_PROF
        const long long prof_t4 = __builtin_readcyclecounter();
        if (prof) prof->solve_clk += prof_t4 - prof_t1;
#endif
        if (use_vb && any_rows) { body_vel_store<LPS>(VB, 0, w.A); body_vel_store<LPS>(VB, 1, w.B); }
        if (robot_rows) {
#pragma unroll
            for (int i = 0; i < 9; ++i) qd1[i] = fminf(fmaxf(gen_entry<LPS>(V, i), -sc.vlim[i]), sc.vlim[i]);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) w.qd[i] = (held && i >= 7) ? 0.0f : qd1[i];
        // net contact forces on table / shelf_stand / cubeB: this substep's impulses / h (a step reports its last)
        if (FORCES && last) {
            float ft[3] = {0.f, 0.f, 0.f}, fs[3] = {0.f, 0.f, 0.f}, fb[3] = {0.f, 0.f, 0.f};
            // (which of ft / fs / fb a row adds to is data: selected by value, not through a pointer -- a run-time
            // pointer into local arrays would put them in scratch memory)
            auto add = [&](int which, float lam, const float* d, bool neg) __attribute__((always_inline)) {     // which: 0 table, 1 shelf_stand, 2 cubeB
                const float sI = lam * sc.inv_h;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float cur = pick3(which, ft[i], fs[i], fb[i]);
                    const float nw = mad(neg ? -sI : sI, d[i], cur);
                    ft[i] = (which == 0) ? nw : ft[i]; fs[i] = (which == 1) ? nw : fs[i]; fb[i] = (which == 2) ? nw : fb[i];
                }
            };
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!rs[s].on) continue;
                const int which = (rs[s].target == T_TABLE) ? 0 : (rs[s].target == T_SHELF) ? 1 : (rs[s].target == T_CUBEB) ? 2 : -1;
                if (which >= 0) for (int r3 = 0; r3 < 3; ++r3) add(which, rs[s].lam[r3], rs[s].d[r3], true);
            }
            auto add_m = [&](int m_id, const Manifold& m, int which, bool mover_is_B) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!((m.on >> j) & 1u)) continue;
#pragma unroll
                    for (int r3 = 0; r3 < 3; ++r3) {
                        const float* d = (r3 == 0) ? m.n : (r3 == 1) ? m.t1 : m.t2;
                        const float lam = ms.lam(m_id * 4 + j, r3);
                        add(which, lam, d, true);
                        if (mover_is_B) add(2, lam, d, false);
                    }
                }
            };
            add_m(0, mA, tA ? 0 : 1, false);
            add_m(1, mAB, 2, false);
            add_m(2, mB, tB ? 0 : 1, true);
#pragma unroll
            for (int i = 0; i < 3; ++i) { w.f_table[i] = ft[i]; w.f_shelf[i] = fs[i]; w.f_cubeB[i] = fb[i]; }
        } else if (last) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { w.f_table[i] = 0.0f; w.f_shelf[i] = 0.0f; w.f_cubeB[i] = 0.0f; }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            w.warm_t[s] = rs[s].on ? (float)(rs[s].target + 1) : 0.0f;
            w.warm_l[s] = rs[s].on ? rs[s].lam[0] : 0.0f;
        }
        // 6. sleep
        if (any_act) {
            auto slow = [&](const Body& b) __attribute__((always_inline)) { return dotm(b.v, b.v) < sc.sleep_v2 && dotm(b.w, b.w) < sc.sleep_w2; };
            const bool slA = actA && !touched[0] && slow(w.A), slB = actB && !touched[1] && slow(w.B);
            const bool onA = mA.up == 4, onB = mB.up == 4;
            const bool restA = onA || (onB && mAB.centre_over && mAB.up >= 3);
            const bool restB = onB || (onA && mAB.centre_over && mAB.down >= 3);
            const bool pair = mAB.made > 0;
            const bool okA = pair ? (slA && slB && restA && restB) : (slA && onA);
            const bool okB = pair ? (slA && slB && restA && restB) : (slB && onB);
            if (okA) {
#pragma unroll
                for (int i = 0; i < 3; ++i) { w.A.v[i] = 0.0f; w.A.w[i] = 0.0f; }
                w.awake[0] = 0.0f;
            }
            if (okB) {
#pragma unroll
                for (int i = 0; i < 3; ++i) { w.B.v[i] = 0.0f; w.B.w[i] = 0.0f; }
                w.awake[1] = 0.0f;
            }
        }
        // 7. integration
        float dq_sum = 0.0f;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            float q1 = mad(h, w.qd[i], w.q[i]);
            const float q1c = __builtin_amdgcn_fmed3f(q1, sc.qlo[i], sc.qhi[i]);   // position limits: clamp and stop
            if (q1c != q1) w.qd[i] = 0.0f;
            q1 = q1c;
            if (LAZY && i < 7) dq_sum += fabsf(q1 - w.q[i]);
            w.q[i] = q1;
        }
        if (freeA && w.awake[0] != 0.0f) {
#pragma unroll
            for (int i = 0; i < 3; ++i) w.A.p[i] = mad(h, w.A.v[i], w.A.p[i]);
            integrate_quat(w.A.q, w.A.w, h);
        }
        if (w.awake[1] != 0.0f) {
#pragma unroll
            for (int i = 0; i < 3; ++i) w.B.p[i] = mad(h, w.B.v[i], w.B.p[i]);
            integrate_quat(w.B.q, w.B.w, h);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) w.obs_p[i] = mad(h, w.obs_v[i], w.obs_p[i]);
#ifdef M3_PABL_PROF
        const long long prof_t3 = __builtin_readcyclecounter();
        if (prof) prof->mid_clk += prof_t3 - prof_t4;
#endif
        // 8. kinematics of the new configuration; the grasp rule (spec v1.1, position level)
        Frame hand;
        float pl[3], pr[3];
        bool have_fk = true;
        if constexpr (LAZY) {
            *trav = *trav + PANDA_LEVER * dq_sum;
            if (!last) {
                // needed by: a held cube in a wave that is near a box (its sphere's pose), a free cube's grasp test
                bool need = false;
                if (w.held != 0.0f) need = near;
                else {
                    const float gz = fabsf(sc.grasp_z) + PADS_DZ;      // (the region of the pads' action, spec v2.1)
                    const float lim = sqrtf((PADS_DX * PADS_DX + sc.finger_max * sc.finger_max) + gz * gz) + *trav + 1.0e-3f;
                    const float dx = w.A.p[0] - hp[0], dy = w.A.p[1] - hp[1], dz = w.A.p[2] - hp[2];
                    const bool idle = !(u[7] < 0.0f && u[8] < 0.0f) && !(w.q[7] + w.q[8] < 2.0f * sc.cube_half);
                    need = !(idle || (dx * dx + dy * dy) + dz * dz > lim * lim);
                }
                have_fk = __builtin_amdgcn_ballot_w64(need) != 0ull;
            }
        }
        if (have_fk) {
            if constexpr (CARRY_JAC) {
                GripperT<LPS> gn;
                panda_fk<false, true, LPS>(sc, w.q, hand, pl, pr, nullptr, &gn);
#pragma unroll
                for (int i = 0; i < 3; ++i) { fkc->Jv[i] = gn.Jv[0][i]; fkc->Jw[i] = gn.Jw[0][i]; }
            } else panda_fk<false>(sc, w.q, hand, pl, pr, nullptr);
            if constexpr (CARRY) fkc->hand = hand;
            if constexpr (LAZY) { hp[0] = hand.p[0]; hp[1] = hand.p[1]; hp[2] = hand.p[2]; *trav = 0.0f; }
        }
        if constexpr (CARRY) fkc->valid = have_fk;
        if (w.held != 0.0f) {
            if (have_fk) {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    w.A.p[i] = hand.p[i] + ((w.rel_p[0] * hand.x[i] + w.rel_p[1] * hand.y[i]) + w.rel_p[2] * hand.z[i]);
                float Rr[9];
                quat2mat(w.rel_q, Rr);
                Frame c;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    c.x[i] = (hand.x[i] * Rr[0] + hand.y[i] * Rr[3]) + hand.z[i] * Rr[6];
                    c.y[i] = (hand.x[i] * Rr[1] + hand.y[i] * Rr[4]) + hand.z[i] * Rr[7];
                    c.z[i] = (hand.x[i] * Rr[2] + hand.y[i] * Rr[5]) + hand.z[i] * Rr[8];
                }
                mat2quat(c, w.A.q);
#pragma unroll
                for (int i = 0; i < 3; ++i) { w.A.v[i] = 0.0f; w.A.w[i] = 0.0f; }
            }
        } else if (have_fk) {
            GraspGeom gg;
            grasp_geom(sc, w, hand, gg);
            // spec v1.1 / v2.1, the pad channel: the cube's centre lies between the two pad faces, the pads meet its side
            // faces (in_pads); they hold it in the grasp rule's region (in_region)
            if (gg.in_pads && gg.cy < w.q[7] && gg.cy > -w.q[8]) {
                float gap = w.q[7] + w.q[8];
                const float wdt = 2.0f * sc.cube_half;
                if (gap < wdt) {
                    const float mid = 0.5f * (w.q[7] - w.q[8]);
                    w.q[7] = 0.5f * wdt + mid; w.q[8] = 0.5f * wdt - mid;
                    gap = wdt;
                }
                if (u[7] < 0.0f && u[8] < 0.0f) {
                    // closing pads sweep the cube along the hand's y so that it stays between them; it slides on its
                    // support: the horizontal part of the displacement, horizontal velocity lost
                    const float lo = sc.cube_half - w.q[8], hi = w.q[7] - sc.cube_half;
                    const float cyn = fminf(fmaxf(gg.cy, lo), hi);
                    if (cyn != gg.cy) {
                        const float sh = cyn - gg.cy;
                        w.A.p[0] = w.A.p[0] + sh * hand.y[0];
                        w.A.p[1] = w.A.p[1] + sh * hand.y[1];
                        w.A.v[0] = 0.0f; w.A.v[1] = 0.0f;
                        const float d[3] = {w.A.p[0] - hand.p[0], w.A.p[1] - hand.p[1], w.A.p[2] - hand.p[2]};
                        gg.cx = dot3(d, hand.x); gg.cz = dot3(d, hand.z);
                    }
                }
                if (gg.in_region && gap <= wdt + sc.grasp_tol && u[7] < 0.0f && u[8] < 0.0f) {
                    w.held = 1.0f;
                    w.qd[7] = 0.0f; w.qd[8] = 0.0f;
                    w.rel_p[0] = gg.cx; w.rel_p[1] = 0.5f * (w.q[7] - w.q[8]); w.rel_p[2] = gg.cz;
                    set_rel_rot(w, hand, gg.Rc);
#pragma unroll
                    for (int i = 0; i < 3; ++i) { w.A.v[i] = 0.0f; w.A.w[i] = 0.0f; }
                }
            }
        }
#ifdef M3_PABL_PROF
        if (prof) { prof->post_clk += __builtin_readcyclecounter() - prof_t3; prof->n_fk += have_fk ? 1 : 0; }
#endif
        if (last) {
            // observables for the cost: finger link poses at the FINAL joint values (the pad clamp may have moved q7/q8)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float fo = mad(0.0584f, hand.z[i], hand.p[i]);   // trans(0, 0, 0.0584), zero terms dropped
                obs.left[i] = mad(w.q[7], hand.y[i], fo);
                obs.right[i] = mad(-w.q[8], hand.y[i], fo);
            }
            mat2quat(hand, obs.left_q);
        }
    }
}

// ---- costs ------------------------------------------------------------------------------
__device__ __forceinline__ float coldot(const float* A, int ca, const float* B, int cb) {
    return A[ca] * B[cb] + A[3 + ca] * B[3 + cb] + A[6 + ca] * B[6 + cb];
}
__device__ __forceinline__ float min3f(float a, float b, float c) { return fminf(fminf(a, b), c); }

__device__ __forceinline__ float ori_cube2goal(const float* qc, const float* qg) {
    float C[9], G[9];
    quat2mat(qc, C);
    quat2mat(qg, G);
    const float cx = min3f(1 - fabsf(coldot(G, 0, C, 0)), 1 - fabsf(coldot(G, 0, C, 1)), 1 - fabsf(coldot(G, 0, C, 2)));
    const float cy = min3f(1 - fabsf(coldot(G, 1, C, 0)), 1 - fabsf(coldot(G, 1, C, 1)), 1 - fabsf(coldot(G, 1, C, 2)));
    return cx + cy;
}
__device__ __forceinline__ float ori_ee2cube(const float* qe, const float* qc, float tilt, const float* qc0) {
    float E[9], C[9];
    quat2mat(qe, E);
    quat2mat(qc, C);
    float cost_z;
    if (tilt == 0.0f) {
        cost_z = min3f(1 - fabsf(coldot(E, 2, C, 2)), 1 - fabsf(coldot(E, 2, C, 0)), 1 - fabsf(coldot(E, 2, C, 1)));
    } else {
        float C0[9];
        quat2mat(qc0, C0);
        int sel = 0;
        float best = fabsf(C0[0]);
        if (fabsf(C0[1]) > best) { best = fabsf(C0[1]); sel = 1; }
        if (fabsf(C0[2]) > best) { best = fabsf(C0[2]); sel = 2; }
        const float d = (sel == 0) ? coldot(E, 2, C, 0) : (sel == 1) ? coldot(E, 2, C, 1) : coldot(E, 2, C, 2);
        cost_z = fabsf(tilt - d);
    }
    const float cost_y = min3f(1 - fabsf(coldot(E, 1, C, 0)), 1 - fabsf(coldot(E, 1, C, 1)), 1 - fabsf(coldot(E, 1, C, 2)));
    return cost_z + cost_y;
}

struct PandaCostParams {
    int task, multi_modal, half_K;
    float goal[7];
    float pre_height_diff, tilt_cos_theta;
};

// cube0 / q_half0: cubeA position of env 0 and orientation of the slice's first env -- what the reference's reach cost
// reads (cost_functions.py:97 `cube_state[0, :3]`, skill_utils.py:274; quirk Q8).  Under world spec v2 a rollout's
// gripper can move its cube, so these are NOT the sample's own cube: the rollout kernel carries samples 0 and K / 2 as
// shadow lanes of every wavefront and reads their cube with v_readlane (rollout_panda.hip); callers that cannot
// (a rank of a sharded command) pass the sample's own.
__device__ __forceinline__ float panda_cost(const PandaCostParams& cp, const PandaWorld& w,
                                            const PandaObs& o, int k, const float* cube0, const float* q_half0) {
    if (cp.task == 4) {  // reach
        float goal[3] = {cube0[0], cube0[1], cube0[2]};
        if (!cp.multi_modal || k < cp.half_K) {
            goal[2] = goal[2] + cp.pre_height_diff;
        } else {
            goal[0] = goal[0] - cp.pre_height_diff * cp.tilt_cos_theta;
            goal[2] = goal[2] + cp.pre_height_diff * sqrtf(1.0f - cp.tilt_cos_theta * cp.tilt_cos_theta);
        }
        const float dx = (o.left[0] + o.right[0]) / 2.0f - goal[0];
        const float dy = (o.left[1] + o.right[1]) / 2.0f - goal[1];
        const float dz = (o.left[2] + o.right[2]) / 2.0f - goal[2];
        const float reach = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float tilt = (cp.multi_modal && k >= cp.half_K) ? cp.tilt_cos_theta : 0.0f;
        const float ori = ori_ee2cube(o.left_q, w.A.q, tilt, q_half0);
        return 10.0f * reach + 3.0f * ori;
    }
    if (cp.task == 5) {  // pick
        const float dx = cp.goal[0] - w.A.p[0], dy = cp.goal[1] - w.A.p[1], dz = cp.goal[2] - w.A.p[2];
        const float gc = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float ori = ori_cube2goal(w.A.q, &cp.goal[3]);
        const float fx = (w.f_table[0] + 4.0f * w.f_shelf[0]) + w.f_cubeB[0];
        const float fy = (w.f_table[1] + 4.0f * w.f_shelf[1]) + w.f_cubeB[1];
        const float coll = fabsf(fx) + fabsf(fy);
        return (10.0f * gc + 15.0f * ori) + ((coll > 0.1f) ? 1000.0f : 0.0f);
    }
    if (cp.task == 6) {  // place
        const float dx = o.left[0] - o.right[0], dy = o.left[1] - o.right[1], dz = o.left[2] - o.right[2];
        return 2.0f * (1.0f - sqrtf((dx * dx + dy * dy) + dz * dz));
    }
    return 0.0f;
}
__device__ __forceinline__ float panda_cost(const PandaCostParams& cp, const PandaWorld& w, const PandaObs& o, int k) {
    return panda_cost(cp, w, o, k, w.A.p, w.A.q);
}

// EXTENSION (m3_set_panda_cost_weights; the defaults = the reference's literals): every literal WEIGHT of the three panda
// tasks, the same seven floats in the same order as m3_panda_cost_weights of the public header.  The 0.1 force threshold,
// the `1 -` of the place cost and the finger-pad offset stay literals; pre_height_diff and tilt_cos_theta are the
// objective's (PandaCostParams).  Not a member of PandaCostParams: only the weighted kernels (rollout_panda_weights.hip)
// receive it, as an argument of their own.
struct PandaCostWeights {
    float reach_dist;    // 10    cost_functions.py:114   |ee - pre-pick goal|
    float reach_tilt;    // 3     :156  get_pick_tilt_cost: ee-to-cube orientation
    float pick_goal;     // 10    :125  |pre-place - cubeA|
    float pick_ori;      // 15    :125  cube-to-goal orientation
    float collision;     // 1000  :170  get_motion_cost's penalty (pick)
    float shelf_force;   // 4     :163  the shelf stand's contact force inside the collision test
    float place_grip;    // 2     :134
};
constexpr PandaCostWeights PANDA_COST_WEIGHTS_DEFAULT = {10.0f, 3.0f, 10.0f, 15.0f, 1000.0f, 4.0f, 2.0f};

// The weighted form (an overload: the literal form above keeps serving every kernel it served): panda_cost with each
// literal weight replaced by its field, one for one -- same operations, same order, so at PANDA_COST_WEIGHTS_DEFAULT it
// returns panda_cost's bits (tests/test_panda_cost_weights_cpu.py on a host build of this text,
// tests/test_panda_cost_weights_gpu.py on the kernels).
__device__ __forceinline__ float panda_cost(const PandaCostParams& cp, const PandaCostWeights& wt, const PandaWorld& w,
                                            const PandaObs& o, int k, const float* cube0, const float* q_half0) {
    if (cp.task == 4) {  // reach
        float goal[3] = {cube0[0], cube0[1], cube0[2]};
        if (!cp.multi_modal || k < cp.half_K) {
            goal[2] = goal[2] + cp.pre_height_diff;
        } else {
            goal[0] = goal[0] - cp.pre_height_diff * cp.tilt_cos_theta;
            goal[2] = goal[2] + cp.pre_height_diff * sqrtf(1.0f - cp.tilt_cos_theta * cp.tilt_cos_theta);
        }
        const float dx = (o.left[0] + o.right[0]) / 2.0f - goal[0];
        const float dy = (o.left[1] + o.right[1]) / 2.0f - goal[1];
        const float dz = (o.left[2] + o.right[2]) / 2.0f - goal[2];
        const float reach = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float tilt = (cp.multi_modal && k >= cp.half_K) ? cp.tilt_cos_theta : 0.0f;
        const float ori = ori_ee2cube(o.left_q, w.A.q, tilt, q_half0);
        return wt.reach_dist * reach + wt.reach_tilt * ori;
    }
    if (cp.task == 5) {  // pick
        const float dx = cp.goal[0] - w.A.p[0], dy = cp.goal[1] - w.A.p[1], dz = cp.goal[2] - w.A.p[2];
        const float gc = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float ori = ori_cube2goal(w.A.q, &cp.goal[3]);
        const float fx = (w.f_table[0] + wt.shelf_force * w.f_shelf[0]) + w.f_cubeB[0];
        const float fy = (w.f_table[1] + wt.shelf_force * w.f_shelf[1]) + w.f_cubeB[1];
        const float coll = fabsf(fx) + fabsf(fy);
        return (wt.pick_goal * gc + wt.pick_ori * ori) + ((coll > 0.1f) ? wt.collision : 0.0f);
    }
    if (cp.task == 6) {  // place
        const float dx = o.left[0] - o.right[0], dy = o.left[1] - o.right[1], dz = o.left[2] - o.right[2];
        return wt.place_grip * (1.0f - sqrtf((dx * dx + dy * dy) + dz * dz));
    }
    return 0.0f;
}

}  // namespace m3
