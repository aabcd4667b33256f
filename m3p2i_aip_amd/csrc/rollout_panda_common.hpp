// rollout_panda_common.hpp -- what the panda_env kernels of rollout_panda.hip (the reference's workspace compiled in) and
// rollout_panda_scene.hip (the workspace of m3_set_panda_scene as a kernel argument) share: the world's loads from the raw
// row and from the wrapper's tensors, the solver's per-lane LDS store, the step-mode SoA rows and the refresh of the
// wrapper's views.  The same text in both translation units, so that both compile the same operations.
#pragma once
#include "m3_internal.hpp"
#include "panda_dyn.hpp"

#include <cstddef>

namespace m3 {

// raw world, 57 floats: q9 qd9 | cubeA13 | cubeB13 | dyn-obs13 (each: pos3 quat4(xyzw) linvel3 angvel3)
__device__ __forceinline__ void body_from13(const float* b, Body& o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { o.p[i] = b[i]; o.v[i] = b[7 + i]; o.w[i] = b[10 + i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) o.q[i] = b[3 + i];
}
__device__ __forceinline__ void panda_world_clear_derived(PandaWorld& w) {
    w.held = 0.0f;
    w.rel_p[0] = w.rel_p[1] = w.rel_p[2] = 0.0f;
    w.rel_q[0] = w.rel_q[1] = w.rel_q[2] = 0.0f; w.rel_q[3] = 1.0f;
    w.awake[0] = w.awake[1] = 1.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.f_table[i] = 0.0f; w.f_shelf[i] = 0.0f; w.f_cubeB[i] = 0.0f; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { w.warm_t[i] = 0.0f; w.warm_l[i] = 0.0f; }
}
__device__ __forceinline__ void panda_world_from_raw(const float* p, PandaWorld& w) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { w.q[i] = p[i]; w.qd[i] = p[9 + i]; }
    body_from13(p + 18, w.A);
    body_from13(p + 31, w.B);
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.obs_p[i] = p[44 + i]; w.obs_v[i] = p[51 + i]; }
    panda_world_clear_derived(w);
}

// env 0 of the wrapper's tensors: dof_state row = 9 x (pos, vel) interleaved
// (isaacgym_wrapper.py:98-100), root_state row = pos3 quat4 vel3 ang3 (:102-104)
__device__ __forceinline__ void panda_world_from_sim(const float* dof, const float* root, int ia, int ib, int io,
                                                     PandaWorld& w) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { w.q[i] = dof[2 * i]; w.qd[i] = dof[2 * i + 1]; }
    body_from13(root + (size_t)ia * 13, w.A);
    body_from13(root + (size_t)ib * 13, w.B);
    const float* o = root + (size_t)io * 13;
#pragma unroll
    for (int i = 0; i < 3; ++i) { w.obs_p[i] = o[i]; w.obs_v[i] = o[7 + i]; }
    panda_world_clear_derived(w);
}

// the per-lane store of the contact solver in LDS (manifold contact points: 120 floats per lane = 30 KB per wavefront; with one
// lane per sample also the gripper contacts' generalized rows: 312 floats, 78 KB), lane-strided: conflict-free, one wavefront
// per workgroup
#define PANDA_CORNER_LDS(LPS) __shared__ float corner_lds[panda_store_floats(LPS) * 64]; const CornerStore cs{corner_lds + threadIdx.x, 64}

__device__ __forceinline__ float in_vgpr(float v) {   // keep a uniform value in a vector register
    asm volatile("" : "+v"(v));
    return v;
}

// The cost hook: the one place where the rollout body (rollout_panda_body.inc) and the reach-cost body
// (panda_reach_cost_body.inc) form a step's cost, selected at compile time.  Every translation unit but
// rollout_panda_weights.hip takes this default -- panda_cost with the reference's literals, the call the bodies always made.
// rollout_panda_weights.hip defines the hook before this header, with the kernel argument `wt` (m3_set_panda_cost_weights).
#ifndef PANDA_BODY_COST
#define PANDA_BODY_COST(w, o, k, cube0, qh0) panda_cost(pa.cp, w, o, k, cube0, qh0)
#endif

// The scene hook: where the rollout body has copied the kernel-argument scene into `sc` and knows its sample index `i`
// (a_.lanes, the shadow slots and the ragged last wavefront applied).  Empty everywhere but in rollout_panda_rows.hip, which
// overwrites the workspace words of `sc` from row i of the per-sample table (panda_scene_rows.hpp) there.
#ifndef PANDA_BODY_SCENE
#define PANDA_BODY_SCENE(sc, i)
#endif

// The kernels' `wt` (the weighted families: rollout_panda_weights.hip, rollout_panda_rows.hip) as it lies in the kernel-argument
// segment (arguments are laid out like the members of a struct), read through a pointer the compiler cannot see through: named
// as an ordinary argument, the seven floats were loaded at kernel entry and held (spilled) over the whole step loop -- eight
// scalar spills more than the twin in every rollout build.  This way each step issues its own scalar load where the cost is
// formed, and nothing of the weights lives across the substeps.
// offset of the last of the listed argument types: each argument at the next multiple of its alignment
template <class Last>
constexpr size_t kernarg_offset(size_t at) { return (at + alignof(Last) - 1) / alignof(Last) * alignof(Last); }
template <class First, class Second, class... Rest>
constexpr size_t kernarg_offset(size_t at) { return kernarg_offset<Second, Rest...>(kernarg_offset<First>(at) + sizeof(First)); }
template <size_t OFFSET>
__device__ __forceinline__ PandaCostWeights kernarg_weights() {
    typedef const char __attribute__((address_space(4)))* kernarg_bytes;
    typedef const float __attribute__((address_space(4)))* kernarg_floats;
    kernarg_floats p = (kernarg_floats)((kernarg_bytes)__builtin_amdgcn_kernarg_segment_ptr() + OFFSET);
    asm volatile("" : "+s"(p));
    return PandaCostWeights{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}

// k_panda_reach_cost (rollout_panda.hip) and its weighted twin (rollout_panda_weights.hip)
constexpr int RC_TS = 4, RC_CH = 32;      // time slices per workgroup; steps per LDS chunk

// ======================= step mode ======================================================
// SoA world rows (NWP = 77): q 0-8 | qd 9-17 | cubeA 18-30 (pos3 quat4 vel3 angvel3) | cubeB 31-43 | plate pos 44-46,
// vel 47-49 | held 50 | rel_p 51-53 | rel_q 54-57 | awake 58-59 | f_table 60-62 | f_shelf 63-65 | f_cubeB 66-68 |
// warm_t 69-72 | warm_l 73-76
__device__ __forceinline__ void psoa_load(const float* wd, int Kl, int i, PandaWorld& w) {
    const float* p = wd + i;
    auto body = [&](int r0, Body& b) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { b.p[j] = p[(r0 + j) * Kl]; b.v[j] = p[(r0 + 7 + j) * Kl]; b.w[j] = p[(r0 + 10 + j) * Kl]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) b.q[j] = p[(r0 + 3 + j) * Kl];
    };
#pragma unroll
    for (int j = 0; j < 9; ++j) { w.q[j] = p[j * Kl]; w.qd[j] = p[(9 + j) * Kl]; }
    body(18, w.A);
    body(31, w.B);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        w.obs_p[j] = p[(44 + j) * Kl]; w.obs_v[j] = p[(47 + j) * Kl]; w.rel_p[j] = p[(51 + j) * Kl];
        w.f_table[j] = p[(60 + j) * Kl]; w.f_shelf[j] = p[(63 + j) * Kl]; w.f_cubeB[j] = p[(66 + j) * Kl];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { w.rel_q[j] = p[(54 + j) * Kl]; w.warm_t[j] = p[(69 + j) * Kl]; w.warm_l[j] = p[(73 + j) * Kl]; }
    w.held = p[50 * Kl];
    w.awake[0] = p[58 * Kl]; w.awake[1] = p[59 * Kl];
}
__device__ __forceinline__ void psoa_store(float* wd, int Kl, int i, const PandaWorld& w) {
    float* p = wd + i;
    auto body = [&](int r0, const Body& b) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { p[(r0 + j) * Kl] = b.p[j]; p[(r0 + 7 + j) * Kl] = b.v[j]; p[(r0 + 10 + j) * Kl] = b.w[j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) p[(r0 + 3 + j) * Kl] = b.q[j];
    };
#pragma unroll
    for (int j = 0; j < 9; ++j) { p[j * Kl] = w.q[j]; p[(9 + j) * Kl] = w.qd[j]; }
    body(18, w.A);
    body(31, w.B);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        p[(44 + j) * Kl] = w.obs_p[j]; p[(47 + j) * Kl] = w.obs_v[j]; p[(51 + j) * Kl] = w.rel_p[j];
        p[(60 + j) * Kl] = w.f_table[j]; p[(63 + j) * Kl] = w.f_shelf[j]; p[(66 + j) * Kl] = w.f_cubeB[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { p[(54 + j) * Kl] = w.rel_q[j]; p[(69 + j) * Kl] = w.warm_t[j]; p[(73 + j) * Kl] = w.warm_l[j]; }
    p[50 * Kl] = w.held;
    p[58 * Kl] = w.awake[0]; p[59 * Kl] = w.awake[1];
}

// SoA world of environment i -> the wrapper's views (link poses through the forward kinematics)
template <class SC>
__device__ __forceinline__ void panda_push_views(const SC& sc, const SimViews& v, int i, const PandaWorld& w) {
    if (v.dof_state) {
        float* d = v.dof_state + (size_t)i * 18;
#pragma unroll
        for (int j = 0; j < 9; ++j) { d[2 * j] = w.q[j]; d[2 * j + 1] = w.qd[j]; }
    }
    auto body13 = [&](const Body& b, float* o) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { o[j] = b.p[j]; o[7 + j] = b.v[j]; o[10 + j] = b.w[j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) o[3 + j] = b.q[j];
    };
    if (v.root_state) {
        float* base = v.root_state + (size_t)i * v.n_actors * 13;
        body13(w.A, base + v.box_actor * 13);
        body13(w.B, base + v.dyn_actor * 13);
        float* o = base + v.obs_actor * 13;      // the plate: position and linear velocity (it does not rotate)
#pragma unroll
        for (int j = 0; j < 3; ++j) { o[j] = w.obs_p[j]; o[7 + j] = w.obs_v[j]; }
    }
    if (v.rigid_body_state) {
        float* base = v.rigid_body_state + (size_t)i * v.n_bodies * 13;
        body13(w.A, base + v.box_body * 13);
        body13(w.B, base + v.dyn_body * 13);
        float* o = base + v.obs_body * 13;
#pragma unroll
        for (int j = 0; j < 3; ++j) { o[j] = w.obs_p[j]; o[7 + j] = w.obs_v[j]; }
        // robot links: bodies robot_body .. robot_body + 10 (link0..7, hand, left, right)
        float links[11 * 7];
        Frame hand;
        float pl[3], pr[3];
        panda_fk<true>(sc, w.q, hand, pl, pr, links);
        for (int l = 0; l < 11; ++l) {
            float* ol = base + (v.robot_body + l) * 13;
            for (int j = 0; j < 7; ++j) ol[j] = links[l * 7 + j];
            for (int j = 7; j < 13; ++j) ol[j] = 0.0f;  // link velocities are not reported
        }
    }
    if (v.net_contact_force) {
        float* f = v.net_contact_force + (size_t)i * v.n_bodies * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            f[v.table_body * 3 + j] = w.f_table[j];
            f[v.shelf_body * 3 + j] = w.f_shelf[j];
            f[v.dyn_body * 3 + j] = w.f_cubeB[j];
        }
    }
}

}  // namespace m3
