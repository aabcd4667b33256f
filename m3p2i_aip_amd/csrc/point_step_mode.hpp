// point_step_mode.hpp -- device helpers of the point_env step mode shared by rollout_point.hip (k_sim_*, k_episodes_*) and
// rollout_point_scene.hip (their run-time-scene twins): the SoA world, the wrapper's views, one step of one environment.
#pragma once
#include "m3_internal.hpp"
#include "episode_lane.hpp"
#include "point_views.hpp"

namespace m3 {

__device__ __forceinline__ void soa_load(const float* wd, int Kl, int i, PointWorld& w) {
    const float* p = wd + i;
    w.rx = p[0 * Kl]; w.ry = p[1 * Kl]; w.rvx = p[2 * Kl]; w.rvy = p[3 * Kl];
    w.B.x = p[4 * Kl]; w.B.y = p[5 * Kl]; w.B.c = p[6 * Kl]; w.B.s = p[7 * Kl];
    w.B.vx = p[8 * Kl]; w.B.vy = p[9 * Kl]; w.B.w = p[10 * Kl];
    w.D.x = p[11 * Kl]; w.D.y = p[12 * Kl]; w.D.c = p[13 * Kl]; w.D.s = p[14 * Kl];
    w.D.vx = p[15 * Kl]; w.D.vy = p[16 * Kl]; w.D.w = p[17 * Kl];
    w.fRx = p[18 * Kl]; w.fRy = p[19 * Kl]; w.fBx = p[20 * Kl]; w.fBy = p[21 * Kl];
    w.fcDx = p[22 * Kl]; w.fcDy = p[23 * Kl]; w.fcBx = p[24 * Kl]; w.fcBy = p[25 * Kl];
    w.fcRx = p[26 * Kl]; w.fcRy = p[27 * Kl];
}
__device__ __forceinline__ void soa_store(float* wd, int Kl, int i, const PointWorld& w) {
    float* p = wd + i;
    p[0 * Kl] = w.rx; p[1 * Kl] = w.ry; p[2 * Kl] = w.rvx; p[3 * Kl] = w.rvy;
    p[4 * Kl] = w.B.x; p[5 * Kl] = w.B.y; p[6 * Kl] = w.B.c; p[7 * Kl] = w.B.s;
    p[8 * Kl] = w.B.vx; p[9 * Kl] = w.B.vy; p[10 * Kl] = w.B.w;
    p[11 * Kl] = w.D.x; p[12 * Kl] = w.D.y; p[13 * Kl] = w.D.c; p[14 * Kl] = w.D.s;
    p[15 * Kl] = w.D.vx; p[16 * Kl] = w.D.vy; p[17 * Kl] = w.D.w;
    p[18 * Kl] = w.fRx; p[19 * Kl] = w.fRy; p[20 * Kl] = w.fBx; p[21 * Kl] = w.fBy;
    p[22 * Kl] = w.fcDx; p[23 * Kl] = w.fcDy; p[24 * Kl] = w.fcBx; p[25 * Kl] = w.fcBy;
    p[26 * Kl] = w.fcRx; p[27 * Kl] = w.fcRy;
}

// SoA world of environment i -> the wrapper's views (what a refresh_*_tensor call of Isaac Gym does)
__device__ __forceinline__ void push_views(const SimViews& v, int i, const PointWorld& w) {
    if (v.dof_state) {
        *reinterpret_cast<float4*>(v.dof_state + (size_t)i * 4) = make_float4(w.rx, w.rvx, w.ry, w.rvy);
    }
    if (v.root_state) {
        float* base = v.root_state + (size_t)i * v.n_actors * 13;
        write_body13(base + v.box_actor * 13, w.B.x, w.B.y, w.B.c, w.B.s, w.B.vx, w.B.vy, w.B.w);
        write_body13(base + v.dyn_actor * 13, w.D.x, w.D.y, w.D.c, w.D.s, w.D.vx, w.D.vy, w.D.w);
        // (fixed base of the robot: stays at its init pose)
    }
    if (v.rigid_body_state) {
        float* base = v.rigid_body_state + (size_t)i * v.n_bodies * 13;
        write_body13(base + v.box_body * 13, w.B.x, w.B.y, w.B.c, w.B.s, w.B.vx, w.B.vy, w.B.w);
        write_body13(base + v.dyn_body * 13, w.D.x, w.D.y, w.D.c, w.D.s, w.D.vx, w.D.vy, w.D.w);
        // robot links: plane (fixed), link_x (x only), link_y (x, y)
        write_body13(base + (v.robot_body - 1) * 13, w.rx, 0.0f, 1.0f, 0.0f, w.rvx, 0.0f, 0.0f);
        write_body13(base + v.robot_body * 13, w.rx, w.ry, 1.0f, 0.0f, w.rvx, w.rvy, 0.0f);
    }
    if (v.net_contact_force) {
        float* f = v.net_contact_force + (size_t)i * v.n_bodies * 3;
        f[v.box_body * 3 + 0] = w.fcBx; f[v.box_body * 3 + 1] = w.fcBy;
        f[v.dyn_body * 3 + 0] = w.fcDx; f[v.dyn_body * 3 + 1] = w.fcDy;
        f[v.robot_body * 3 + 0] = w.fcRx; f[v.robot_body * 3 + 1] = w.fcRy;
    }
}

// one sim.step() of every environment and the refresh of the wrapper's views in the same launch
// (u_keep != u: the targets come from the caller's tensor and are kept for the steps after this one, as a
// set_dof_velocity_target_tensor in front of the step would have done)
template <class SC>
__device__ __forceinline__ void sim_step_body(const SC& sc, const SimViews& v, float* wd, const float* u, float* u_keep, int Kl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= Kl) return;
    PointWorld w;
    soa_load(wd, Kl, i, w);
    const float2 uu = *reinterpret_cast<const float2*>(u + (size_t)i * 2);
    if (u_keep != u) *reinterpret_cast<float2*>(u_keep + (size_t)i * 2) = uu;
    point_step<true>(sc, w, uu.x, uu.y);
    soa_store(wd, Kl, i, w);
    push_views(v, i, w);
}
// after the command of an episode tick: trace row, suction, step + views, collision count, the last tick's end -- the body of
// k_episodes_post (rollout_point.hip) and of its run-time-scene twin k_episodes_post_s (rollout_point_scene.hip)
template <class SC>
__device__ __forceinline__ void episodes_post_body(const SC& sc, const EpisodeArgs& a, int tick) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.n) return;
    const SimViews& v = a.v;
    const EpisodeLane L = a.lane[e];
    m3_episode_status& st = a.st[e];
    const bool live = st.done_tick < 0;
    const float* action = L.plan;            // row 0 of the plan: the velocity target of the 1-env world
    const float ux = action[0], uy = action[1];
    if (live && a.trace) {   // closed_loop.run(trace=True): robot x, y | box body x, y, qz, qw | dyn-obs root x, y | action
        float* o = a.trace + ((size_t)tick * a.n + e) * 10;
        const float* rb = v.rigid_body_state + ((size_t)e * v.n_bodies + v.box_body) * 13;
        const float* dy = v.root_state + ((size_t)e * v.n_actors + v.dyn_actor) * 13;
        o[0] = v.dof_state[(size_t)e * 4 + 0]; o[1] = v.dof_state[(size_t)e * 4 + 2];
        o[2] = rb[0]; o[3] = rb[1]; o[4] = rb[5]; o[5] = rb[6];
        o[6] = dy[0]; o[7] = dy[1];
        o[8] = ux; o[9] = uy;
    }
    const int Kl = a.n;
    float* p = a.world + e;
    if (L.suction != EP_SUCTION_OFF) {
        // check_and_apply_suction: k_sim_suction's action path with apply = 1, its expressions verbatim, and
        // (b) a gate per episode instead of one scalar for all environments.
        // (a) threshold 1.5: each episode is a 1-env "real world" (skill_utils.py: num_envs == 1), although this
        //     world's K_local is N -- m3_sim_check_and_apply_suction on it would pick 1.8.
        const float thresh = 1.5f, reach = 0.6f, kp = L.kp;
        const bool enabled = a.gate[e] != 0;
        const float ex = p[4 * Kl] - p[0 * Kl], ey = p[5 * Kl] - p[1 * Kl];   // robot -> box
        const float len = sqrtf(ex * ex + ey * ey);
        const float inv = 1.0f / len;
        float fx = 0.0f, fy = 0.0f;                                          // force on the robot
        if (inv > thresh) {
            fx = clamp500(kp * (ex * inv));
            fy = clamp500(kp * (ey * inv));
        }
        const float along = action[0] * (-ex) + action[1] * (-ey);   // action . (robot - box)
        const bool pulling = enabled && len < reach && along > 0.0f;
        if (pulling) {
            p[18 * Kl] = fx; p[19 * Kl] = fy; p[20 * Kl] = -fx; p[21 * Kl] = -fy;
        }
    }
    // step(): k_sim_step's body on row e (set_dof_velocity_target_tensor(action) in front of it)
    PointWorld w;
    soa_load(a.world, Kl, e, w);
    point_step<true>(sc, w, ux, uy);
    soa_store(a.world, Kl, e, w);
    push_views(v, e, w);
    if (!live) return;
    // (c) the dyn-obs contact force of the views after the step, as closed_loop.run reads it
    if (ep_collision(w.fcDx, w.fcDy)) st.collision_ticks += 1;
    if (tick == a.last_tick) {   // out of ticks: the episode ends unsuccessful with the state after this step
        st.done_tick = tick; st.success = 0;
        st.final_pos[0] = L.task == 0 ? w.rx : w.B.x;
        st.final_pos[1] = L.task == 0 ? w.ry : w.B.y;
    }
}

}  // namespace m3
