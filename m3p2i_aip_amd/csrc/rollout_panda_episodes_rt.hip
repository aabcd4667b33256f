// rollout_panda_episodes_rt.hip -- the pre and post kernels of a lockstep panda_env episode set created with
// M3_PANDA_EPISODES_RUNTIME (m3_panda_episodes_create_ex): the two written-out bodies of
// k_panda_episodes_pre / _post (rollout_panda.hip) on PandaSceneRT, over the same device header under the same flags, lane e's
// workspace from row e of one of the set's two tables (panda_scene_rows.hpp; panda_episode_tables.hpp fills them):
//   pre  -- update_plan's sim.step() on row 0 of planner e's own simulator: the PLANNING table, row e the workspace that row steps
//           in (the planner's single scene, or row 0 of its per-sample rows);
//   post -- the step of row e of the real world: the WORLD table, row e the world's scenes[e] (or its single scene).
// One family for a single run-time scene and for rows: a single scene is n equal rows.  The scene is loaded after the guard and
// the early exits, as in k_psim_step_v: a lane that leaves never reads the table, every read is inside [22][n].
// New kernels only: a set created without the flag never launches one of these.
#include "m3_internal.hpp"
#include "noise_stream.hpp"
#include "panda_dyn.hpp"
#include "panda_episode_lane.hpp"
#include "panda_scene_rows.hpp"
#include "panda_step_mode.hpp"
#include "rollout_panda_common.hpp"
#include "wave_min.hpp"

namespace m3 {

// before the command: what run_tamp's state upload and update_plan's sim.step() leave in row 0 of the planner's simulator
__global__ __launch_bounds__(64) void k_panda_episodes_pre_v(const PandaSceneRT uni, const float* scene_rows, const PandaEpisodeArgs a) {
    PANDA_CORNER_LDS(1);
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.n) return;
    if (a.st[e].phase != PE_RUNNING) return;      // (an ended episode's planner is not asked any more)
    const PandaSceneRT sc = panda_scene_row_scene(uni, scene_rows, a.n, e);
    const SimViews& v = a.v;
    // (0) the rows of the planning view no step writes -- the table, the shelf stand, the robot's mount: where the planner's own
    //     simulator has them, which is where ITS workspace puts them (the views hold positions, no sizes; the set's copy of the
    //     world's views at create would show the world's).  panda_env's actors 0 .. 5 are its bodies 0 .. 5
    {
        const SimViews& pv = a.pv;
        float* root = pv.root_state + (size_t)e * pv.n_actors * 13;
        float* rb = pv.rigid_body_state + (size_t)e * pv.n_bodies * 13;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            root[pv.table_body * 13 + j] = sc.table[j];
            root[pv.shelf_body * 13 + j] = sc.shelf[j];
            root[pv.robot_actor * 13 + j] = sc.base[j];
            rb[pv.table_body * 13 + j] = sc.table[j];
            rb[pv.shelf_body * 13 + j] = sc.shelf[j];
        }
    }
    PandaWorld w;
    // (1) set_dof_state_tensor / set_actor_root_state_tensor of the world's row: k_psim_pull_v.  Everything derived (sleep flags,
    //     warm-started impulses, contact forces) is cleared and the held latch inferred from geometry there -- in the PLANNER's
    //     workspace, as its simulator does
    panda_world_from_sim(v.dof_state + (size_t)e * 18, v.root_state + (size_t)e * v.n_actors * 13,
                         v.box_actor, v.dyn_actor, v.obs_actor, w);
    panda_infer_held(sc, w);
    // (2) update_plan's sim.step(): k_psim_step_v under the targets that simulator holds
    float uu[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) uu[j] = a.kept[(size_t)e * 9 + j];
    PandaObs obs;
    panda_step(sc, w, uu, obs, cs);
    // (3) the views after that step, the link poses through the planner's base
    panda_push_views(sc, a.pv, e, w);
}
void launch_panda_episodes_pre_rows(const PandaEpisodesLaunchScene& sc, const PandaEpisodeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_panda_episodes_pre_v, dim3((a.n + 63) / 64), dim3(64), 0, s, *sc.uni, sc.plan_rows, a);
}

// after the command: trace row, the world's step of row e in row e's workspace (k_psim_step_v's body), the end of an episode
__global__ __launch_bounds__(64) void k_panda_episodes_post_v(const PandaSceneRT uni, const float* scene_rows, const PandaEpisodeArgs a,
                                                              int tick) {
    PANDA_CORNER_LDS(1);
    const int e = blockIdx.x * 64 + threadIdx.x;
    const SimViews& v = a.v;
    // everything that is not the step itself comes first and leaves nothing in registers across panda_step: from the scene's
    // load on the kernel is k_psim_step_v
    if (e >= a.n) return;
    int op;
    {
        m3_panda_episode_status st = a.st[e];
        op = pe_advance(st, a.ended[e], tick, a.last_tick, a.settle_ticks);   // (4) panda_episode_lane.hpp
        if (op != 0) a.st[e] = st;
    }
    if (!(op & PE_OP_STEP)) return;
    float uu[9];
    {
        const float* plan = a.plan[e];
#pragma unroll
        for (int j = 0; j < 9; ++j) uu[j] = pe_target(op, plan, j);
    }
    if ((op & PE_OP_TRACE) && a.trace) {   // (5) the views BEFORE the step, the action the step runs under
        float* o = a.trace + ((size_t)tick * a.n + e) * PE_TRACE_FLOATS;
        const float* d = v.dof_state + (size_t)e * 18;
        const float* r = v.root_state + (size_t)e * v.n_actors * 13;
        const float* rb = v.rigid_body_state + (size_t)e * v.n_bodies * 13;
        for (int j = 0; j < 18; ++j) o[PE_TR_DOF + j] = d[j];
        for (int j = 0; j < PE_TR_ACTION - PE_TR_ROOT; ++j) o[PE_TR_ROOT + j] = r[j];
        for (int j = 0; j < 9; ++j) o[PE_TR_ACTION + j] = uu[j];
        for (int j = 0; j < 7; ++j) {
            o[PE_TR_HAND + j] = rb[(v.robot_body + 8) * 13 + j];     // panda_hand: link 8 of the robot's 11
            o[PE_TR_CUBE + j] = rb[v.box_body * 13 + j];
        }
    }
    // set_dof_velocity_target_tensor(action) + step(): k_psim_step_v on row e
    const PandaSceneRT sc = panda_scene_row_scene(uni, scene_rows, a.n, e);
    PandaWorld w;
    psoa_load(a.world, a.n, e, w);
    PandaObs obs;
    panda_step(sc, w, uu, obs, cs);
    psoa_store(a.world, a.n, e, w);
    panda_push_views(sc, v, e, w);
    // (6) no lane steps after its episode's last step (op == 0 from then on): row e of the views KEEPS the cubes' positions the
    // serial loop reads after its loops -- m3_panda_episodes_status takes them from there
}
void launch_panda_episodes_post_rows(const PandaEpisodesLaunchScene& sc, const PandaEpisodeArgs& a, int tick, hipStream_t s) {
    hipLaunchKernelGGL(k_panda_episodes_post_v, dim3((a.n + 63) / 64), dim3(64), 0, s, *sc.uni, sc.world_rows, a, tick);
}

}  // namespace m3
