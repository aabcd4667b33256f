// prior_controllers.hip -- the ancillary controllers of a handle with a prior controller (m3_set_prior_controller) on the
// device: the kernel that fills the handle's table of prior samples from the world the rollout is about to start from, launched
// on the handle's stream directly ahead of the rollout (m3_rollout, so m3_command as well) -- no upload, no synchronisation, no
// allocation.  The arithmetic is prior_controllers.hpp's, the world comes through the rollout's own loaders.  A translation
// unit of its own: every kernel that was in the library keeps its code.
#include "prior_controllers.hpp"
#include "rollout_point_kernel.hpp"

namespace m3 {

// One lane per sequence (c.pc.n <= M3_MAX_PRIOR_CONTROLLER_SEQS = 16 of the 64 lanes work).  Lane j walks the T steps and
// writes row j of the table [M3_MAX_PRIOR_SAMPLES][T][2], one float2 per step.  a: the command's own arguments -- the world
// (row 0 of the bound views, else world0), the goal, u_max and T are the rollout's.
__device__ __forceinline__ void prior_controllers_body(const RolloutArgs& a, const PriorControllerArgs& c) {
    const int j = threadIdx.x;
    if (j >= c.pc.n || j >= M3_MAX_PRIOR_CONTROLLER_SEQS) return;
    PointWorld w;
    if (a.sim_dof) load_world_from_sim(a.sim_dof, a.sim_root, a.sim_box, a.sim_dyn, w);
    else load_world(a.world0, w);
    const float speed = prior_controller_speed(c.pc.speed[j], a.u_max[0], a.u_max[1]);
    float2* row = reinterpret_cast<float2*>(c.tab) + (size_t)j * a.T;
    prior_controller_sequence(c.pc.kind, w.rx, w.ry, w.B.x, w.B.y, a.cp.goal[0], a.cp.goal[1], a.T, c.dt, speed, c.pc.standoff,
                              c.pc.reach, [row](int t, float ux, float uy) { row[t] = make_float2(ux, uy); });
}

__global__ __launch_bounds__(64) void k_prior_controllers(const RolloutArgs a, const PriorControllerArgs c) {
    prior_controllers_body(a, c);
}

void launch_prior_controllers(const RolloutArgs& a, const PriorControllerArgs& c, hipStream_t s) {
    hipLaunchKernelGGL(k_prior_controllers, dim3(1), dim3(64), 0, s, a, c);
}

// The batched form (m3_batch_command on a batch with the priors section): blockIdx.y picks the entry of the table's priors
// section; an entry whose table is the caller's (kind 0) has nothing to do.  One launch for all entries, ahead of the batch's
// rollout launches on the same stream.
__global__ __launch_bounds__(64) void kb_prior_controllers(const BatchRolloutEntryPR* __restrict__ tab) {
    const BatchRolloutEntryPR& e = tab[blockIdx.y];
    if (e.ctl.pc.kind == 0) return;
    prior_controllers_body(e.a, e.ctl);
}

void launch_prior_controllers_batch(const BatchRolloutEntryPR* tab, int n, hipStream_t s) {
    hipLaunchKernelGGL(kb_prior_controllers, dim3(1, n), dim3(64), 0, s, tab);
}

}  // namespace m3
