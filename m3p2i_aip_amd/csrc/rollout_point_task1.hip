// rollout_point_task1.hip -- the point_env rollout kernel with the reference's default sampler and the task
// `push` compiled in (rollout_point_kernel.hpp); its own translation unit so that the instances build in parallel.
#include "rollout_point_kernel.hpp"

namespace m3 {

void launch_rollout_point_push(const RolloutArgs& a, const PointScene& sc, int blocks, hipStream_t s) {
    launch_rollout_point_instance<false, 1>(a, sc, blocks, s);
}
void launch_rollout_point_push2(const RolloutArgs& a, const PointScene& sc, int blocks, int* err, hipStream_t s) {
    launch_rollout_point2_instance<1>(a, sc, blocks, err, s);
}
void launch_rollout_point_push_batch(const BatchRolloutEntry* tab, int blocks, int n, bool ref, hipStream_t s) {
    launch_rollout_point_batch_instance<false, 1>(tab, blocks, n, ref, s);
}

}  // namespace m3
