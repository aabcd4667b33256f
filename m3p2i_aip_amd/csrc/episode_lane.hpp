// episode_lane.hpp -- the per-lane decisions of the batched closed-loop episodes (m3_episodes_*), written
// so that the host compiler builds them too (tests/test_episodes_cpu.py checks them against the Python expressions of
// tools/closed_loop.run).  Everything here is what closed_loop.run does for its 1-env world, one episode per lane.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define M3_EP_HD __host__ __device__
#else
#define M3_EP_HD
#endif

namespace m3 {

enum { EP_SUCTION_OFF = 0, EP_SUCTION_ON = 1, EP_SUCTION_PULL_PREFERENCE = 2 };

// update_dyn_obs(t) (isaacgym_wrapper.py): forth while period / 4 < t % period < period / 4 * 3, period 100; t = tick +
// the episode's phase (t >= 0, so C's % is Python's)
M3_EP_HD inline bool ep_walk_forth(int t) {
    const int m = t % 100;
    return 25 < m && m < 75;
}

// torch.norm of a 2-vector in f32: each square rounded, then their sum (the reduction keeps one accumulator per element
// and adds them), then a correctly rounded sqrt.  No contraction into an fma.
M3_EP_HD inline float ep_norm2(float dx, float dy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float xx = dx * dx;
    const float yy = dy * dy;
    return sqrtf(xx + yy);
}

// (c) PLANNER_SIMPLE.check_task_success (task_planner.py): torch compares the f32 norm with the Python scalar 0.1 in f32,
// i.e. with 0.1f; navigation is strict, push / pull / push_pull are not.  Any other task never succeeds.
M3_EP_HD inline bool ep_success(int task, float px, float py, float gx, float gy) {
    const float d = ep_norm2(px - gx, py - gy);
    if (task == 0) return d < 0.1f;
    if (task >= 1 && task <= 3) return d <= 0.1f;
    return false;
}

// (c) closed_loop.run's collision test: float(|fx| + |fy|) > 0.1 -- the f32 sum, compared in DOUBLE, so a sum of exactly
// 0.1f (> 0.1) is a collision
M3_EP_HD inline bool ep_collision(float fx, float fy) {
    const float s = fabsf(fx) + fabsf(fy);
    return (double)s > 0.1;
}

// (b) the suction gate of tick i: run_tamp reads get_pull_preference() BEFORE its command, the world applies suction with
// it AFTER the command -- so it is the PREVIOUS command's m3_info.pull_preference (snapshotted by the pre-command kernel
// before the batched command overwrites it).  pull: cfg.suction_active stays True (compat.py); push / navigation: none.
M3_EP_HD inline int ep_gate(int mode, int prev_pull_preference) {
    if (mode == EP_SUCTION_ON) return 1;
    if (mode == EP_SUCTION_PULL_PREFERENCE) return prev_pull_preference != 0 ? 1 : 0;
    return 0;
}

}  // namespace m3
