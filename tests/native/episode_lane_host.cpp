// Host build of m3p2i_aip_amd/csrc/episode_lane.hpp (the per-lane decisions of k_episodes_pre / k_episodes_post) and the
// layout of the episode structs of include/m3p2i_hip.h, for tests/test_episodes_cpu.py.
#include <cstddef>
#include "../../include/m3p2i_hip.h"
#include "../../m3p2i_aip_amd/csrc/episode_lane.hpp"

extern "C" {
int ep_walk_forth_h(int t) { return m3::ep_walk_forth(t) ? 1 : 0; }
float ep_norm2_h(float dx, float dy) { return m3::ep_norm2(dx, dy); }
int ep_success_h(int task, float px, float py, float gx, float gy) { return m3::ep_success(task, px, py, gx, gy) ? 1 : 0; }
int ep_collision_h(float fx, float fy) { return m3::ep_collision(fx, fy) ? 1 : 0; }
int ep_gate_h(int mode, int prev) { return m3::ep_gate(mode, prev); }
// sizeof and offsets: spec (task, goal, dyn_phase, suction, kp_suction), status (done_tick, success, collision_ticks, final_pos)
void ep_layout_h(long* out) {
    out[0] = sizeof(m3_episode_spec);
    out[1] = offsetof(m3_episode_spec, task); out[2] = offsetof(m3_episode_spec, goal);
    out[3] = offsetof(m3_episode_spec, dyn_phase); out[4] = offsetof(m3_episode_spec, suction);
    out[5] = offsetof(m3_episode_spec, kp_suction);
    out[6] = sizeof(m3_episode_status);
    out[7] = offsetof(m3_episode_status, done_tick); out[8] = offsetof(m3_episode_status, success);
    out[9] = offsetof(m3_episode_status, collision_ticks); out[10] = offsetof(m3_episode_status, final_pos);
    out[11] = M3_SUCTION_OFF; out[12] = M3_SUCTION_ON; out[13] = M3_SUCTION_PULL_PREFERENCE;
    out[14] = m3::EP_SUCTION_OFF; out[15] = m3::EP_SUCTION_ON; out[16] = m3::EP_SUCTION_PULL_PREFERENCE;
}
}
