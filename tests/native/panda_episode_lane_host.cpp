// Host build of m3p2i_aip_amd/csrc/panda_episode_lane.hpp (the per-lane decisions of k_panda_episodes_post and of
// m3_panda_episodes_act's host mirror) and the layout of m3_panda_episode_status, for tests/test_panda_episodes_cpu.py.
#include <cstddef>
#include "../../include/m3p2i_hip.h"
#include "../../m3p2i_aip_amd/csrc/panda_episode_lane.hpp"

extern "C" {
// one pe_advance on a status word; returns the PE_OP_* bits
int pe_advance_h(m3_panda_episode_status* st, int ended, int tick, int last_tick, int settle_ticks) {
    return m3::pe_advance(*st, ended, tick, last_tick, settle_ticks);
}
float pe_target_h(int op, const float* plan_row0, int j) { return m3::pe_target(op, plan_row0, j); }
void pe_layout_h(long* out) {
    out[0] = sizeof(m3_panda_episode_status);
    out[1] = offsetof(m3_panda_episode_status, phase); out[2] = offsetof(m3_panda_episode_status, done_tick);
    out[3] = offsetof(m3_panda_episode_status, success); out[4] = offsetof(m3_panda_episode_status, settle_left);
    out[5] = offsetof(m3_panda_episode_status, cubeA); out[6] = offsetof(m3_panda_episode_status, cubeB);
    out[7] = m3::PE_RUNNING; out[8] = m3::PE_SETTLING; out[9] = m3::PE_FROZEN;
    out[10] = m3::PE_TR_DOF; out[11] = m3::PE_TR_ROOT; out[12] = m3::PE_TR_ACTION; out[13] = m3::PE_TR_HAND;
    out[14] = m3::PE_TR_CUBE; out[15] = m3::PE_TRACE_FLOATS; out[16] = M3_PANDA_EPISODE_TRACE_FLOATS;
    out[17] = m3::PE_OP_STEP; out[18] = m3::PE_OP_ZERO; out[19] = m3::PE_OP_TRACE; out[20] = m3::PE_OP_FREEZE;
}
}
