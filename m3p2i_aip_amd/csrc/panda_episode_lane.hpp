// panda_episode_lane.hpp -- the per-lane decisions of the batched panda_env episodes (m3_panda_episodes_*)
// that are not panda_step itself: what an episode does at a tick (step or not, under which targets, trace row, freeze),
// the settle count-down and the trace row's layout.  Built for the host too: m3_panda_episodes_act advances its host
// mirror of the status words with the SAME function the post kernel runs (so `act` needs no read-back), and
// tests/test_panda_episodes_cpu.py checks it against the Python expressions of tools/closed_loop.run.
#pragma once
#include "episode_lane.hpp"

namespace m3 {

enum { PE_RUNNING = 0, PE_SETTLING = 1, PE_FROZEN = 2 };                            // m3_panda_episode_status::phase
enum { PE_OP_STEP = 1, PE_OP_ZERO = 2, PE_OP_TRACE = 4, PE_OP_FREEZE = 8 };         // what a lane does at a tick

// One trace row (closed_loop.run(trace=True) on the panda_env: its `trace` and `full` rows are cut from this on the host):
// the 1-env world's dof_state row (18) | root_state row (7 actors x 13) | the action (9) | rigid-body pose of panda_hand (7) |
// of cubeA (7) -- all BEFORE the tick's step, the action the one the step runs under.
constexpr int PE_TR_DOF = 0, PE_TR_ROOT = 18, PE_TR_ACTION = 109, PE_TR_HAND = 118, PE_TR_CUBE = 125, PE_TRACE_FLOATS = 132;

// Episode e at `tick`, after the host's task planners have spoken (ended != 0: check_task_success held at this tick).
// closed_loop.run, one episode:
//   for i in range(ticks):  ... success -> break BEFORE the step;  trace row;  step under action
//   for k in range(settle_ticks if success else 0):  step under the zero action
//   cube / goal positions
// (a) a running episode steps under row 0 of its plan and traces; at tick max_ticks - 1 it ends unsuccessful AFTER that step,
//     with no settling;
// (b) a success ends the episode before its step: the tick's step is the first settle step (zero targets), or, with
//     settle_ticks = 0, no step at all -- the positions are the ones the last tick's step left;
// (c) after its last settle step the positions are frozen and the lane does nothing any more.
// S: m3_panda_episode_status (or a test's mirror of it).  Returns the PE_OP_* bits of this tick.
template <class S>
M3_EP_HD inline int pe_advance(S& st, int ended, int tick, int last_tick, int settle_ticks) {
    if (st.phase == PE_FROZEN) return 0;
    if (st.phase == PE_RUNNING) {
        if (!ended) {
            int op = PE_OP_STEP | PE_OP_TRACE;
            if (tick >= last_tick) { st.done_tick = tick; st.success = 0; st.phase = PE_FROZEN; op |= PE_OP_FREEZE; }
            return op;
        }
        st.done_tick = tick; st.success = 1; st.settle_left = settle_ticks > 0 ? settle_ticks : 0; st.phase = PE_SETTLING;
    }
    if (st.settle_left <= 0) { st.phase = PE_FROZEN; return PE_OP_FREEZE; }
    st.settle_left -= 1;
    int op = PE_OP_STEP | PE_OP_ZERO;
    if (st.settle_left == 0) { st.phase = PE_FROZEN; op |= PE_OP_FREEZE; }
    return op;
}

// velocity target j of the tick's step: row 0 of the planner's action-out (command(...)[0]) while running, the planner
// side's torch.zeros once the task is done
M3_EP_HD inline float pe_target(int op, const float* plan_row0, int j) { return (op & PE_OP_ZERO) ? 0.0f : plan_row0[j]; }

}  // namespace m3
