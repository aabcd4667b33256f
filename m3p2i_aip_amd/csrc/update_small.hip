// update_small.hip -- k_update_small: the WHOLE importance-weight update in ONE launch for the sizes of the reference's
// configs (update.hip's header comment; shared device code: update_common.hpp).
#include "update_common.hpp"

namespace m3 {

// ---------------------------------------------------------------------------------------
// Unsharded command() with K <= 4096 (C2, C3, C4): the whole update in ONE launch.
// The softmin over <= 4096 costs is a few microseconds of work for one workgroup but ~7 us as its
// own launch (dispatch + first-load latency + its reductions, all exposed between the rollout and
// the next command) -- and the multi-modal search was three launches (k_mins, k_ladder, k_weights:
// 29 us at K = 4000, most of it dispatch).  Here every one of the T column workgroups of the
// weighted sums does the softmin itself: costs AND the workgroup's action rows are loaded together
// into registers; min / sum-of-exps / argmax go through the same block reductions with the same
// element -> thread mapping as k_weights (single mode: identical eta and weights); the multi-modal
// beta searches run the reference's rule directly (m3p2i.py:24-64), all three side by side, one
// register pass + one block reduction per iteration (~0.7 us; the ladder of k_ladder only pays
// when the costs do not fit one workgroup's registers); the sums accumulate in k_wsum's order.
// Workgroup 0 also stores the weights and m3_info, workgroup T is the top-k stage, the last
// workgroup to finish does the mean update / filter (same hand-off as in k_wsum) and writes the
// adapted beta -- after every workgroup has read the old one.
template <int NU, bool MULTI, int JR, int WT = 256>
__global__ __launch_bounds__(WT) void k_update_small(const UpdateArgs a) {
#include "update_small_body.inc"
}
// Whether a command takes this kernel is the update plan's decision (update_plan.hpp: update_small_applies, the size ranges).
// The instance of a's command: template arguments (JR: register rows of 256 costs), workgroup width and top-k workgroups.
// n_cand is what the launched copy of the arguments holds.
SmallUpdateInstance update_small_instance(const UpdateArgs& a) {
    const bool multi = a.multi_modal && !a.mode_simple;
    const int rows = (a.Kg + 255) / 256;
    SmallUpdateInstance in{a.nu, multi ? 1 : 0, rows <= 8 ? 8 : 16, 256, a.n_cand};
    if (a.nu != 2) return in;
    // multi-modal with more than 2048 costs: 512-thread workgroups (half the register rows per thread: every per-row loop of
    // the kernel -- loads, ladder points, weights, sums -- halves; C3 24.2 -> 22.4 us, K = 8000 33 -> 27.7 us), ONE top-k
    // workgroup (32 rows of 256 costs).  Single mode measured no gain (panda -1 %) or a loss (C2: +10 us on the command
    // although the kernel itself is not slower -- the wider workgroups delay the next rollout's dispatch).
#ifdef M3_EXP_UPDATE_WT256   // (experiment build: the 256-thread instances)
    constexpr bool wide = false;
#else
    constexpr bool wide = true;
#endif
    if (multi && wide && rows > 8) { in.wt = 512; in.n_cand = 1; in.jr = rows > 16 ? 16 : 8; }
    else if (multi && rows > 16) in.jr = 32;
    else if (multi) {}
    else if (rows <= 16) {}
    else if (rows <= 32) in.jr = 32;
    else in.jr = 64;
    return in;
}
void launch_update_small(const UpdateArgs& a_, hipStream_t s) {
    // (a.ladder_spins: bounded wait of the in-launch ladder exchange, ~20 ms; m3_set_ladder_spins(h, 0) makes every
    // workgroup give up at once and run all its passes itself -- tests/test_hip_edge_cases.py: same decisions)
    const SmallUpdateInstance in = update_small_instance(a_);
    UpdateArgs a = a_;
    a.n_cand = in.n_cand;
    const dim3 grid(a.T + in.n_cand);
    const size_t lds = (size_t)a.T * a.nu * sizeof(float);
#define M3_LAUNCH_SMALL(NU_, MULTI_, JR_, WT_) hipLaunchKernelGGL((k_update_small<NU_, MULTI_, JR_, WT_>), grid, dim3(WT_), lds, s, a)
    // (the instances in the order they were first written here: their code keeps its place in the code object)
    if (in.nu == 2 && in.multi) {
        if (in.wt == 512) { if (in.jr == 16) M3_LAUNCH_SMALL(2, true, 16, 512); else M3_LAUNCH_SMALL(2, true, 8, 512); }
        else if (in.jr == 32) M3_LAUNCH_SMALL(2, true, 32, 256);
        else if (in.jr == 8) M3_LAUNCH_SMALL(2, true, 8, 256);
        else M3_LAUNCH_SMALL(2, true, 16, 256);
    } else if (in.nu == 2) {
        if (in.jr == 8) M3_LAUNCH_SMALL(2, false, 8, 256);
        else if (in.jr == 16) M3_LAUNCH_SMALL(2, false, 16, 256);
        else if (in.jr == 32) M3_LAUNCH_SMALL(2, false, 32, 256);
        else M3_LAUNCH_SMALL(2, false, 64, 256);
    } else if (in.multi) {
        if (in.jr == 8) M3_LAUNCH_SMALL(9, true, 8, 256); else M3_LAUNCH_SMALL(9, true, 16, 256);
    } else if (in.jr == 8) M3_LAUNCH_SMALL(9, false, 8, 256);
    else M3_LAUNCH_SMALL(9, false, 16, 256);
#undef M3_LAUNCH_SMALL
}

// ---- batched command (m3_batch_command) ---------------------------------------------------------------------------
// One workgroup of the handle tab[blockIdx.y], its own grid's workgroup blockIdx.x: the unchanged body.  The table is
// read-only during the launch (`__restrict__`); a handle's workgroups only ever meet through that handle's own counters
// and buffers (wcount, lad, cand), exactly as in its own launch.
template <bool MULTI, int JR, int WT>
__global__ __launch_bounds__(WT) void kb_update_small(const UpdateArgs* __restrict__ tab) {
    constexpr int NU = 2;
    const UpdateArgs& a = tab[blockIdx.y];
#include "update_small_body.inc"
}

// Workgroups of a batched multi-modal update resident on one CU at a time: the column workgroups of a handle wait for
// each other inside the launch (bounded), so m3_batch_command splits a group into launches whose whole grid fits the chip
// (256 CUs x this).  From the code objects of kb_update_small<true, JR, WT> (tools/codeobj_info.py: .vgpr_count = arch +
// acc, .sgpr_count, LDS): waves per SIMD = min(8, 512 / (VGPRs rounded up to 8), 800 / (SGPRs rounded up to 16, + 16)) --
// the SGPR bound is where the occupancy query reads one workgroup per CU too high for SGPR-heavy kernels -- divided by the
// workgroup's waves per SIMD (WT / 256), at most 4 workgroups of 256 threads (2 of 512) per CU; LDS (~21 KB static + the
// plan, <= 2 KB) would admit 7.  tests/test_batch_cpu.py re-derives these from the built library.
int update_small_batch_blocks_per_cu(const SmallUpdateInstance& in) {
    if (in.wt == 512) return 1;   // <true, 8 | 16, 512>: 147 VGPRs -> 3 waves per SIMD -> one workgroup of 8 waves
    if (in.jr == 32) return 2;    // <true, 32, 256>: 240 VGPRs -> 2 waves per SIMD
    return 4;                     // <true, 8 | 16, 256>: 73 / 126 VGPRs, 106 SGPRs -> 6 / 4 waves per SIMD, 4 at most
}

// The nu = 9 (panda_env) twin: a kernel of its own name, so that kb_update_small keeps exactly its instances.
template <bool MULTI, int JR>
__global__ __launch_bounds__(256) void kb_update_small9(const UpdateArgs* __restrict__ tab) {
    constexpr int NU = 9, WT = 256;
    const UpdateArgs& a = tab[blockIdx.y];
#include "update_small_body.inc"
}

// The same bound for kb_update_small9<true, JR> (the rule above; the plan in LDS is up to T * nu = 2048 floats, 8 KB):
// tests/test_batch_panda_cpu.py re-derives it from the built library.
int update_small9_batch_blocks_per_cu(const SmallUpdateInstance& in) {
    if (in.jr == 16) return 2;    // <true, 16>: 238 VGPRs -> 2 waves per SIMD
    return 4;                     // <true, 8>: 127 VGPRs -> 4 waves per SIMD
}

void launch_update_small_batch(const UpdateArgs* tab, int n, const SmallUpdateInstance& in, int T, hipStream_t s) {
    const dim3 grid(T + in.n_cand, n);
    if (in.nu == 9) {
        const size_t lds9 = (size_t)T * 9 * sizeof(float);
        if (in.multi) {
            if (in.jr == 8) hipLaunchKernelGGL((kb_update_small9<true, 8>), grid, dim3(256), lds9, s, tab);
            else hipLaunchKernelGGL((kb_update_small9<true, 16>), grid, dim3(256), lds9, s, tab);
        } else if (in.jr == 8) hipLaunchKernelGGL((kb_update_small9<false, 8>), grid, dim3(256), lds9, s, tab);
        else hipLaunchKernelGGL((kb_update_small9<false, 16>), grid, dim3(256), lds9, s, tab);
        return;
    }
    const size_t lds = (size_t)T * 2 * sizeof(float);
#define M3_LAUNCH_BATCH(MULTI_, JR_, WT_) hipLaunchKernelGGL((kb_update_small<MULTI_, JR_, WT_>), grid, dim3(WT_), lds, s, tab)
    if (in.multi) {
        if (in.wt == 512) { if (in.jr == 8) M3_LAUNCH_BATCH(true, 8, 512); else M3_LAUNCH_BATCH(true, 16, 512); }
        else if (in.jr == 8) M3_LAUNCH_BATCH(true, 8, 256);
        else if (in.jr == 16) M3_LAUNCH_BATCH(true, 16, 256);
        else M3_LAUNCH_BATCH(true, 32, 256);
    } else {
        if (in.jr == 8) M3_LAUNCH_BATCH(false, 8, 256);
        else if (in.jr == 16) M3_LAUNCH_BATCH(false, 16, 256);
        else if (in.jr == 32) M3_LAUNCH_BATCH(false, 32, 256);
        else M3_LAUNCH_BATCH(false, 64, 256);
    }
#undef M3_LAUNCH_BATCH
}

int init_ladder_table_small() { return init_ladder_table_tu(); }

}  // namespace m3
