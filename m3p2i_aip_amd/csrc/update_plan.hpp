// update_plan.hpp -- which kernels an importance-weight update runs, on which view of the samples, under which sharding protocol
// and what m3_create allocates for it: decided here and nowhere else (host only; no HIP dependency, so that
// tests/native/update_plan_host.cpp can walk every input on its own).  m3_api.hip fills UpdatePlanInput from the handle, walks
// the plan (run_update_plan) and maps the refusals to their texts; the launchers of m3_internal.hpp do the rest.
// DESIGN.md section 7i3.
#pragma once

namespace m3 {

// how the ranks of a handle's sample set reach one plan -- a function of the configuration and nothing else
enum UpdateProtocol {
    UPDATE_UNSHARDED,       // K_local == K_global: no collective
    UPDATE_GATHER_REDUCE,   // sharded, cfg.shard_mix = 0: all-gather of the costs, all-reduce of the sums
    UPDATE_MIX,             // cfg.shard_mix on a single / simple-mode shard: one all-gather of small records, k_mix
    UPDATE_RECORD_1,        // cfg.shard_mix = 1, multi-modal: one all-gather of the shards' costs + top-k; five launches on all samples
    UPDATE_RECORD_2,        // cfg.shard_mix = 2: ... + minima and ladder tables; k_search mixes them, k_regen_part / k_regen_done
    UPDATE_RECORD_3         // cfg.shard_mix = 3: ... and O(K_local) work after the gather, a second small exchange (m3_update_b)
};
inline UpdateProtocol update_protocol(int shard_mix, int K_local, int K_global, bool multi_modal, bool mode_simple) {
    if (K_local == K_global) return UPDATE_UNSHARDED;
    if (!shard_mix) return UPDATE_GATHER_REDUCE;
    if (!(multi_modal && !mode_simple)) return UPDATE_MIX;
    return shard_mix == 3 ? UPDATE_RECORD_3 : shard_mix >= 2 ? UPDATE_RECORD_2 : UPDATE_RECORD_1;
}
constexpr bool update_sharded(UpdateProtocol p) { return p != UPDATE_UNSHARDED; }
// there is a record at all (M3_BUF_RECORD / M3_BUF_RECORDS_ALL, the p2p exchange block)
constexpr bool update_has_record(UpdateProtocol p) { return p >= UPDATE_MIX; }
// the record is the one-collective mix's (header | REDUCE-shaped body), read by k_mix
constexpr bool update_mix_record(UpdateProtocol p) { return p == UPDATE_MIX; }
// the multi-modal record protocols: every rank runs (part of) the update on all K_global samples after the gather, so ...
constexpr bool update_record_protocol(UpdateProtocol p) { return p >= UPDATE_RECORD_1; }
// ... the noise rows of all ranks live here (the other ranks' actions are re-generated from them) ...
constexpr bool update_noise_of_all_ranks(UpdateProtocol p) { return update_record_protocol(p); }
// ... and the shard's costs are the head of its record (M3_BUF_TRAJ_COST aliases it)
constexpr bool update_costs_head_record(UpdateProtocol p) { return update_record_protocol(p); }
// the records carry the shards' minima and ladder tables
constexpr bool update_records_carry_tables(UpdateProtocol p) { return p >= UPDATE_RECORD_2; }
// there is a second record (M3_BUF_RECORD_B) and channel 1 of the p2p exchange
constexpr bool update_second_record(UpdateProtocol p) { return p == UPDATE_RECORD_3; }

struct UpdatePlanInput {
    UpdateProtocol protocol;
    int K_local, K_global, T, nu;
    bool multi_modal, mode_simple;   // cfg's, as they stand (mode_simple takes the single-mode kernels)
    bool fused;                      // UPDATE_ENTRY_UPDATE only: the finalize is fused into the update (else phases)
    bool five_launches;              // m3_set_update_launches(h, 5)
    bool rollout_minima;             // the costs are this command's rollout's: its workgroups left the rows of minima
};
constexpr bool update_multi(const UpdatePlanInput& in) { return in.multi_modal && !in.mode_simple; }

// ---- the size ranges, each stated once ----------------------------------------------------------------------------------------
constexpr int UPDATE_FUSE_MAX_PLAN = 2048;      // T * nu of a plan that k_wsum's last workgroup stages in 8 KB of LDS
constexpr int UPDATE_SMALL_MAX_K_PANDA = 4096;  // k_update_small: nu = 9
constexpr int UPDATE_SMALL_MAX_K_MULTI = 8192;  // ... nu = 2 with cfg.multi_modal: 32 register rows of 256 costs (a C5 shard's size)
constexpr int UPDATE_SMALL_MAX_K = 16384;       // ... nu = 2 else: 64 register rows (the north-star size)
constexpr int UPDATE_LARGE_MIN_K = 4096;        // the three-launch form: above this ...
constexpr int UPDATE_LARGE_MAX_K = 131072;      // ... up to this

// fuse: a command on an unsharded handle lets the update's last workgroup do k_finalize's work
inline bool can_fuse_finalize(const UpdatePlanInput& in) {
    return !update_sharded(in.protocol) && (long long)in.T * in.nu <= UPDATE_FUSE_MAX_PLAN;
}
// k_update_small, the whole update in one launch: unsharded with the finalize fused in, or the local softmin of a one-collective
// mix rank.  (cfg.multi_modal as it stands: mppi_mode 'simple' takes the single-mode kernel, with the multi-modal bound.)  The
// template instance is update_small.hip's choice (update_small_instance).
inline bool update_small_applies(const UpdatePlanInput& in) {
#ifdef M3_EXP_SPLIT_UPDATE   // (experiment build: the multi-launch path at every size)
    return false;
#endif
    const bool mix = update_mix_record(in.protocol);
    if (mix ? (in.multi_modal || in.fused) : (update_sharded(in.protocol) || !in.fused)) return false;
    const int K = mix ? in.K_local : in.K_global;
    const int kmax = (in.nu != 2) ? UPDATE_SMALL_MAX_K_PANDA : in.multi_modal ? UPDATE_SMALL_MAX_K_MULTI : UPDATE_SMALL_MAX_K;
    return K <= kmax && (in.nu == 2 || in.nu == 9);
}
// the three-launch form (k_mins or the rollout's minima, k_ladder_search, k_regen_part / k_regen_done with loaded actions): an
// unsharded multi-modal handle in this range has what it needs.  Up to UPDATE_SMALL_MAX_K_MULTI with nu = 2 k_update_small
// comes first.
inline bool update_large_range(const UpdatePlanInput& in) {
    return !update_sharded(in.protocol) && update_multi(in) && in.K_global > UPDATE_LARGE_MIN_K && in.K_global <= UPDATE_LARGE_MAX_K &&
           (long long)in.T * in.nu <= UPDATE_FUSE_MAX_PLAN;
}

// what m3_create allocates for the forms the handle's plans can take
struct UpdateAlloc {
    bool large_form;      // the three-launch form's wave_min rows and lflag words
    bool partials_all;    // wpart / apart sized for launches that cover all K_global samples in k_regen_part's chunks
    bool record, record_b, noise_all;   // M3_BUF_RECORD(S_ALL); M3_BUF_RECORD(S)_B(_ALL); the noise rows of all ranks + local_top_idx
};
inline UpdateAlloc update_alloc(const UpdatePlanInput& in) {
    const bool large = update_large_range(in);
    return {large, large || update_record_protocol(in.protocol), update_has_record(in.protocol),
            update_second_record(in.protocol), update_noise_of_all_ranks(in.protocol)};
}

// ---- the plans ----------------------------------------------------------------------------------------------------------------
enum UpdateEntry {
    UPDATE_ENTRY_UPDATE,            // m3_update (in.fused: the update of a command)
    UPDATE_ENTRY_UPDATE_FINALIZE,   // m3_update_finalize, m3_command
    UPDATE_ENTRY_UPDATE_B,          // m3_update_b
    UPDATE_ENTRY_FINALIZE           // m3_finalize
};
enum UpdateLaunch {   // the launch_* functions of m3_internal.hpp
    UPDATE_LAUNCH_MINS, UPDATE_LAUNCH_LADDER, UPDATE_LAUNCH_WEIGHTS, UPDATE_LAUNCH_WSUM, UPDATE_LAUNCH_FINALIZE,
    UPDATE_LAUNCH_SMALL, UPDATE_LAUNCH_LADDER_SEARCH, UPDATE_LAUNCH_FUSED_LARGE,
    UPDATE_LAUNCH_LOCAL_TOPK, UPDATE_LAUNCH_MIX, UPDATE_LAUNCH_REGEN_FAST,
    UPDATE_LAUNCH_P3_SEARCH, UPDATE_LAUNCH_P3_LOCAL_WEIGHTS, UPDATE_LAUNCH_P3_DONE
};
enum UpdateView {
    UPDATE_VIEW_FILLED,   // the arguments as the handle fills them: K_local samples at k_offset of K_global
    UPDATE_VIEW_LOCAL,    // the launch sees the local shard as if it were all there is, and reports global indices
    UPDATE_VIEW_ALL       // the launch covers every sample of every rank
};
enum UpdateDest {
    UPDATE_DEST_BUFFERS,  // the handle's buffers
    UPDATE_DEST_RECORD,   // this rank's record, in its protocol's layout
    UPDATE_DEST_RECORD_B  // this rank's second record
};
struct UpdateStep {
    UpdateLaunch launch;
    UpdateView view;
    UpdateDest dest;
    bool fast, regen, fuse_finalize;   // UpdateArgs' flags of the same names
    bool rollout_minima;               // the rows of minima are the rollout's (else k_mins')
    bool ends_update;                  // the update phase ends here: error check, timing event 2
};
enum UpdateRefusal {
    UPDATE_REFUSAL_NONE,
    UPDATE_REFUSED_SHARDED,      // m3_update_finalize / m3_command on a sharded handle: the collectives go between the phases
    UPDATE_REFUSED_NOT_P3,       // m3_update_b on anything but UPDATE_RECORD_3
    UPDATE_REFUSED_LONG_PLAN     // m3_finalize of UPDATE_RECORD_2 with T * nu > UPDATE_FUSE_MAX_PLAN
};
constexpr int UPDATE_MAX_STEPS = 6;
struct UpdatePlan {
    UpdateRefusal refusal;
    int n;
    UpdateStep step[UPDATE_MAX_STEPS];
    bool ends_command;   // after the last step: the end-of-command timing event 3 and the call count ...
    bool covariance;     // ... behind the covariance step of a handle that has one
};

inline UpdateRefusal update_refusal(const UpdatePlanInput& in, UpdateEntry entry) {
    if (entry == UPDATE_ENTRY_UPDATE_FINALIZE && update_sharded(in.protocol)) return UPDATE_REFUSED_SHARDED;
    if (entry == UPDATE_ENTRY_UPDATE_B && !update_second_record(in.protocol)) return UPDATE_REFUSED_NOT_P3;
    if (entry == UPDATE_ENTRY_FINALIZE && in.protocol == UPDATE_RECORD_2 && (long long)in.T * in.nu > UPDATE_FUSE_MAX_PLAN)
        return UPDATE_REFUSED_LONG_PLAN;
    return UPDATE_REFUSAL_NONE;
}

// The refusals' texts and codes are part of the C API's contract (M3_ERR_STATE, but the long plan: M3_ERR_UNSUPPORTED).
// m3_command words the sharded refusal its own way: it says which calls to make instead.
constexpr bool update_refusal_is_state(UpdateRefusal r) { return r != UPDATE_REFUSED_LONG_PLAN; }
inline const char* update_refusal_text(UpdateRefusal r, bool from_command = false) {
    switch (r) {
        case UPDATE_REFUSED_SHARDED:
            return from_command ? "m3_command: sharded handle (K_local != K_global): call m3_rollout, m3_update, "
                                  "m3_finalize with the collective(s) in between (include/m3p2i_hip.h)"
                                : "m3_update_finalize: sharded handle (m3_update, collectives, m3_finalize)";
        case UPDATE_REFUSED_NOT_P3: return "m3_update_b: only for cfg.shard_mix = 3 handles";
        case UPDATE_REFUSED_LONG_PLAN: return "m3_finalize: shard_mix = 2 needs T * nu <= 2048";
        case UPDATE_REFUSAL_NONE: break;
    }
    return "";
}

inline void update_plan_add(UpdatePlan& p, UpdateLaunch l, UpdateView v, UpdateDest d, bool fuse, bool regen = false, bool fast = false,
                            bool rollout_minima = false) {
    p.step[p.n++] = UpdateStep{l, v, d, fast, regen, fuse, rollout_minima, false};
}

// the update phase: everything before the (first) collective of a sharded handle, the whole update of an unsharded one
inline void update_plan_update(UpdatePlan& p, const UpdatePlanInput& in) {
    const bool fuse = in.fused;
    if (update_record_protocol(in.protocol)) {
        // the rollout left the shard's costs at the head of the record: add the shard's own top-k (costs, global indices,
        // trajectories) and, with tables, its minima + ladder table
        update_plan_add(p, UPDATE_LAUNCH_LOCAL_TOPK, UPDATE_VIEW_LOCAL, UPDATE_DEST_RECORD, fuse, false, update_records_carry_tables(in.protocol));
    } else if (update_mix_record(in.protocol)) {
        // softmin over the LOCAL shard into this rank's record; the sums see the arguments as filled
        if (update_small_applies(in)) {
            update_plan_add(p, UPDATE_LAUNCH_SMALL, UPDATE_VIEW_LOCAL, UPDATE_DEST_RECORD, fuse);
        } else {
            update_plan_add(p, UPDATE_LAUNCH_WEIGHTS, UPDATE_VIEW_LOCAL, UPDATE_DEST_RECORD, fuse);
            update_plan_add(p, UPDATE_LAUNCH_WSUM, UPDATE_VIEW_FILLED, UPDATE_DEST_RECORD, fuse);
        }
    } else if (update_small_applies(in)) {
        update_plan_add(p, UPDATE_LAUNCH_SMALL, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, fuse);
    } else if (fuse && update_large_range(in) && !in.five_launches) {
        // three launches: the minima are the rows the rollout's workgroups left behind when the costs are this command's
        // rollout's, k_mins' rows otherwise (costs written by the caller)
        if (!in.rollout_minima) update_plan_add(p, UPDATE_LAUNCH_MINS, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, fuse);
        update_plan_add(p, UPDATE_LAUNCH_LADDER_SEARCH, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, fuse, false, false, in.rollout_minima);
        update_plan_add(p, UPDATE_LAUNCH_FUSED_LARGE, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, fuse, false, false, in.rollout_minima);
    } else {
        // (minima + beta ladder for the multi-modal search) -> weights (+ top-k stage A as extra workgroups) -> weighted sums
        // (+ top-k stage B as an extra workgroup when K > 4096)
        if (update_multi(in)) {
            update_plan_add(p, UPDATE_LAUNCH_MINS, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, fuse);
            update_plan_add(p, UPDATE_LAUNCH_LADDER, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, fuse);
        }
        update_plan_add(p, UPDATE_LAUNCH_WEIGHTS, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, fuse);
        update_plan_add(p, UPDATE_LAUNCH_WSUM, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, fuse);
    }
    p.step[p.n - 1].ends_update = true;
}

// the finalize phase: after the (last) collective of a sharded handle
inline void update_plan_finalize(UpdatePlan& p, const UpdatePlanInput& in) {
    p.ends_command = true;
    p.covariance = !update_record_protocol(in.protocol);
    switch (in.protocol) {
        case UPDATE_RECORD_3:   // after the second exchange: sums in rank order, best rows, plan
            update_plan_add(p, UPDATE_LAUNCH_P3_DONE, UPDATE_VIEW_ALL, UPDATE_DEST_BUFFERS, false);
            break;
        case UPDATE_RECORD_2:   // k_search mixes the shards' ladder tables, k_regen_part / k_regen_done do the rest
            update_plan_add(p, UPDATE_LAUNCH_REGEN_FAST, UPDATE_VIEW_ALL, UPDATE_DEST_BUFFERS, true, true, true);
            break;
        case UPDATE_RECORD_1: { // the unsharded kernels on all K_global samples, the weighted sums re-generating the actions
            const bool fuse = (long long)in.T * in.nu <= UPDATE_FUSE_MAX_PLAN;
            const UpdateLaunch five[4] = {UPDATE_LAUNCH_MINS, UPDATE_LAUNCH_LADDER, UPDATE_LAUNCH_WEIGHTS, UPDATE_LAUNCH_WSUM};
            for (UpdateLaunch l : five) update_plan_add(p, l, UPDATE_VIEW_ALL, UPDATE_DEST_BUFFERS, fuse, true);
            if (!fuse) update_plan_add(p, UPDATE_LAUNCH_FINALIZE, UPDATE_VIEW_ALL, UPDATE_DEST_BUFFERS, fuse, true);
            break;
        }
        case UPDATE_MIX:        // records -> the REDUCE buffer an all-reduce would hold, + finalize
            update_plan_add(p, UPDATE_LAUNCH_MIX, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, false);
            break;
        default:
            update_plan_add(p, UPDATE_LAUNCH_FINALIZE, UPDATE_VIEW_FILLED, UPDATE_DEST_BUFFERS, false);
    }
}

inline UpdatePlan update_plan(const UpdatePlanInput& in, UpdateEntry entry) {
    UpdatePlan p{};
    p.refusal = update_refusal(in, entry);
    if (p.refusal != UPDATE_REFUSAL_NONE) return p;
    switch (entry) {
        case UPDATE_ENTRY_UPDATE:
            update_plan_update(p, in);
            break;
        case UPDATE_ENTRY_UPDATE_FINALIZE: {
            UpdatePlanInput u = in;
            u.fused = can_fuse_finalize(in);
            update_plan_update(p, u);
            if (u.fused) { p.ends_command = true; p.covariance = true; }
            else update_plan_finalize(p, u);
            break;
        }
        case UPDATE_ENTRY_UPDATE_B:
            // between the two exchanges: the searches on the mixed tables (+ the global top-k), then the weights of this rank's
            // OWN samples and their weighted action sums + best rows into its second record
            update_plan_add(p, UPDATE_LAUNCH_P3_SEARCH, UPDATE_VIEW_ALL, UPDATE_DEST_BUFFERS, false, true, true);
            update_plan_add(p, UPDATE_LAUNCH_P3_LOCAL_WEIGHTS, UPDATE_VIEW_LOCAL, UPDATE_DEST_RECORD_B, false);
            update_plan_add(p, UPDATE_LAUNCH_WSUM, UPDATE_VIEW_FILLED, UPDATE_DEST_RECORD_B, false);
            break;
        case UPDATE_ENTRY_FINALIZE:
            update_plan_finalize(p, in);
            break;
    }
    return p;
}

}  // namespace m3
