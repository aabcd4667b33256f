// Host program of the update plan for tests/test_update_plan_cpu.py: the product's csrc/update_plan.hpp compiled by g++ (it has no
// HIP dependency).  It walks the full product of the decision's inputs and compares the header's answers -- protocol predicates,
// allocation answers, refusals with code and text, and per entry point the ordered launches with their views, destinations, flags
// and tail -- with the code of m3_api.hip and update_small.hip as they stood BEFORE the header existed (commit bcfdbc8),
// transcribed below line by line onto plain structs with the handle's field names.  The launch_* functions of the transcription
// record their arguments; nothing else about them differs.  The reference is that commit, not the code under test.
// A program with its own main, so that it also runs under -fsanitize=address,undefined as it is.
//   g++ -O2 -std=c++17 update_plan_host.cpp -o update_plan_host && ./update_plan_host
#include <cstdio>
#include <cstring>

#include "../../m3p2i_aip_amd/csrc/update_plan.hpp"

namespace {
using namespace m3;

long checks = 0;
int failures = 0;

// ---- the reference: m3_api.hip / update_small.hip of bcfdbc8 -------------------------------------------------------------------
enum { M3_OK = 0, M3_ERR_STATE = -3, M3_ERR_UNSUPPORTED = -5 };   // (any three distinct values: compared by name below)
struct Config { int shard_mix, K_local, K_global, k_offset, T, nu, multi_modal, mode_simple; };
// pointers become tags: which buffer, and for the weights the offset added
enum Ptr { P_NULL, P_TRAJ_COST, P_TRAJ_COST_ALL, P_RECORD, P_RECORD_B, P_REDUCE, P_TOP_TRAJS, P_REDUCE_TOP, P_LOCAL_TOP_IDX, P_TOP_IDX,
           P_PART_MIN, P_WAVE_MIN };
struct Args {   // the fields of UpdateArgs that the chains write
    int Kg, Kl, k0, kbase, fuse_finalize, regen, fast, n_chunk_of, n_cand_of, n_cand_one, w_off, w1_off;
    Ptr Jall, record, rec_topj, rec_b, reduce, top_dst, top_idx, Jout, part_min, rec_mins;
};
struct Handle {
    Config cfg;
    bool regen, regen_fast, p3;
    bool lflag;          // h->lflag != nullptr: m3_create's fused_large
    bool five_launches, use_wave_min;
    bool wpart_all;      // m3_create sized wpart / apart for all samples
    bool own_traj_cost, own_noise, record, record_b;
    const char* err;
};
struct Launched { UpdateLaunch what; Args a; };
struct Trace {
    Launched l[8];
    int n;
    int ev2_after;     // number of launches enqueued when timing event 2 was recorded (-1: never)
    bool ev3, calls, cov;
    int rc;
};
Trace* g_t;
void rec(UpdateLaunch w, const Args& a) { g_t->l[g_t->n].what = w; g_t->l[g_t->n].a = a; g_t->n += 1; }
void launch_mins(const Args& a) { rec(UPDATE_LAUNCH_MINS, a); }
void launch_ladder(const Args& a) { rec(UPDATE_LAUNCH_LADDER, a); }
void launch_weights(const Args& a) { rec(UPDATE_LAUNCH_WEIGHTS, a); }
void launch_wsum(const Args& a) { rec(UPDATE_LAUNCH_WSUM, a); }
void launch_finalize(const Args& a) { rec(UPDATE_LAUNCH_FINALIZE, a); }
void launch_update_small(const Args& a) { rec(UPDATE_LAUNCH_SMALL, a); }
void launch_ladder_search(const Args& a) { rec(UPDATE_LAUNCH_LADDER_SEARCH, a); }
void launch_fused_large(const Args& a) { rec(UPDATE_LAUNCH_FUSED_LARGE, a); }
void launch_local_topk(const Args& a) { rec(UPDATE_LAUNCH_LOCAL_TOPK, a); }
void launch_mix(const Args& a) { rec(UPDATE_LAUNCH_MIX, a); }
void launch_regen_fast(const Args& a) { rec(UPDATE_LAUNCH_REGEN_FAST, a); }
void launch_p3_search(const Args& a) { rec(UPDATE_LAUNCH_P3_SEARCH, a); }
void launch_p3_local_weights(const Args& a) { rec(UPDATE_LAUNCH_P3_LOCAL_WEIGHTS, a); }
void launch_p3_done(const Args& a) { rec(UPDATE_LAUNCH_P3_DONE, a); }
int fail(Handle* h, int code, const char* msg) { h->err = msg; return code; }

// m3_create (245-247, 278, 287, 302-321, 327-335)
void ref_create(Handle* h) {
    const Config* c = &h->cfg;
    h->regen = c->shard_mix && c->K_local != c->K_global && c->multi_modal && !c->mode_simple;
    h->regen_fast = h->regen && c->shard_mix >= 2;
    h->p3 = h->regen && c->shard_mix == 3;
    const long long Kl = c->K_local, Kg = c->K_global, T = c->T, nu = c->nu;
    h->own_traj_cost = !h->regen;
    h->own_noise = !h->regen;
    h->record = h->record_b = false;
    if (h->regen) {
        h->record = true;
        if (h->p3) h->record_b = true;
    } else if (c->shard_mix && Kl != Kg) {
        h->record = true;
    }
    const bool fused_large = Kl == Kg && c->multi_modal && !c->mode_simple && Kg > 4096 && Kg <= 131072 && T * nu <= 2048;
    h->wpart_all = h->regen || fused_large;
    h->lflag = fused_large;
}

// fill_update_args (1692-1755), the fields the chains go on to patch
void fill_update_args(Handle* h, Args& a) {
    const Config& c = h->cfg;
    std::memset(&a, 0, sizeof(a));
    a.Kg = c.K_global; a.Kl = c.K_local; a.k0 = c.k_offset;
    a.part_min = P_PART_MIN;
    a.n_cand_of = c.K_global;      // a.n_cand = topk_workgroups(c.K_global)
    a.n_chunk_of = c.K_local;      // a.n_chunk = wsum_chunks(c.K_local)
    a.Jall = P_TRAJ_COST_ALL;
    a.top_idx = P_TOP_IDX;
    a.reduce = P_REDUCE;
    a.top_dst = (c.K_local == c.K_global) ? P_TOP_TRAJS : P_REDUCE_TOP;
    a.kbase = 0;
    a.rec_topj = P_NULL;
    a.rec_mins = P_NULL;
    a.rec_b = P_NULL;
    a.fast = 0;
    a.regen = 0;
    a.Jout = P_NULL;
}

bool mix_mode(const Handle* h) { return h->cfg.shard_mix && h->cfg.K_local != h->cfg.K_global && !h->regen; }

bool can_fuse_finalize(const Handle* h) {
    const Config& c = h->cfg;
    return c.K_local == c.K_global && (long long)c.T * c.nu <= 2048;
}

void fill_update_impl_args(Handle* h, Args& a, bool fuse) {
    fill_update_args(h, a);
    a.fuse_finalize = fuse ? 1 : 0;
    if (h->cfg.K_local == h->cfg.K_global)
        a.Jall = P_TRAJ_COST;
}

// update_small.hip (76-87).  a.n_cand == topk_workgroups(a.Kg) holds when n_cand was computed for the K the launch sees.
bool update_small_applies(const Args& a, const Config& c) {
    const bool record = a.record != P_NULL;
    if (!(a.fuse_finalize || record) || (record && (c.multi_modal || a.fuse_finalize))) return false;
    const int kmax = (c.nu != 2) ? 4096 : c.multi_modal ? 8192 : 16384;
    return a.Kl == a.Kg && a.Kg <= kmax && a.n_cand_of == a.Kg && (c.nu == 2 || c.nu == 9);
}

int update_impl(Handle* h, bool fuse) {
    const Config& c = h->cfg;
    Args a;
    fill_update_impl_args(h, a, fuse);
    if (h->regen) {
        a.Kg = c.K_local;
        a.Jall = P_RECORD;
        a.kbase = c.k_offset;
        a.n_cand_one = c.K_local <= 8192; a.n_cand_of = c.K_local;   // a.n_cand = c.K_local <= 8192 ? 1 : topk_workgroups(c.K_local)
        a.top_idx = P_LOCAL_TOP_IDX;
        a.rec_topj = P_RECORD;
        a.top_dst = P_RECORD;
        if (h->regen_fast) {
            a.fast = 1;
            a.rec_mins = P_RECORD;
        }
        launch_local_topk(a);
        g_t->ev2_after = g_t->n;
        return M3_OK;
    }
    if (mix_mode(h)) {
        a.record = P_RECORD;
        a.rec_topj = P_RECORD;
        a.reduce = P_RECORD;
        a.top_dst = P_RECORD;
        a.n_cand_of = c.K_local;
        Args aw = a;
        aw.Kg = c.K_local;
        aw.Jall = P_TRAJ_COST;
        aw.w_off = c.k_offset;
        aw.kbase = c.k_offset;
        if (update_small_applies(aw, c)) {
            launch_update_small(aw);
        } else {
            launch_weights(aw);
            launch_wsum(a);
        }
        g_t->ev2_after = g_t->n;
        return M3_OK;
    }
    if (update_small_applies(a, c)) {
        launch_update_small(a);
        g_t->ev2_after = g_t->n;
        return M3_OK;
    }
    if (fuse && h->lflag && c.multi_modal && !c.mode_simple && !h->five_launches) {
        if (h->use_wave_min) { a.part_min = P_WAVE_MIN; }
        else launch_mins(a);
        launch_ladder_search(a);
        launch_fused_large(a);
        g_t->ev2_after = g_t->n;
        return M3_OK;
    }
    if (c.multi_modal && !c.mode_simple) {
        launch_mins(a);
        launch_ladder(a);
    }
    launch_weights(a);
    launch_wsum(a);
    g_t->ev2_after = g_t->n;
    return M3_OK;
}

int m3_update(Handle* h) { return update_impl(h, false); }

int regen_finalize(Handle* h) {
    const Config& c = h->cfg;
    Args a;
    fill_update_args(h, a);
    a.regen = 1;
    if (h->regen_fast) {
        if ((long long)c.T * c.nu > 2048) return fail(h, M3_ERR_UNSUPPORTED, "m3_finalize: shard_mix = 2 needs T * nu <= 2048");
        a.fast = 1;
        a.Kl = c.K_global; a.k0 = 0;
        a.n_chunk_of = c.K_global;
        a.top_dst = P_TOP_TRAJS;
        a.fuse_finalize = 1;
        launch_regen_fast(a);
        return M3_OK;
    }
    a.Jout = P_TRAJ_COST_ALL;
    a.Kl = c.K_global; a.k0 = 0;
    a.n_chunk_of = c.K_global;
    a.top_dst = P_TOP_TRAJS;
    const bool fuse = (long long)c.T * c.nu <= 2048;
    a.fuse_finalize = fuse ? 1 : 0;
    launch_mins(a);
    launch_ladder(a);
    launch_weights(a);
    launch_wsum(a);
    if (!fuse) launch_finalize(a);
    return M3_OK;
}

int m3_update_b(Handle* h) {
    if (!h->p3) return fail(h, M3_ERR_STATE, "m3_update_b: only for cfg.shard_mix = 3 handles");
    const Config& c = h->cfg;
    {
        Args a;
        fill_update_args(h, a);
        a.regen = 1; a.fast = 1;
        a.Kl = c.K_global; a.k0 = 0;
        a.top_dst = P_TOP_TRAJS;
        launch_p3_search(a);
    }
    {
        Args a;
        fill_update_args(h, a);
        a.Kg = c.K_local;
        a.Jall = P_RECORD;
        a.kbase = c.k_offset;
        a.w_off = c.k_offset;
        a.w1_off = c.k_offset;
        a.rec_b = P_RECORD_B;
        launch_p3_local_weights(a);
    }
    {
        Args a;
        fill_update_args(h, a);
        a.reduce = P_RECORD_B;
        a.n_cand_of = 0;
        a.fuse_finalize = 0;
        launch_wsum(a);
    }
    return M3_OK;
}

int finish_command(Handle*) {   // after_finalize (the covariance step of a handle that has one), event 3, the call count
    g_t->cov = true;
    g_t->ev3 = true;
    g_t->calls = true;
    return M3_OK;
}

int m3_finalize(Handle* h) {
    if (h->p3) {
        Args a;
        fill_update_args(h, a);
        a.Kl = h->cfg.K_global; a.k0 = 0;
        launch_p3_done(a);
        g_t->ev3 = true;
        g_t->calls = true;
        return M3_OK;
    }
    if (h->regen) {
        const int rc = regen_finalize(h);
        if (rc != M3_OK) return rc;
        g_t->ev3 = true;
        g_t->calls = true;
        return M3_OK;
    }
    Args a;
    fill_update_args(h, a);
    if (mix_mode(h)) launch_mix(a);
    else launch_finalize(a);
    return finish_command(h);
}

int m3_update_finalize(Handle* h) {
    if (h->cfg.K_local != h->cfg.K_global)
        return fail(h, M3_ERR_STATE, "m3_update_finalize: sharded handle (m3_update, collectives, m3_finalize)");
    if (!can_fuse_finalize(h)) {
        const int rc = m3_update(h);
        return rc != M3_OK ? rc : m3_finalize(h);
    }
    const int rc = update_impl(h, true);
    return rc != M3_OK ? rc : finish_command(h);
}

// m3_command: the refusal ahead of the rollout; use_wave_min set around m3_update_finalize (the caller of this program sets it)
int m3_command(Handle* h) {
    if (h->cfg.K_local != h->cfg.K_global)
        return fail(h, M3_ERR_STATE, "m3_command: sharded handle (K_local != K_global): call m3_rollout, m3_update, "
                                     "m3_finalize with the collective(s) in between (include/m3p2i_hip.h)");
    return m3_update_finalize(h);
}

// ---- the comparison ------------------------------------------------------------------------------------------------------------
void expect(bool ok, const char* what, const Handle& h, int entry) {
    ++checks;
    if (ok) return;
    if (++failures <= 30)
        std::fprintf(stderr, "MISMATCH %s: entry %d shard_mix %d Kl %d Kg %d T %d nu %d multi %d simple %d five %d wave_min %d\n", what, entry,
                     h.cfg.shard_mix, h.cfg.K_local, h.cfg.K_global, h.cfg.T, h.cfg.nu, h.cfg.multi_modal, h.cfg.mode_simple, h.five_launches,
                     h.use_wave_min);
}

// what the executor's views and destinations (m3_api.hip: view_local_shard, view_all_samples, dest_record) make of a step, in the
// transcription's terms.  Fields that a view sets beyond what the old chain set for that launch are fields its kernel does not
// read (n_chunk and top_dst outside k_wsum / topk_finish; w and w1 in k_local_topk and the single-mode kernels): compared where the
// old chain set them, listed in `loose` otherwise.
Args expected_args(const Handle& h, const UpdateStep& st) {
    Handle hh = h;
    Args a;
    fill_update_impl_args(&hh, a, st.fuse_finalize);
    const Config& c = h.cfg;
    a.regen = st.regen; a.fast = st.fast;
    if (st.view == UPDATE_VIEW_LOCAL) { a.Kg = c.K_local; a.kbase = c.k_offset; a.Jall = h.regen ? P_RECORD : P_TRAJ_COST; a.w_off = a.w1_off = c.k_offset; }
    if (st.view == UPDATE_VIEW_ALL) { a.Kl = c.K_global; a.k0 = 0; a.n_chunk_of = c.K_global; a.top_dst = P_TOP_TRAJS; }
    if (st.dest == UPDATE_DEST_RECORD_B) {
        if (st.launch == UPDATE_LAUNCH_WSUM) { a.reduce = P_RECORD_B; a.n_cand_of = 0; }
        else a.rec_b = P_RECORD_B;
    } else if (st.dest == UPDATE_DEST_RECORD && update_mix_record(update_protocol(c.shard_mix, c.K_local, c.K_global, c.multi_modal, c.mode_simple))) {
        a.record = a.rec_topj = a.reduce = a.top_dst = P_RECORD;
        a.n_cand_of = c.K_local;
    } else if (st.dest == UPDATE_DEST_RECORD) {
        a.n_cand_one = c.K_local <= 8192; a.n_cand_of = c.K_local;
        a.top_idx = P_LOCAL_TOP_IDX;
        a.rec_topj = a.top_dst = P_RECORD;
        if (st.fast) a.rec_mins = P_RECORD;
    }
    if (st.regen && !st.fast) a.Jout = P_TRAJ_COST_ALL;
    if (st.rollout_minima) a.part_min = P_WAVE_MIN;
    return a;
}

void compare_step(const Handle& h, int entry, const Launched& r, const UpdateStep& st) {
    expect(r.what == st.launch, "launch", h, entry);
    const Args e = expected_args(h, st), &a = r.a;
    const bool unsharded = h.cfg.K_local == h.cfg.K_global;
    expect(a.Kg == e.Kg && a.Kl == e.Kl && a.k0 == e.k0 && a.kbase == e.kbase, "view (Kg, Kl, k0, kbase)", h, entry);
    expect(a.fuse_finalize == e.fuse_finalize && a.regen == e.regen && a.fast == e.fast, "flags", h, entry);
    // (the costs: the finalize launches of an unsharded handle read none, and there alone the new fill names the local buffer)
    const bool reads_no_costs = st.launch == UPDATE_LAUNCH_FINALIZE && unsharded;
    expect(a.Jall == e.Jall || reads_no_costs, "Jall", h, entry);
    expect(a.record == e.record && a.rec_topj == e.rec_topj && a.rec_b == e.rec_b && a.reduce == e.reduce && a.top_idx == e.top_idx &&
               a.rec_mins == e.rec_mins && a.n_cand_of == e.n_cand_of && a.n_cand_one == e.n_cand_one,
           "destination", h, entry);
    expect(a.Jout == e.Jout && a.part_min == e.part_min, "Jout / minima", h, entry);
    // loose fields: equal wherever the kernel reads them
    const bool reads_chunks = st.launch == UPDATE_LAUNCH_WSUM;   // (k_regen_part's launchers set their own)
    expect(a.n_chunk_of == e.n_chunk_of || !reads_chunks, "n_chunk", h, entry);
    const bool reads_top_dst = st.launch != UPDATE_LAUNCH_P3_DONE;   // (finalize_body<false>: the rows are in place)
    expect(a.top_dst == e.top_dst || !reads_top_dst, "top_dst", h, entry);
    const bool multi = h.cfg.multi_modal && !h.cfg.mode_simple;
    const bool writes_w = st.launch != UPDATE_LAUNCH_LOCAL_TOPK;
    expect(a.w_off == e.w_off || !writes_w, "w", h, entry);
    expect(a.w1_off == e.w1_off || !(writes_w && multi), "w1", h, entry);
}

void compare_entry(const Handle& h0, int entry, bool fused) {
    Handle h = h0;
    h.err = nullptr;
    Trace t{};
    t.ev2_after = -1;
    g_t = &t;
    const char* cmd_err = nullptr;
    int cmd_rc = M3_OK;
    switch (entry) {
        case UPDATE_ENTRY_UPDATE: t.rc = update_impl(&h, fused); break;
        case UPDATE_ENTRY_UPDATE_FINALIZE: {
            Handle hc = h;
            Trace tc{};
            g_t = &tc;
            cmd_rc = m3_command(&hc);
            cmd_err = hc.err;
            g_t = &t;
            t.rc = m3_update_finalize(&h);
            // m3_command after its refusal IS m3_update_finalize
            expect(cmd_rc != M3_OK || (tc.n == t.n && std::memcmp(tc.l, t.l, sizeof(Launched) * (size_t)t.n) == 0), "m3_command's launches", h, entry);
            break;
        }
        case UPDATE_ENTRY_UPDATE_B: t.rc = m3_update_b(&h); break;
        case UPDATE_ENTRY_FINALIZE: t.rc = m3_finalize(&h); break;
    }
    const Config& c = h.cfg;
    const UpdatePlanInput in{update_protocol(c.shard_mix, c.K_local, c.K_global, c.multi_modal, c.mode_simple), c.K_local, c.K_global, c.T, c.nu,
                             c.multi_modal != 0, c.mode_simple != 0, fused, h.five_launches, h.use_wave_min};
    const UpdatePlan p = update_plan(in, (UpdateEntry)entry);
    // refusals: code and text
    expect((t.rc == M3_OK) == (p.refusal == UPDATE_REFUSAL_NONE), "refused or not", h, entry);
    if (t.rc != M3_OK) {
        expect(p.refusal != UPDATE_REFUSAL_NONE && (t.rc == M3_ERR_STATE) == update_refusal_is_state(p.refusal), "refusal code", h, entry);
        expect(h.err && std::strcmp(h.err, update_refusal_text(p.refusal)) == 0, "refusal text", h, entry);
        expect(t.n == 0 && p.n == 0, "a refused call launches nothing", h, entry);
    }
    if (entry == UPDATE_ENTRY_UPDATE_FINALIZE) {
        const UpdateRefusal r = update_refusal(in, UPDATE_ENTRY_UPDATE_FINALIZE);
        expect((cmd_rc == M3_OK) == (r == UPDATE_REFUSAL_NONE), "m3_command refused or not", h, entry);
        if (cmd_rc != M3_OK)
            expect(cmd_rc == M3_ERR_STATE && update_refusal_is_state(r) && cmd_err && std::strcmp(cmd_err, update_refusal_text(r, true)) == 0,
                   "m3_command's refusal", h, entry);
    }
    if (t.rc != M3_OK) return;
    expect(t.n == p.n && p.n <= UPDATE_MAX_STEPS, "number of launches", h, entry);
    if (t.n != p.n) return;
    int ev2 = -1;
    for (int i = 0; i < p.n; ++i) {
        compare_step(h, entry, t.l[i], p.step[i]);
        if (p.step[i].ends_update) { expect(ev2 < 0, "one end of the update phase", h, entry); ev2 = i + 1; }
    }
    expect(ev2 == t.ev2_after, "timing event 2", h, entry);
    expect(p.ends_command == t.ev3 && p.ends_command == t.calls, "timing event 3 / call count", h, entry);
    expect((p.ends_command && p.covariance) == t.cov, "covariance step", h, entry);
}

void compare_handle(Handle& h) {
    ref_create(&h);
    const Config& c = h.cfg;
    const UpdateProtocol p = update_protocol(c.shard_mix, c.K_local, c.K_global, c.multi_modal, c.mode_simple);
    expect(update_noise_of_all_ranks(p) == h.regen && update_noise_of_all_ranks(p) == !h.own_noise, "noise of all ranks", h, -1);
    expect(update_costs_head_record(p) == h.regen && update_costs_head_record(p) == !h.own_traj_cost, "costs head the record", h, -1);
    expect(update_records_carry_tables(p) == h.regen_fast, "records carry tables", h, -1);
    expect(update_second_record(p) == h.p3, "second record", h, -1);
    expect(update_has_record(p) == (c.shard_mix && c.K_local != c.K_global), "has a record", h, -1);
    expect(update_mix_record(p) == mix_mode(&h), "mix_mode", h, -1);
    expect(update_sharded(p) == (c.K_local != c.K_global), "sharded", h, -1);
    const UpdatePlanInput in{p, c.K_local, c.K_global, c.T, c.nu, c.multi_modal != 0, c.mode_simple != 0, false, false, false};
    const UpdateAlloc ua = update_alloc(in);
    expect(ua.large_form == h.lflag, "alloc: wave_min / lflag", h, -1);
    expect(ua.partials_all == h.wpart_all, "alloc: wpart / apart", h, -1);
    expect(ua.record == h.record && ua.record_b == h.record_b && ua.noise_all == h.regen, "alloc: records, noise", h, -1);
    expect(m3::can_fuse_finalize(in) == can_fuse_finalize(&h), "can_fuse_finalize", h, -1);
    // batch_refusal (2494-2496): the arguments of a fused command
    Args u;
    fill_update_impl_args(&h, u, true);
    UpdatePlanInput inf = in;
    inf.fused = true;
    expect(m3::update_small_applies(inf) == update_small_applies(u, c), "update_small_applies (batch)", h, -1);
    for (int five = 0; five < 2; ++five)
        for (int wm = 0; wm < 2; ++wm) {
            h.five_launches = five;
            h.use_wave_min = wm;
            for (int fused = 0; fused < 2; ++fused) compare_entry(h, UPDATE_ENTRY_UPDATE, fused);
            compare_entry(h, UPDATE_ENTRY_UPDATE_FINALIZE, false);
            compare_entry(h, UPDATE_ENTRY_UPDATE_B, false);
            compare_entry(h, UPDATE_ENTRY_FINALIZE, false);
        }
}
}  // namespace

int main() {
    const int ranks[] = {1, 2, 4, 32};
    const int bounds[] = {20, 2048, 4096, 8192, 16384, 131072};
    // T per nu: the products on both sides of 2048 that the grid of each nu has (2048 | 2050; 2043 | 2052), a short horizon, and
    // -- with nu = 1, which m3_create never admits but both implementations must still answer alike -- 2048 | 2049 themselves
    const int nus[] = {2, 9, 1};
    const int Ts[3][3] = {{12, 1024, 1025}, {12, 227, 228}, {12, 2048, 2049}};
    long handles = 0;
    for (int shard_mix = 0; shard_mix <= 3; ++shard_mix)
        for (int n : ranks)
            for (int mode = 0; mode < 3; ++mode)   // single, simple, multi
                for (int ni = 0; ni < 3; ++ni)
                    for (int ti = 0; ti < 3; ++ti)
                        for (int b : bounds)
                            for (int d = -1; d <= 1; ++d)
                                for (int by_local = 0; by_local < (n > 1 ? 2 : 1); ++by_local) {
                                    // the boundary as K_global (shards of K / n) and, sharded, as K_local too
                                    const int K = b + d;
                                    Handle h{};
                                    h.cfg.shard_mix = shard_mix;
                                    h.cfg.K_local = by_local ? K : K / n;   // (K >= 19: never 0, never K itself when n > 1)
                                    h.cfg.K_global = by_local ? K * n : K;
                                    h.cfg.k_offset = n > 1 ? h.cfg.K_local : 0;   // rank 1
                                    h.cfg.T = Ts[ni][ti];
                                    h.cfg.nu = nus[ni];
                                    h.cfg.multi_modal = mode == 2;
                                    h.cfg.mode_simple = mode == 1;
                                    compare_handle(h);
                                    // (cfg.multi_modal set under mode 'simple': the single-mode kernels with the multi-modal bound)
                                    if (mode == 1) { h.cfg.multi_modal = 1; compare_handle(h); ++handles; }
                                    ++handles;
                                }
    std::printf("%ld handles, %ld checks, %d failures\n", handles, checks, failures);
    return failures ? 1 : 0;
}
