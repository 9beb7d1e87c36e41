// faasbal_plan.h -- internal, host only: the launch plan of a tick.
//
// plan_tick is the one statement of the rules that pick a tick's launch sequence (DESIGN.md
// §3, §12): a pure function of the context kind, the shapes, the device facts, the state
// the last launches left and the fb_set_path knobs.  It calls no HIP runtime function,
// touches no fb_ctx and allocates nothing (it runs on every launch, on the host-observed
// path); faasbal_api.hip's enqueue_tick builds its input and walks its output, and
// tests/test_plan.py runs it without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "faasbal_layout.h"

namespace fb {

// ---------------------------------------------------------------------------------------
// fb_set_path: the launch sequences of other table sizes on small (oracle-checkable) inputs
// (test paths; DESIGN.md §12 describes each knob)
struct PathKnobs {
    int force_plan = 0;    // "plan": 1 the k_plan2 + k_emit2 path, 2 the chunked k_emit (R > 128)
    int rs_wide = 1;       // 0: 8-bit sort digits only (the path past kRsWideMaxBlocks tiles)
    int logscan = -1;      // -1 auto (k_logscan for large tables when the bitmap fits in LDS)
    int split_slots = -1;  // -1 auto (separate k_slots launch once the records outgrow L2)
    int ev_ll = 1;         // 0: always the radix sort
    int gp_on = 1;         // "gp" 0: large one-GPU tables run k_plan2
    int win_direct = 1;    // 0: k_emit_win chunks by ticket
    int xself_on = 1;      // "xself" 0: k_xscan's last workgroup prefixes the chunks
    int wfirst_on = 1;     // "wfirst" 0: phase-1 k_scan queue blocks first
    int gpcheck = 0;       // 1: diagnostic (stamps builds)
    int cmix_on = 1;       // "cmix": k_emit2 role interleave
    int wtiles = 0;        // slot tiles per k_scan W workgroup (0 auto)
    int qtiles = 0;        // 1 = one queue block per k_scan Q workgroup (0 auto: 4)
    int lazy_on = 1;       // "lazy" 0: commits clear their orphaned log entries
    int xcfirst_on = 1;    // "xcfirst" 0: k_emit_shard_xp's compaction workgroups last
    int xplan_on = 1;      // "xplan" 0: large queues take the phase-2 k_scan path
    // the next fb_tick_wait overwrites the device-reported queue length with this value
    // before validating it (tests of check_lengths; -1 = off)
    int fault_qlen = -1;
};

struct PathKnob {
    const char *name;
    int PathKnobs::*member;
    int n_allowed;  // 0: any value
    int allowed[4];
};

constexpr PathKnob kPathKnobs[] = {
    {"plan", &PathKnobs::force_plan, 3, {0, 1, 2}},
    {"logscan", &PathKnobs::logscan, 3, {-1, 0, 1}},
    {"split_slots", &PathKnobs::split_slots, 3, {-1, 0, 1}},
    {"ev_ll", &PathKnobs::ev_ll, 2, {0, 1}},
    {"rs_wide", &PathKnobs::rs_wide, 2, {0, 1}},
    {"fault_qlen", &PathKnobs::fault_qlen, 0, {}},
    {"xplan", &PathKnobs::xplan_on, 2, {0, 1}},
    {"gp", &PathKnobs::gp_on, 2, {0, 1}},
    {"win_direct", &PathKnobs::win_direct, 2, {0, 1}},
    {"xself", &PathKnobs::xself_on, 2, {0, 1}},
    {"wfirst", &PathKnobs::wfirst_on, 2, {0, 1}},
    {"gpcheck", &PathKnobs::gpcheck, 2, {0, 1}},
    {"cmix", &PathKnobs::cmix_on, 2, {0, 1}},
    {"wtiles", &PathKnobs::wtiles, 4, {0, 1, 2, 4}},
    {"qtiles", &PathKnobs::qtiles, 3, {0, 1, 4}},
    {"lazy", &PathKnobs::lazy_on, 2, {0, 1}},
    {"xcfirst", &PathKnobs::xcfirst_on, 2, {0, 1}},
};

inline bool knob_allows(const PathKnob &k, int value) {
    return k.n_allowed == 0 || std::find(k.allowed, k.allowed + k.n_allowed, value) != k.allowed + k.n_allowed;
}

// ---------------------------------------------------------------------------------------
// Exchange buffer of a sharded tick, summed by one uint8 all-reduce: every byte
// has at most one nonzero contributor (the owner of the slot, event or position),
// so the SUM is exact -- except the block rows, whose bytes are 4-bit digits that at
// most kXRowsMaxWorld ranks add (<= 240).  [rec, c8) -- two copies of the per-rank
// records (by launch parity), the event regions -- is zero before phase 1 (a memset, or
// for an idle tick the previous phase 2's zeroing of this parity's records); c8 and the
// rows are written in full.
struct XLayout {
    size_t rec, front, back, evs, c8, rows, grows, total;
};
// The phase-2 form of a sharded tick of this shape: 0 phase 2 re-counts the exchanged c
// values (k_scan) -- > 16 ranks or a table wider than kRFused rows; 1 phase 1 exchanges
// its per-block round counts as digit rows, a one-launch phase 2 sums them (<= kXRowsMaxBlocks
// queue blocks); 2 (xplan; larger queues, R = kXGroupR, configs[3]: 3.5 K blocks) the same
// digit rows, whose per-block prefixes k_xscan scans before k_emit_shard
inline int xrows_mode(int world, int R, int64_t Qlog) {
    const int64_t nbq = std::max<int64_t>(1, cdiv(Qlog, kBS));
    if (world > kXRowsMaxWorld || world * kXRecLines > kBS || R > kRFused) return 0;
    // (the one-launch phase 2 walks the digit rows and this rank's rows in the same rounds:
    // their parts per column must agree, as they do for the 32 / 64 / 128-row tables)
    if (nbq <= kXRowsMaxBlocks && xr_parts(R) == kBS / (R / 4)) return 1;
    return (nbq > kXRowsMaxBlocks && R == kXGroupR) ? 2 : 0;  // (k_xscan decodes 32-round rows)
}
inline size_t xrows_bytes(int world, int R, int64_t Qlog) {
    const int64_t nbq = std::max<int64_t>(1, cdiv(Qlog, kBS));
    return xrows_mode(world, R, Qlog) ? (size_t)nbq * xr_row(R) : 0;
}
// ... and the group rows (one-launch form, R = kXGroupR only)
inline size_t xgrows_bytes(int world, int R, int64_t Qlog) {
    if (R != kXGroupR || xrows_mode(world, R, Qlog) != 1) return 0;
    const int64_t nbq = std::max<int64_t>(1, cdiv(Qlog, kBS));
    return (size_t)cdiv(nbq, kXGroupBlocks) * xg_row(R);
}
// The rows a tick of this shape exchanges under the knobs: fb_exchange_bytes sizes the
// buffer with them and plan_tick lays it out with them
// (fb_set_path("xplan", 0): large queues re-count in a phase-2 k_scan, no rows)
struct XRows {
    size_t rows, grows;
};
inline XRows exchange_rows(const PathKnobs &k, int world, int R, int64_t Qlog) {
    const bool xoff = !k.xplan_on && xrows_mode(world, R, Qlog) == 2;
    return {xoff ? 0 : xrows_bytes(world, R, Qlog), xgrows_bytes(world, R, Qlog)};
}
// xcw: bytes per exchanged c (1 while the round table has <= kRFused rows, else 2)
inline XLayout xlayout(int world, int64_t E, int64_t Qlog, int xcw = 1, size_t rows = 0, size_t grows = 0) {
    XLayout x;
    x.rec = 0;
    x.front = (size_t)2 * 8 * kXRecWords * world;
    x.back = x.front + 4 * (size_t)E;
    x.evs = x.back + 4 * (size_t)E;
    x.c8 = (x.evs + (size_t)E + 1) & ~(size_t)1;  // 2-byte aligned for the wide form
    x.rows = (x.c8 + (size_t)xcw * (size_t)Qlog + 15) & ~(size_t)15;
    x.grows = (x.rows + rows + 15) & ~(size_t)15;
    x.total = (x.grows + grows + 15) & ~(size_t)15;
    return x;
}
inline int xc_width(int R) { return R > kRFused ? 2 : 1; }

// The rows of the round table for a largest free count: the smallest power of two >= 32 that
// holds it, saturating at `limit` (a power of two: kMaxR, sharded kShardMaxR) -- any int32
// ends the loop, and a count beyond the limit gets the limit's table, which is exact up to
// the fill level fill_verdict (faasbal_fill.h) accepts
inline int choose_R(int32_t maxc, int limit = kMaxR) {
    int R = 32;
    while (R < maxc && R < limit) R <<= 1;
    return R;
}

// ---------------------------------------------------------------------------------------
// Whether the tick about to launch runs as a window tick, and how much of
// the window it scans: the tasks (T plus about the last tick's orphans), the positions
// between them that are no longer live, a slack that grows whenever a window tick missed
// its first unserved element.  Only level-0 ticks qualify (the last tick was one), with
// messages (the purge rides in k_ev_apply_ll's launch), on the linked-list path.
struct WindowIn {
    bool win_cap;  // the context can run window ticks (buffers allocated)
    int mode;      // fb_set_window: -1 auto (large tables), 0 off, 1 on
    bool lists, ev_ll, compact, purge_only, deque, shard;
    int E, W, max_lds, last_L;
    int64_t T, last_O, win_slack, Qn, qoff, qcap;
};
inline bool plan_window(const WindowIn &w, int &nchW) {
    if (!w.win_cap || w.mode == 0 || w.E <= 0 || !w.lists || !w.ev_ll || w.compact || w.purge_only || w.deque ||
        w.shard)
        return false;
    if (w.mode < 0 && w.last_L != 0) return false;  // auto: after a level-0 tick
    if (w.mode > 0 && w.last_L > 0) return false;
    const int64_t want = (w.T + 2 * w.last_O + 256) * 5 / 4 + w.win_slack;
    const int64_t scan = std::min<int64_t>(w.Qn, want);
    if (w.mode < 0 && scan * 2 > w.Qn) return false;  // auto: only when most of the queue stays put
    const int n = (int)cdiv(scan, kWinCh);
    if (n == 0) return false;
    if (logscan_bitmap_lds(w.W).bytes > (size_t)w.max_lds) return false;  // k_logscan's bitmap in LDS
    const int nchB = (int)cdiv(w.E, kWinCh);
    if (2 * nchB + n > kWinMaxCh) return false;
    // room for the appends (backs, served workers with c > 1) behind the window
    // (an underestimate only costs a rerun: k_emit_win flags a store past the buffer)
    if (w.qoff + w.Qn + (int64_t)w.E + w.T + w.last_O + 1024 > w.qcap) return false;
    nchW = n;
    return true;
}

// ---------------------------------------------------------------------------------------
// The facts plan_tick's rules read, and nothing else.
struct PlanIn {
    // context kind
    int shard = 0, phase = 0, world = 1;  // sharded rank; 1 / 2: the phase being enqueued
    int deque = 0;
    bool heartbeat = false;  // one-GPU heartbeat context (in-flight budgets, deferred clears)
    bool lists = false;      // messages can be grouped by linked lists (k_ev_link's buffers exist)
    bool qaos = false;       // the committed queue carries its free counts and heartbeats by position
    int compact = 0;         // fb_set_compact
    bool cout = false;       // fb_set_compact_out: registered pinned outputs, and their capacities
    int64_t cout_cap = 0, cout_ecap = 0, cout_ocap = 0;
    // shapes
    int W = 0, W_global = 0, E = 0, R = 32;
    int64_t head = 0, head_local = 0, Qn = 0, T = 0;
    // device facts
    int ncu = 0, max_lds = 0, win_occ = 0;
    // per-launch state
    bool l_win = false;  // plan_window said yes (and no rerun took it back) ...
    int l_nchW = 0;      // ... for this many window chunks
    bool pos_ok = true;  // the window's slot positions are exact (else a window tick rebuilds them)
    bool l_resort = false, l_purge_only = false;
    bool stale_any = false;  // lazy clears: entries of dead registrations may be in the log
    // the last tick's deferred commit, if it is still pending
    bool cm_pending = false, cm_oseg = false;
    int cm_E = 0, cm_win = 0, cm_n_clr = 0, cm_shard = 0, cm_oseg_tiles = 0;
    int64_t cm_n_orph = 0;
    PathKnobs knobs;
};

// A launch of the tick, named by its fb_timing_read label (pos_rebuild and orph_gather
// carry none).  plan: k_plan / k_plan2, or sharded k_xscan; emit: the tick kind's emission.
enum class Stage : uint8_t {
    pos_rebuild, commit, ev_link, ev_apply, rs_sort, slots, scan, logscan, plan, scan2, emit, orph_gather
};
inline const char *stage_name(Stage s) {
    constexpr const char *n[] = {"pos_rebuild", "commit", "ev_link", "ev_apply", "rs_sort", "slots",
                                 "scan", "logscan", "plan", "scan2", "emit", "orph_gather"};
    return n[(int)s];
}
enum class TickKind : uint8_t { window, shard_phase1, shard_phase2, local };
enum class Grouping : uint8_t { none, lists, sort };  // how the messages are grouped per slot
// the last tick's deferred commit: stays pending / its own launch first / extra blocks of
// this tick's k_ev_link / folded into this (idle) tick's k_scan (TickArgs cm_*)
enum class CommitPlan : uint8_t { none, first, in_ev_link, in_scan };
enum class PlanError : uint8_t { none, group_rows, sort_passes, shard_rows };

// What the plan decides beyond the flags it writes into TickArgs.
struct TickPlan {
    TickKind kind = TickKind::local;
    Grouping grouping = Grouping::none;
    int passes = 0, db = 0, rs_blocks = 0;  // the sort: passes of db-bit digits over rs_blocks tiles
    bool wide = false;
    int ev_wtiles = 1;  // linked lists: slot tiles per purge workgroup of k_ev_apply_ll's launch
    int nbf = 0;        // log tiles (TickArgs nbf is 0 for deque contexts: no log scan)
    int ls_grid = 1;    // k_logscan's workgroups
    bool gplan = false;  // large one-GPU tables for k_emit2: group rows, scanned by k_plan2
    bool sgrp = false;   // sharded phase 2 with <= 128 rows and no block rows: group rows, no k_plan
    XLayout xl{};
    size_t xrb = 0, xgb = 0;  // exchanged block rows / group rows (bytes; 0: none)
    bool l_compact = false, l_cout = false, l_oseg = false;
    CommitPlan commit = CommitPlan::none;
    PlanError err = PlanError::none;
    int n_stages = 0;
    Stage stages[16] = {};
};

// The launch plan of the tick `in` describes: the selection flags go straight into the
// TickArgs fields the kernels read (`a` arrives zeroed), everything else into `p`.
inline void plan_tick(const PlanIn &in, TickArgs &a, TickPlan &p) {
    const PathKnobs &k = in.knobs;
    const int E = in.E, W = in.W, R = in.R;
    const int64_t head = in.head, Qn = in.Qn;
    const int64_t Qlog = Qn + 2 * (int64_t)E;
    const int nbw = (int)std::max<int64_t>(1, cdiv(W, kBS));
    // sharded: the log shard holds head_local entries (head is the global sequence)
    const int nbf = (int)cdiv(in.shard ? in.head_local : head, kFTile);
    const int nbq = (int)std::max<int64_t>(1, cdiv(Qlog, kBS));
    p = TickPlan{};
    p.nbf = nbf;
    auto push = [&p](Stage s) { p.stages[p.n_stages++] = s; };

    if (in.shard) {
        const XRows xr = exchange_rows(k, in.world, R, Qlog);
        p.xrb = xr.rows;
        p.xgb = xr.grows;
    }
    p.xl = xlayout(in.world, E, Qlog, xc_width(R), p.xrb, p.xgb);

    // lazy clears (one-GPU heartbeat contexts): the live test once entries of dead
    // registrations may remain in the log
    a.live_chk = (k.lazy_on && !in.shard && !in.deque && in.stale_any) ? 1 : 0;
    a.W = W;
    a.E = E;
    a.R = R;
    a.nbw = nbw;
    a.nbf = in.deque ? 0 : nbf;  // start(): nobody dies, no log scan
    a.nbq = nbq;
    a.deque = in.deque;
    a.redist = in.l_purge_only ? 0 : 1;
    a.Qn = Qn;
    a.Qlog = Qlog;
    a.head_in = head;
    a.T = in.T;
    // small round tables: k_emit derives the cross-block prefixes itself (2 launches per tick)
    // fused: k_emit2 reduces the (small) round table in every block, no k_plan launch
    a.fused = (!in.shard && !k.force_plan && R <= kRFused && (int64_t)nbq * R <= (int64_t)kTabLd * kBS * 4) ? 1 : 0;
    // large tables with R <= 128: k_emit2 after k_plan (fb_set_path("plan", 2): the chunked k_emit)
    a.segw = (!in.shard && R <= kRFused && k.force_plan != 2) ? 1 : 0;
    p.gplan = !a.fused && a.segw && !in.shard;
    p.sgrp = in.shard && in.phase == 2 && R <= kRFused && !p.xrb;
    if ((a.fused || p.gplan || p.sgrp) && !in.l_win) {  // (a window tick uses no group rows)
        // group rows: fused / sharded, about sqrt(nbq) groups of 2^gshift queue blocks (the
        // emit reads both); k_plan2, the smallest groups that make at most 64 rows (one
        // workgroup each)
        int gs = 0;
        if (a.fused || p.sgrp)
            gs = group_shift(nbq);
        else
            while (cdiv(nbq, (int64_t)1 << gs) > 64) ++gs;
        a.grp_on = 1;
        a.gshift = gs;
        a.gstride = p.sgrp ? 2 * R + 4 : R + 4;
        a.ngrp = (int)cdiv(nbq, 1 << gs);
        if (a.ngrp > 64 || (int64_t)a.ngrp * a.gstride > kGrpWords) p.err = PlanError::group_rows;
    }
    a.lds_bitmap = W <= kLdsBitmapSlots ? 1 : 0;
    // the log scan gathers one 16-byte record per in-flight entry; past 128K slots
    // (2 MB of records) those gathers miss L2, so k_slots first writes the
    // died bitmap (W/8 bytes, L2-resident) and the scan tests bits instead
    a.slots_in_scan = (k.split_slots > 0 || (k.split_slots < 0 && W > kLdsBitmapSlots)) ? 0 : 1;
    // ... or better, while the bitmap fits in one workgroup's LDS: the W-role of
    // k_scan writes it and k_logscan tests every entry against an LDS copy
    a.f_sep = (head > 0 && !in.deque && (k.logscan > 0 || (k.logscan < 0 && W > kLdsBitmapSlots)) &&
               logscan_bitmap_lds(W).bytes <= (size_t)in.max_lds && !(in.shard && in.phase == 2)) ? 1 : 0;
    if (a.f_sep) a.slots_in_scan = 1;
    // fused one-GPU ticks: O from the slot purge's in-flight counts, the orphans flagged
    // and compacted by k_emit2's log workgroups (k_scan without log blocks); not when the
    // log role was asked to run as k_logscan (fb_set_path("logscan", 1))
    const int nbfe = quarter(nbf);
    a.f_emit = (in.heartbeat && a.fused && !a.f_sep && W <= kLdsBitmapSlots && nbfe <= kFEmitMaxBlocks &&
                emit2_bitmap_lds(W).bytes <= (size_t)in.max_lds && !in.l_win) ? 1 : 0;
    // f_emit and window ticks leave their orphans in per-tile segments
    p.l_oseg = a.f_emit != 0 || in.l_win;
    p.ls_grid = std::max(1, std::min(in.ncu, (int)cdiv(nbf, kLsBS / 64)));

    if (in.l_win && !in.pos_ok) push(Stage::pos_rebuild);  // the first window tick after general ticks

    // the last tick's deferred commit: into this launch's first kernel (k_ev_link, or k_scan
    // for an idle tick after an idle tick -- decided below), else as its own launch now
    const bool ll = E > 0 && in.lists && k.ev_ll && !in.l_resort;
    const bool cm_idle = in.cm_pending && in.cm_E == 0 && !in.cm_win && in.cm_n_clr == 0 && !in.cm_shard;
    const bool cm_late = !ll && E == 0 && cm_idle;
    if (in.cm_pending && !cm_late) {
        p.commit = ll ? CommitPlan::in_ev_link : CommitPlan::first;
        if (!ll) push(Stage::commit);
    }
    if (ll) {
        // the messages grouped per slot by linked lists (no sort): two launches; the slot purge
        // (k_scan's W role) runs in k_ev_apply_ll's launch -- extra blocks for the untouched
        // slots, each owner thread for its touched slot
        p.grouping = Grouping::lists;
        p.ev_wtiles = k.wtiles ? k.wtiles : (nbw >= 1024 ? 4 : 1);
        push(Stage::ev_link);
        push(Stage::ev_apply);
    } else if (E > 0 && !(in.shard && in.phase == 2)) {
        // stable radix sort of the messages by slot
        p.grouping = Grouping::sort;
        int bits = 1;
        while ((1ll << bits) < (int64_t)(in.shard ? in.W_global : W)) ++bits;
        p.rs_blocks = (int)cdiv(E, kRsTile);
        // digits of up to 11 bits while the batch is small enough for the scatter's
        // table walk (1 M workers: two passes of 10 bits instead of three of 8)
        p.wide = k.rs_wide && p.rs_blocks <= kRsWideMaxBlocks;
        p.passes = p.wide ? (bits + 10) / 11 : (bits + 7) / 8;
        p.db = p.wide ? (bits + p.passes - 1) / p.passes : 8;
        if (p.passes > 4) {
            p.err = PlanError::sort_passes;
            return;
        }
        for (int ps = 0; ps < p.passes; ++ps) push(Stage::rs_sort);
        push(Stage::ev_apply);
    }
    a.slots_in_apply = ll ? 1 : 0;
    a.qaos = (!in.shard && in.qaos) ? 1 : 0;
    a.cq_direct = (E == 0 && a.qaos && a.segw && !in.deque) ? 1 : 0;
    // past the L2-resident sizes the purge is bandwidth-bound: skip untouched post records
    a.post_lazy = W > kLdsBitmapSlots ? 1 : 0;
    a.repl = p.gplan ? 1 : 0;  // k_plan2 writes a copy per group
    p.l_compact = in.compact && !in.shard;
    // registered pinned outputs: the compact form and the evicted slots go straight to the
    // host (fused ticks, whose orphans a gather launch after the emission sends there too)
    p.l_cout = p.l_compact && in.cout && a.fused && a.f_emit && Qlog <= in.cout_cap && W <= in.cout_ecap &&
               head <= in.cout_ocap;

    if (in.l_win) {
        // window tick (E > 0, purge in the apply launch): k_logscan writes the orphans into
        // per-tile segments and a partial count per workgroup (nothing, when no registration
        // died: died_tag); k_emit_win counts the chunks of [backs][fronts][window prefix] by
        // decoupled look-back, serves, appends and reports the window
        p.kind = TickKind::window;
        a.win = 1;
        a.wseg = 1;
        a.nbf = nbf;
        a.nchB = (int)cdiv(E, kWinCh);
        a.nchF = a.nchB;
        a.nchW = in.l_nchW;
        const int nch = emit_win_layout(a).grid();
        // few enough chunks to be resident together: chunk = workgroup index, no ticket round
        // before the element loads.  A chunk's look-back waits on lower chunks only, so the
        // direct form needs every lower-indexed workgroup resident or done -- guaranteed while
        // the whole grid fits at once (the occupancy calculator's workgroups per CU, context
        // creation), with half of it left to concurrent work on the device
        a.win_direct = (k.win_direct && 2 * (int64_t)nch <= (int64_t)in.win_occ * in.ncu) ? 1 : 0;
        a.n_lpart = head > 0 ? p.ls_grid : 0;
        if (head > 0) push(Stage::logscan);
        push(Stage::emit);
        return;
    }
    if (in.shard) {
        a.shard = in.phase == 2 ? 2 : 1;
        // (only while the log role is fused into k_scan: with k_logscan the slot blocks are
        // the short ones)
        a.wfirst = (a.shard == 1 && !a.f_sep && k.wfirst_on) ? 1 : 0;
        // sharded phase 1: 4 slot tiles per workgroup while the log role has its own launch
        // (N = 2 at configs[3]: scan 18.4 -> 17.8 us), 1 behind wfirst (N = 8: no gain)
        if (a.shard == 1) a.wtiles = k.wtiles ? k.wtiles : (a.wfirst ? 1 : 4);
        a.xcw = xc_width(R);
        a.xplan = (k.xplan_on && xrows_mode(in.world, R, Qlog) == 2) ? 1 : 0;
        // (<= 64 chunks of kXsBlocks queue blocks: 16 loads per k_emit_shard_xp thread)
        a.xself = (a.xplan && k.xself_on && cdiv(Qlog, kBS) <= 64 * kXsBlocks) ? 1 : 0;
        // k_emit_shard_xp's compaction workgroups first when they are many (configs[3], N = 2:
        // 975 beside 1 774 queue workgroups, emit 30.3 -> 26.9 us; N = 8: 244, no gain)
        const EmitShardLayout xp = emit_shard_layout(a, kXpBlocks);
        a.xcfirst = (a.xplan && k.xcfirst_on && 4 * (xp.n[kShardLog] + xp.n[kShardSlots]) > xp.n[kShardQueue]) ? 1 : 0;
        if (a.shard == 1) {
            // phase 1: own slots' purge, orphan flags and free counts into the exchange buffer
            p.kind = TickKind::shard_phase1;
            if (!a.slots_in_scan) push(Stage::slots);
            push(Stage::scan);
            if (a.f_sep) push(Stage::logscan);
            return;
        }
        p.kind = TickKind::shard_phase2;
        if (R > kShardMaxR) {
            p.err = PlanError::shard_rows;
            return;
        }
        if (p.xrb || a.xplan) {
            // exchanged block rows: k_emit_shard alone (it also zeroes the other records copy,
            // which the next tick's phase 1 writes); xplan: k_xscan's counts and prefixes of the
            // exchanged c bytes first
            if (a.xplan) push(Stage::plan);
            push(Stage::emit);
            return;
        }
        push(Stage::scan2);
        if (!a.grp_on) push(Stage::plan);  // wide tables: k_plan's column scans
        push(Stage::emit);
        return;
    }
    a.free_pre = (a.segw && a.slots_in_scan && !a.slots_in_apply && !in.deque) ? 1 : 0;
    if (cm_late) {
        // an idle tick's commit (evicted records, orphaned log entries) rides in k_scan when
        // k_scan purges the slots and reads no log entry itself
        // (per-tile orphan segments are cleared by k_emit2's log workgroups, tile by tile)
        const bool seg_ok = !in.cm_oseg || (a.f_emit && in.cm_oseg_tiles <= nbf);
        if (a.slots_in_scan && !a.slots_in_apply && (a.f_emit || a.f_sep) && !in.deque && seg_ok) {
            p.commit = CommitPlan::in_scan;
            a.cm_fold = 1;
            a.cm_tiles = in.cm_oseg ? in.cm_oseg_tiles : 0;
            a.cm_n_orph = in.cm_oseg ? 0 : in.cm_n_orph;
            a.cm_blocks = in.cm_oseg ? 0 : std::max(1, (int)cdiv(in.cm_n_orph, kBS));
        } else {
            p.commit = CommitPlan::first;
            push(Stage::commit);
        }
    }
    // large one-GPU tables (<= 64 group rows): no k_plan2 -- k_emit2's queue blocks reduce
    // the group rows, its compaction workgroups the tile counts before theirs
    if (!a.fused && a.segw && a.grp_on && !in.deque && k.gp_on && nbf <= 4096 * 4 && nbw <= 4096 * 4) {
        a.gp = 1;
        a.gpcheck = k.gpcheck;
    }
    a.cmix = (k.cmix_on && !a.fused && !a.f_emit);
    // slot tiles per k_scan W-role workgroup: unfused (large) tables 4 -- fewer, longer
    // workgroups (configs[3]: scan 16.3 -> 14.8 us with 2, tick 55.4 -> 53.4 us with 4)
    a.wtiles = k.wtiles ? k.wtiles : (a.fused ? 1 : 4);
    // queue blocks per k_scan Q-role workgroup in the same (4-tile) instance: one-GPU unfused
    // tables with ride-along queue records
    a.qtiles = (k.qtiles != 1 && a.wtiles == 4 && !a.fused && !in.deque && a.qaos && a.R <= kRFused) ? 4 : 1;
    if (!a.slots_in_scan && !a.slots_in_apply) push(Stage::slots);
    push(Stage::scan);
    if (a.f_sep) push(Stage::logscan);
    if (!a.fused && (!a.gp || a.gpcheck)) push(Stage::plan);
    push(Stage::emit);  // k_emit2 (segw) or the chunked k_emit
    if (p.l_cout && head > 0) push(Stage::orph_gather);
}

}  // namespace fb
