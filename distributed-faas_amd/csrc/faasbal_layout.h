// faasbal_layout.h -- internal, host and device: the grid of every multi-role kernel and the
// size of every died-bitmap staging in LDS, each stated once.
//
// A layout holds the workgroups per role (n[role], in the roles' canonical order), the grid,
// and canon(): the canonical index of a workgroup (its permutation; kPadding = the
// workgroup exits).  Role r owns the canonical indices [first(r), end(r)).  A launcher takes
// its dim3 from X_layout(args).grid(); a kernel compares canon(blockIdx.x) with first() /
// end() of X_layout(args, gridDim.x) -- the form with a grid takes the one count the kernel
// never computed from the grid, the form without states that count forwards and goes
// through the same code.  k_scan and k_emit2 call the functions their layouts are made of
// one by one instead (see there; profiles/NOTES_layouts.md has the device code's figures).
// tests/test_plan.py walks every workgroup of every planned launch through role_at() on the
// CPU (tests/plan_probe.cpp).
#pragma once
#include "faasbal_kernels.h"

#define FB_HD __host__ __device__ __forceinline__

namespace fb {

struct Role {
    int role, idx;
};
constexpr int kPadding = -1;

template <int N>
struct Roles {
    static constexpr int kRoles = N;
    int n[N];
    FB_HD int count(int r) const { return n[r]; }
    FB_HD int first(int r) const {
        int s = 0;
        for (int i = 0; i < r; ++i) s += n[i];
        return s;
    }
    FB_HD int end(int r) const { return first(r) + n[r]; }
    // canonical index bid's index in role r: bid - first(r), the earlier roles taken off one by
    // one (the kernels' own order of subtractions: the sum first costs a 64-bit sign extension)
    FB_HD int rel(int r, int bid) const {
        for (int i = 0; i < r; ++i) bid -= n[i];
        return bid;
    }
    FB_HD int canon(int blk) const { return blk; }
    FB_HD int grid() const { return end(N - 1); }
};
// the role and the index in it of workgroup blk (role kRoles: a canonical index past every role)
template <class L>
FB_HD Role role_at(const L &l, int blk) {
    const int bid = l.canon(blk);
    if (bid == kPadding) return {kPadding, 0};
    for (int r = 0; r < L::kRoles; ++r)
        if (bid < l.end(r)) return {r, bid - l.first(r)};  // (= l.rel(r, bid))
    return {L::kRoles, bid};
}

// workgroups of four wave-sized tiles (the compaction roles: a tile per wave)
FB_HD int quarter(int tiles) { return (tiles + 3) >> 2; }

// ---------------------------------------------------------------------------------------
// k_commit, and the same body in k_ev_link's extra blocks: the slots, the orphaned log
// entries (dense, or a wave per tile of the per-tile segments), the entries the tick's
// results completed, then (window ticks; nbap and n_tomb are 0 otherwise) the appended
// positions and the tomb list
enum { kCmSlots, kCmOrphans, kCmCleared, kCmAppended, kCmTombs };
struct CommitLayout : Roles<5> {};
FB_HD CommitLayout commit_layout(int nbw, int nbo, int n_clr, int nbap, int n_tomb) {
    return {{{nbw, nbo, (n_clr + kBS - 1) / kBS, nbap, (n_tomb + kBS - 1) / kBS}}};
}
FB_HD CommitLayout commit_layout(const CommitArgs &a) { return commit_layout(a.nbw, a.nbo, a.n_clr, a.nbap, a.n_tomb); }

// ---------------------------------------------------------------------------------------
// k_ev_link: the link blocks (a message per thread, and the clears of the tick's counters
// grid-stride), then the previous tick's deferred commit (cm_blocks = its CommitLayout's grid)
enum { kLinkLink, kLinkCommit };
struct EvLinkLayout : Roles<2> {};
FB_HD EvLinkLayout ev_link_layout(EvArgs a, int grid) { return {{{grid - a.cm_blocks, a.cm_blocks}}}; }
FB_HD EvLinkLayout ev_link_layout(EvArgs a) {
    const int64_t ev = cdiv(a.E, kBS), clr = cdiv(a.tbits_words, kBS) < 1024 ? cdiv(a.tbits_words, kBS) : 1024;
    const int64_t link = ev > clr ? ev : clr;
    return ev_link_layout(a, (int)(link > 1 ? link : 1) + a.cm_blocks);
}

// k_ev_apply_ll: a message per thread, then the slot purge of the untouched slots (wtiles
// = 4: four 256-slot tiles per workgroup, else one)
enum { kApplyMsgs, kApplyPurge };
struct EvApplyLayout : Roles<2> {};
FB_HD int ev_purge_wgs(EvArgs a) { return a.wtiles == 4 ? (a.nbw + 3) / 4 : a.nbw; }
FB_HD EvApplyLayout ev_apply_ll_layout(EvArgs a, int grid) {
    const int purge = ev_purge_wgs(a);
    return {{{grid - purge, purge}}};
}
FB_HD EvApplyLayout ev_apply_ll_layout(EvArgs a) {
    return ev_apply_ll_layout(a, (int)cdiv(a.E, kBS) + ev_purge_wgs(a));
}

// ---------------------------------------------------------------------------------------
// k_scan<MODE, WT>: queue workgroups first (the critical path: their loads go out before the
// log role's gathers fill the memory queues), then log tiles, then slot workgroups of WT
// tiles, then the blocks of a folded commit's dense orphan list.  Sharded phase 1
// (a.wfirst): the log and slot workgroups ahead of the queue workgroups in the grid -- there
// they are the longer ones (4-5 us against the queue blocks' 3 at configs[3], N = 8) and
// nothing waits on the queue role before the exchange.
enum { kScanQueue, kScanLog, kScanSlots, kScanCommit };
// k_scan and k_emit2 are register-bound: built in their prologue, a whole layout cost them up
// to 26 SGPR spills.  They call the count and order functions below one by one, in the forms
// that compile to the code they had; the layout, which the launcher and the tests use, is
// made of the same functions.
// (phase 2 re-derives only the queue counts; the log role may have its own launch or ride
// in k_emit2, the slot purge its own launch or ride in k_ev_apply_ll's)
FB_HD int scan_log_wgs(TickArgs a) { return (a.shard == 2 || a.f_sep || a.f_emit) ? 0 : a.nbf; }
// the first workgroup of a folded commit in a grid (= ScanLayout::first(kScanCommit); a macro:
// as a function, whatever it took, it cost k_scan's instances up to 24 SGPR spills)
#define FB_SCAN_FIRST_COMMIT(grid, a) ((grid) - (a).cm_blocks)
FB_HD int scan_queue_wgs(const TickArgs &a, int wt) { return (wt == 4 && a.qtiles == 4) ? quarter(a.nbq) : a.nbq; }
FB_HD int scan_commit_wgs(const TickArgs &a) { return a.cm_fold ? a.cm_blocks : 0; }
// the log and slot workgroups of a grid: what the queue workgroups and the commit's leave of it
FB_HD int scan_logslot_wgs(int grid, int q, int cm) { return grid - q - cm; }
// q queue workgroups, fw log and slot workgroups, then the commit's
FB_HD int scan_canon(int wfirst, int q, int fw, int blk) {
    return !wfirst ? blk : (blk < fw ? q + blk : (blk < fw + q ? blk - fw : blk));
}
inline int scan_slot_wgs(const TickArgs &a) {
    return (a.shard == 2 || !a.slots_in_scan || a.slots_in_apply) ? 0
           : (a.wtiles > 1 ? (a.nbw + a.wtiles - 1) / a.wtiles : a.nbw);
}
// the instance that runs: without slot workgroups the one-tile one, whatever a.wtiles says
// (so a.qtiles groups queue blocks only where slot workgroups of 4 tiles exist)
inline int scan_wt(const TickArgs &a) { return scan_slot_wgs(a) ? a.wtiles : 1; }
struct ScanLayout : Roles<4> {
    int wfirst;
    FB_HD int canon(int blk) const { return scan_canon(wfirst, n[kScanQueue], n[kScanLog] + n[kScanSlots], blk); }
};
inline ScanLayout scan_layout(const TickArgs &a) {
    return {{{scan_queue_wgs(a, scan_wt(a)), scan_log_wgs(a),
              scan_slot_wgs(a), scan_commit_wgs(a)}}, a.wfirst};
}

// ---------------------------------------------------------------------------------------
// k_emit (chunked): a workgroup per queue block, per log tile, per slot tile
enum { kEmitQueue, kEmitLog, kEmitSlots };
struct EmitLayout : Roles<3> {};
FB_HD EmitLayout emit_layout(TickArgs a) { return {{{a.nbq, a.nbf, a.nbw}}}; }

// k_emit2: queue blocks, then the compaction workgroups -- log: 4 tiles each (f_emit: one
// tile each, flagged and compacted there), then the slot tiles 4 per workgroup.  a.cmix
// (fb_set_path("cmix")): the compaction rows of 8 workgroups (one per XCD) spread evenly
// among the queue rows, so they run beside the queue blocks' load latency instead of after
// them; a queue block keeps its XCD (role index mod 8 = blockIdx mod 8); the rows' tails pad
enum { kEmit2Queue, kEmit2Log, kEmit2Slots };
FB_HD int emit2_log_wgs(int f_emit, int nbf) { return f_emit ? nbf : quarter(nbf); }
// cmix: workgroup blk's canonical index among q queue blocks and nc compaction workgroups
// into bid, or `pad` for a padding workgroup.  A macro, so that k_emit2's padding workgroups
// leave from inside the mapping as they always did (a returned kPadding that the kernel then
// tests cost every instance two scalar instructions in the prologue).
#define FB_CMIX_CANON(q, nc, blk, bid, pad)                                  \
    do {                                                                     \
        const int x_ = (blk) & 7, y_ = (blk) >> 3;                           \
        const int nqr_ = ((q) + 7) >> 3, ncr_ = ((nc) + 7) >> 3, nr_ = nqr_ + ncr_; \
        const int cr_ = (int)((int64_t)y_ * ncr_ / nr_);                     \
        if ((int)((int64_t)(y_ + 1) * ncr_ / nr_) > cr_) {                   \
            if (8 * cr_ + x_ >= (nc)) pad;                                   \
            bid = (q) + 8 * cr_ + x_;                                        \
        } else {                                                             \
            if (8 * (y_ - cr_) + x_ >= (q)) pad;                             \
            bid = 8 * (y_ - cr_) + x_;                                       \
        }                                                                    \
    } while (0)
struct Emit2Layout : Roles<3> {
    int cmix;
    FB_HD int grid() const {
        const int nc = n[kEmit2Log] + n[kEmit2Slots];
        return cmix ? 8 * (((n[kEmit2Queue] + 7) >> 3) + ((nc + 7) >> 3)) : n[kEmit2Queue] + nc;
    }
    FB_HD int canon(int blk) const {
        int bid = blk;
        if (cmix) FB_CMIX_CANON(n[kEmit2Queue], n[kEmit2Log] + n[kEmit2Slots], blk, bid, return kPadding);
        return bid;
    }
};
inline Emit2Layout emit2_layout(const TickArgs &a) {
    return {{{a.nbq, emit2_log_wgs(a.f_emit, a.nbf), quarter(a.nbw)}}, a.cmix};
}

// k_emit_shard, k_emit_shard_wide (nsb = 1) and k_emit_shard_xp<NSB>: a workgroup per nsb
// queue blocks, then shard_compact's: the log tiles, then the slot tiles, 4 per workgroup.
// k_emit_shard_xp with a.xcfirst: the compaction workgroups first in the grid (they are
// short, and behind more queue workgroups than fit on the device at once they started only
// as the first of those left, ~10 us in, and ended the kernel)
enum { kShardQueue, kShardLog, kShardSlots };
struct EmitShardLayout : Roles<3> {
    int total, xcfirst;
    FB_HD int grid() const { return total; }
    FB_HD int canon(int blk) const {
        const int q = n[kShardQueue], nc = total - q;
        return !xcfirst ? blk : (blk < nc ? q + blk : blk - nc);
    }
};
FB_HD EmitShardLayout emit_shard_layout(TickArgs a, int nsb, int grid) {
    const int q = (a.nbq + nsb - 1) / nsb, f = quarter(a.nbf);
    return {{{q, f, grid - q - f}}, grid, nsb > 1 ? a.xcfirst : 0};
}
FB_HD EmitShardLayout emit_shard_layout(TickArgs a, int nsb) {
    return emit_shard_layout(a, nsb, (a.nbq + nsb - 1) / nsb + quarter(a.nbf) + quarter(a.nbw));
}
constexpr int kXpBlocks = 2;  // queue blocks per k_emit_shard_xp workgroup (four measured no faster)

// ---------------------------------------------------------------------------------------
// k_plan: the scan of the log tile counts, of the slot tile counts, the totals, then a
// workgroup per round: the column scan of all positions' counts, and (sharded) of this rank's
enum { kPlanLogScan, kPlanSlotScan, kPlanTotals, kPlanRows, kPlanOwnRows };
struct PlanLayout : Roles<5> {};
FB_HD PlanLayout plan_layout(TickArgs a) { return {{{1, 1, 1, a.R, a.shard ? a.R : 0}}}; }

// k_plan2: a workgroup per group row, then the two tile-count scans
enum { kPlan2Groups, kPlan2LogScan, kPlan2SlotScan };
struct Plan2Layout : Roles<3> {};
FB_HD Plan2Layout plan2_layout(TickArgs a) { return {{{a.ngrp, 1, 1}}}; }

// k_xscan: a workgroup per chunk of kXsBlocks queue blocks
enum { kXscanChunks };
struct XscanLayout : Roles<1> {};
FB_HD XscanLayout xscan_layout(TickArgs, int grid) { return {{{grid}}}; }
FB_HD XscanLayout xscan_layout(TickArgs a) { return xscan_layout(a, (a.nbq + kXsBlocks - 1) / kXsBlocks); }

// k_emit_win: kWinCh-element chunks of the virtual order [backs][fronts][window prefix]
// (indexed by chunk: the workgroup index, or its ticket)
enum { kWinBacks, kWinFronts, kWinWindow };
struct EmitWinLayout : Roles<3> {};
FB_HD EmitWinLayout emit_win_layout(TickArgs a) { return {{{a.nchB, a.nchF, a.nchW}}}; }

// ---------------------------------------------------------------------------------------
// k_copy_multi: copy i (role i) takes the blocks [blk0[i], blk0[i + 1]) -- copy_blocks of its
// words, which is how the caller fills blk0 --, then a block per orphan tile (role kCopyGather)
constexpr int kCopyGather = 4;
FB_HD int copy_blocks(int64_t words) {
    const int64_t b = (words + 4 * kBS - 1) / (4 * kBS);
    return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}
struct CopyMultiLayout {
    static constexpr int kRoles = 5;
    const CopyMulti &m;
    int copy;  // the copies' blocks
    FB_HD int count(int r) const { return r == kCopyGather ? m.otiles : (r < m.n ? end(r) - m.blk0[r] : 0); }
    FB_HD int first(int r) const { return r == kCopyGather ? copy : m.blk0[r]; }  // (blk0 of an unused copy: 0)
    FB_HD int end(int r) const { return r == kCopyGather ? copy + m.otiles : (r + 1 < m.n ? m.blk0[r + 1] : copy); }
    FB_HD int canon(int blk) const { return blk; }
    FB_HD int grid() const { return copy + m.otiles; }
    FB_HD int copy_of(int blk) const {  // the copy of a block before first(kCopyGather)
        int i = 0;
        while (i + 1 < m.n && blk >= m.blk0[i + 1]) ++i;
        return i;
    }
};
FB_HD CopyMultiLayout copy_multi_layout(const CopyMulti &m, int grid) { return {m, grid - m.otiles}; }
FB_HD CopyMultiLayout copy_multi_layout(const CopyMulti &m) {
    return copy_multi_layout(m, (m.n > 0 ? m.blk0[m.n - 1] + copy_blocks(m.words[m.n - 1]) : 0) + m.otiles);
}

// ---------------------------------------------------------------------------------------
// A scratch allocation's regions, handed out front to back at 256-byte aligned byte offsets.
struct Regions {
    size_t o = 0;
    size_t take(size_t b) {
        const size_t at = o;
        o += (b + 255) & ~(size_t)255;
        return at;
    }
};

// ---------------------------------------------------------------------------------------
// Log compaction: fb_log_compact on one GPU, fb_log_compact_shard_mark / _apply on a rank of a
// shard group.  One kernel family over kLcTile-entry tiles, a wave per tile (four per
// workgroup), around LcTable, the rank table over a live bitmap (faasbal_kernels.h):
//   k_lc_flag<kShard>  a workgroup per four tiles of the entries: the local table's bitmap
//                      (kLcWords 64-bit words per tile, whole tiles: bits past the last entry
//                      are 0), wrel and tcnt
//   k_lc_scan          one workgroup: a table's tpre from its tcnt
//   k_lcs_mark         a thread per word of the exchange bitmap (the caller's buffer, nwg
//                      words, every one written): the rank's live bits by sequence
//   k_lcs_count        a workgroup per four tiles of the reduced exchange bitmap: the global
//                      table's wrel and tcnt, the bits given
//   k_lc_move<kShard>  the tile workgroups scatter the survivors (dst; one GPU: kept, their old
//                      sequences; a shard: dseq, their new ones), a workgroup per kBS slots
//                      remaps the epochs, then (a shard with want_kept) the global tile
//                      workgroups expand the reduced bitmap (kept)
// One GPU: flag, scan, move over one table of the log's indices, which are its sequences.
// A shard of head_local entries (seq: their global sequences, ascending) of the `head`
// sequences keeps two tables, the local over the shard's indices, the global over sequences:
//   mark:   flag, scan (local: tpre[ntl] = the rank's live count), mark
//   apply:  count, scan (global: tpre[ntg] = the group's live count), move
// lc_plan and lcs_plan state the grids, the counts and the scratch's regions for the two; the
// launchers and the allocation both read them from there (tests/lc_probe.cpp and
// tests/lcs_probe.cpp walk them on the CPU).
constexpr int kLcTile = kFTile;
constexpr int kLcWords = kLcTile / 64;
constexpr int kLcScanGrid = 1;
enum { kLcMoveTiles, kLcMoveSlots, kLcMoveKept };
struct LcMoveLayout : Roles<3> {};
FB_HD LcMoveLayout lc_move_layout(int nt, int W, int ntg_kept) {
    return {{{quarter(nt), (int)cdiv(W, kBS), quarter(ntg_kept)}}};
}
// LcTable's regions: nt * kLcWords x 8, nt * kLcWords x 4, nt x 4, (nt + 1) x 4 bytes.  The
// shard's global table has no bits region (own_bits = false: `bits` is not an offset).
struct LcTableAt {
    size_t bits, wrel, tcnt, tpre;
};
inline LcTableAt lc_table_at(Regions &r, int nt, bool own_bits) {
    const size_t nw = (size_t)nt * kLcWords;
    LcTableAt t{};
    if (own_bits) t.bits = r.take(nw * 8);
    t.wrel = r.take(nw * 4);
    t.tcnt = r.take((size_t)nt * 4);
    t.tpre = r.take(((size_t)nt + 1) * 4);
    return t;
}
// (one GPU: the tables are one, ntg = ntl and nwg = nwl; no mark, count, dseq, keep or
// exchange.)  A shard's local table comes first: it is written by the mark and read by the
// apply, and stays where it is (or is copied, `keep` bytes) when the apply grows the scratch
// for a kept list.
struct LcPlan {
    int ntl, ntg;      // local tiles (of the entries' indices), global tiles (of sequences)
    int64_t nwl, nwg;  // local bitmap words, global (exchange) bitmap words
    int flag_grid, mark_grid, count_grid, scan_grid;
    LcMoveLayout move;
    LcTableAt loc, glob;
    size_t dst, dseq, kept;  // regions: entries x 4, entries x 4, head x 8 bytes
    size_t keep;       // the bytes a mark leaves for its apply: [0, keep)
    size_t bytes;
    int64_t xbytes;    // the exchange bitmap: nwg x 8 bytes
};
inline LcPlan lc_plan(int64_t head, int W, bool want_kept) {
    LcPlan p{};
    p.ntl = p.ntg = (int)cdiv(head, kLcTile);
    p.nwl = p.nwg = (int64_t)p.ntl * kLcWords;
    p.flag_grid = quarter(p.ntl);
    p.scan_grid = kLcScanGrid;
    p.move = lc_move_layout(p.ntl, W, 0);
    Regions r;
    p.loc = p.glob = lc_table_at(r, p.ntl, true);
    p.dst = r.take((size_t)head * 4);
    p.kept = r.take(want_kept ? (size_t)head * 8 : 0);
    p.bytes = r.o;
    return p;
}
inline LcPlan lcs_plan(int64_t head, int64_t head_local, int W, bool want_kept) {
    LcPlan p{};
    p.ntl = (int)cdiv(head_local, kLcTile);
    p.ntg = (int)cdiv(head, kLcTile);
    p.nwl = (int64_t)p.ntl * kLcWords;
    p.nwg = (int64_t)p.ntg * kLcWords;
    p.flag_grid = quarter(p.ntl);
    p.mark_grid = (int)cdiv(p.nwg, kBS);
    p.count_grid = quarter(p.ntg);
    p.scan_grid = kLcScanGrid;
    p.move = lc_move_layout(p.ntl, W, want_kept ? p.ntg : 0);
    p.xbytes = p.nwg * 8;
    Regions r;
    p.loc = lc_table_at(r, p.ntl, true);
    p.keep = r.o;
    p.glob = lc_table_at(r, p.ntg, false);
    p.dst = r.take((size_t)head_local * 4);
    p.dseq = r.take((size_t)head_local * 4);
    p.kept = r.take(want_kept ? (size_t)head * 8 : 0);
    p.bytes = r.o;
    return p;
}

// ---------------------------------------------------------------------------------------
// fb_log_reclaim: the compaction family's walk and table over the prefix [0, B) of a one-GPU
// log, B = min(below_seq, head), in the compactions' scratch (a rank of a shard
// group: lrs_plan below):
//   k_lr_flag   a workgroup per four tiles of the prefix: the table's bitmap of the entries to
//               reclaim (whole tiles: bits at or past B are 0), wrel and tcnt
//   k_lc_scan   as it is: tpre; tpre[nt] is the count the host checks against the caller's cap
//   k_lr_take   the tile workgroups again: a set bit's sequence and slot go to their rank in
//               seq / slot, -1 into the log, one off the slot's budget where budgets exist
// The slot mask (W bytes; read only when the caller gave one) and the two output lists (B
// entries: the count's bound, known before the count) follow the table.
struct LrPlan {
    int64_t B;   // the prefix: min(below_seq, head)
    int nt;      // its tiles
    int64_t nw;  // bitmap words
    int flag_grid, scan_grid, take_grid;
    LcTableAt tab;
    size_t mask, seq, slot;  // regions: W, B x 8, B x 4 bytes
    size_t bytes;
};
inline LrPlan lr_plan(int64_t head, int64_t below_seq, int W) {
    LrPlan p{};
    p.B = below_seq < head ? below_seq : head;
    if (p.B < 0) p.B = 0;
    p.nt = (int)cdiv(p.B, kLcTile);
    p.nw = (int64_t)p.nt * kLcWords;
    p.flag_grid = p.take_grid = quarter(p.nt);
    p.scan_grid = kLcScanGrid;
    Regions r;
    p.tab = lc_table_at(r, p.nt, true);
    p.mask = r.take((size_t)(W > 0 ? W : 0));
    p.seq = r.take((size_t)p.B * 8);
    p.slot = r.take((size_t)p.B * 4);
    p.bytes = r.o;
    return p;
}
// fb_log_reclaim_shard, a rank of a shard group: the same three launches over the rank's
// head_local entries, whose sequences B bounds (LrArgs: the prefix test is seq[i] < B, so how
// many entries lie below B is not known before the walk).  The table is over all the local
// tiles -- a tile past the bound costs its wave one load and a zero row -- and the two lists
// hold head_local entries each, the count's bound.  That is the one-GPU plan of a log of
// head_local entries walked whole (B here: the entries, not the caller's bound), stated so.
inline LrPlan lrs_plan(int64_t head_local, int W) { return lr_plan(head_local, head_local, W); }

// ---------------------------------------------------------------------------------------
// fb_pool_stats: three launches, none of which writes anything but the scratch.
//   k_ps_slots  slot workgroups (kPsTiles tiles of kBS slots each: the counts, sums, minima
//               and histograms of a row of kPsCols words, and the expired bitmap, a 64-bit
//               word per wave and tile), then queue workgroups (kPsTiles tiles of kBS
//               positions of the window [qoff, qoff + Qn): a row of kPsQCols words)
//   k_ps_log    a wave per kLcTile-entry tile, four per workgroup: a row of kPsLCols words
//   k_ps_fold   one workgroup of kPsFoldBS threads: the rows folded into the record
// Every workgroup writes its whole row, so the scratch needs no clearing.  ps_plan states the
// grids and the scratch's regions (256-byte aligned byte offsets) for W slots, a window of
// Qn positions and a log of `head` entries (tests/ps_probe.cpp walks it on the CPU).
constexpr int kPsTiles = 4;
constexpr int kPsSpan = kPsTiles * kBS;  // slots / positions per workgroup
constexpr int kPsFreeBins = 33, kPsAgeBins = kPsMaxEdges + 1;
// columns of a slot row and of the folded record (sums, but for the three marked)
enum {
    kPsReg, kPsExp, kPsQ, kPsQExp, kPsDisp, kPsFree, kPsLive, kPsLiveExp,
    kPsInflMax,          // maximum (unsigned)
    kPsHbN,              // heartbeats that went into the minimum and the maximum
    kPsHbMin, kPsHbMax,  // doubles' bit patterns: minimum (from +inf), maximum (from -inf)
    kPsFreeHist,
    kPsAgeHist = kPsFreeHist + kPsFreeBins,
    kPsUsed = kPsAgeHist + kPsAgeBins
};
constexpr int kPsCols = 64;
static_assert(kPsUsed <= kPsCols, "a row is one 64-lane wave load");
constexpr int kPsQCols = 4;  // a queue row: queued, queued on expired slots, dispatchable, 0
constexpr int kPsLCols = 2;  // a log row: live entries on slots not expired, on expired slots
constexpr int kPsFoldBS = 1024;
enum { kPsSlotsSlots, kPsSlotsQueue };
struct PsSlotsLayout : Roles<2> {};
FB_HD PsSlotsLayout ps_slots_layout(int W, int64_t Qn) { return {{{(int)cdiv(W, kPsSpan), (int)cdiv(Qn, kPsSpan)}}}; }
struct PsPlan {
    int nt;        // log tiles
    int64_t nxw;   // expired bitmap words
    PsSlotsLayout slots;
    int log_grid, fold_grid;
    size_t xbits, srow, qrow, lrow;  // regions: nxw x 8, slot wgs x kPsCols x 8, queue wgs x kPsQCols x 8, log wgs x kPsLCols x 8 bytes
    size_t bytes;
};
inline PsPlan ps_plan(int W, int64_t Qn, int64_t head) {
    PsPlan p{};
    p.nt = (int)cdiv(head, kLcTile);
    p.nxw = cdiv(W, 64);
    p.slots = ps_slots_layout(W, Qn);
    p.log_grid = quarter(p.nt);
    p.fold_grid = 1;
    Regions r;
    p.xbits = r.take((size_t)(p.nxw > 0 ? p.nxw : 1) * 8);  // (word 0 is read, and masked, by a log without slots)
    p.srow = r.take((size_t)p.slots.count(kPsSlotsSlots) * kPsCols * 8);
    p.qrow = r.take((size_t)p.slots.count(kPsSlotsQueue) * kPsQCols * 8);
    p.lrow = r.take((size_t)p.log_grid * kPsLCols * 8);
    p.bytes = r.o;
    return p;
}

// ---------------------------------------------------------------------------------------
// The died bitmap (a bit per slot, 64-bit words) staged in dynamic LDS by whole int4: the
// bytes a launch requests and the int4 count the kernel's copy loops over.
struct BitmapLds {
    size_t bytes;
    int n4;
};
FB_HD int bitmap_n4(int W) { return (((W + 63) >> 6) + 1) >> 1; }
// k_logscan: plus a spare slot, where the copy's stores past the bitmap land
FB_HD BitmapLds logscan_bitmap_lds(int W) { return {(size_t)(bitmap_n4(W) + 1) * 16, bitmap_n4(W)}; }
// k_emit2's log workgroups (f_emit)
FB_HD BitmapLds emit2_bitmap_lds(int W) { return {(size_t)bitmap_n4(W) * 16, bitmap_n4(W)}; }
// k_scan's log role when k_slots wrote the bitmap: the launch has always requested the words
// themselves, so for an odd word count the copy's last int4 ends 8 bytes past the request
// (n4 * 16 bytes would cover it: a change of the request, left to its own commit)
FB_HD BitmapLds scan_bitmap_lds(int W) { return {(size_t)((W + 63) >> 6) * 8, bitmap_n4(W)}; }
// ... and the dynamic LDS of a launch
inline size_t scan_lds_bytes(const TickArgs &a) {
    return (a.lds_bitmap && !a.slots_in_scan && scan_layout(a).n[kScanLog]) ? scan_bitmap_lds(a.W).bytes : 0;
}
FB_HD size_t emit2_lds_bytes(TickArgs a) { return a.f_emit ? emit2_bitmap_lds(a.W).bytes : 0; }

}  // namespace fb

#undef FB_HD
