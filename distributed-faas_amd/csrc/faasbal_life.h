// faasbal_life.h -- internal, host only: the life of a tick.
//
// The one statement of which public calls are legal at each point of a tick's life and what
// each owes the committed state first (DESIGN.md "The life of a tick" carries the table).
// Like faasbal_plan.h it calls no HIP runtime function, touches no fb_ctx and allocates
// nothing: faasbal_api.hip's enter() evaluates life_gate at the top of every entry point and
// performs the duties, the transitions below are the only writers of a Life, and
// tests/test_life.py runs all of it without a GPU.
#pragma once
#include <cstdint>

namespace fb {

// What the context kind does with the log entry a result completes, fixed at creation.
enum class Clears : uint8_t {
    deferred,  // one GPU, heartbeat, <= kLdsBitmapSlots: the commit clears it (bud / ev_clr)
    in_place,  // sharded, deque, larger one-GPU tables: the launch clears it and notes it (undo_idx)
};
struct CtxCaps {
    Clears clears = Clears::in_place;
    bool lists = false;  // messages grouped per slot by linked lists (ev_head): one GPU, heartbeat
    bool sharded = false, deque = false;
};

// Where the launched tick is.
enum class Pos : uint8_t {
    none,      // no tick: created, committed, loaded over, compacted away
    phase1,    // sharded: phase 1 enqueued, the exchange and fb_tick_continue to come
    launched,  // the whole tick (sharded: phase 2) enqueued
    waited,    // fb_tick_wait returned its result; fb_tick_commit to come
    failed,    // fb_tick_wait failed and the launch stays: it never commits, a new launch replaces it
    dropped,   // fb_tick_wait failed and dropped the launch, whose in-place clears are still owed
               // (without such clears a dropped launch is `none`)
};

struct Life {
    bool staged = false;  // fb_tick_stage done, fb_tick_launch_staged not yet
    Pos pos = Pos::none;
    // the launched tick's qualifiers (all false at none / dropped)
    bool win = false;     // a window tick: the committed window moves at its commit
    bool eager = false;   // its commit is enqueued right behind it (until a rerun cancels it)
    bool enospc = false;  // failed with the log full: it read only committed state
    // what the committed state is owed
    bool cm_pending = false;  // the last commit is deferred into the next launch (or a flush)
    int undo_E = 0;           // > 0: messages of a launch whose in-place clears are not committed
    bool stale = false;       // lazy clears: entries of dead registrations may be in the log
    // sharded: fb_log_compact_shard_mark done, its apply or cancel to come (no tick meanwhile:
    // pos is none, nothing is staged, nothing is owed)
    bool marked = false;
};

inline bool life_launched(const Life &l) { return l.pos != Pos::none && l.pos != Pos::dropped; }
inline bool life_waited(const Life &l) { return l.pos == Pos::waited; }
// sharded ticks: the phase plan_tick plans (one-GPU plans do not read it)
inline int life_phase(const Life &l) { return l.pos == Pos::phase1 ? 1 : life_launched(l) ? 2 : 0; }

// One value per public entry point that reads or changes a Life.  (fb_tick_launch, fb_tick,
// fb_purge_launch, fb_purge, fb_assign and fb_apply_events are sequences of these.)
#define FB_LIFE_CALLS(X)                                                                          \
    X(load_state) X(load_shard) X(read_state) X(read_inflight) X(read_shard_log) X(device_view)   \
    X(log_compact) X(pool_stats) X(pool_stats_shard) X(log_reclaim) X(log_reclaim_shard)          \
    X(log_compact_shard_mark) X(log_compact_shard_apply) X(log_compact_shard_cancel)              \
    X(exchange_bytes) X(stage) X(launch) X(tick_continue) X(wait) X(commit)                       \
    X(get_local_assignments) X(get_assignments) X(get_orphans) X(get_evicted) X(get_outputs)      \
    X(get_outputs_compact) X(expand_compact) X(get_event_status) X(set_window)                    \
    X(set_eager_commit) X(set_compact_out) X(set_full_assign) X(set_round_hint) X(set_path)       \
    X(debug_read) X(sync)
enum class Call : uint8_t {
#define X(n) n,
    FB_LIFE_CALLS(X)
#undef X
    count_
};
constexpr const char *kCallNames[] = {
#define X(n) #n,
    FB_LIFE_CALLS(X)
#undef X
};

// Duties, performed in this order before the call's own work.
enum Duty : unsigned {
    kFlush = 1,     // the deferred commit as its own launch (also before a refusal that names it)
    kUndo = 2,      // take back the in-place clears of a launch that never commits
    kUndoSync = 4,  // ... and wait for the stream: the log leaves the context's stream
    kDiscard = 8,   // the call, once it succeeds, discards the uncommitted tick (life_replaced, life_lcs_marked)
};
// refuse: the FB_ESTATE message, or null: go on.  A refusal carries at most kFlush.
struct Gate {
    const char *refuse = nullptr;
    unsigned duties = 0;
};

constexpr const char *kLifeMarkedRefusal = "a log compaction is marked: apply or cancel first";

// The three refusals of a call that runs between ticks only, under the call's name.
#define FB_BETWEEN_TICKS(name)                                                                    \
    between_ticks(name " with staged events pending: launch and commit their tick first",         \
                  name " between a tick's wait and its commit: fb_tick_commit first",             \
                  name " with a tick launched: fb_tick_wait and fb_tick_commit first")

inline Gate life_gate(const Life &l, const CtxCaps &k, Call call) {
    const bool launched = life_launched(l), waited = life_waited(l), in_flight = launched && !waited;
    // a launched window tick moves the committed window (its commit may already have run on the
    // device, eager) while the host's view of it changes only at fb_tick_commit
    const bool win_open = launched && l.win;
    const unsigned flush = l.cm_pending ? kFlush : 0;
    // a launch still to be waited for or committed keeps its clears; a failed wait's go back
    const unsigned undo = (l.undo_E > 0 && (l.pos == Pos::failed || l.pos == Pos::dropped)) ? kUndo : 0;
    const auto no = [](const char *m, unsigned d = 0) { return Gate{m, d}; };
    const auto ok = [](unsigned d = 0) { return Gate{nullptr, d}; };
    // Between ticks only -- nothing staged, nothing launched -- and then the flush and the undo:
    // the calls that read or edit the committed pool and log on the device.  The undo comes
    // first: a launch the wait dropped has its in-place clears taken back, so the entries its
    // results named count as live.
    const auto between_ticks = [&](const char *m_staged, const char *m_waited, const char *m_launched) {
        if (l.staged) return no(m_staged);
        if (waited) return no(m_waited);
        if (launched) return no(m_launched);
        return ok(flush | undo);
    };
    // Between a group compaction's mark and its apply the ranks hold a bitmap of this log: every
    // call that reads or changes the log or launches a tick waits.  What touches neither goes
    // on, and so do the two calls that end the mark.
    const bool held = l.marked && call != Call::exchange_bytes && call != Call::debug_read && call != Call::sync &&
                      call != Call::log_compact_shard_apply && call != Call::log_compact_shard_cancel;
    // (four calls name a wrong context kind before they say "marked": points no context reaches)
    const bool kind_first = call == Call::pool_stats_shard || call == Call::log_reclaim ||
                            call == Call::log_reclaim_shard || call == Call::log_compact_shard_mark;
    if (held && !kind_first) return no(kLifeMarkedRefusal);
    switch (call) {
    case Call::load_state:  // (accepted over any tick, window ticks included; a staged batch stays)
        return k.sharded ? no("sharded context: use fb_load_shard", flush) : ok(flush);
    case Call::load_shard:
        return !k.sharded ? no("fb_load_shard on a one-GPU context", flush) : ok(flush);
    case Call::read_state:
        if (win_open) return no("fb_read_state between the launch and the commit of a window tick: fb_tick_commit first");
        return ok(flush | undo);
    case Call::read_inflight:  // (deferred clears: no launch ever owes an undo)
        if (win_open) return no("fb_read_inflight between the launch and the commit of a window tick: fb_tick_commit first");
        if (k.clears != Clears::deferred) return no("in-flight counts exist on one-GPU heartbeat contexts only", flush);
        return ok(flush);
    case Call::read_shard_log:  // (the sequence numbers only: not the entries an undo restores)
        return !k.sharded ? no("fb_read_shard_log on a one-GPU context", flush) : ok(flush);
    case Call::device_view:
        if (win_open) return no("fb_device_view_get between the launch and the commit of a window tick: fb_tick_commit first");
        return ok(flush | undo | (undo ? kUndoSync : 0));
    case Call::log_compact:
        if (k.sharded) return no("fb_log_compact on a sharded context: its sequence numbers are global across ranks");
        if (l.staged) return no("fb_log_compact with staged events pending: their sequences would go stale");
        if (waited) return no("fb_log_compact between a tick's wait and its commit: fb_tick_commit first");
        // a tick whose wait failed with FB_ENOSPC read only committed state: it is discarded, as a
        // load discards it; a window tick's launch moved the window, which this cannot undo
        if (launched && (!l.enospc || l.win))
            return no("fb_log_compact with a tick launched: fb_tick_wait and fb_tick_commit first");
        return ok(flush | undo | (launched ? kDiscard : 0));
    case Call::pool_stats:
        if (k.sharded) return no("fb_pool_stats on a sharded context: the pool is the group's, a summary needs a collective");
        return FB_BETWEEN_TICKS("fb_pool_stats");
    case Call::pool_stats_shard:  // a rank's part of its group's summary
        if (!k.sharded) return no("fb_pool_stats_shard on a one-GPU context: use fb_pool_stats", flush);
        if (held) return no(kLifeMarkedRefusal);
        return FB_BETWEEN_TICKS("fb_pool_stats");  // (a wart callers see: fb_pool_stats' name, not this call's)
    case Call::log_reclaim:
        // A deque context has no liveness, so nothing to reclaim from.  A sharded context's
        // sequences are global across the ranks and its bound is the group's: the rank's part is
        // fb_log_reclaim_shard.  (Neither refusal carries a duty, not even the flush.)
        if (k.deque) return no("fb_log_reclaim on a deque context: it keeps no liveness, nothing is in flight on a record");
        if (k.sharded)
            return no("fb_log_reclaim on a sharded context: its sequence numbers are global across ranks (unlike "
                      "fb_log_compact_shard_mark / _apply it needs no exchange): use fb_log_reclaim_shard");
        if (held) return no(kLifeMarkedRefusal);
        return FB_BETWEEN_TICKS("fb_log_reclaim");
    case Call::log_reclaim_shard:  // a rank's part of its group's reclaim: no exchange, it renumbers nothing
        if (!k.sharded) return no("fb_log_reclaim_shard on a one-GPU context: use fb_log_reclaim", flush);
        if (held) return no(kLifeMarkedRefusal);
        return FB_BETWEEN_TICKS("fb_log_reclaim_shard");
    case Call::log_compact_shard_mark:
        // A rank's first half of its group's compaction.  Like a load it discards a tick that was
        // never committed -- waited for (another rank failed), failed or dropped -- after taking
        // its in-place clears back (kDiscard: life_lcs_marked).  A tick in flight may still write
        // the log, staged events carry sequences of the old numbering, and an eager commit (no
        // sharded context enqueues one) would have moved the committed state already.
        if (!k.sharded) return no("fb_log_compact_shard_mark on a one-GPU context: use fb_log_compact", flush);
        if (held) return no(kLifeMarkedRefusal);  // (a second mark: no duties)
        if (l.staged) return no("fb_log_compact_shard_mark with staged events pending: their sequences would go stale");
        if (l.pos == Pos::phase1 || l.pos == Pos::launched || (launched && l.eager))
            return no("fb_log_compact_shard_mark with a tick in flight: fb_tick_wait first");
        return ok(flush | (l.undo_E > 0 ? kUndo : 0) | (launched ? kDiscard : 0));
    case Call::log_compact_shard_apply:  // only after a mark (which left no tick, nothing staged, nothing owed)
        if (!k.sharded) return no("fb_log_compact_shard_apply on a one-GPU context: use fb_log_compact", flush);
        return !l.marked ? no("fb_log_compact_shard_apply without fb_log_compact_shard_mark") : ok();  // (no duties)
    case Call::log_compact_shard_cancel:  // (drops a mark if there is one: in every state, on every kind)
    case Call::exchange_bytes:
    case Call::stage:
        return ok();
    case Call::launch:
        if (!l.staged) return no("fb_tick_launch_staged without fb_tick_stage");
        if (launched && l.eager) return no("the last tick was committed eagerly: fb_tick_wait and fb_tick_commit first");
        // the last launch was never committed (abandoned, failed, or asked for this relaunch);
        // the deferred commit stays: this launch's first kernel takes it
        return ok(l.undo_E > 0 ? kUndo : 0);
    case Call::tick_continue:
        if (!k.sharded) return no("fb_tick_continue on a one-GPU context");
        return l.pos != Pos::phase1 ? no("fb_tick_continue without fb_tick_launch") : ok();
    case Call::wait:
        if (!launched) return no("fb_tick_wait without fb_tick_launch");
        return l.pos == Pos::phase1 ? no("sharded tick: exchange, then fb_tick_continue") : ok();
    case Call::commit:
        return !waited ? no("fb_tick_commit without a waited tick") : ok();
    case Call::get_local_assignments:
        return !waited ? no("no waited tick", flush) : ok(flush);
    case Call::get_assignments:
    case Call::get_orphans:
    case Call::get_evicted:
    case Call::get_outputs:
    case Call::get_outputs_compact:
    case Call::expand_compact:
    case Call::get_event_status:
        return !waited ? no("no waited tick") : ok();
    case Call::set_window:
        if (k.sharded || k.deque) return no("window ticks exist on one-GPU heartbeat contexts only");
        return launched ? no("fb_set_window between ticks only") : ok(flush);
    case Call::set_eager_commit:
        return in_flight ? no("fb_set_eager_commit with a tick in flight") : ok();
    case Call::set_compact_out:
        if (k.sharded) return no("compact assignments exist on one-GPU contexts only");
        return in_flight ? no("fb_set_compact_out with a tick in flight") : ok();
    case Call::set_full_assign:
        if (launched) return no("fb_set_full_assign between ticks only");
        return !k.sharded ? no("fb_set_full_assign on a one-GPU context (it always has them)") : ok();
    case Call::set_round_hint:
        return launched ? no("fb_set_round_hint between ticks only") : ok();
    case Call::set_path:
        return launched ? no("fb_set_path between ticks only") : ok(flush);
    case Call::debug_read:
    case Call::sync:
        return ok(flush);
    case Call::count_:
        break;
    }
    return no("unknown call");
}
#undef FB_BETWEEN_TICKS

// The second gate, where a log pointer or copy is handed out: the deferred clears of the
// entries lazy commits left, all at once (after the flush above).
inline bool life_settle_due(const Life &l) { return l.stale; }

// ---------------------------------------------------------------------------------------
// Transitions: the only writers of a Life.

inline void life_idle_(Life &l) {
    l.pos = Pos::none;
    l.win = l.eager = l.enospc = false;
}

inline void life_stage(Life &l, bool accepted) { l.staged = accepted; }

// fb_tick_launch_staged, after the gate's undo; E the tick's messages
inline void life_launch(Life &l, const CtxCaps &k, int E, bool win) {
    l.staged = false;
    l.pos = k.sharded ? Pos::phase1 : Pos::launched;
    l.win = win;
    l.eager = l.enospc = false;
    l.undo_E = k.clears == Clears::in_place ? E : 0;
}
inline void life_eager_enqueued(Life &l) { l.eager = true; }
inline void life_continue(Life &l) { l.pos = Pos::launched; }

enum class Wait : uint8_t {
    ok,
    rerun,             // the same tick enqueued again, a wider table: cancels an eager commit
    rerun_general,     // ... on the general path: no window tick any more
    invalid_message,   // a device-checked batch held one: the launch is dropped
    lengths_rejected,  // check_lengths refused a device-reported length: dropped
    log_full,          // FB_ENOSPC
    too_narrow,        // FB_ERANGE
    relaunch_wanted,   // FB_ERERUN
    other,             // any other error (the HIP runtime's, a deque past its capacity)
};
constexpr const char *kWaitNames[] = {"ok", "rerun", "rerun_general", "invalid_message", "lengths_rejected",
                                      "log_full", "too_narrow", "relaunch_wanted", "other"};

inline void life_wait_done(Life &l, Wait w) {
    switch (w) {
    case Wait::ok: l.pos = Pos::waited; return;
    case Wait::rerun_general: l.win = false; [[fallthrough]];
    case Wait::rerun: l.eager = false; return;
    case Wait::invalid_message:
    case Wait::lengths_rejected:  // the launch read only committed state: it is gone
        life_idle_(l);
        if (l.undo_E > 0) l.pos = Pos::dropped;
        return;
    case Wait::log_full: l.enospc = true; [[fallthrough]];
    case Wait::too_narrow:
    case Wait::relaunch_wanted: l.eager = false; [[fallthrough]];
    case Wait::other: l.pos = Pos::failed; return;
    }
}

// fb_tick_commit: the tick's completed entries stay completed
inline void life_commit(Life &l, bool deferred, bool orphans_stay) {
    life_idle_(l);
    l.undo_E = 0;
    if (deferred) l.cm_pending = true;
    if (orphans_stay) l.stale = true;
}
// the deferred commit ran: flushed as its own launch, or taken by a launch's first kernel
inline void life_commit_ran(Life &l) { l.cm_pending = false; }
// kUndo done: the clears are taken back
inline void life_undone(Life &l) {
    l.undo_E = 0;
    if (l.pos == Pos::dropped) l.pos = Pos::none;
}
inline void life_settled(Life &l) { l.stale = false; }
// A successful fb_load_state / fb_load_shard / fb_log_compact / fb_log_compact_shard_apply: the
// new log holds only live entries, and a launch's notes name entries of the log it replaced (or
// the old numbering).
// A rejected load or compaction changes nothing.  (A staged batch stays.)
inline void life_replaced(Life &l) {
    life_idle_(l);
    l.undo_E = 0;
    l.stale = false;
    l.marked = false;
}
// fb_log_compact_shard_mark succeeded (after the gate's undo): the uncommitted tick is gone, as
// after a load; the committed state, lazily kept entries included, is what it was
inline void life_lcs_marked(Life &l) {
    life_idle_(l);
    l.undo_E = 0;
    l.marked = true;
}
// fb_log_compact_shard_cancel, or an apply whose count disagreed: the mark is dropped
inline void life_lcs_unmarked(Life &l) { l.marked = false; }

}  // namespace fb
