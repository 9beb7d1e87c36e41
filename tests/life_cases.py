"""The life of a tick as the library kept it before csrc/faasbal_life.h: ten flags of the
context and one hand-written ladder per entry point, transcribed here flag by flag from that
faasbal_api.hip (commit c3d9d32).  tests/test_life.py holds life_gate and the life_*
transitions to it without a GPU, tests/test_gpu_life.py the library itself.

A state of the old context is a Raw; canon() names the Life it corresponds to (several Raws
share one: the old flags kept values nothing read any more, e.g. l_failed after a load).
gate() answers for a Raw and a call what the old ladder did: the refusal's message (always
FB_ESTATE) or None, and the duties -- "flush" (flush_commit launched the deferred commit),
"undo" (log_undo_failed took a failed launch's clears back; at a launch, log_undo any
uncommitted launch's), "sync" (and waited for the stream), "discard" (fb_log_compact over the
FB_ENOSPC tick).  actions() lists what can happen next, apply() the Raw afterwards, steps()
the life_* transitions faasbal_api.hip runs for the same action.

The maintenance calls that came after that library (fb_pool_stats_shard, fb_log_reclaim,
fb_log_reclaim_shard, fb_log_compact_shard_mark / _apply / _cancel) and the `marked` flag the
mark sets are in the same table: gate() states their rules as their pull requests did, and on
the sharded kind actions() adds a successful mark, apply and cancel, so the closure reaches
the marked state.  On the other kinds `marked` stays 0 in every reachable state.

The one deliberate difference (LOAD_REJECTED_KEEPS_STALE): the old fb_load_state /
fb_load_shard cleared stale_any before validating, so a rejected load switched the liveness
test off over a log that still held stale entries.
"""
import collections

KINDS = ("hb", "hb_large", "deque", "shard")
LISTS = ("hb", "hb_large")          # ev_head: one GPU, heartbeat
DEFERRED = ("hb",)                  # bud / ev_clr; every other kind notes in-place clears (undo_idx)
LOAD_REJECTED_KEEPS_STALE = True

CALLS = ("load_state", "load_shard", "read_state", "read_inflight", "read_shard_log", "device_view", "log_compact",
         "pool_stats", "pool_stats_shard", "log_reclaim", "log_reclaim_shard", "log_compact_shard_mark",
         "log_compact_shard_apply", "log_compact_shard_cancel", "exchange_bytes", "stage", "launch", "tick_continue", "wait",
         "commit", "get_local_assignments", "get_assignments", "get_orphans", "get_evicted", "get_outputs",
         "get_outputs_compact", "expand_compact", "get_event_status", "set_window", "set_eager_commit", "set_compact_out",
         "set_full_assign", "set_round_hint", "set_path", "debug_read", "sync")
WAITS = ("ok", "rerun", "rerun_general", "invalid_message", "lengths_rejected", "log_full", "too_narrow",
         "relaunch_wanted", "other")

# marked: fb_log_compact_shard_mark done, its apply or cancel to come (the one flag the old context
# did not have: the maintenance calls came after it, and their rules are written below as the
# pull requests that added them stated them)
Raw = collections.namedtuple("Raw", "staged launched waited l_failed l_enospc l_eager phase undo_E cm_pending "
                                    "stale_any l_win marked")
CREATED = Raw(False, False, False, False, False, False, 0, 0, False, False, False, False)
E_MSGS = 3  # messages of a launch that carries some


def canon(kind, r):
    """The Life of a Raw: "staged,pos,win,eager,enospc,cm_pending,undo_E,stale,marked" (tests/life_probe.cpp)."""
    if r.launched and r.waited:
        pos = "waited"
    elif r.launched and r.l_failed:
        pos = "failed"
    elif r.launched and kind == "shard" and r.phase == 1:
        pos = "phase1"
    elif r.launched:
        pos = "launched"
    elif r.l_failed and r.undo_E > 0:
        pos = "dropped"
    else:
        pos = "none"
    live = pos not in ("none", "dropped")
    return "%d,%s,%d,%d,%d,%d,%d,%d,%d" % (r.staged, pos, live and r.l_win, live and r.l_eager,
                                           pos == "failed" and r.l_enospc, r.cm_pending, r.undo_E, r.stale_any, r.marked)


WIN_MSG = "%s between the launch and the commit of a window tick: fb_tick_commit first"
NO_WAITED = "no waited tick"
MARKED = "a log compaction is marked: apply or cancel first"
# what touches neither the log nor a tick goes on while a compaction is marked, and so do the two
# calls that end the mark
MARKED_PASSES = ("exchange_bytes", "debug_read", "sync", "log_compact_shard_apply", "log_compact_shard_cancel")
# ... and four calls name a wrong context kind before they say "marked" (points no context reaches)
KIND_FIRST = ("pool_stats_shard", "log_reclaim", "log_reclaim_shard", "log_compact_shard_mark")
ONE_GPU = {"pool_stats_shard": "fb_pool_stats_shard on a one-GPU context: use fb_pool_stats",
           "log_reclaim_shard": "fb_log_reclaim_shard on a one-GPU context: use fb_log_reclaim",
           "log_compact_shard_mark": "fb_log_compact_shard_mark on a one-GPU context: use fb_log_compact",
           "log_compact_shard_apply": "fb_log_compact_shard_apply on a one-GPU context: use fb_log_compact"}
RECLAIM_DEQUE = "fb_log_reclaim on a deque context: it keeps no liveness, nothing is in flight on a record"
RECLAIM_SHARDED = ("fb_log_reclaim on a sharded context: its sequence numbers are global across ranks (unlike "
                   "fb_log_compact_shard_mark / _apply it needs no exchange): use fb_log_reclaim_shard")
MARK_STAGED = "fb_log_compact_shard_mark with staged events pending: their sequences would go stale"
MARK_IN_FLIGHT = "fb_log_compact_shard_mark with a tick in flight: fb_tick_wait first"
APPLY_UNMARKED = "fb_log_compact_shard_apply without fb_log_compact_shard_mark"


def between_ticks(name, r, duties):
    """Between ticks only: refused with staged events, between wait and commit, with a tick
    launched, under the name given; otherwise `duties` (the flush, the undo of a failed launch)."""
    if r.staged:
        return name + " with staged events pending: launch and commit their tick first", []
    if r.launched and r.waited:
        return name + " between a tick's wait and its commit: fb_tick_commit first", []
    if r.launched:
        return name + " with a tick launched: fb_tick_wait and fb_tick_commit first", []
    return None, duties


def gate(kind, r, call):
    """(refusal or None, duties) of the old ladder, in its order."""
    shard, deque = kind == "shard", kind == "deque"
    flush = ["flush"] if r.cm_pending else []
    undo_failed = ["undo"] if r.undo_E > 0 and r.l_failed else []
    win_uncommitted = r.launched and r.l_win
    if r.marked and call not in MARKED_PASSES + KIND_FIRST:
        return MARKED, []
    if call == "load_state":
        return ("sharded context: use fb_load_shard" if shard else None), flush
    if call == "load_shard":
        return (None if shard else "fb_load_shard on a one-GPU context"), flush
    if call == "read_state":
        if win_uncommitted:
            return WIN_MSG % "fb_read_state", []
        return None, flush + undo_failed
    if call == "read_inflight":
        if win_uncommitted:
            return WIN_MSG % "fb_read_inflight", []
        if kind not in DEFERRED:
            return "in-flight counts exist on one-GPU heartbeat contexts only", flush
        return None, flush
    if call == "read_shard_log":
        return (None if shard else "fb_read_shard_log on a one-GPU context"), flush
    if call == "device_view":
        if win_uncommitted:
            return WIN_MSG % "fb_device_view_get", []
        return None, flush + undo_failed + (["sync"] if undo_failed else [])
    if call == "log_compact":
        if shard:
            return "fb_log_compact on a sharded context: its sequence numbers are global across ranks", []
        if r.staged:
            return "fb_log_compact with staged events pending: their sequences would go stale", []
        if r.launched and r.waited:
            return "fb_log_compact between a tick's wait and its commit: fb_tick_commit first", []
        if r.launched and (not r.l_enospc or r.l_win):
            return "fb_log_compact with a tick launched: fb_tick_wait and fb_tick_commit first", []
        return None, flush + undo_failed + (["discard"] if r.launched else [])
    if call == "pool_stats":
        if shard:
            return "fb_pool_stats on a sharded context: the pool is the group's, a summary needs a collective", []
        return between_ticks("fb_pool_stats", r, flush + undo_failed)
    if call in ONE_GPU and not shard:  # (whatever the state; at most the flush)
        return ONE_GPU[call], flush
    if call == "log_reclaim" and (deque or shard):  # (no duties, not even the flush)
        return (RECLAIM_DEQUE if deque else RECLAIM_SHARDED), []
    if call in KIND_FIRST and r.marked:
        return MARKED, []
    if call == "pool_stats_shard":
        # fb_pool_stats' refusals and duties with the sharded refusal set aside (its name in the texts too)
        return between_ticks("fb_pool_stats", r, flush + undo_failed)
    if call == "log_reclaim":
        return between_ticks("fb_log_reclaim", r, flush + undo_failed)
    if call == "log_reclaim_shard":
        # refused exactly where fb_pool_stats_shard is, under its own name; a dropped launch's
        # clears are taken back first: the entries its results named count as live
        return between_ticks("fb_log_reclaim_shard", r, flush + undo_failed)
    if call == "log_compact_shard_mark":
        if r.staged:
            return MARK_STAGED, []
        if r.launched and (r.l_eager or not (r.waited or r.l_failed)):  # phase1, launched, or committed eagerly
            return MARK_IN_FLIGHT, []
        # a waited-uncommitted, failed or dropped tick is discarded, its clears taken back first
        return None, flush + (["undo"] if r.undo_E > 0 else []) + (["discard"] if r.launched else [])
    if call == "log_compact_shard_apply":  # only after a mark
        return (None if r.marked else APPLY_UNMARKED), []
    if call == "log_compact_shard_cancel":  # in every state, on every kind: it drops a mark if there is one
        return None, []
    if call in ("exchange_bytes", "stage"):
        return None, []
    if call == "launch":
        if not r.staged:
            return "fb_tick_launch_staged without fb_tick_stage", []
        if r.launched and r.l_eager:
            return "the last tick was committed eagerly: fb_tick_wait and fb_tick_commit first", []
        return None, (["undo"] if r.undo_E > 0 else [])
    if call == "tick_continue":
        if not shard:
            return "fb_tick_continue on a one-GPU context", []
        if not r.launched or r.phase != 1:
            return "fb_tick_continue without fb_tick_launch", []
        return None, []
    if call == "wait":
        if not r.launched:
            return "fb_tick_wait without fb_tick_launch", []
        if shard and r.phase != 2:
            return "sharded tick: exchange, then fb_tick_continue", []
        return None, []
    if call == "commit":
        return (None if r.waited else "fb_tick_commit without a waited tick"), []
    if call == "get_local_assignments":
        return (None if r.waited else NO_WAITED), flush
    if call in ("get_assignments", "get_orphans", "get_evicted", "get_outputs", "get_outputs_compact",
                "expand_compact", "get_event_status"):
        return (None if r.waited else NO_WAITED), []
    if call == "set_window":
        if shard or deque:
            return "window ticks exist on one-GPU heartbeat contexts only", []
        if r.launched:
            return "fb_set_window between ticks only", []
        return None, flush
    if call == "set_eager_commit":
        return ("fb_set_eager_commit with a tick in flight" if r.launched and not r.waited else None), []
    if call == "set_compact_out":
        if shard:
            return "compact assignments exist on one-GPU contexts only", []
        return ("fb_set_compact_out with a tick in flight" if r.launched and not r.waited else None), []
    if call == "set_full_assign":
        if r.launched:
            return "fb_set_full_assign between ticks only", []
        return (None if shard else "fb_set_full_assign on a one-GPU context (it always has them)"), []
    if call == "set_round_hint":
        return ("fb_set_round_hint between ticks only" if r.launched else None), []
    if call == "set_path":
        if r.launched:
            return "fb_set_path between ticks only", []
        return None, flush
    if call in ("debug_read", "sync"):
        return None, flush
    raise KeyError(call)


# what a call that passed its gate goes on to do to the flags, by variant:
#   "ok"        it succeeds;  "rejected"  its arguments (or fb_log_compact's expect_kept) are refused
#   "log"       fb_read_state asked for the log / fb_device_view_get / fb_set_path("lazy", 0): log_settle
#   "unmarked"  fb_log_compact_shard_apply's count disagreed with the group's: the mark is dropped
VARIANTS = {"load_state": ("ok", "rejected"), "load_shard": ("ok", "rejected"), "log_compact": ("ok", "rejected"),
            "read_state": ("ok", "log"), "device_view": ("log",), "set_path": ("ok", "log"),
            "log_compact_shard_apply": ("ok", "unmarked")}


def actions(kind, r):
    """Every next step of a context of this kind in this state: (name, args...)."""
    out = [("stage", 1), ("stage", 0)] if gate(kind, r, "stage")[0] is None else []  # (refused while marked)
    if gate(kind, r, "launch")[0] is None:
        out += [("launch", 0, 0, 0), ("launch", E_MSGS, 0, 0)]
        if kind in LISTS:  # plan_window: messages, lists (fb_set_window allocates the buffers on "hb")
            out += [("launch", E_MSGS, 1, 0), ("launch", E_MSGS, 1, 1)]
    if gate(kind, r, "tick_continue")[0] is None:
        out.append(("continue",))
    if gate(kind, r, "wait")[0] is None:
        if r.waited:
            ws = ["ok"]  # the same results again
        elif r.l_failed:
            ws = list(WAITS[3:])  # what failed fails again: the device's results stand
        else:
            ws = list(WAITS)
        for w in ws:
            if w == "relaunch_wanted" and kind != "shard":
                continue
            if w == "rerun" and kind == "shard":
                continue
            if w == "invalid_message" and kind not in LISTS:
                continue
            if w == "rerun_general" and not (kind in LISTS or r.l_win):
                continue
            out.append(("wait", w))
    if gate(kind, r, "commit")[0] is None:
        deferred = kind in LISTS and not r.l_win and not r.l_eager  # (fb_set_path("ev_ll", 0), W == 0: never)
        for d in sorted({0, int(deferred)}):
            out.append(("commit", d, 0))
            if kind in LISTS:  # lazy clears
                out.append(("commit", d, 1))
    for call in CALLS:
        if call in ("stage", "launch", "tick_continue", "wait", "commit"):
            continue
        for v in VARIANTS.get(call, ("ok",)):
            out.append(("call", call, v))
    return out


def apply(kind, r, act):
    """(refusal or None, duties, Raw afterwards) of the old library."""
    name = act[0]
    if name == "stage":
        return None, [], r._replace(staged=bool(act[1]))
    if name == "launch":
        _, E, win, eager = act
        refuse, duties = gate(kind, r, "launch")
        assert refuse is None
        return None, duties, r._replace(staged=False, phase=1, launched=True, waited=False, l_enospc=False,
                                        l_win=bool(win), l_failed=False, undo_E=0 if kind in DEFERRED else E,
                                        cm_pending=False,  # every plan runs or takes the pending commit
                                        l_eager=bool(eager))
    if name == "continue":
        return None, [], r._replace(phase=2)
    if name == "wait":
        w = act[1]
        if w == "ok":
            return None, [], r._replace(waited=True)
        if w == "rerun":
            return None, [], r._replace(l_eager=False)
        if w == "rerun_general":
            return None, [], r._replace(l_eager=False, l_win=False)
        if w in ("invalid_message", "lengths_rejected"):
            return None, [], r._replace(l_eager=False, launched=False, l_failed=True)
        if w == "log_full":
            return None, [], r._replace(l_eager=False, l_enospc=True, l_failed=True)
        if w in ("too_narrow", "relaunch_wanted"):
            return None, [], r._replace(l_eager=False, l_failed=True)
        return None, [], r._replace(l_failed=True)
    if name == "commit":
        _, deferred, orphans = act
        return None, [], r._replace(cm_pending=r.cm_pending or bool(deferred), l_eager=False,
                                    stale_any=r.stale_any or bool(orphans), undo_E=0, launched=False, waited=False,
                                    phase=0)
    _, call, v = act
    refuse, duties = gate(kind, r, call)
    if "flush" in duties:
        r = r._replace(cm_pending=False)
    if refuse is not None:
        return refuse, duties, r
    if "undo" in duties:
        r = r._replace(undo_E=0)
    if call in ("load_state", "load_shard"):
        if v == "ok":
            r = r._replace(stale_any=False, launched=False, waited=False, undo_E=0)
        elif not LOAD_REJECTED_KEEPS_STALE:
            r = r._replace(stale_any=False)
    elif call == "log_compact" and v == "ok":
        r = r._replace(stale_any=False, launched=False, waited=False, undo_E=0, l_enospc=False)
    elif call == "log_compact_shard_mark":  # the uncommitted tick is gone, the committed state is what it was
        r = r._replace(launched=False, waited=False, undo_E=0, marked=True)
    elif call == "log_compact_shard_apply" and v == "ok":
        r = r._replace(stale_any=False, launched=False, waited=False, undo_E=0, marked=False)
    elif call == "log_compact_shard_cancel" or v == "unmarked":
        r = r._replace(marked=False)
    elif v == "log":
        r = r._replace(stale_any=False)  # log_settle (its flush ran above)
    return None, duties, r


def steps(act, duties, settle_due):
    """The life_* transitions faasbal_api.hip runs for an action whose gate named `duties`."""
    name = act[0]
    pre = [{"flush": "commit_ran", "undo": "undone"}[d] for d in duties if d in ("flush", "undo")]
    if name == "stage":
        return ["stage:%d" % act[1]]
    if name == "launch":
        return pre + ["launch:%d:%d" % (act[1], act[2]), "commit_ran"] + (["eager"] if act[3] else [])
    if name == "continue":
        return ["continue"]
    if name == "wait":
        return ["wait:" + act[1]]
    if name == "commit":
        return ["commit:%d:%d" % (act[1], act[2])]
    _, call, v = act
    if v == "log" and settle_due:
        pre.append("settled")
    if v == "ok" and call in ("load_state", "load_shard", "log_compact", "log_compact_shard_apply"):
        pre.append("replaced")
    if call == "log_compact_shard_mark":
        pre.append("marked")
    if call == "log_compact_shard_cancel" or v == "unmarked":
        pre.append("unmarked")
    return pre


def closure(kind):
    """Every Raw the old library reaches from a created context of this kind."""
    seen, todo = {CREATED}, [CREATED]
    while todo:
        r = todo.pop()
        for act in actions(kind, r):
            n = apply(kind, r, act)[2]
            if n not in seen:
                seen.add(n)
                todo.append(n)
    return seen


# The Lifes of closure(kind), written out: the table's rows.  (python tests/life_cases.py prints them.)
STATES = {
    "hb": (
        "0,failed,0,0,0,0,0,0,0", "0,failed,0,0,0,0,0,1,0", "0,failed,0,0,1,0,0,0,0", "0,failed,0,0,1,0,0,1,0",
        "0,failed,1,0,0,0,0,0,0", "0,failed,1,0,0,0,0,1,0", "0,failed,1,0,1,0,0,0,0", "0,failed,1,0,1,0,0,1,0",
        "0,failed,1,1,0,0,0,0,0", "0,failed,1,1,0,0,0,1,0", "0,launched,0,0,0,0,0,0,0", "0,launched,0,0,0,0,0,1,0",
        "0,launched,1,0,0,0,0,0,0", "0,launched,1,0,0,0,0,1,0", "0,launched,1,1,0,0,0,0,0", "0,launched,1,1,0,0,0,1,0",
        "0,none,0,0,0,0,0,0,0", "0,none,0,0,0,0,0,1,0", "0,none,0,0,0,1,0,0,0", "0,none,0,0,0,1,0,1,0",
        "0,waited,0,0,0,0,0,0,0", "0,waited,0,0,0,0,0,1,0", "0,waited,1,0,0,0,0,0,0", "0,waited,1,0,0,0,0,1,0",
        "0,waited,1,1,0,0,0,0,0", "0,waited,1,1,0,0,0,1,0", "1,failed,0,0,0,0,0,0,0", "1,failed,0,0,0,0,0,1,0",
        "1,failed,0,0,1,0,0,0,0", "1,failed,0,0,1,0,0,1,0", "1,failed,1,0,0,0,0,0,0", "1,failed,1,0,0,0,0,1,0",
        "1,failed,1,0,1,0,0,0,0", "1,failed,1,0,1,0,0,1,0", "1,failed,1,1,0,0,0,0,0", "1,failed,1,1,0,0,0,1,0",
        "1,launched,0,0,0,0,0,0,0", "1,launched,0,0,0,0,0,1,0", "1,launched,1,0,0,0,0,0,0", "1,launched,1,0,0,0,0,1,0",
        "1,launched,1,1,0,0,0,0,0", "1,launched,1,1,0,0,0,1,0", "1,none,0,0,0,0,0,0,0", "1,none,0,0,0,0,0,1,0",
        "1,none,0,0,0,1,0,0,0", "1,none,0,0,0,1,0,1,0", "1,waited,0,0,0,0,0,0,0", "1,waited,0,0,0,0,0,1,0",
        "1,waited,1,0,0,0,0,0,0", "1,waited,1,0,0,0,0,1,0", "1,waited,1,1,0,0,0,0,0", "1,waited,1,1,0,0,0,1,0",
    ),
    "hb_large": (
        "0,dropped,0,0,0,0,3,0,0", "0,dropped,0,0,0,0,3,1,0", "0,failed,0,0,0,0,0,0,0", "0,failed,0,0,0,0,0,1,0",
        "0,failed,0,0,0,0,3,0,0", "0,failed,0,0,0,0,3,1,0", "0,failed,0,0,1,0,0,0,0", "0,failed,0,0,1,0,0,1,0",
        "0,failed,0,0,1,0,3,0,0", "0,failed,0,0,1,0,3,1,0", "0,failed,1,0,0,0,3,0,0", "0,failed,1,0,0,0,3,1,0",
        "0,failed,1,0,1,0,3,0,0", "0,failed,1,0,1,0,3,1,0", "0,failed,1,1,0,0,3,0,0", "0,failed,1,1,0,0,3,1,0",
        "0,launched,0,0,0,0,0,0,0", "0,launched,0,0,0,0,0,1,0", "0,launched,0,0,0,0,3,0,0", "0,launched,0,0,0,0,3,1,0",
        "0,launched,1,0,0,0,3,0,0", "0,launched,1,0,0,0,3,1,0", "0,launched,1,1,0,0,3,0,0", "0,launched,1,1,0,0,3,1,0",
        "0,none,0,0,0,0,0,0,0", "0,none,0,0,0,0,0,1,0", "0,none,0,0,0,1,0,0,0", "0,none,0,0,0,1,0,1,0",
        "0,waited,0,0,0,0,0,0,0", "0,waited,0,0,0,0,0,1,0", "0,waited,0,0,0,0,3,0,0", "0,waited,0,0,0,0,3,1,0",
        "0,waited,1,0,0,0,3,0,0", "0,waited,1,0,0,0,3,1,0", "0,waited,1,1,0,0,3,0,0", "0,waited,1,1,0,0,3,1,0",
        "1,dropped,0,0,0,0,3,0,0", "1,dropped,0,0,0,0,3,1,0", "1,failed,0,0,0,0,0,0,0", "1,failed,0,0,0,0,0,1,0",
        "1,failed,0,0,0,0,3,0,0", "1,failed,0,0,0,0,3,1,0", "1,failed,0,0,1,0,0,0,0", "1,failed,0,0,1,0,0,1,0",
        "1,failed,0,0,1,0,3,0,0", "1,failed,0,0,1,0,3,1,0", "1,failed,1,0,0,0,3,0,0", "1,failed,1,0,0,0,3,1,0",
        "1,failed,1,0,1,0,3,0,0", "1,failed,1,0,1,0,3,1,0", "1,failed,1,1,0,0,3,0,0", "1,failed,1,1,0,0,3,1,0",
        "1,launched,0,0,0,0,0,0,0", "1,launched,0,0,0,0,0,1,0", "1,launched,0,0,0,0,3,0,0", "1,launched,0,0,0,0,3,1,0",
        "1,launched,1,0,0,0,3,0,0", "1,launched,1,0,0,0,3,1,0", "1,launched,1,1,0,0,3,0,0", "1,launched,1,1,0,0,3,1,0",
        "1,none,0,0,0,0,0,0,0", "1,none,0,0,0,0,0,1,0", "1,none,0,0,0,1,0,0,0", "1,none,0,0,0,1,0,1,0",
        "1,waited,0,0,0,0,0,0,0", "1,waited,0,0,0,0,0,1,0", "1,waited,0,0,0,0,3,0,0", "1,waited,0,0,0,0,3,1,0",
        "1,waited,1,0,0,0,3,0,0", "1,waited,1,0,0,0,3,1,0", "1,waited,1,1,0,0,3,0,0", "1,waited,1,1,0,0,3,1,0",
    ),
    "deque": (
        "0,dropped,0,0,0,0,3,0,0", "0,failed,0,0,0,0,0,0,0", "0,failed,0,0,0,0,3,0,0", "0,failed,0,0,1,0,0,0,0",
        "0,failed,0,0,1,0,3,0,0", "0,launched,0,0,0,0,0,0,0", "0,launched,0,0,0,0,3,0,0", "0,none,0,0,0,0,0,0,0",
        "0,waited,0,0,0,0,0,0,0", "0,waited,0,0,0,0,3,0,0", "1,dropped,0,0,0,0,3,0,0", "1,failed,0,0,0,0,0,0,0",
        "1,failed,0,0,0,0,3,0,0", "1,failed,0,0,1,0,0,0,0", "1,failed,0,0,1,0,3,0,0", "1,launched,0,0,0,0,0,0,0",
        "1,launched,0,0,0,0,3,0,0", "1,none,0,0,0,0,0,0,0", "1,waited,0,0,0,0,0,0,0", "1,waited,0,0,0,0,3,0,0",
    ),
    "shard": (
        "0,dropped,0,0,0,0,3,0,0", "0,failed,0,0,0,0,0,0,0", "0,failed,0,0,0,0,3,0,0", "0,failed,0,0,1,0,0,0,0",
        "0,failed,0,0,1,0,3,0,0", "0,launched,0,0,0,0,0,0,0", "0,launched,0,0,0,0,3,0,0", "0,none,0,0,0,0,0,0,0",
        "0,none,0,0,0,0,0,0,1",  # marked: the state a mark leaves, whatever it found
        "0,phase1,0,0,0,0,0,0,0", "0,phase1,0,0,0,0,3,0,0", "0,waited,0,0,0,0,0,0,0", "0,waited,0,0,0,0,3,0,0",
        "1,dropped,0,0,0,0,3,0,0", "1,failed,0,0,0,0,0,0,0", "1,failed,0,0,0,0,3,0,0", "1,failed,0,0,1,0,0,0,0",
        "1,failed,0,0,1,0,3,0,0", "1,launched,0,0,0,0,0,0,0", "1,launched,0,0,0,0,3,0,0", "1,none,0,0,0,0,0,0,0",
        "1,phase1,0,0,0,0,0,0,0", "1,phase1,0,0,0,0,3,0,0", "1,waited,0,0,0,0,0,0,0", "1,waited,0,0,0,0,3,0,0",
    ),
}


# ------------------------------------------------------------------ the scripted case of the difference
RESTALE_CAP = 4096


def restale_scenario():
    """(initial state, [(tick arguments, the oracle's outputs) or (a rejected load's arguments,
    None)], the oracle's final state), from the oracle alone: on a 64-slot heartbeat context
    slot 0 dies with entries 0 .. 3 in flight (they stay in the device's log, stale), a load
    with a queue entry out of range is rejected, slot 0 registers again, takes tasks and dies
    again.  Asserts that the run reaches "stale entries of the re-registered slot exist at its
    second death"."""
    import numpy as np
    from faasbal import synth
    from oracle import Oracle

    W, now, tte = 64, 1000.0, 10.0
    st = dict(reg=np.ones(W, np.uint8), free=np.full(W, 2, np.int32), hb=np.full(W, now - 1.0),
              epoch=np.zeros(W, np.uint32), queue=np.arange(W, dtype=np.int32),
              log=np.asarray([0, 0, 0, 0, 1, 2], np.int32))
    st["hb"][0] = now - 9.0
    o = Oracle(W, RESTALE_CAP)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])

    def others(t, reg0=False):
        """A heartbeat of every slot but 0 at the clock t; reg0: and slot 0's registration."""
        n = W - 1 + int(reg0)
        kind = np.full(n, synth.EV_HEARTBEAT, np.uint8)
        slot = np.arange(1, n + 1, dtype=np.int32)
        val = np.zeros(n, np.int32)
        if reg0:
            kind[-1], slot[-1], val[-1] = synth.EV_REGISTER, 0, 2
        return kind, slot, val, np.full(n, t), np.full(n, -1, np.int64)

    plan = [(now + 2.0, others(now + 2.0), 0),              # slot 0 expires: entries 0 .. 3 are redistributed
            None,                                           # the rejected load
            (now + 3.0, others(now + 3.0, True), 200),      # slot 0 registers again and takes tasks
            (now + 10.0, others(now + 10.0), 1),            # (the others stay alive)
            (now + 14.0, others(now + 14.0), 0)]            # ... and expires again
    steps, carried, stale0 = [], 0, None
    for p in plan:
        if p is None:
            steps.append(((st["reg"], st["free"], st["hb"], st["epoch"], np.asarray([W + 5], np.int32)), None))
            continue
        t, ev, n_new = p
        args = (t, tte, *ev, carried + n_new)
        before = o.export()["log"].copy()
        b = o.tick(*args)
        carried = args[-1] + len(b["orphans"]) - len(b["assign"])
        mine = [int(q) for q in b["orphans"] if before[q] == 0]
        if stale0 is None:
            stale0 = mine
            assert stale0 == [0, 1, 2, 3], stale0
        elif n_new == 0:
            # slot 0's second death: its new entries are orphans while the old ones are still in the device's log
            assert mine and min(mine) > max(stale0), (mine, stale0)
            assert o.export()["epoch"][0] > max(stale0)
        else:
            assert not len(b["orphans"])
        steps.append((args, b))
    return st, steps, o.export()


if __name__ == "__main__":
    for k in KINDS:
        print('    "%s": (' % k)
        for s in sorted({canon(k, r) for r in closure(k)}):
            print('        "%s",' % s)
        print("    ),")
