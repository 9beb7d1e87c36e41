"""Launch-plan cases: which stages a tick launches, by context kind, shape, knobs and history.

One literal table, asserted twice: tests/test_gpu_plan.py runs every case on the GPU and
compares fb_timing_read's names and launch counts, tests/test_plan.py feeds the same cases
to plan_tick (csrc/faasbal_plan.h) on the CPU.  The ``expect`` entries were captured from
fb_timing_read before plan_tick existed (the rules were then inline in enqueue_tick).

Every case starts from ``case_state``: W registered, live workers with ``free`` free
processes each, all queued in slot order, and H in-flight log entries.  History ticks carry
no tasks and their messages are heartbeats, so the shapes (queue W, log H) are the same at
every launch.  Operations:

  idle   a tick without messages          msgs   a tick with E_MSG heartbeats (distinct slots)
  crowd  msgs plus CROWD heartbeats of slot 0 (more than k_ev_apply_ll groups: the tick
         reruns through the sort)
  purge  fb_purge_launch                  read   read_state (flushes a deferred commit)

``history`` operations run whole and commit; ``measure`` operations are launched and waited
for (T_MEASURE pending tasks), not committed, with the timing enabled.
"""
import numpy as np

NOW, TTE = 1000.0, 10.0
E_MSG, CROWD = 64, 20
T_MEASURE = 100
MAX_EVENTS = 4096
BIG = (1 << 17) + 5      # past kLdsBitmapSlots: the auto rules of large tables
QBIG = 70000             # a queue of more than 256 blocks (sharded: past the one-launch phase 2)
EV_HEARTBEAT = 2


def case_state(W, free, H):
    return dict(W=W, reg=np.ones(W, np.uint8), free=np.full(W, free, np.int32),
                hb=np.full(W, NOW - 1.0, np.float64), epoch=np.zeros(W, np.uint32),
                queue=np.arange(W, dtype=np.int32), log=(np.arange(H, dtype=np.int64) % W).astype(np.int32))


def messages(W, op):
    """(kind, slot, val, ts, seq) of a ``msgs`` / ``crowd`` operation."""
    slot = np.arange(E_MSG, dtype=np.int32) * (W // E_MSG)
    if op == "crowd":
        slot = np.concatenate([slot, np.zeros(CROWD, np.int32)])
    E = len(slot)
    return (np.full(E, EV_HEARTBEAT, np.uint8), slot, np.zeros(E, np.int32), np.full(E, NOW, np.float64),
            np.full(E, -1, np.int64))


def n_messages(op):
    return {"msgs": E_MSG, "crowd": E_MSG + CROWD}.get(op, 0)


def _c(name, expect, kind="local", W=4096, free=1, H=6000, knobs=None, window=0, history=(), measure=("idle",)):
    return dict(name=name, kind=kind, W=W, free=free, H=H, knobs=dict(knobs or {}), window=window,
                history=tuple(history), measure=tuple(measure), expect=expect)


CASES = [
    # ---- one-GPU heartbeat contexts
    _c("fused_idle", {"scan": 1, "emit": 1}),
    _c("fused_msgs_ll", {"ev_link": 1, "ev_apply": 1, "scan": 1, "emit": 1}, measure=["msgs"]),
    _c("sort_wide", {"rs_sort": 2, "ev_apply": 1, "scan": 1, "logscan": 1, "emit": 1}, W=BIG, H=10000,
       knobs={"ev_ll": 0, "rs_wide": 1}, measure=["msgs"]),
    _c("sort_narrow", {"rs_sort": 3, "ev_apply": 1, "scan": 1, "logscan": 1, "emit": 1}, W=BIG, H=10000,
       knobs={"ev_ll": 0, "rs_wide": 0}, measure=["msgs"]),
    _c("sort_small", {"rs_sort": 2, "ev_apply": 1, "scan": 1, "emit": 1}, knobs={"ev_ll": 0}, measure=["msgs"]),
    _c("resort_rerun", {"ev_link": 1, "ev_apply": 2, "scan": 2, "emit": 2, "rs_sort": 2}, measure=["crowd"]),
    _c("logscan_idle", {"scan": 1, "logscan": 1, "emit": 1}, knobs={"logscan": 1}),
    _c("logscan_msgs", {"ev_link": 1, "ev_apply": 1, "scan": 1, "logscan": 1, "emit": 1}, knobs={"logscan": 1},
       measure=["msgs"]),
    _c("split_slots_idle", {"slots": 1, "scan": 1, "emit": 1}, knobs={"split_slots": 1}),
    _c("split_slots_msgs", {"ev_link": 1, "ev_apply": 1, "scan": 1, "emit": 1}, knobs={"split_slots": 1},
       measure=["msgs"]),
    _c("plan1_gp1", {"scan": 1, "emit": 1}, knobs={"plan": 1, "gp": 1}),
    _c("plan1_gp0", {"scan": 1, "plan": 1, "emit": 1}, knobs={"plan": 1, "gp": 0}),
    _c("plan1_gp0_msgs", {"ev_link": 1, "ev_apply": 1, "scan": 1, "plan": 1, "emit": 1}, knobs={"plan": 1, "gp": 0},
       measure=["msgs"]),
    _c("plan2", {"scan": 1, "plan": 1, "emit": 1}, knobs={"plan": 2}),
    _c("big_idle", {"scan": 1, "logscan": 1, "emit": 1}, W=BIG, H=10000),
    _c("big_msgs", {"ev_link": 1, "ev_apply": 1, "scan": 1, "logscan": 1, "emit": 1}, W=BIG, H=10000,
       measure=["msgs"]),
    _c("wide_idle", {"scan": 1, "plan": 1, "emit": 1}, free=200),
    _c("wide_msgs", {"ev_link": 1, "ev_apply": 1, "scan": 1, "plan": 1, "emit": 1}, free=200, measure=["msgs"]),
    # ---- the deferred commit of the last tick
    _c("commit_folds_into_scan", {"scan": 1, "emit": 1}, history=["idle"]),
    _c("commit_rides_in_ev_link", {"ev_link": 1, "ev_apply": 1, "scan": 1, "emit": 1}, history=["idle"],
       measure=["msgs"]),
    _c("commit_first_after_msgs", {"commit": 1, "scan": 1, "emit": 1}, history=["msgs"]),
    _c("commit_first_split_slots", {"commit": 1, "slots": 1, "scan": 1, "emit": 1}, knobs={"split_slots": 1},
       history=["idle"]),
    _c("commit_flushed_by_read", {"commit": 1}, history=["idle"], measure=["read"]),
    # ---- other tick kinds
    _c("purge_only", {"scan": 1, "emit": 1}, measure=["purge"]),
    _c("window_direct", {"ev_link": 1, "ev_apply": 1, "logscan": 1, "emit": 1}, window=1, measure=["msgs"]),
    _c("window_ticket", {"ev_link": 1, "ev_apply": 1, "logscan": 1, "emit": 1}, window=1, knobs={"win_direct": 0},
       measure=["msgs"]),
    _c("window_after_general", {"ev_link": 1, "ev_apply": 1, "logscan": 1, "emit": 1}, window=1, history=["idle"],
       measure=["msgs"]),
    _c("cfg2_msgs", {"ev_link": 1, "ev_apply": 1, "scan": 1, "emit": 1}, W=65536, H=50000, measure=["msgs"]),
    _c("deque_idle", {"scan": 1, "emit": 1}, kind="deque"),
    _c("deque_msgs", {"rs_sort": 2, "ev_apply": 1, "scan": 1, "emit": 1}, kind="deque", measure=["msgs"]),
    _c("deque_plan1", {"scan": 1, "plan": 1, "emit": 1}, kind="deque", knobs={"plan": 1}),
    _c("big_gp0", {"scan": 1, "logscan": 1, "plan": 1, "emit": 1}, W=BIG, H=10000, knobs={"gp": 0}),
    # ---- sharded, world = 2 (rank 0's launches: phase 1, then phase 2)
    _c("shard_rows_grouped_idle", {"scan": 1, "emit": 1}, kind="shard"),
    _c("shard_rows_grouped_msgs", {"rs_sort": 2, "ev_apply": 1, "scan": 1, "emit": 1}, kind="shard",
       measure=["msgs"]),
    _c("shard_rows_plain", {"scan": 1, "emit": 1}, kind="shard", free=40),
    _c("shard_recount", {"scan": 1, "scan2": 1, "emit": 1}, kind="shard", W=QBIG, free=40, H=10000),
    _c("shard_xplan", {"scan": 1, "plan": 1, "emit": 1}, kind="shard", W=QBIG, H=10000),
    _c("shard_xplan_off_xself0", {"scan": 1, "scan2": 1, "emit": 1}, kind="shard", W=QBIG, H=10000,
       knobs={"xplan": 0, "xself": 0}),
    _c("shard_xplan_off_xself1", {"scan": 1, "scan2": 1, "emit": 1}, kind="shard", W=QBIG, H=10000,
       knobs={"xplan": 0, "xself": 1}),
    _c("shard_phase1_logscan", {"scan": 1, "logscan": 1, "emit": 1}, kind="shard", knobs={"logscan": 1}),
]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ---------------------------------------------------------------------------------------
# The same cases as plan_tick inputs (tests/test_plan.py): what enqueue_tick's PlanIn holds
# at each launch of a case's measured operations.  The MI355X's device facts; the plan of
# these shapes does not depend on their exact values.
DEVICE = dict(ncu=256, max_lds=160 * 1024, win_occ=4)
LDS_BITMAP_SLOTS = 1 << 17   # kLdsBitmapSlots: contexts up to this size keep in-flight budgets
R_FUSED = 128                # kRFused: a sharded tick starts with at most this many rows


ROW_LIMIT = 4096             # kMaxR / kShardMaxR: the widest round table (choose_R saturates here)


def choose_R(maxc, limit=ROW_LIMIT):
    R = 32
    while R < maxc and R < limit:
        R <<= 1
    return R


def context_inputs(kind, W, free, H, knobs, world=2):
    """The PlanIn fields that stay put over a case: context kind, shapes, device, knobs."""
    d = dict(DEVICE, W=W, W_global=W, R=choose_R(free), head=H, Qn=W)
    if kind == "shard":
        per = -(-W // world)  # rank 0's slots
        d.update(shard=1, world=world, W=per, R=min(d["R"], R_FUSED),
                 head_local=int(np.count_nonzero(np.arange(H, dtype=np.int64) % W < per)))
    elif kind == "deque":
        d.update(deque=1)
    else:
        d.update(lists=1, qaos=1, heartbeat=int(W <= LDS_BITMAP_SLOTS))
    d.update({"knob." + k: v for k, v in knobs.items()})
    return d


# The benchmark's shapes (bench.py: in_flight / queue of its config line) and the labelled
# launches of one tick, in order: the names `bench.py --full` printed (tick.kernels_avg_ms;
# stream: tick.kernels_us_per_tick) on the library before plan_tick existed.  configs[2]
# with messages is not a bench workload: the table's cfg2_msgs case ran it.  The stream's
# list also names "commit" (the eager commit behind a window tick, not part of the tick's
# plan) and "scan" (its 6 window fallbacks, general ticks): the window tick is the first four.
CFG2 = dict(W=65536, head=468889, Qn=56943, T=1_000_000)
CFG3 = dict(W=1 << 20, head=7584506, Qn=907865, T=16_000_000)
STREAM_E = 65536 + 1048 + 10485
# configs[3] sharded N ways, rank 0 (phase 1, then phase 2): fb_timing_read of a one-process
# group of N ranks on one GPU (as tests/test_gpu_sharded.py runs them) at bench.py's cfg3
# state, same library -- a multi-GPU `bench.py --gpus N` run was not available
SHARDED_CFG3 = {2: ["scan", "logscan", "plan", "emit"], 4: ["scan", "logscan", "plan", "emit"],
                8: ["scan", "plan", "emit"]}


def _one_gpu(shape, **more):
    return dict(context_inputs("local", shape["W"], 32, shape["head"], {}), Qn=shape["Qn"], T=shape["T"], **more)


def _cfg3_rank(world):
    return dict(context_inputs("shard", CFG3["W"], 32, 0, {}, world=world), head=CFG3["head"],
                head_local=CFG3["head"] // world, Qn=CFG3["Qn"], T=CFG3["T"])


def workloads(window):
    """[(name, [PlanIn fields per launch], labelled stages in order)]; ``window`` as in
    case_launches (the stream's ticks are window ticks by the auto rule of large tables)."""
    is_win, nchW = window(dict(win_cap=1, mode=-1, lists=1, ev_ll=1, E=STREAM_E, W=CFG3["W"],
                               max_lds=DEVICE["max_lds"], last_L=0, T=65536, last_O=1024, win_slack=8192,
                               Qn=CFG3["Qn"], qoff=0, qcap=2 * CFG3["W"] + 2 * STREAM_E + 4096))
    out = [
        ("configs[2] idle", [_one_gpu(CFG2)], ["scan", "emit"]),
        ("configs[2] with messages", [_one_gpu(CFG2, E=E_MSG)], ["ev_link", "ev_apply", "scan", "emit"]),
        ("configs[3] one GPU", [_one_gpu(CFG3)], ["scan", "logscan", "emit"]),
        ("configs[4] stream tick", [_one_gpu(dict(CFG3, T=65536), E=STREAM_E, l_win=int(is_win), l_nchW=nchW, stale_any=1)],
         ["ev_link", "ev_apply", "logscan", "emit"]),
    ]
    for world in (2, 4, 8):
        r = _cfg3_rank(world)
        out.append(("configs[3] sharded N=%d" % world, [dict(r, phase=1), dict(r, phase=2)],
                    SHARDED_CFG3[world]))
    return out


def case_launches(case, window):
    """[(PlanIn fields, stages launched outside enqueue_tick)] per enqueue_tick call of the
    case's measured operations.  ``window(fields)`` -> (eligible, nchW) is plan_window."""
    base = context_inputs(case["kind"], case["W"], case["free"], case["H"], case["knobs"])
    # fb_tick_commit defers the commit of a one-GPU heartbeat-loop tick on the linked-list
    # path (window ticks excepted) into the next launch
    defers = case["kind"] == "local" and case["knobs"].get("ev_ll", 1) == 1
    pending, pos_ok, last_L = None, True, -1
    out = []

    def win_fields(E, T):
        return dict(win_cap=int(bool(case["window"])), mode=case["window"], lists=base.get("lists", 0),
                    ev_ll=case["knobs"].get("ev_ll", 1), deque=base.get("deque", 0), shard=base.get("shard", 0), E=E,
                    W=base["W"], max_lds=base["max_lds"], last_L=last_L, T=T, last_O=0, win_slack=8192,
                    Qn=base["Qn"], qoff=0, qcap=2 * case["W"] + 2 * MAX_EVENTS + 4096)

    def launch(op, T, measured):
        nonlocal pending, pos_ok
        E = n_messages(op)
        is_win, nchW = window(win_fields(E, T)) if case["window"] and op != "purge" else (False, 0)
        d = dict(base, E=E, T=T, l_win=int(is_win), l_nchW=nchW, pos_ok=int(pos_ok),
                 l_purge_only=int(op == "purge"))
        phases = (1, 2) if case["kind"] == "shard" else (0,)
        for ph in phases:
            dd = dict(d, phase=ph)
            if pending is not None:
                dd.update(cm_pending=1, cm_E=pending, cm_n_clr=pending if base.get("heartbeat") else 0)
                pending = None  # every launch takes the pending commit one way or another
            if measured:
                out.append((dd, {}))
        if op == "crowd":  # a slot with more messages than k_ev_apply_ll groups: again, sorted
            if measured:
                out.append((dict(d, phase=0, l_win=0, l_nchW=0, l_resort=1), {}))
            is_win = False
        if is_win:
            pos_ok = True
        return E, is_win

    for op in case["history"]:
        if op == "read":
            pending = None
            continue
        E, is_win = launch(op, 0, False)
        if defers and not is_win:
            pending = E
        if not is_win:
            pos_ok = False  # a general tick's commit: positions are rebuilt by the next window tick
        last_L = 0
    for op in case["measure"]:
        if op == "read":
            out.append((None, {"commit": 1} if pending is not None else {}))
            pending = None
        else:
            launch(op, 0 if op == "purge" else T_MEASURE, True)
    return out
