"""Scenarios whose ticks run back to back, driven from the oracle alone (no GPU here).

On a one-GPU heartbeat context a commit leaves the log entries it redistributed in the
log (lazy clears): an entry q naming slot s is live only if s holds a record and
q >= epoch[s].  The oracle clears them, so its log never shows them; this module keeps
what the device's log still holds -- ``stale[s]``, the redistributed entries that named s
-- and aims results at them.  tests/test_gpu_carried.py runs the same scenarios on the
GPU without settling the log between ticks; tests/test_carried_coverage.py counts, with
the oracle only, how often they reach the cases that matter.
"""
from collections import defaultdict

import numpy as np

from faasbal import synth
from oracle import Oracle


def state_of(scen):
    return dict(reg=scen["init_reg"], free=scen["init_free"], hb=scen["init_hb"], epoch=scen["init_epoch"],
                queue=scen["init_queue"], log=scen["init_log"])


# ------------------------------------------------------------------ scenario families
# (those of test_random_multitick_vs_oracle, test_random_results_any_entry_vs_oracle and
# test_window_random_vs_oracle: W <= 3000, <= 10 ticks, E <= 3000 -- log tiles of 2048
# entries, several queue blocks and slots with more than 16 messages all occur)
def multitick(seed):
    W = [5, 37, 300, 1000][seed % 4]
    scen = synth.random_scenario(1000 + seed, W=W, n_ticks=6, max_events=[20, 200, 2000][seed % 3],
                                 max_new=[50, 400, 3000][(seed // 3) % 3])
    return scen, len(scen["init_log"]) + 40000, 4096, resolve_own


def any_entry(seed):
    W = [7, 64, 500, 3000][seed % 4]
    scen = synth.random_scenario(5000 + seed, W=W, n_ticks=8, max_events=[40, 400, 3000][seed % 3],
                                 max_new=[60, 500, 4000][(seed // 3) % 3])
    return scen, len(scen["init_log"]) + 60000, 4096, AnyEntry(seed)


def window(seed):
    W = [300, 1000, 3000][seed % 3]
    scen = synth.random_scenario(9000 + seed, W=W, n_ticks=10, max_events=[50, 400, 1500][(seed // 3) % 3],
                                 max_new=[40, 150, 600, 4000][(seed // 9) % 3 + (seed % 2)])
    return scen, 2 * len(scen["init_log"]) + 60000, 4096, resolve_own


# The seed sets of tests/test_gpu_carried.py's random tests; the floors of
# tests/test_carried_coverage.py are stated for exactly these.
SEEDS = {
    "multitick": (multitick, tuple(range(40))),
    "any_entry": (any_entry, tuple(range(16))),
    "window": (window, tuple(range(24))),
    "window_eager": (window, tuple(range(0, 24, 3))),
    # the other launch sequences (fb_set_path), `none` mode only: seeds with many deaths of
    # stale-named slots and many aimed results
    "paths": (multitick, (7, 11, 23, 35)),
    "window_wtiles": (window, (7, 8, 13, 17)),
}


# ------------------------------------------------------------------ result resolution
def resolve_own(tk, log, head):
    """A result names one of the sender's in-flight entries (one in five: none)."""
    seq = np.full(len(tk["ev_kind"]), -1, np.int64)
    for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
        mine = np.nonzero(log == tk["ev_slot"][i])[0]
        if len(mine) and tk["ev_pick"][i] % 5 != 4:
            seq[i] = mine[tk["ev_pick"][i] % len(mine)]
    return seq


class AnyEntry:
    """Results name any log entry; half of them one of the sender's own, often twice."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self, tk, log, head):
        rng = self.rng
        seq = rng.integers(-1, max(head, 1), len(tk["ev_kind"])).astype(np.int64)
        own = np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]
        for i in own[: len(own) // 2]:
            mine = np.nonzero(log == tk["ev_slot"][i])[0]
            if len(mine):
                seq[i] = mine[rng.integers(0, min(len(mine), 2))]
        return seq


def aim_at_stale(tk, seq, stale):
    """The aiming rule: a result whose sender has stale entries and whose ev_pick % 3 == 0
    names stale[s][ev_pick % len(stale[s])].  Returns how many results were aimed."""
    n = 0
    for i in np.nonzero(tk["ev_kind"] == synth.EV_RESULT)[0]:
        mine = stale.get(int(tk["ev_slot"][i]))
        if mine and tk["ev_pick"][i] % 3 == 0:
            seq[i] = mine[tk["ev_pick"][i] % len(mine)]
            n += 1
    return n


# ------------------------------------------------------------------ the oracle's side
class OracleRun:
    """The oracle, the tasks carried from tick to tick and the stale sets of one scenario.
    Sequence numbers are resolved from the oracle's log only."""

    def __init__(self, st, log_cap, purge_mode=1):
        self.W = len(st["reg"])
        self.o = Oracle(self.W, log_cap, purge_mode=purge_mode)
        self.o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
        self.stale = defaultdict(list)   # slot -> redistributed entries that named it
        self.carried = 0
        self.log_before = None
        # what the scenario reached (tests/test_carried_coverage.py)
        self.ticks_with_stale = 0        # ticks that began with a non-empty stale set
        self.redeaths = 0                # deaths with orphans of a slot that older stale entries name
        self.aimed = 0                   # results aimed at stale entries

    def args(self, tk, tte, resolve, aim=True):
        """The tick's arguments (the same for the GPU and for the oracle)."""
        ex = self.o.export()
        self.log_before = ex["log"]
        if self.stale:
            self.ticks_with_stale += 1
        seq = resolve(tk, ex["log"], ex["head"])
        if aim:
            self.aimed += aim_at_stale(tk, seq, self.stale)
        return (tk["now"], tte, tk["ev_kind"], tk["ev_slot"], tk["ev_val"], tk["ev_ts"], seq,
                self.carried + tk["n_new"])

    def tick(self, args):
        b = self.o.tick(*args)
        # the registrations whose entries this tick redistributed
        died = set(self.log_before[b["orphans"]].tolist())
        self.redeaths += sum(1 for s in died if self.stale.get(s))
        for q in b["orphans"]:
            self.stale[int(self.log_before[q])].append(int(q))
        self.carried = args[-1] + len(b["orphans"]) - len(b["assign"])
        return b


def coverage(family, seeds, aim=True):
    """(ticks that began with stale entries, scenarios with a death of a slot that older stale
    entries name, such deaths, results aimed at stale entries) over a family's seeds."""
    ticks = scens = deaths = aimed = 0
    for seed in seeds:
        scen, cap, _, resolve = family(seed)
        run = OracleRun(state_of(scen), cap)
        for tk in scen["ticks"]:
            run.tick(run.args(tk, scen["tte"], resolve, aim))
        ticks += run.ticks_with_stale
        scens += 1 if run.redeaths else 0
        deaths += run.redeaths
        aimed += run.aimed
    return ticks, scens, deaths, aimed
