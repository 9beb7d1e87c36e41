"""The life of a tick (csrc/faasbal_life.h) without a GPU: tests/life_probe.cpp, compiled here,
answers life_gate and the life_* transitions; tests/life_cases.py is the table -- what the
library did when ten context flags and one ladder per entry point kept these rules, and the
rules of the maintenance calls added since (the pool summaries, the reclaims, a shard group's
compaction and its `marked` state).  The gate sections of tests/test_pool_stats_shard_host.py,
test_log_compact_shard_host.py, test_log_reclaim_host.py and test_log_reclaim_shard_host.py
drive the same probe through _build and _asker below.

1. For every context kind, every state of the table and every call, life_gate refuses with
   the table's message or names the table's duties.
2. Every action of the table leaves the state the table says.  The walk starts from a created
   context and follows both sides, so it also shows that a Life loses nothing the old flags
   told a ladder (two flag states with one Life are never told apart by any call).
3. The states the transitions reach from "created" are exactly the table's rows.
4. No Call is missing from the table, no Wait outcome either.
5. The probe builds with the address and undefined-behaviour sanitizers (host code, a
   stand-alone program) and runs clean over the whole table.
"""
import os
import re
import shutil
import subprocess

import pytest

import life_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _build(tmp, name, extra=()):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the life probe cannot be compiled")
    exe = str(tmp / name)
    subprocess.run(["hipcc", "-std=c++17", "-O1", *extra, "-I" + os.path.join(REPO, "distributed-faas_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), os.path.join(HERE, "life_probe.cpp"), "-o", exe], check=True)
    return exe


def _asker(exe, env=None):
    def ask(lines):
        if not lines:
            return []
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        out = p.stdout.splitlines()
        assert len(out) == len(lines), p.stdout[-2000:]
        for a, ln in zip(out, lines):
            assert not a.startswith("error="), (ln, a)
        return out
    return ask


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _asker(_build(tmp_path_factory.mktemp("life"), "life_probe"))


def _gate(answer):
    """(refusal or None, duties, settle due) of a probe gate line."""
    head, refuse = answer.split(" refuse=", 1)
    w = dict(x.split("=", 1) for x in head.split())
    return (None if refuse == "-" else refuse), ([] if w["duties"] == "-" else w["duties"].split(",")), w["settle"] == "1"


def _call_of(act):
    return {"stage": "stage", "launch": "launch", "continue": "tick_continue", "wait": "wait",
            "commit": "commit"}.get(act[0]) or act[1]


def walk(ask, kind):
    """Follow the table and the probe side by side from a created context.  Returns the Lifes
    reached and the number of (state, action) pairs compared."""
    start = lc.canon(kind, lc.CREATED)
    life_of = {lc.CREATED: start}
    todo, seen_life, n = [lc.CREATED], {start}, 0
    while todo:
        level, todo = todo, []
        pairs = [(r, act) for r in level for act in lc.actions(kind, r)]
        gates = ask(["gate %s %s %s" % (kind, life_of[r], _call_of(act)) for r, act in pairs])
        want, reqs = [], []
        for (r, act), g in zip(pairs, gates):
            refuse, duties, settle = _gate(g)
            w_refuse, w_duties, w_next = lc.apply(kind, r, act)
            assert (refuse, duties) == (w_refuse, w_duties), (kind, r, act, g)
            if refuse is None:
                st = lc.steps(act, duties, settle)
            else:  # (a refusal carries at most the flush)
                assert set(duties) <= {"flush"}, (kind, r, act, g)
                st = ["commit_ran"] if duties else []
            want.append(w_next)
            reqs.append("step %s %s %s" % (kind, life_of[r], " ".join(st)))
        for (r, act), w_next, got in zip(pairs, want, ask(reqs)):
            assert got == lc.canon(kind, w_next), (kind, r, act, got, lc.canon(kind, w_next))
            n += 1
            seen_life.add(got)
            if w_next not in life_of:
                life_of[w_next] = got
                todo.append(w_next)
    assert set(life_of) == lc.closure(kind)
    return seen_life, n


@pytest.fixture(scope="module")
def walks(probe):
    return {k: walk(probe, k) for k in lc.KINDS}


@pytest.mark.parametrize("kind", lc.KINDS)
def test_gate_matches_table(probe, kind):
    """Every row: each state of the table x each Call (the walk only asks the calls a flag
    state offers; here every one, on the canonical states)."""
    by_life = {}
    for r in lc.closure(kind):
        by_life.setdefault(lc.canon(kind, r), []).append(r)
    assert sorted(by_life) == sorted(lc.STATES[kind])
    rows = [(s, c) for s in lc.STATES[kind] for c in lc.CALLS]
    for (s, c), g in zip(rows, probe(["gate %s %s %s" % (kind, s, c) for s, c in rows])):
        refuse, duties, _ = _gate(g)
        for r in by_life[s]:  # whichever flags stood for this Life, the old ladder agrees
            assert lc.gate(kind, r, c) == (refuse, duties), (kind, s, c, r, g)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_transitions_match_table(walks, kind):
    reached, n = walks[kind]
    assert set(reached) == set(lc.STATES[kind]) and n >= len(lc.closure(kind))


@pytest.mark.parametrize("kind", lc.KINDS)
def test_reachable_states_are_the_table(walks, kind):
    assert sorted(walks[kind][0]) == sorted(lc.STATES[kind])


def test_no_call_missing(probe):
    assert tuple(probe(["calls"])[0].split()) == lc.CALLS
    assert tuple(probe(["waits"])[0].split()) == lc.WAITS
    # every public entry point of the header that reads the lifecycle is a Call or a sequence of them
    hdr = open(os.path.join(REPO, "include", "faasbal.h")).read()
    api = open(os.path.join(REPO, "distributed-faas_amd", "csrc", "faasbal_api.hip")).read()
    for c in lc.CALLS:
        assert re.search(r"enter\(c, [^;]*\bCall::%s\b" % c, api), c
    # ... and enters by name: no entry point hands enter() a gate of its own making
    csrc = os.path.join(REPO, "distributed-faas_amd", "csrc")
    for m in re.finditer(r"^(?:static )?int (fb_\w+|\w+_run)\([^;{]*\{\n(.*?)^\}\n", api, re.M | re.S):
        args = re.findall(r"\benter\(c, ([^;]*)\)\) return rc_;", m.group(2))
        assert len(args) == m.group(2).count("enter("), m.group(1)
        for arg in args:
            names = re.findall(r"Call::(\w+)", arg)
            assert names and set(names) <= set(lc.CALLS), (m.group(1), arg)
            assert re.fullmatch(r"(\w+ \? )?Call::\w+( : Call::\w+)?", arg), (m.group(1), arg)
    assert len(re.findall(r"\benter\(c, ", api)) >= len(lc.CALLS) - 2  # (the two pairs that share a body)
    assert len(re.findall(r"\bGate\b[^;\n]*\blife_gate\(", api)) == 1  # enter() itself
    for f in os.listdir(csrc):
        assert "life_gate" + "_" not in open(os.path.join(csrc, f)).read(), f  # (a gate beside life_gate)
    for flag in ("c->launched", "c->waited", "c->staged", "c->l_failed", "c->l_eager", "c->l_enospc", "c->phase",
                 "c->cm_pending", "c->stale_any", "c->undo_E", "c->l_win"):
        assert flag not in api, flag
    assert "fb_tick_wait" in hdr


def test_item4_rejected_load_keeps_stale(probe):
    """The one deliberate difference from the old library: a rejected load leaves the Life."""
    s = "0,none,0,0,0,0,0,1,0"
    assert s in lc.STATES["hb"]
    refuse, duties, _ = _gate(probe(["gate hb %s load_state" % s])[0])
    assert refuse is None and duties == []
    assert probe(["step hb %s %s" % (s, " ".join(lc.steps(("call", "load_state", "rejected"), [], True)))])[0] == s
    assert lc.LOAD_REJECTED_KEEPS_STALE


def test_item4_oracle_reaches_the_second_death():
    """The scripted GPU case of that difference, from the oracle alone: stale entries of the
    re-registered slot exist at its second death (restale_scenario asserts it)."""
    st, steps, final = lc.restale_scenario()
    assert [w is None for _, w in steps] == [False, True, False, False, False]
    assert len(steps[0][1]["orphans"]) == 4 and len(steps[4][1]["orphans"]) == 2 and final["reg"][0] == 0


def test_probe_sanitized(tmp_path):
    """Address + undefined-behaviour sanitizers on the host code, as a stand-alone program."""
    exe = _build(tmp_path, "life_probe_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    ask = _asker(exe, env)
    for kind in lc.KINDS:
        reached, _ = walk(ask, kind)
        assert sorted(reached) == sorted(lc.STATES[kind])
        ask(["gate %s %s %s" % (kind, s, c) for s in lc.STATES[kind] for c in lc.CALLS])
    marked = [s for s in lc.STATES["shard"] if s.endswith(",1")]
    assert marked == ["0,none,0,0,0,0,0,0,1"] and not any(s.endswith(",1") for k in lc.KINDS[:3] for s in lc.STATES[k])
    assert ask(["step shard %s %s" % (marked[0], ev) for ev in ("marked", "unmarked", "replaced")]) == \
        [marked[0], "0,none,0,0,0,0,0,0,0", "0,none,0,0,0,0,0,0,0"]
