"""plan_tick (csrc/faasbal_plan.h) without a GPU: tests/plan_probe.cpp, compiled here, prints
the plan of each request.

1. Every case of tests/plan_cases.py launches what the table says -- the table
   tests/test_gpu_plan.py holds the real launches to.
2. The benchmark's shapes take the sequences `bench.py --full` names (kernels_avg_ms /
   kernels_us_per_tick), recorded from the library before plan_tick existed.
3. fb_exchange_bytes' rows helper and plan_tick's layout agree across the xrows_mode
   boundaries.
"""
import collections
import os
import shutil
import subprocess

import pytest

import plan_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
UNLABELLED = ("pos_rebuild", "orph_gather")  # launches fb_timing_read does not name


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: the plan probe cannot be compiled")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_probe")
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-I" + os.path.join(REPO, "distributed-faas_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), os.path.join(HERE, "plan_probe.cpp"), "-o", exe], check=True)

    def raw(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout

    def ask(requests):
        """One answer dict per request line ("cmd k=v ..." or (cmd, {k: v}))."""
        lines = [r if isinstance(r, str) else r[0] + "".join(" %s=%d" % kv for kv in r[1].items()) for r in requests]
        out = raw("\n".join(lines) + "\n")
        ans = [dict(w.split("=", 1) for w in ln.split()) for ln in out.splitlines()]
        assert len(ans) == len(lines), out
        for a, ln in zip(ans, lines):
            assert "error" not in a, (ln, a)
        return ans

    ask.raw = raw
    return ask


def _stages(ans):
    return [s for s in ans["stages"].split(",") if s]


def _window(probe):
    def f(fields):
        a = probe([("window", fields)])[0]
        return a["window"] == "1", int(a["nchW"])
    return f


# ------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES])
def test_plan_matches_table(probe, name):
    case = pc.BY_NAME[name]
    got = collections.Counter()
    for fields, outside in pc.case_launches(case, _window(probe)):
        got.update(outside)
        if fields is not None:
            got.update(s for s in _stages(probe([("plan", fields)])[0]) if s not in UNLABELLED)
    assert dict(got) == case["expect"]


def test_table_flags(probe):
    """What the table's counts cannot show: where the commit goes, the sort's digits, the
    unlabelled launches, the phase-2 forms."""
    def plans(name):
        return probe([("plan", f) for f, _ in pc.case_launches(pc.BY_NAME[name], _window(probe)) if f is not None])

    assert plans("commit_folds_into_scan")[0]["cm_fold"] == "1"
    assert plans("commit_rides_in_ev_link")[0]["commit"] == "2"       # CommitPlan::in_ev_link
    assert _stages(plans("commit_first_after_msgs")[0])[0] == "commit"
    assert plans("fused_idle")[0]["commit"] == "0"
    wide, narrow = plans("sort_wide")[0], plans("sort_narrow")[0]
    assert (wide["passes"], wide["db"], wide["wide"]) == ("2", "9", "1")  # 18 slot bits
    assert (narrow["passes"], narrow["db"], narrow["wide"]) == ("3", "8", "0")
    first, rerun = plans("resort_rerun")
    assert (first["grouping"], rerun["grouping"]) == ("1", "2")       # lists, then the sort
    assert _stages(plans("window_after_general")[0])[0] == "pos_rebuild"
    assert "pos_rebuild" not in _stages(plans("window_direct")[0])
    assert plans("window_direct")[0]["win_direct"] == "1" and plans("window_ticket")[0]["win_direct"] == "0"
    assert plans("plan1_gp1")[0]["gp"] == "1" and plans("plan1_gp0")[0]["gp"] == "0"
    p1, p2 = plans("shard_rows_grouped_idle")
    assert int(p1["xrb"]) > 0 and int(p1["xgb"]) > 0 and p1["xrb"] == p2["xrb"]
    assert int(plans("shard_rows_plain")[1]["xrb"]) > 0 and plans("shard_rows_plain")[1]["xgb"] == "0"
    assert plans("shard_recount")[1]["xrb"] == "0" and plans("shard_recount")[1]["sgrp"] == "1"
    assert plans("shard_xplan")[1]["xplan"] == "1" and plans("shard_xplan")[1]["xself"] == "1"
    assert plans("shard_xplan_off_xself0")[1]["xplan"] == "0" and plans("shard_xplan_off_xself0")[1]["xrb"] == "0"


def test_knob_table(probe):
    """fb_set_path's names and accepted values (include/faasbal.h)."""
    assert probe(["knobs"])[0] == {
        "plan": "0,1,2", "logscan": "-1,0,1", "split_slots": "-1,0,1", "ev_ll": "0,1", "rs_wide": "0,1",
        "fault_qlen": "any", "xplan": "0,1", "gp": "0,1", "win_direct": "0,1", "xself": "0,1", "wfirst": "0,1",
        "gpcheck": "0,1", "cmix": "0,1", "wtiles": "0,1,2,4", "qtiles": "0,1,4", "lazy": "0,1", "xcfirst": "0,1"}
    # a value outside a knob's list is refused, as fb_set_path refuses it
    out = probe.raw("plan knob.wtiles=3\nplan knob.nosuch=1\nplan knob.wtiles=4\n")
    assert [("error" in ln) for ln in out.splitlines()] == [True, True, False]


# ------------------------------------------------------------------ 2. the benchmark's shapes
def test_workload_shapes(probe):
    for name, launches, expect in pc.workloads(_window(probe)):
        got = [s for a in probe([("plan", f) for f in launches]) for s in _stages(a) if s not in UNLABELLED]
        assert got == expect, name


# ------------------------------------------------------------------ 3. the exchange layout
def test_exchange_layout_agrees(probe):
    """The buffer fb_exchange_bytes asks for and the layout phase 1 writes, over the three
    xrows_mode boundaries: 256 queue blocks, R = 32 / 64 / 128 / 256, 16 / 17 ranks."""
    grid = [dict(world=w, R=R, Qlog=q, E=E, xplan=x)
            for w in (2, 16, 17) for R in (32, 64, 128, 256) for q in (300, 255 * 256 + 1, 256 * 256, 256 * 256 + 1, 70000)
            for E in (0, 77) for x in (0, 1)]
    for g, a in zip(grid, probe([("xbytes", g) for g in grid])):
        assert (a["rows"], a["grows"], a["total"], a["rows_at"]) == \
               (a["plan_rows"], a["plan_grows"], a["plan_total"], a["plan_rows_at"]), g
        nbq = -(-g["Qlog"] // 256)
        mode = 0 if g["world"] > 16 or g["R"] > 128 else 1 if nbq <= 256 else 2 if g["R"] == 32 else 0
        assert int(a["mode"]) == mode, g
        rows = mode == 1 or (mode == 2 and g["xplan"])
        assert (int(a["rows"]) > 0) == rows and (int(a["grows"]) > 0) == (mode == 1 and g["R"] == 32), g
