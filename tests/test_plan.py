"""plan_tick (csrc/faasbal_plan.h) without a GPU: tests/plan_probe.cpp, compiled here, prints
the plan of each request.

1. Every case of tests/plan_cases.py launches what the table says -- the table
   tests/test_gpu_plan.py holds the real launches to.
2. The benchmark's shapes take the sequences `bench.py --full` names (kernels_avg_ms /
   kernels_us_per_tick), recorded from the library before plan_tick existed.
3. fb_exchange_bytes' rows helper and plan_tick's layout agree across the xrows_mode
   boundaries.
4. Every multi-role kernel's layout (csrc/faasbal_layout.h: what the launcher sizes the grid
   with and the kernel decodes blockIdx.x with) covers its roles exactly: workgroups
   0 .. grid-1 give every (role, index) once, the rest padding -- for every launch of 1. and
   2. and for sweeps around the places where the arithmetic can go wrong.  The dynamic LDS
   a plan requests fits the device's, and plan_window answers as it did when it tested its
   own spelling of k_logscan's bitmap size.
5. choose_R ends for every int32 and saturates at the row limit (kMaxR, sharded kShardMaxR),
   and the plans of a table at the limit stay inside the table cap or name a PlanError.
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

    def raw(text, timeout=60):
        # (a time limit: a request that never ends fails its test instead of stalling the run)
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=timeout).stdout

    def ask(requests, timeout=60):
        """One answer dict per request line ("cmd k=v ..." or (cmd, {k: v}))."""
        lines = [r if isinstance(r, str) else r[0] + "".join(" %s=%d" % kv for kv in r[1].items()) for r in requests]
        out = raw("\n".join(lines) + "\n", timeout)
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


# ------------------------------------------------------------------ 4. grids and LDS
def _kernels(ans):
    """{kernel: {grid, n, pad, cover, ...}} of a layout / walk answer."""
    out = collections.defaultdict(dict)
    for k, v in ans.items():
        if "." in k:
            out[k.split(".")[0]][k.split(".")[1]] = v
    return dict(out)


def _check_cover(ans, where, pad_ok=()):
    ks = _kernels(ans)
    for name, k in ks.items():
        if "cover" not in k:
            continue  # (k_logscan: one role, its grid is the plan's)
        n = [int(x) for x in k["n"].split(",")]
        assert k["cover"] == "1", (where, name, k)
        assert int(k["grid"]) == sum(n) + int(k["pad"]) and min(n) >= 0, (where, name, k)
        assert int(k["pad"]) == 0 or name in pad_ok, (where, name, k)
    return ks


# the kernel(s) each stage of a plan launches through a layout
def _expected_kernels(a):
    st = _stages(a)
    want = []
    for s in st:
        if s == "ev_link":
            want += ["k_ev_link"] + (["k_commit"] if a["commit"] == "2" else [])
        elif s == "ev_apply" and a["grouping"] == "1":
            want.append("k_ev_apply_ll")
        elif s == "scan":
            want.append("k_scan")
        elif s == "scan2":
            want.append("k_scan2")
        elif s == "commit":
            want.append("k_commit")
        elif s == "plan":
            want.append("k_xscan" if a["xplan"] == "1" else "k_plan2" if a["grp_on"] == "1" else "k_plan")
        elif s == "emit":
            want.append({"0": "k_emit_win", "2": "k_emit_shard"}.get(a["kind"], "k_emit2" if a["segw"] == "1" else "k_emit"))
    return want


def _layout_fields(f):
    """A launch's PlanIn fields plus the pending commit's CommitArgs as fb_tick_commit builds them."""
    f = dict(f)
    if f.get("cm_pending"):
        f.update({"cm.nbw": -(-f["W"] // 256), "cm.nbo": -(-f.get("cm_n_orph", 0) // 256), "cm.n_clr": f.get("cm_n_clr", 0)})
    f["tbits"] = 0 if f.get("shard") or f.get("deque") else 1
    return f


def _check_plan_layouts(probe, fields, where):
    a = probe([("layout", _layout_fields(fields))])[0]
    ks = _check_cover(a, where, pad_ok=("k_emit2",))
    walked = [k for k in ks if "cover" in ks[k]]
    assert sorted(walked) == sorted(set(_expected_kernels(a))), (where, walked, _stages(a))
    for k in ks.values():  # every dynamic-LDS request fits
        assert int(k.get("lds", 0)) <= fields["max_lds"], (where, k)
    if a["f_sep"] == "1" or a["kind"] == "0":
        assert "logscan" not in _stages(a) or "lds" in ks["k_logscan"], where
    return a, ks


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES])
def test_layouts_cover_table(probe, name):
    for i, (fields, _) in enumerate(pc.case_launches(pc.BY_NAME[name], _window(probe))):
        if fields is not None:
            _check_plan_layouts(probe, fields, (name, i))


def test_layouts_cover_workloads(probe):
    for name, launches, _ in pc.workloads(_window(probe)):
        for i, f in enumerate(launches):
            _check_plan_layouts(probe, f, (name, i))


def _walk(probe, kernel, grid):
    reqs = [dict(g) for g in grid]
    lines = ["walk kernel=%s" % kernel + "".join(" %s=%d" % kv for kv in g.items()) for g in reqs]
    return list(zip(reqs, probe(lines)))


def test_cmix_and_emit2_sweep(probe):
    """k_emit2: queue blocks 1..40 x compaction workgroups 0..40 under cmix (whole rows of 8,
    the tails padding) and without; tile counts at 4k-1, 4k, 4k+1; f_emit's one-tile log role."""
    grid = [dict(nbq=q, nbf=4 * (nc // 2), nbw=4 * (nc - nc // 2), cmix=cm) for q in range(1, 41) for nc in range(41)
            for cm in (0, 1)]
    grid += [dict(nbq=q, nbf=f, nbw=w, cmix=cm, f_emit=fe) for q in (1, 8, 9) for f in (0, 3, 4, 5, 7, 8, 9)
             for w in (1, 3, 4, 5, 7, 8, 9) for cm in (0, 1) for fe in (0, 1)]
    for g, a in _walk(probe, "k_emit2", grid):
        k = _check_cover(a, g, pad_ok=("k_emit2",))["k_emit2"]
        nf = g["nbf"] if g.get("f_emit") else -(-g["nbf"] // 4)
        assert k["n"] == "%d,%d,%d" % (g["nbq"], nf, -(-g["nbw"] // 4)), g
        nc = nf + -(-g["nbw"] // 4)
        assert int(k["grid"]) == (8 * (-(-g["nbq"] // 8) + -(-nc // 8)) if g["cmix"] else g["nbq"] + nc), g
        assert g["cmix"] or k["pad"] == "0", g


def test_scan_sweep(probe):
    """k_scan: wfirst's permutation (queue blocks 1..39 x log + slot workgroups 0..39, with and
    without a folded commit's blocks); wtiles x qtiles x slot workgroups present or absent --
    without them the one-tile instance runs and qtiles groups nothing."""
    grid = [dict(nbq=q, nbf=x // 2, nbw=x - x // 2, wfirst=wf, shard=1, slots_in_scan=1, wtiles=1, cm_fold=cf, cm_blocks=3)
            for q in range(1, 40) for x in range(40) for wf in (0, 1) for cf in (0, 1)]
    for g, a in _walk(probe, "k_scan", grid):
        k = _check_cover(a, g)["k_scan"]
        assert k["n"] == "%d,%d,%d,%d" % (g["nbq"], g["nbf"], g["nbw"], 3 * g["cm_fold"]), g
        assert not g["cm_fold"] or int(k["commit0"]) == g["nbq"] + g["nbf"] + g["nbw"], g
    grid = [dict(nbq=q, nbf=f, nbw=w, wtiles=wt, qtiles=qt, slots_in_scan=sl, f_emit=fe, cm_fold=cf, cm_blocks=2)
            for q in (1, 3, 4, 5, 8, 9) for f in (0, 5) for w in (1, 3, 4, 5, 7, 8, 9) for wt in (1, 2, 4) for qt in (1, 4)
            for sl in (0, 1) for fe in (0, 1) for cf in (0, 1)]
    for g, a in _walk(probe, "k_scan", grid):
        k = _check_cover(a, g)["k_scan"]
        nw = -(-g["nbw"] // g["wtiles"]) if g["slots_in_scan"] else 0
        wt = g["wtiles"] if nw else 1
        nq = -(-g["nbq"] // 4) if (wt == 4 and g["qtiles"] == 4) else g["nbq"]
        assert (k["wt"], k["n"]) == (str(wt), "%d,%d,%d,%d" % (nq, 0 if g["f_emit"] else g["nbf"], nw, 2 * g["cm_fold"])), g
    # phase 2 (scan2): queue workgroups only
    for g, a in _walk(probe, "k_scan", [dict(nbq=7, nbf=5, nbw=9, shard=2, slots_in_scan=1, wtiles=4, qtiles=4)]):
        assert _check_cover(a, g)["k_scan"]["n"] == "7,0,0,0"


def test_emit_shard_sweep(probe):
    """k_emit_shard / _wide (a queue block per workgroup) and k_emit_shard_xp (two), xcfirst on
    and off, queue blocks odd and even, tile counts around multiples of 4."""
    grid = [dict(nbq=q, nbf=f, nbw=w, nsb=nsb, xcfirst=xc) for q in (1, 2, 7, 8, 39, 40) for f in (0, 3, 4, 5, 8, 9)
            for w in (1, 3, 4, 5, 8, 9) for nsb in (1, 2) for xc in (0, 1)]
    for g, a in _walk(probe, "k_emit_shard", grid):
        k = _check_cover(a, g)["k_emit_shard"]
        assert k["n"] == "%d,%d,%d" % (-(-g["nbq"] // g["nsb"]), -(-g["nbf"] // 4), -(-g["nbw"] // 4)), g


def test_message_and_commit_grids(probe):
    """k_ev_apply_ll with E at 1, 256, 257; k_ev_link with and without commit blocks; the
    commit's five ranges empty and non-empty (window ranges only on window commits; an eager
    commit differs in nbap alone); k_copy_multi's copies and orphan tiles."""
    grid = [{"ev.E": E, "ev.nbw": w, "ev.wtiles": wt} for E in (1, 256, 257) for w in (1, 3, 4, 5, 1024) for wt in (1, 2, 4)]
    for g, a in _walk(probe, "k_ev_apply_ll", grid):
        k = _check_cover(a, g)["k_ev_apply_ll"]
        assert k["n"] == "%d,%d" % (-(-g["ev.E"] // 256), -(-g["ev.nbw"] // 4) if g["ev.wtiles"] == 4 else g["ev.nbw"]), g
    grid = [{"ev.E": E, "ev.tbits_words": tb, "ev.cm_blocks": cm} for E in (1, 256, 257, 70000) for tb in (0, 128, 1 << 20)
            for cm in (0, 1, 17)]
    for g, a in _walk(probe, "k_ev_link", grid):
        k = _check_cover(a, g)["k_ev_link"]
        link = max(1, -(-g["ev.E"] // 256), min(-(-g["ev.tbits_words"] // 256), 1024))
        assert k["n"] == "%d,%d" % (link, g["ev.cm_blocks"]), g
    grid = [{"cm.nbw": s, "cm.nbo": o, "cm.n_clr": c, "cm.win": w, "cm.nbap": ap * w, "cm.n_tomb": tb * w}
            for s in (0, 5) for o in (0, 3) for c in (0, 1, 256, 257) for w in (0, 1) for ap in (0, 1, 1024)
            for tb in (-1, 0, 1, 512, 513)]
    for g, a in _walk(probe, "k_commit", grid):
        k = _check_cover(a, g)["k_commit"]
        tb = max(0, -(-g["cm.n_tomb"] // 256))
        assert k["n"] == "%d,%d,%d,%d,%d" % (g["cm.nbw"], g["cm.nbo"], -(-g["cm.n_clr"] // 256), g["cm.nbap"], tb), g
    grid = [{"copy.n": n, "copy.words0": w0, "copy.words1": 10, "copy.words2": 1024 * 513, "copy.words3": 1, "copy.otiles": ot}
            for n in range(5) for w0 in (1, 1024, 1025, 1 << 22) for ot in (0, 3)]
    for g, a in _walk(probe, "k_copy_multi", grid):
        k = _check_cover(a, g)["k_copy_multi"]
        blocks = [min(max(1, -(-w // 1024)), 512) for w in (g["copy.words0"], 10, 1024 * 513, 1)]
        assert k["n"] == ",".join(str(b) for b in blocks[:g["copy.n"]] + [0] * (4 - g["copy.n"]) + [g["copy.otiles"]]), g


def test_small_grids(probe):
    """k_emit, k_plan, k_plan2, k_xscan, k_emit_win: the counts the launchers used to spell out."""
    for g, a in _walk(probe, "k_emit", [dict(nbq=q, nbf=f, nbw=w) for q in (1, 5) for f in (0, 7) for w in (1, 4)]):
        assert _check_cover(a, g)["k_emit"]["n"] == "%d,%d,%d" % (g["nbq"], g["nbf"], g["nbw"])
    for g, a in _walk(probe, "k_plan", [dict(R=R, shard=sh) for R in (32, 256, 4096) for sh in (0, 2)]):
        assert _check_cover(a, g)["k_plan"]["grid"] == str(3 + (2 if g["shard"] else 1) * g["R"])
    for g, a in _walk(probe, "k_plan2", [dict(ngrp=n) for n in (1, 2, 64)]):
        assert _check_cover(a, g)["k_plan2"]["grid"] == str(g["ngrp"] + 2)
    for g, a in _walk(probe, "k_xscan", [dict(nbq=n) for n in (1, 64, 65, 3547)]):
        assert _check_cover(a, g)["k_xscan"]["grid"] == str(-(-g["nbq"] // 64))
    for g, a in _walk(probe, "k_emit_win", [dict(nchB=b, nchF=b, nchW=w) for b in (1, 76) for w in (1, 100)]):
        assert _check_cover(a, g)["k_emit_win"]["grid"] == str(2 * g["nchB"] + g["nchW"])


# plan_window's answers to WINDOW_SWEEP's (W, max_lds), from the probe built at the commit before
# the layouts: it tested ((W + 63) / 64 + 2) * 8 against max_lds, a spelling of k_logscan's
# request that is 8 bytes short for an odd word count -- the same answer wherever max_lds is a
# multiple of 16.  W: small, either side of kLdsBitmapSlots, of a 64 KB and of the 160 KB limit.
WINDOW_W = [1, 63, 64, 65, 127, 128, (1 << 17) - 1, 1 << 17, (1 << 17) + 1,
            524096, 524097, 524159, 524160, 524161, 524224, 524225,
            1310464, 1310465, 1310528, 1310529, 1310591, 1310592, 1310593, 1310656, 1310657]
WINDOW_YES = {65536: 524160, 160 * 1024: 1310592}   # max_lds: the largest W with the answer yes
# Where the two spellings differ -- an odd word count and max_lds = 8 mod 16, which no device
# reports (LDS sizes are multiples of 16) -- plan_window now says no where it said yes: the
# launch it plans would ask for 8 bytes more than max_lds.  (W, max_lds, answer at the commit
# before the layouts, answer now); the even word counts beside it answer as before.
WINDOW_ODD = [(64 * 4093, 32760, 1, 0), (64 * 4092, 32760, 1, 1), (64 * 4094, 32760, 0, 0),
              (64 * 4093, 32752, 0, 0), (64 * 4093, 32768, 1, 1)]


def _logscan_bytes(W):
    return ((-(-W // 64) + 1) // 2 + 1) * 16


def test_window_and_lds_limits(probe):
    win = _window(probe)
    for W, max_lds, before, now in WINDOW_ODD:
        yes, _ = win(dict(win_cap=1, mode=1, lists=1, ev_ll=1, E=64, W=W, max_lds=max_lds, last_L=0, T=100, last_O=0,
                          win_slack=8192, Qn=W, qoff=0, qcap=4 * W + 100000))
        assert yes == bool(now) == (_logscan_bytes(W) <= max_lds), (W, max_lds)
        assert before == int((-(-W // 64) + 2) * 8 <= max_lds), (W, max_lds)  # the old spelling
    for max_lds, w_yes in WINDOW_YES.items():
        for W in WINDOW_W:
            yes, _ = win(dict(win_cap=1, mode=1, lists=1, ev_ll=1, E=64, W=W, max_lds=max_lds, last_L=0, T=100, last_O=0,
                              win_slack=8192, Qn=W, qoff=0, qcap=4 * W + 100000))
            assert yes == (W <= w_yes), (W, max_lds)
            assert yes == (_logscan_bytes(W) <= max_lds), (W, max_lds)
            # the plans of this table size: whatever they request fits
            base = dict(pc.DEVICE, max_lds=max_lds, W=W, W_global=W, R=32, head=5000, Qn=W, T=100, lists=1, qaos=1,
                        heartbeat=int(W <= pc.LDS_BITMAP_SLOTS))
            for more in (dict(), {"knob.logscan": 1}, dict(E=64), dict(E=64, l_win=int(yes), l_nchW=1)):
                a, ks = _check_plan_layouts(probe, dict(base, **more), (W, max_lds, more))
                if a["f_sep"] == "1" or a["kind"] == "0":
                    assert int(ks["k_logscan"]["lds"]) == _logscan_bytes(W) <= max_lds
                if a["f_emit"] == "1":
                    assert int(ks["k_emit2"]["lds"]) == _logscan_bytes(W) - 16 <= max_lds


def test_xcfirst_defaults_on_at_the_knob_shapes(probe):
    """tests/test_gpu_shard_forms.py runs its ladder and its 65 792-position scenario at world 2
    with xcfirst = 0: that is another launch order only where xcfirst defaults to 1
    (4 x (log + slot workgroups) > queue workgroups).  Every xplan phase 2 of both scenarios,
    on both ranks, asked of plan_tick."""
    import test_gpu_shard_forms as sf

    n = 0
    for scen, forms in ((sf._edge(65_792, 32), sf._edge_forms(32)), (sf._ladder(), sf.LADDER_FORMS)):
        fields = [(t, r, f) for t, r, f in sf.plan_fields(scen, 2) if forms[t][0] == "xplan"]
        for (t, r, f), a in zip(fields, probe([("plan", f) for _, _, f in fields])):
            assert _stages(a) == ["plan", "emit"] and a["xplan"] == "1", (t, r, a)
            assert a["xcfirst"] == "1", (t, r, f)
            n += 1
    assert n == 2 * (3 + sum(m[0] == "xplan" for m in sf.LADDER_FORMS))



# ------------------------------------------------------------------ 5. the round range
INT32_MAX = (1 << 31) - 1


def _choose_R(probe, maxc, shard=0):
    """(R, limit) -- each request in a process of its own under a time limit, so a loop that
    never ends fails here."""
    a = probe.raw("choose_R maxc=%d shard=%d\n" % (maxc, shard), timeout=10).split()
    a = dict(w.split("=", 1) for w in a)
    return int(a["R"]), int(a["limit"])


@pytest.mark.parametrize("shard", [0, 1])
def test_choose_R_ends_and_saturates(probe, shard):
    """For every largest free count an int32 can hold: a power of two, monotone in maxc, at
    least min(maxc, limit) and never beyond the limit (include/faasbal.h: FB_ERANGE)."""
    limit = _choose_R(probe, 1, shard)[1]
    assert limit == 4096
    assert pc.ROW_LIMIT == limit
    last = 0
    for maxc in (1, 31, 32, 33, limit - 1, limit, limit + 1, 1 << 30, (1 << 30) + 1, INT32_MAX):
        R, lim = _choose_R(probe, maxc, shard)
        assert lim == limit
        assert R >= 32 and R & (R - 1) == 0, (maxc, R)
        assert R >= last, (maxc, R, last)
        assert min(maxc, limit) <= R <= limit, (maxc, R)
        assert R == pc.choose_R(maxc), (maxc, R)
        last = R
    # (values an int32 holds but no free count should: the loop ends all the same)
    for maxc in (0, -1, -INT32_MAX - 1):
        assert _choose_R(probe, maxc, shard)[0] == 32


def test_plans_at_the_row_limit(probe):
    """A table of the limit's rows is planned like any other wide table -- no PlanError on one
    GPU nor in either sharded phase, within limit x nbq entries -- and a sharded table beyond
    the limit is the PlanError the host turns into FB_ERANGE, never a launch."""
    limit = pc.ROW_LIMIT
    for W in (40, 600, 70000):
        base = dict(pc.DEVICE, W=W, W_global=W, head=4 * W, Qn=W, T=W * (limit - 2))
        for maxc in (limit, limit + 1, (1 << 30) + 1, INT32_MAX):
            R = _choose_R(probe, maxc)[0]
            assert R == limit
            one = probe([("plan", dict(base, R=R, lists=1, qaos=1, heartbeat=1))], timeout=10)[0]
            assert one["err"] == "0" and _stages(one) == ["scan", "plan", "emit"], one
            assert (one["fused"], one["segw"]) == ("0", "0")  # the chunked k_emit
            for phase, want in ((1, ["scan"]), (2, ["scan2", "plan", "emit"])):
                sh = probe([("plan", dict(base, R=R, shard=1, world=2, phase=phase, head_local=2 * W))], timeout=10)[0]
                assert sh["err"] == "0" and _stages(sh) == want, sh
        over = probe([("plan", dict(base, R=2 * limit, shard=1, world=2, phase=2, head_local=2 * W))], timeout=10)[0]
        assert over["err"] == "3" and "emit" not in _stages(over), over  # PlanError::shard_rows


def test_fill_seam_shapes(probe):
    """The shapes tests/test_gpu_fill_seams.py relies on: 600 workers keep every table of at
    most 128 rows fused, the large case is unfused at 128 rows by itself (group rows reduced by
    k_emit2, no k_plan2), and tables beyond 128 rows take k_plan and the chunked k_emit."""
    import fill_cases as fc
    base = dict(pc.DEVICE, lists=1, qaos=1, heartbeat=1)
    small = dict(base, W=600, W_global=600, head=1200, Qn=600, T=1000)
    for R, fused in ((32, "1"), (64, "1"), (128, "1"), (256, "0"), (4096, "0")):
        a = probe([("plan", dict(small, R=R))])[0]
        assert (a["fused"], a["segw"]) == (fused, fused), (R, a)
        assert ("plan" in _stages(a)) == (R > 128), (R, a)
    W = fc.UNFUSED_W
    a = probe([("plan", dict(base, W=W, W_global=W, head=2 * W, Qn=W, T=W, R=128))])[0]
    assert (a["fused"], a["segw"], a["gp"]) == ("0", "1", "1") and "plan" not in _stages(a), a
