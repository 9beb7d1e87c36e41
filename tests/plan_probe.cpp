// plan_probe -- the launch plan (csrc/faasbal_plan.h) from the command line, no GPU.
//
// Reads one request per line on stdin, answers each with one line of key=value words:
//   plan   k=v ...   plan_tick of a PlanIn (fields by name, "knob.<fb_set_path name>=v")
//   window k=v ...   plan_window of a WindowIn
//   xbytes world=.. R=.. Qlog=.. E=.. xplan=..
//                    the exchange layout as fb_exchange_bytes sizes it (exchange_rows) and
//                    as plan_tick lays it out for phase 1 of the same shape
//   knobs            the fb_set_path table: name=allowed values
//   choose_R maxc=.. [shard=1]
//                    the round table's rows for a largest free count, and the row limit it
//                    saturates at (kMaxR; shard=1: kShardMaxR)
//   layout k=v ...   the plan of a PlanIn, then every multi-role kernel it launches walked
//                    through its layout (csrc/faasbal_layout.h): "<kernel>.grid", ".n" (the
//                    workgroups per role), ".pad" and ".cover" (1: workgroups 0 .. grid-1 gave
//                    every (role, index) exactly once, the rest padding); ".lds" where the
//                    launch requests dynamic LDS.  "cm.<CommitArgs field>" describe the pending
//                    commit, "tbits=0" a context without the touched bitmap
//   walk kernel=<name> k=v ...
//                    one kernel's layout from its argument block's fields: TickArgs by name,
//                    "ev.", "cm.", "copy." (n, words0 .. words3, otiles) for the others, nsb
// Built by tests/test_plan.py; it makes no HIP runtime call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "faasbal_plan.h"

using namespace fb;

namespace {

bool set_knob(PathKnobs &k, const std::string &name, long long v) {
    for (const PathKnob &d : kPathKnobs)
        if (name == d.name && knob_allows(d, (int)v)) {
            k.*d.member = (int)v;
            return true;
        }
    return false;
}

bool set_plan_field(PlanIn &in, const std::string &key, long long v) {
#define F(name)          \
    if (key == #name) {  \
        in.name = v;     \
        return true;     \
    }
    F(shard) F(phase) F(world) F(deque) F(heartbeat) F(lists) F(qaos) F(compact) F(cout) F(cout_cap) F(cout_ecap)
    F(cout_ocap) F(W) F(W_global) F(E) F(R) F(head) F(head_local) F(Qn) F(T) F(ncu) F(max_lds) F(win_occ) F(l_win)
    F(l_nchW) F(pos_ok) F(l_resort) F(l_purge_only) F(stale_any) F(cm_pending) F(cm_oseg) F(cm_E) F(cm_win)
    F(cm_n_clr) F(cm_shard) F(cm_oseg_tiles) F(cm_n_orph)
#undef F
    if (key.rfind("knob.", 0) == 0) return set_knob(in.knobs, key.substr(5), v);
    return false;
}

bool set_window_field(WindowIn &w, const std::string &key, long long v) {
#define F(name)          \
    if (key == #name) {  \
        w.name = v;      \
        return true;     \
    }
    F(win_cap) F(mode) F(lists) F(ev_ll) F(compact) F(purge_only) F(deque) F(shard) F(E) F(W) F(max_lds) F(last_L)
    F(T) F(last_O) F(win_slack) F(Qn) F(qoff) F(qcap)
#undef F
    return false;
}

// ---- layouts
struct LayoutArgs {
    TickArgs a{};
    EvArgs ev{};
    CommitArgs cm{};
    CopyMulti copy{};
    int nsb = 1, tbits = 1;
};

bool set_layout_field(LayoutArgs &l, const std::string &key, long long v) {
#define F(pre, obj, name)          \
    if (key == pre #name) {        \
        l.obj.name = v;            \
        return true;               \
    }
    F("", a, W) F("", a, E) F("", a, R) F("", a, nbw) F("", a, nbf) F("", a, nbq) F("", a, f_sep) F("", a, f_emit)
    F("", a, slots_in_scan) F("", a, slots_in_apply) F("", a, shard) F("", a, wtiles) F("", a, qtiles)
    F("", a, cm_fold) F("", a, cm_blocks) F("", a, wfirst) F("", a, cmix) F("", a, xcfirst) F("", a, ngrp)
    F("", a, nchB) F("", a, nchF) F("", a, nchW) F("", a, lds_bitmap)
    F("ev.", ev, E) F("ev.", ev, nbw) F("ev.", ev, wtiles) F("ev.", ev, cm_blocks) F("ev.", ev, tbits_words)
    F("cm.", cm, nbw) F("cm.", cm, nbo) F("cm.", cm, n_clr) F("cm.", cm, win) F("cm.", cm, nbap) F("cm.", cm, n_tomb)
    F("copy.", copy, n) F("copy.", copy, otiles)
#undef F
    if (key.rfind("copy.words", 0) == 0 && key.size() == 11 && key[10] >= '0' && key[10] <= '3') {
        l.copy.words[key[10] - '0'] = v;
        return true;
    }
    if (key == "nsb") l.nsb = (int)v;
    else if (key == "tbits") l.tbits = (int)v;
    else return false;
    return true;
}

// every workgroup of the grid through role_at: each (role, index) once, the rest padding
template <class L>
void walk(const char *name, const L &l) {
    std::vector<std::vector<int>> seen(L::kRoles);
    for (int r = 0; r < L::kRoles; ++r) seen[r].assign((size_t)std::max(0, l.count(r)), 0);
    int pad = 0;
    bool ok = l.grid() >= 0;
    for (int blk = 0; blk < l.grid(); ++blk) {
        const Role ro = role_at(l, blk);
        if (ro.role == kPadding) ++pad;
        else if (ro.role < 0 || ro.role >= L::kRoles || ro.idx < 0 || ro.idx >= l.count(ro.role)) ok = false;
        else ++seen[ro.role][ro.idx];
    }
    std::printf(" %s.grid=%d %s.n=", name, l.grid(), name);
    for (int r = 0; r < L::kRoles; ++r) {
        std::printf("%s%d", r ? "," : "", l.count(r));
        for (int c : seen[r]) ok = ok && c == 1;
    }
    std::printf(" %s.pad=%d %s.cover=%d", name, pad, name, (int)ok);
}

void walk_scan(const char *name, const TickArgs &a) {
    walk(name, scan_layout(a));
    // (commit0: where k_scan itself puts a folded commit's first workgroup in this grid)
    std::printf(" %s.wt=%d %s.lds=%zu %s.commit0=%d", name, scan_wt(a), name, scan_lds_bytes(a), name,
                FB_SCAN_FIRST_COMMIT(scan_layout(a).grid(), a));
}
void walk_emit2(const TickArgs &a) {
    walk("k_emit2", emit2_layout(a));
    std::printf(" k_emit2.lds=%zu", emit2_lds_bytes(a));
}
void walk_copy(CopyMulti m) {
    // blk0 as fb_get_compact fills it
    for (int i = 1; i < m.n; ++i) m.blk0[i] = m.blk0[i - 1] + copy_blocks(m.words[i - 1]);
    walk("k_copy_multi", copy_multi_layout(m));
}

bool walk_named(const std::string &k, const LayoutArgs &l) {
    if (k == "k_ev_link") walk("k_ev_link", ev_link_layout(l.ev));
    else if (k == "k_ev_apply_ll") walk("k_ev_apply_ll", ev_apply_ll_layout(l.ev));
    else if (k == "k_scan") walk_scan("k_scan", l.a);
    else if (k == "k_emit") walk("k_emit", emit_layout(l.a));
    else if (k == "k_emit2") walk_emit2(l.a);
    else if (k == "k_emit_shard") walk("k_emit_shard", emit_shard_layout(l.a, l.nsb));
    else if (k == "k_plan") walk("k_plan", plan_layout(l.a));
    else if (k == "k_plan2") walk("k_plan2", plan2_layout(l.a));
    else if (k == "k_xscan") walk("k_xscan", xscan_layout(l.a));
    else if (k == "k_emit_win") walk("k_emit_win", emit_win_layout(l.a));
    else if (k == "k_commit") walk("k_commit", commit_layout(l.cm));
    else if (k == "k_copy_multi") walk_copy(l.copy);
    else return false;
    return true;
}

// the multi-role kernels of a plan, with the layout fields as fill_ev_args and the launch
// functions of faasbal_api.hip set them
void walk_plan(const TickArgs &a, const TickPlan &p, const LayoutArgs &l) {
    EvArgs ev{};
    ev.E = a.E;
    ev.tbits_words = l.tbits ? (int)cdiv(a.W, 32) : 0;
    ev.nbw = a.nbw;
    ev.wtiles = p.ev_wtiles;
    if (p.commit == CommitPlan::in_ev_link) ev.cm_blocks = commit_layout(l.cm).grid();
    for (int i = 0; i < p.n_stages; ++i) {
        const Stage s = p.stages[i];
        if (s == Stage::commit || (s == Stage::ev_link && p.commit == CommitPlan::in_ev_link))
            walk("k_commit", commit_layout(l.cm));
        if (s == Stage::ev_link) walk("k_ev_link", ev_link_layout(ev));
        else if (s == Stage::ev_apply && p.grouping == Grouping::lists) walk("k_ev_apply_ll", ev_apply_ll_layout(ev));
        else if (s == Stage::scan) walk_scan("k_scan", a);
        else if (s == Stage::scan2) walk_scan("k_scan2", a);
        else if (s == Stage::logscan) std::printf(" k_logscan.grid=%d k_logscan.lds=%zu", p.ls_grid, logscan_bitmap_lds(a.W).bytes);
        else if (s == Stage::plan && a.xplan) walk("k_xscan", xscan_layout(a));
        else if (s == Stage::plan && a.grp_on) walk("k_plan2", plan2_layout(a));
        else if (s == Stage::plan) walk("k_plan", plan_layout(a));
        else if (s == Stage::emit && p.kind == TickKind::window) walk("k_emit_win", emit_win_layout(a));
        else if (s == Stage::emit && p.kind == TickKind::shard_phase2)
            walk("k_emit_shard", emit_shard_layout(a, a.xplan ? kXpBlocks : 1));  // (k_emit_shard_xp, else one block each)
        else if (s == Stage::emit && a.segw) walk_emit2(a);
        else if (s == Stage::emit) walk("k_emit", emit_layout(a));
    }
}

void print_plan(const TickArgs &a, const TickPlan &p, bool newline = true) {
    std::printf("stages=");
    for (int i = 0; i < p.n_stages; ++i) std::printf("%s%s", i ? "," : "", stage_name(p.stages[i]));
    std::printf(" kind=%d grouping=%d passes=%d db=%d wide=%d ls_grid=%d gplan=%d sgrp=%d xrb=%zu xgb=%zu xtotal=%zu"
                " l_cout=%d l_oseg=%d commit=%d err=%d",
                (int)p.kind, (int)p.grouping, p.passes, p.db, (int)p.wide, p.ls_grid, (int)p.gplan, (int)p.sgrp, p.xrb,
                p.xgb, p.xl.total, (int)p.l_cout, (int)p.l_oseg, (int)p.commit, (int)p.err);
    std::printf(" fused=%d segw=%d grp_on=%d ngrp=%d f_sep=%d f_emit=%d slots_in_scan=%d slots_in_apply=%d gp=%d"
                " cmix=%d wtiles=%d qtiles=%d cm_fold=%d live_chk=%d xplan=%d xself=%d xcfirst=%d wfirst=%d"
                " win_direct=%d nchW=%d%s",
                a.fused, a.segw, a.grp_on, a.ngrp, a.f_sep, a.f_emit, a.slots_in_scan, a.slots_in_apply, a.gp, a.cmix,
                a.wtiles, a.qtiles, a.cm_fold, a.live_chk, a.xplan, a.xself, a.xcfirst, a.wfirst, a.win_direct,
                a.nchW, newline ? "\n" : "");
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string cmd, kv;
        if (!(ss >> cmd)) continue;
        PlanIn in;
        WindowIn w{};
        LayoutArgs lay;
        std::string kernel;
        long long world = 1, R = 32, Qlog = 0, E = 0, xplan = 1, maxc = 0, shard = 0;
        bool ok = cmd == "choose_R" || cmd == "plan" || cmd == "window" || cmd == "xbytes" || cmd == "knobs" || cmd == "layout" || cmd == "walk";
        while (ok && ss >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) {
                ok = false;
                break;
            }
            const std::string key = kv.substr(0, eq);
            const long long v = std::atoll(kv.c_str() + eq + 1);
            if (cmd == "plan") ok = set_plan_field(in, key, v);
            else if (cmd == "layout") ok = set_plan_field(in, key, v) || set_layout_field(lay, key, v);
            else if (cmd == "walk" && key == "kernel") kernel = kv.substr(eq + 1);
            else if (cmd == "walk") ok = set_layout_field(lay, key, v);
            else if (cmd == "window") ok = set_window_field(w, key, v);
            else if (cmd == "choose_R" && key == "maxc") maxc = v;
            else if (cmd == "choose_R" && key == "shard") shard = v;
            else if (key == "world") world = v;
            else if (key == "R") R = v;
            else if (key == "Qlog") Qlog = v;
            else if (key == "E") E = v;
            else if (key == "xplan") xplan = v;
            else ok = false;
            if (!ok) std::printf("error=bad_field:%s\n", kv.c_str());
        }
        if (!ok) {
            if (kv.empty()) std::printf("error=bad_request\n");
            continue;
        }
        if (cmd == "choose_R") {
            const int limit = shard ? kShardMaxR : kMaxR;
            std::printf("R=%d limit=%d\n", choose_R((int32_t)maxc, limit), limit);
            std::fflush(stdout);
        } else if (cmd == "plan") {
            TickArgs a{};
            TickPlan p;
            plan_tick(in, a, p);
            print_plan(a, p);
        } else if (cmd == "layout") {
            TickArgs a{};
            TickPlan p;
            plan_tick(in, a, p);
            print_plan(a, p, false);
            walk_plan(a, p, lay);
            std::printf("\n");
        } else if (cmd == "walk") {
            std::printf("kernel=%s", kernel.c_str());
            if (!walk_named(kernel, lay)) std::printf(" error=bad_kernel");
            std::printf("\n");
        } else if (cmd == "window") {
            int nchW = 0;
            const bool yes = plan_window(w, nchW);
            std::printf("window=%d nchW=%d\n", (int)yes, nchW);
        } else if (cmd == "xbytes") {
            PathKnobs k;
            k.xplan_on = (int)xplan;
            const XRows xr = exchange_rows(k, (int)world, (int)R, Qlog);
            const XLayout xl = xlayout((int)world, E, Qlog, xc_width((int)R), xr.rows, xr.grows);
            in.shard = 1;
            in.phase = 1;
            in.world = (int)world;
            in.R = (int)R;
            in.E = (int)E;
            in.Qn = Qlog - 2 * E;
            in.knobs = k;
            TickArgs a{};
            TickPlan p;
            plan_tick(in, a, p);
            std::printf("mode=%d rows=%zu grows=%zu total=%zu plan_rows=%zu plan_grows=%zu plan_total=%zu"
                        " plan_rows_at=%zu rows_at=%zu\n",
                        xrows_mode((int)world, (int)R, Qlog), xr.rows, xr.grows, xl.total, p.xrb, p.xgb, p.xl.total,
                        p.xl.rows, xl.rows);
        } else {
            for (const PathKnob &d : kPathKnobs) {
                std::printf("%s=%s", d.name, d.n_allowed ? "" : "any");
                for (int i = 0; i < d.n_allowed; ++i) std::printf("%s%d", i ? "," : "", d.allowed[i]);
                std::printf(" ");
            }
            std::printf("\n");
        }
    }
    return 0;
}
