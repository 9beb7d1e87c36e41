// plan_probe -- the launch plan (csrc/faasbal_plan.h) from the command line, no GPU.
//
// Reads one request per line on stdin, answers each with one line of key=value words:
//   plan   k=v ...   plan_tick of a PlanIn (fields by name, "knob.<fb_set_path name>=v")
//   window k=v ...   plan_window of a WindowIn
//   xbytes world=.. R=.. Qlog=.. E=.. xplan=..
//                    the exchange layout as fb_exchange_bytes sizes it (exchange_rows) and
//                    as plan_tick lays it out for phase 1 of the same shape
//   knobs            the fb_set_path table: name=allowed values
// Built by tests/test_plan.py; it makes no HIP runtime call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

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

void print_plan(const TickArgs &a, const TickPlan &p) {
    std::printf("stages=");
    for (int i = 0; i < p.n_stages; ++i) std::printf("%s%s", i ? "," : "", stage_name(p.stages[i]));
    std::printf(" kind=%d grouping=%d passes=%d db=%d wide=%d ls_grid=%d gplan=%d sgrp=%d xrb=%zu xgb=%zu xtotal=%zu"
                " l_cout=%d l_oseg=%d commit=%d err=%d",
                (int)p.kind, (int)p.grouping, p.passes, p.db, (int)p.wide, p.ls_grid, (int)p.gplan, (int)p.sgrp, p.xrb,
                p.xgb, p.xl.total, (int)p.l_cout, (int)p.l_oseg, (int)p.commit, (int)p.err);
    std::printf(" fused=%d segw=%d grp_on=%d ngrp=%d f_sep=%d f_emit=%d slots_in_scan=%d slots_in_apply=%d gp=%d"
                " cmix=%d wtiles=%d qtiles=%d cm_fold=%d live_chk=%d xplan=%d xself=%d xcfirst=%d wfirst=%d"
                " win_direct=%d nchW=%d\n",
                a.fused, a.segw, a.grp_on, a.ngrp, a.f_sep, a.f_emit, a.slots_in_scan, a.slots_in_apply, a.gp, a.cmix,
                a.wtiles, a.qtiles, a.cm_fold, a.live_chk, a.xplan, a.xself, a.xcfirst, a.wfirst, a.win_direct,
                a.nchW);
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
        long long world = 1, R = 32, Qlog = 0, E = 0, xplan = 1;
        bool ok = cmd == "plan" || cmd == "window" || cmd == "xbytes" || cmd == "knobs";
        while (ok && ss >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) {
                ok = false;
                break;
            }
            const std::string key = kv.substr(0, eq);
            const long long v = std::atoll(kv.c_str() + eq + 1);
            if (cmd == "plan") ok = set_plan_field(in, key, v);
            else if (cmd == "window") ok = set_window_field(w, key, v);
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
        if (cmd == "plan") {
            TickArgs a{};
            TickPlan p;
            plan_tick(in, a, p);
            print_plan(a, p);
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
