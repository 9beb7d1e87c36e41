// life_lcs_probe -- the gates of a shard group's log compaction (life_gate_log_compact_shard_mark,
// life_gate_log_compact_shard_apply and the "marked" refusal of life_gate, csrc/faasbal_life.h)
// from the command line, no GPU; tests/life_probe.cpp's answer format:
//   mark  <kind> <state>          the mark's gate
//   apply <kind> <state>          the apply's gate
//   gate  <kind> <state> <call>   life_gate of an existing Call
//   stats <kind> <state>          life_gate_pool_stats_shard
//       "duties=<flush,undo,sync,discard or -> settle=<0|1> refuse=<message or ->"
//   step  <kind> <state> <marked | unmarked | replaced | undone> ...   the state afterwards
// <kind>: hb | hb_large | deque | shard.
// <state>: staged,pos,win,eager,enospc,cm_pending,undo_E,stale,marked with pos by name.
// Built by tests/test_log_compact_shard_host.py; it makes no HIP runtime call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "faasbal_life.h"

using namespace fb;

namespace {

const char *const kPosNames[] = {"none", "phase1", "launched", "waited", "failed", "dropped"};

bool parse_kind(const std::string &s, CtxCaps &k) {
    k = CtxCaps{};
    if (s == "hb") {
        k.clears = Clears::deferred;
        k.lists = true;
    } else if (s == "hb_large") {
        k.lists = true;
    } else if (s == "deque") {
        k.deque = true;
    } else if (s == "shard") {
        k.sharded = true;
    } else {
        return false;
    }
    return true;
}

bool parse_state(const std::string &s, Life &l) {
    std::istringstream in(s);
    std::string f[9];
    for (auto &x : f)
        if (!std::getline(in, x, ',')) return false;
    int pos = -1;
    for (int i = 0; i < 6; ++i)
        if (f[1] == kPosNames[i]) pos = i;
    if (pos < 0) return false;
    l.staged = f[0] == "1";
    l.pos = (Pos)pos;
    l.win = f[2] == "1";
    l.eager = f[3] == "1";
    l.enospc = f[4] == "1";
    l.cm_pending = f[5] == "1";
    l.undo_E = atoi(f[6].c_str());
    l.stale = f[7] == "1";
    l.marked = f[8] == "1";
    return true;
}

void print_gate(const Gate &g, const Life &l) {
    std::string d;
    const char *const dn[] = {"flush", "undo", "sync", "discard"};
    for (int i = 0; i < 4; ++i)
        if (g.duties & (1u << i)) d += std::string(d.empty() ? "" : ",") + dn[i];
    printf("duties=%s settle=%d refuse=%s\n", d.empty() ? "-" : d.c_str(), (int)life_settle_due(l), g.refuse ? g.refuse : "-");
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, kind, state, what;
        in >> cmd >> kind >> state;
        CtxCaps k;
        Life l;
        if (!parse_kind(kind, k) || !parse_state(state, l)) {
            printf("error=request\n");
            continue;
        }
        if (cmd == "mark") {
            print_gate(life_gate_log_compact_shard_mark(l, k), l);
        } else if (cmd == "apply") {
            print_gate(life_gate_log_compact_shard_apply(l, k), l);
        } else if (cmd == "stats") {
            print_gate(life_gate_pool_stats_shard(l, k), l);
        } else if (cmd == "gate") {
            in >> what;
            int call = -1;
            for (int i = 0; i < (int)Call::count_; ++i)
                if (what == kCallNames[i]) call = i;
            if (call < 0) {
                printf("error=call\n");
                continue;
            }
            print_gate(life_gate(l, k, (Call)call), l);
        } else if (cmd == "step") {
            bool bad = false;
            while (!bad && in >> what) {
                if (what == "marked") life_lcs_marked(l);
                else if (what == "unmarked") life_lcs_unmarked(l);
                else if (what == "replaced") life_replaced(l);
                else if (what == "undone") life_undone(l);
                else if (what == "commit_ran") life_commit_ran(l);
                else bad = true;
            }
            if (bad) {
                printf("error=event\n");
                continue;
            }
            printf("%d,%s,%d,%d,%d,%d,%d,%d,%d\n", (int)l.staged, kPosNames[(int)l.pos], (int)l.win, (int)l.eager,
                   (int)l.enospc, (int)l.cm_pending, l.undo_E, (int)l.stale, (int)l.marked);
        } else {
            printf("error=command\n");
        }
    }
    return 0;
}
