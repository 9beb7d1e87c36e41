// life_shard_probe -- fb_pool_stats_shard's gate (life_gate_pool_stats_shard,
// csrc/faasbal_life.h) from the command line, no GPU; tests/life_probe.cpp's request and
// answer formats, one request:
//   gate <kind> <state>     "duties=<flush,undo,sync,discard or -> settle=<0|1> refuse=<message or ->"
// <kind>: hb | hb_large | deque | shard.
// <state>: staged,pos,win,eager,enospc,cm_pending,undo_E,stale with pos by name.
// Built by tests/test_pool_stats_shard_host.py; it makes no HIP runtime call.
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
    std::string f[8];
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
    return true;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, kind, state;
        in >> cmd >> kind >> state;
        CtxCaps k;
        Life l;
        if (cmd != "gate" || !parse_kind(kind, k) || !parse_state(state, l)) {
            printf("error=request\n");
            continue;
        }
        const Gate g = life_gate_pool_stats_shard(l, k);
        std::string d;
        const char *const dn[] = {"flush", "undo", "sync", "discard"};
        for (int i = 0; i < 4; ++i)
            if (g.duties & (1u << i)) d += std::string(d.empty() ? "" : ",") + dn[i];
        printf("duties=%s settle=%d refuse=%s\n", d.empty() ? "-" : d.c_str(), (int)life_settle_due(l),
               g.refuse ? g.refuse : "-");
    }
    return 0;
}
