// life_probe -- the life of a tick (csrc/faasbal_life.h) from the command line, no GPU.
//
// Reads one request per line on stdin, answers each with one line:
//   calls                          the Call names, in enum order
//   waits                          the Wait outcome names
//   gate <kind> <state> <call>     "duties=<flush,undo,sync,discard or -> settle=<0|1> refuse=<message or ->"
//   step <kind> <state> <event[:a[:b]]> ...
//                                  the state after the transitions, in order: stage:accepted | launch:E:window
//                                  | eager | continue | wait:outcome | commit:deferred:orphans_stay
//                                  | commit_ran | undone | settled | replaced | marked | unmarked
// <kind>: hb (deferred clears, lists) | hb_large (in place, lists) | deque | shard.
// <state>: staged,pos,win,eager,enospc,cm_pending,undo_E,stale,marked with pos by name.
// Built by tests/test_life.py; it makes no HIP runtime call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "faasbal_life.h"

using namespace fb;

namespace {

const char *const kPosNames[] = {"none", "phase1", "launched", "waited", "failed", "dropped"};
constexpr int kCalls = (int)Call::count_;
static_assert(sizeof(kCallNames) / sizeof(kCallNames[0]) == (size_t)kCalls, "a Call without a name");

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

void print_state(const Life &l) {
    printf("%d,%s,%d,%d,%d,%d,%d,%d,%d\n", (int)l.staged, kPosNames[(int)l.pos], (int)l.win, (int)l.eager, (int)l.enospc,
           (int)l.cm_pending, l.undo_E, (int)l.stale, (int)l.marked);
}

template <typename T, size_t N>
int find_name(const char *const (&names)[N], const std::string &s, T &out) {
    for (size_t i = 0; i < N; ++i)
        if (s == names[i]) {
            out = (T)i;
            return 1;
        }
    return 0;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, kind, state, what;
        in >> cmd;
        if (cmd == "calls" || cmd == "waits") {
            if (cmd == "calls")
                for (const char *n : kCallNames) printf("%s ", n);
            else
                for (const char *n : kWaitNames) printf("%s ", n);
            printf("\n");
            continue;
        }
        in >> kind >> state;
        CtxCaps k;
        Life l;
        if (!parse_kind(kind, k) || !parse_state(state, l)) {
            printf("error=request\n");
            continue;
        }
        if (cmd == "gate") {
            Call call;
            in >> what;
            if (!find_name(kCallNames, what, call)) {
                printf("error=call\n");
                continue;
            }
            const Gate g = life_gate(l, k, call);
            std::string d;
            const char *const dn[] = {"flush", "undo", "sync", "discard"};
            for (int i = 0; i < 4; ++i)
                if (g.duties & (1u << i)) d += std::string(d.empty() ? "" : ",") + dn[i];
            printf("duties=%s settle=%d refuse=%s\n", d.empty() ? "-" : d.c_str(), (int)life_settle_due(l),
                   g.refuse ? g.refuse : "-");
        } else if (cmd == "step") {
            bool bad = false;
            while (!bad && in >> what) {
                std::string a, b;
                std::istringstream ev(what);
                std::getline(ev, what, ':');
                std::getline(ev, a, ':');
                std::getline(ev, b, ':');
                Wait w;
                if (what == "stage") life_stage(l, a == "1");
                else if (what == "launch") life_launch(l, k, atoi(a.c_str()), b == "1");
                else if (what == "eager") life_eager_enqueued(l);
                else if (what == "continue") life_continue(l);
                else if (what == "wait" && find_name(kWaitNames, a, w)) life_wait_done(l, w);
                else if (what == "commit") life_commit(l, a == "1", b == "1");
                else if (what == "commit_ran") life_commit_ran(l);
                else if (what == "undone") life_undone(l);
                else if (what == "settled") life_settled(l);
                else if (what == "replaced") life_replaced(l);
                else if (what == "marked") life_lcs_marked(l);
                else if (what == "unmarked") life_lcs_unmarked(l);
                else bad = true;
            }
            if (bad) {
                printf("error=event\n");
                continue;
            }
            print_state(l);
        } else {
            printf("error=command\n");
        }
    }
    return 0;
}
