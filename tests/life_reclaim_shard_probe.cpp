// life_reclaim_shard_probe -- fb_log_reclaim_shard's gate (life_gate_log_reclaim_shard,
// csrc/faasbal_life.h) walked from the command line, no GPU.
//
// Takes no input: walks every Pos x staged x kind (hb: one GPU with deferred clears, hb_large:
// one GPU with in-place clears, deque, shard) x cm_pending x undo_E (0, 3) x marked and prints
// one line per point,
//   kind=<k> staged=<0|1> pos=<name> cm=<0|1> undo_E=<n> marked=<0|1>
//   duties=<flush,undo,sync,discard or -> ps_duties=<...> ps_refused=<0|1> same_life=<0|1>
//   refuse=<message or ->
// with fb_pool_stats_shard's gate at the same point beside it (ps_*) and whether the Life the
// gate was given is the Life it left (the gate makes no transition).  The message comes last:
// it holds spaces.
// Built by tests/test_log_reclaim_shard_host.py; it makes no HIP runtime call.
#include <cstdio>
#include <cstring>
#include <string>

#include "faasbal_life.h"

using namespace fb;

namespace {

const char *const kPosNames[] = {"none", "phase1", "launched", "waited", "failed", "dropped"};
const char *const kKinds[] = {"hb", "hb_large", "deque", "shard"};

CtxCaps caps_of(int kind) {
    CtxCaps k{};
    if (kind == 0) {
        k.clears = Clears::deferred;
        k.lists = true;
    } else if (kind == 1) {
        k.lists = true;
    } else if (kind == 2) {
        k.deque = true;
    } else {
        k.sharded = true;
    }
    return k;
}

std::string duties(unsigned d) {
    const char *const dn[] = {"flush", "undo", "sync", "discard"};
    std::string s;
    for (int i = 0; i < 4; ++i)
        if (d & (1u << i)) s += std::string(s.empty() ? "" : ",") + dn[i];
    return s.empty() ? "-" : s;
}

}  // namespace

int main() {
    for (int kind = 0; kind < 4; ++kind)
        for (int staged = 0; staged < 2; ++staged)
            for (int pos = 0; pos < 6; ++pos)
                for (int cm = 0; cm < 2; ++cm)
                    for (int undo_E = 0; undo_E <= 3; undo_E += 3)
                        for (int marked = 0; marked < 2; ++marked) {
                            const CtxCaps k = caps_of(kind);
                            Life l;
                            l.staged = staged != 0;
                            l.pos = (Pos)pos;
                            l.cm_pending = cm != 0;
                            l.undo_E = undo_E;
                            l.marked = marked != 0;
                            const Life before = l;
                            const Gate g = life_gate_log_reclaim_shard(l, k);
                            const Gate ps = life_gate_pool_stats_shard(l, k);
                            const bool same = std::memcmp(&before, &l, sizeof(Life)) == 0;
                            std::printf("kind=%s staged=%d pos=%s cm=%d undo_E=%d marked=%d duties=%s ps_duties=%s ps_refused=%d"
                                        " same_life=%d refuse=%s\n",
                                        kKinds[kind], staged, kPosNames[pos], cm, undo_E, marked, duties(g.duties).c_str(),
                                        duties(ps.duties).c_str(), (int)(ps.refuse != nullptr), (int)same,
                                        g.refuse ? g.refuse : "-");
                        }
    return 0;
}
