// faasbal_load.h -- internal, host only: what a loaded state must satisfy, and what the device
// receives of it.
//
// The one statement behind fb_load_state and fb_load_shard ("What a load installs",
// carries the table of the kinds' differences).  Like faasbal_plan.h and faasbal_life.h it calls no HIP runtime
// function, uses no HIP type and touches no fb_ctx: faasbal_api.hip fills a LoadIn, asks
// load_check, and uploads load_image's arrays; tests/test_load_host.py runs both without a GPU.
//
// A one-GPU load is the shard case with slot_base = 0, the entry's index for its sequence
// (log_seq null) and log_head = log_len, as lc_batch frames a one-GPU compaction.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "faasbal.h"
#include "faasbal_kernels.h"  // kPart2

namespace fb {

// The context's facts a load depends on, fixed at creation (win_cap: or by fb_set_window).
struct LoadKind {
    bool deque = false, sharded = false;
    bool inflight = false;  // in-flight counts exist (Clears::deferred: fb_read_inflight's contexts)
    bool win_cap = false;   // window buffers exist (never on a sharded or deque context)
    int32_t W_cap = 0, W_global = 0, Wq_cap = 0;
    int64_t log_cap = 0;
};

// The caller's arrays: n_workers slots from global slot slot_base on.
struct LoadIn {
    int32_t slot_base = 0, n_workers = 0;
    const uint8_t *registered = nullptr;
    const int32_t *free_processes = nullptr;
    const double *last_heartbeat = nullptr;
    const uint32_t *epoch = nullptr;  // null: every epoch 0
    const int32_t *queue = nullptr;   // global slots, LRU order
    int64_t queue_len = 0;
    const int32_t *log_slot = nullptr;  // global slots, -1: completed
    const uint32_t *log_seq = nullptr;  // sharded: the entries' global sequences; one GPU: null, the index
    int64_t log_len = 0, log_head = 0;
};

// The liveness rule of a loaded log entry, the only host statement of it (k_log_normalize,
// the compactions and fb_log_reclaim apply the same rule on the device): an entry of sequence
// seq naming a slot is kept only if the slot holds a record and the entry is not older than the
// record's registration.  Any other entry can never be redistributed (build-defined).
// A deque context keeps no liveness: load_image keeps every entry there.
inline bool load_entry_live(bool has_record, uint32_t epoch, uint64_t seq) { return has_record && seq >= epoch; }

// Every condition load_check refuses, with the message it leaves (FB_EINVAL each).
#define FB_LOAD_REFUSALS(X)                                                                       \
    X(null_array, "%s is null with %s = %lld")                                                    \
    X(n_workers, "n_workers %d outside [0, %d]")                                                  \
    X(slot_range, "slot range [%d, %d + %d) outside the %d-slot table")                           \
    X(log_len, "log_len %lld exceeds capacity")                                                   \
    X(log_len_head, "log_len %lld / log_head %lld")                                               \
    X(queue_len, "queue_len %lld")                                                                \
    X(queue_entry, "queue[%lld] = %d is out of range, unregistered or duplicated")                \
    X(queue_entry_shard, "queue[%lld] = %d is out of range or duplicated")                        \
    X(queue_unregistered, "queue[%lld] = %d is not registered")                                   \
    X(log_slot, "log_slot[%lld] = %d out of range")                                               \
    X(log_slot_shard, "log_slot[%lld] = %d is not one of this rank's slots")                      \
    X(log_seq, "log_seq must ascend below log_head (entry %lld)")
enum class LoadRefusal : uint8_t {
#define X(n, f) n,
    FB_LOAD_REFUSALS(X)
#undef X
    count_
};
constexpr struct {
    const char *name, *fmt;
} kLoadRefusals[] = {
#define X(n, f) {#n, f},
    FB_LOAD_REFUSALS(X)
#undef X
};

inline int load_refuse_(std::string &msg, LoadRefusal r, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, r);
    vsnprintf(buf, sizeof buf, kLoadRefusals[(int)r].fmt, ap);
    va_end(ap);
    msg = buf;
    return FB_EINVAL;
}

// FB_OK, or FB_EINVAL with the first failing condition in msg.  It reads the caller's arrays
// only; each difference between the kinds is one commented branch.
inline int load_check(const LoadKind &k, const LoadIn &in, std::string &msg) {
    using R = LoadRefusal;
    const int32_t W = in.n_workers, base = in.slot_base;
    // an array the counts say is read (a negative count fails its own condition below)
    const struct {
        const void *p;
        const char *name, *count;
        int64_t n;
    } arrays[] = {{in.registered, "registered", "n_workers", W},
                  {in.free_processes, "free_processes", "n_workers", W},
                  {in.last_heartbeat, "last_heartbeat", "n_workers", W},
                  {in.queue, "queue", "queue_len", in.queue_len},
                  {in.log_slot, "log_slot", "log_len", in.log_len},
                  {k.sharded ? (const void *)in.log_seq : "", "log_seq", "log_len", in.log_len}};
    for (const auto &a : arrays)
        if (!a.p && a.n > 0) return load_refuse_(msg, R::null_array, a.name, a.count, (long long)a.n);
    // the table and the log: a shard's slots lie in the group's table, and its sequences
    // below a head that fits the device's 32-bit sequence words
    if (!k.sharded) {
        if (W < 0 || W > k.W_cap) return load_refuse_(msg, R::n_workers, W, k.W_cap);
        if (in.log_len < 0 || in.log_len > k.log_cap) return load_refuse_(msg, R::log_len, (long long)in.log_len);
    } else {
        if (W < 0 || W > k.W_cap || base < 0 || (int64_t)base + W > k.W_global)
            return load_refuse_(msg, R::slot_range, base, base, W, k.W_global);
        if (in.log_len < 0 || in.log_len > k.log_cap || in.log_head < in.log_len || in.log_head >= ((int64_t)1 << 31))
            return load_refuse_(msg, R::log_len_head, (long long)in.log_len, (long long)in.log_head);
    }
    // the queue: a deque holds tokens (as many as it has room for), a shard the group's queue
    const int32_t Wq = k.sharded ? k.W_global : W;  // the slots a queue entry may name
    if (in.queue_len < 0 || in.queue_len > (k.deque ? k.Wq_cap : Wq))
        return load_refuse_(msg, R::queue_len, (long long)in.queue_len);
    std::vector<uint8_t> seen((size_t)Wq, 0);
    for (int64_t i = 0; i < in.queue_len; ++i) {
        const int32_t s = in.queue[i];
        if (!k.sharded) {
            // one GPU: registered slots without repeats; a deque's tokens may repeat a slot
            if (s < 0 || s >= W || !in.registered[s] || (seen[s] && !k.deque))
                return load_refuse_(msg, R::queue_entry, (long long)i, s);
        } else {
            // a shard: any global slot, repeats judged over the group's table, registration
            // only for the rank's own slots (the others' records are on their ranks)
            if (s < 0 || s >= Wq || seen[s]) return load_refuse_(msg, R::queue_entry_shard, (long long)i, s);
            if (s >= base && s - base < W && !in.registered[s - base])
                return load_refuse_(msg, R::queue_unregistered, (long long)i, s);
        }
        seen[s] = 1;
    }
    for (int64_t i = 0; i < in.log_len; ++i) {
        const int32_t s = in.log_slot[i];
        if (!k.sharded) {
            // one GPU: completed or any slot of the table
            if (s < -1 || s >= W) return load_refuse_(msg, R::log_slot, (long long)i, s);
        } else {
            // a shard: completed or one of the rank's slots, sequences ascending strictly below the head
            if (s < -1 || (s >= 0 && (s < base || s >= base + W)))
                return load_refuse_(msg, R::log_slot_shard, (long long)i, s);
            if ((int64_t)in.log_seq[i] >= in.log_head || (i && in.log_seq[i] <= in.log_seq[i - 1]))
                return load_refuse_(msg, R::log_seq, (long long)i);
        }
    }
    return FB_OK;
}

// The host arrays the device receives, by local slot (queue position, log index).  An array
// the kind does not have stays empty.  The queue itself and a shard's log_seq go up as the
// caller gave them.
struct LoadPair {
    int32_t free, inq;  // the device's {free_processes, queued} per slot
};
struct LoadImage {
    std::vector<uint8_t> reg;   // 0 / 1
    std::vector<double> hb;     // NaN where there is no record (never "dead")
    std::vector<uint32_t> epoch;
    std::vector<LoadPair> fq;
    std::vector<int32_t> pos;     // win_cap: a queued slot's position (others: never read)
    std::vector<int32_t> qfree;   // one GPU: free_processes and last_heartbeat by queue position
    std::vector<double> qhb;
    std::vector<int32_t> tokcnt;  // deque: tokens per slot, and each token's rank among its slot's
    std::vector<uint32_t> qrank;  // (| kPart2)
    std::vector<int32_t> log;     // dead entries at -1 (load_entry_live)
    std::vector<int32_t> bud;     // inflight: live entries + free processes of a registered slot
    int32_t maxc = 1;             // the first tick's round table: the queued slots' largest free count
};

// Of a LoadIn that load_check accepted.
inline LoadImage load_image(const LoadKind &k, const LoadIn &in) {
    const size_t W = (size_t)in.n_workers, Q = (size_t)in.queue_len, L = (size_t)in.log_len;
    LoadImage m;
    m.reg.resize(W);
    m.hb.resize(W);
    m.epoch.resize(W);
    m.fq.resize(W);
    for (size_t s = 0; s < W; ++s) {
        m.reg[s] = in.registered[s] ? 1 : 0;
        m.hb[s] = m.reg[s] ? in.last_heartbeat[s] : __builtin_nan("");
        m.epoch[s] = in.epoch ? in.epoch[s] : 0u;
        m.fq[s] = LoadPair{in.free_processes[s], 0};
    }
    if (k.win_cap) m.pos.assign(W, 0);
    if (!k.sharded) {
        m.qfree.resize(Q);
        m.qhb.resize(Q);
    }
    if (k.deque) {
        m.tokcnt.assign(W, 0);
        m.qrank.resize(Q);
    }
    for (size_t i = 0; i < Q; ++i) {
        const int64_t ls = (int64_t)in.queue[i] - in.slot_base;
        if (ls < 0 || ls >= (int64_t)W) continue;  // (a shard: another rank's slot)
        m.fq[ls].inq = 1;
        m.maxc = std::max(m.maxc, in.free_processes[ls]);
        if (k.win_cap) m.pos[ls] = (int32_t)i;
        if (!k.sharded) {
            m.qfree[i] = in.free_processes[ls];
            m.qhb[i] = in.last_heartbeat[ls];
        }
        if (k.deque) m.qrank[i] = (uint32_t)(++m.tokcnt[ls]) | kPart2;
    }
    // the log, and with it the budgets (an empty log: the free processes alone).  A shard
    // keeps no budgets: no sharded context has in-flight counts.
    m.log.assign(in.log_slot, in.log_slot + L);
    if (k.inflight) m.bud.assign(W, 0);
    for (size_t i = 0; i < L; ++i) {
        if (m.log[i] < 0) continue;
        const size_t ls = (size_t)(m.log[i] - in.slot_base);
        if (!k.deque && !load_entry_live(m.reg[ls] != 0, m.epoch[ls], in.log_seq ? in.log_seq[i] : (uint64_t)i))
            m.log[i] = -1;
        else if (k.inflight)
            ++m.bud[ls];
    }
    for (size_t s = 0; s < m.bud.size(); ++s)
        m.bud[s] = m.reg[s] ? (int32_t)((uint32_t)m.bud[s] + (uint32_t)in.free_processes[s]) : 0;
    return m;
}

}  // namespace fb
