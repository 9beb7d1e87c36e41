// faasbal_api.hip -- C ABI of libfaasbal.so (include/faasbal.h).
//
// Host orchestration of one tick on the context's HIP stream.  No CPU
// fallback exists: every decision is computed by the kernels in
// faasbal_kernels.hip; the host only validates arguments, stages event
// arrays (pinned) and reads back a few scalars.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "faasbal.h"
#include "faasbal_kernels.h"
#include "faasbal_life.h"
#include "faasbal_load.h"
#include "faasbal_plan.h"

using namespace fb;

namespace {

// Persistent host workers for the staging pass of large event batches: part i of
// n runs on worker i - 1 (part 0 on the caller).  One pool per context; the ABI
// allows one caller thread per context, so run() is never re-entered.
struct HostPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv, done_cv;
    std::function<void(int)> job;
    long gen = 0;
    int pending = 0;
    bool stop = false;

    explicit HostPool(int n) {
        for (int i = 1; i < n; ++i) th.emplace_back([this, i] { loop(i); });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
    int size() const { return (int)th.size() + 1; }
    void loop(int i) {
        long seen = 0;
        for (;;) {
            std::function<void(int)> f;
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
                f = job;
            }
            f(i);
            std::lock_guard<std::mutex> g(m);
            if (--pending == 0) done_cv.notify_one();
        }
    }
    void run(const std::function<void(int)> &f) {
        {
            std::lock_guard<std::mutex> g(m);
            job = f;
            pending = (int)th.size();
            ++gen;
        }
        cv.notify_all();
        f(0);
        std::unique_lock<std::mutex> l(m);
        done_cv.wait(l, [&] { return pending == 0; });
    }
};


struct TimedLaunch {
    const char *name;
    hipEvent_t a, b;
};

}  // namespace

struct fb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int32_t W_cap = 0, E_cap = 0;
    int64_t log_cap = 0;
    // committed state
    int32_t W = 0;
    int cur = 0;  // index of the committed dense buffers
    int2 *free_[2] = {nullptr, nullptr};  // {free_processes, queued} per slot
    int32_t *queue[2] = {nullptr, nullptr};
    int32_t *qfree[2] = {nullptr, nullptr};  // free_processes by LRU position (one-GPU contexts)
    double *qhb[2] = {nullptr, nullptr};     // last_heartbeat by LRU position
    double *c_hb = nullptr;                  // per tick: heartbeat of a live LRU position
    bool qaos = false;                       // qfree/qhb[cur] describe the committed queue
    uint8_t *reg = nullptr;
    double *hb = nullptr;        // last_heartbeat per slot (NaN: no record)
    uint32_t *epoch = nullptr;   // first log sequence of the slot's current registration
    int32_t *log_slot = nullptr;
    // one-GPU heartbeat contexts: in-flight entries per slot (by commit parity), the
    // post-message counts, the entry each event's result completes (cleared by the
    // commit: the log is read-only during a tick), the launch stamp of the last launch
    // whose result completed an entry, and k_emit2's log-workgroup hand-off granules
    int32_t *bud = nullptr;       // in flight + free processes of a registered slot (committed)
    int32_t *bud_next = nullptr;  // touched slots: the budget after the tick (the commit installs it)
    uint32_t *post_infl = nullptr;
    int32_t *ev_clr = nullptr;
    uint32_t *ctag = nullptr;
    uint32_t lstamp = 0;               // per enqueued launch, reruns included (never 0)
    // f_emit ticks leave their orphans in per-tile segments (orphans[t*2048 + i], i < fcnt[t]);
    // the dense list is gathered into orph_dense when something reads it
    bool l_oseg = false, dense_ok = false;
    int l_nbf = 0;
    int64_t *orph_dense = nullptr;
    // compact assignments (fb_set_compact): slot and min(c, L + 1) per LRU position
    int32_t *rb_slot = nullptr;
    uint8_t *rb_c = nullptr;
    int compact = 0, l_compact = 0;    // the setting, and the one the last launch ran with
    // fb_set_compact_out: pinned buffers the ticks write their compact outputs into directly
    // (device views of them, the caller's pointers, capacities); l_cout: the last launch did
    int32_t *cout_slot = nullptr, *cout_ev = nullptr;
    uint8_t *cout_c = nullptr;
    int64_t *cout_orph = nullptr;
    const void *cout_host[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t cout_cap = 0, cout_ocap = 0, cout_ecap = 0;
    bool l_cout = false;
    HostPool *xpool = nullptr;         // fb_expand_compact's workers (created on first use)
    int32_t *trash = nullptr;  // kTrashRows x kBS words written by inactive lanes (never read)
    int64_t Qn = 0, head = 0;
    // window ticks (one-GPU heartbeat contexts): the committed queue is
    // [qoff, qoff + Qn) of queue[qcur] / qfree[qcur] / qhb[qcur] (qcap entries each; qfree
    // kTomb marks a position whose slot left), pos_of[qcur][s] the position of a queued slot
    int qcur = 0;
    int64_t qoff = 0, qcap = 0, Qtrue = 0;  // Qtrue: the LRU queue's length (tombstones excluded)
    bool win_cap = false;      // the context can run window ticks (buffers allocated)
    int win = -1;              // fb_set_window: -1 auto (large tables), 0 off, 1 on
    int l_nchW = 0;            // the window chunks the last launch scans (a window tick: life.win)
    int64_t l_qoff = 0;
    int32_t *pos_of[2] = {nullptr, nullptr};
    bool pos_ok = false;       // pos_of[qcur] is exact for every queued slot (general ticks do not keep it)
    // k_emit_win: per front / back list entry, the committed position of the queued slot it
    // moved (-1: none), read by the tick's commit
    int32_t *tomb = nullptr;
    int32_t *bad_min = nullptr;  // device word: first invalid message of a device-checked batch (0x7f7f7f7f: none)
    unsigned long long *wlb = nullptr;  // k_emit_win's look-back granules
    uint32_t *wticket = nullptr;
    int64_t *cw = nullptr;  // commit word of the launched tick (device; eager commits read it)
    uint32_t *lpart = nullptr, *wpart = nullptr;
    uint32_t *died_tag = nullptr;  // window ticks: the launch stamp of the last tick a registration died in
    int64_t win_slack = 8192;  // window positions scanned beyond the tasks' estimate (grows on a miss)
    int64_t last_O = 0;
    int last_L = -1;
    int64_t win_ticks = 0, win_fallbacks = 0;
    bool evict_ok = false;     // the waited window tick's dense evicted list is built
    bool win_owned = false;    // window buffers allocated by fb_set_window (one allocation)
    void *win_mem = nullptr;
    uint32_t tick = 1;
    // per-tick sparse post-message records
    uint32_t *touched = nullptr;
    uint32_t *tbits = nullptr;   // one GPU, heartbeat loop: touched bitmap of this launch (tbitsb[tick & 1])
    uint32_t *tbitsb[2] = {nullptr, nullptr};  // by launch parity: a deferred commit reads the last tick's
    // fb_tick_commit of a one-GPU heartbeat context is deferred into the next launch's
    // k_ev_link (extra blocks) or flushed as its own launch by the next call that needs it
    // (life.cm_pending)
    CommitArgs cm{};
    int eager = 0;             // fb_set_eager_commit: window ticks commit on the device right behind the tick
    PostRec *post = nullptr;       // post-message records {hb, free, epoch} of touched slots
    uint8_t *post_rf = nullptr, *st = nullptr;
    unsigned long long *dmask = nullptr;
    // events
    uint8_t *ev_kind = nullptr, *ev_status = nullptr;
    int32_t *ev_val = nullptr, *ev_slot = nullptr;
    double *ev_ts = nullptr;
    int64_t *ev_seq = nullptr;
    uint32_t *keys[2] = {nullptr, nullptr}, *vals[2] = {nullptr, nullptr};
    uint32_t *rs_hist[4] = {nullptr, nullptr, nullptr, nullptr};  // per sort pass: [tile][digit] counts
    int32_t *front_list = nullptr, *back_list = nullptr;
    // one GPU, heartbeat loop: messages grouped per slot by linked lists (k_ev_link)
    unsigned long long *ev_head = nullptr;  // per slot {link stamp, last linked message}
    int32_t *ev_next = nullptr;             // per message
    uint32_t link = 0;                      // stamp of the last k_ev_link launch
    bool l_resort = false;                  // this tick reruns through the sort (a slot had > kLinkMax messages)
    bool l_used_ll = false;                 // the last enqueue grouped by linked lists
    void *h_stage = nullptr;  // two pinned halves of E_cap events each (fb_tick_stage)
    // device event arrays, double-buffered like the pinned halves: fb_tick_stage copies
    // half h on its own stream (overlapping a running tick), the launch waits for it
    uint8_t *evk[2] = {nullptr, nullptr};
    int32_t *evsl[2] = {nullptr, nullptr}, *evv[2] = {nullptr, nullptr};
    double *evt[2] = {nullptr, nullptr};
    int64_t *evq[2] = {nullptr, nullptr};
    hipStream_t cp_s = nullptr;                         // H2D copies of staged events
    hipEvent_t stage_ev[2] = {nullptr, nullptr};        // copies of half h done (on cp_s)
    hipEvent_t tick_ev = nullptr;                       // an eagerly committed tick's last kernel done
    bool tick_ev_set = false;                           // ... signalled by that kernel's launch itself
    hipEvent_t use_ev[2] = {nullptr, nullptr};          // the tick reading device half h done
    bool stage_rec[2] = {false, false}, use_rec[2] = {false, false};
    int stage_half = 1;        // half of the last launch's copies
    int32_t st_E = 0, st_vmax = 0;
    double st_now = 0.0;
    HostPool *pool = nullptr;  // staging workers (FAASBAL_STAGE_THREADS, default 8; 1 = none)
    // a staged pinned batch k_ev_link checks: the caller's kind / slot / ts arrays (read by
    // the host only to name an offending event), and those of the launched tick
    const void *st_chk[3] = {nullptr, nullptr, nullptr};
    const void *l_chk[3] = {nullptr, nullptr, nullptr};
    // device-resident batches (fb_tick_stage of arrays in this GPU's memory): read in place
    bool st_res = false, l_res = false;
    const void *st_dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // scan / plan / emit
    int32_t *c_arr = nullptr, *qbmax = nullptr, *qbm_raw = nullptr;
    unsigned long long *csum = nullptr;
    uint8_t *ofl = nullptr;
    uint32_t *fcnt = nullptr, *wcnt = nullptr;
    int64_t *fpre = nullptr, *wpre = nullptr;
    uint32_t *qcnt = nullptr;
    uint32_t *segcnt = nullptr;  // fused path: per-segment round counts (4 x table)
    uint32_t *grp[2] = {nullptr, nullptr};  // fused path: group rows of round totals, by launch parity
    int gpar = 0;                           // parity of the last fused launch
    int gdirty[2] = {0, 0};                 // words of grp[p] written since it was last zeroed
    int64_t *qpre = nullptr, *A = nullptr;
    int64_t *A_rep = nullptr;     // k_plan2 path: per-group copies of A and the totals
    DevTotals *P_rep = nullptr;
    size_t table_cap = 0;  // entries of qcnt / qpre
    int R_cap = 0;         // entries of A
    int64_t *orphans = nullptr;
    int32_t *evicted = nullptr;
    DevTotals *P = nullptr;
    HostOut *hout = nullptr, *hout_dev = nullptr;  // host-mapped results written by k_emit
    unsigned long long *dbg = nullptr;             // diagnostic stamps
    size_t dbg_n = 0;
    PathKnobs paths;       // fb_set_path (faasbal_plan.h)
    int ncu = 0, max_lds = 0;
    int win_occ = 0;       // k_emit_win workgroups resident per CU (occupancy calculator)
    // deque contexts (fb_create_deque): PushDispatcher.start, task_dispatcher.py:251-322
    int deque = 0;
    int32_t *tokcnt[2] = {nullptr, nullptr}, *xw[2] = {nullptr, nullptr}, *kl[2] = {nullptr, nullptr};
    uint32_t *qrank[2] = {nullptr, nullptr};
    int32_t *front_rank = nullptr, *back_rank = nullptr, *post_tok = nullptr, *post_nf = nullptr;
    int4 *c_tok = nullptr;
    void *arena = nullptr;    // every fixed-size device buffer, carved from one allocation
    size_t arena_bytes = 0;
    bool table_owned = false; // qcnt/qpre grown beyond the arena's reservation
    bool A_owned = false;
    size_t seg_cap = 0;       // entries (per row of 4) of segcnt and the sharded ocnt/opre/osegcnt
    bool seg_owned = false;
    int oA_cap = 0;
    bool oA_owned = false;
    // where the tick is in its life and what the committed state is owed (faasbal_life.h):
    // written by the life_* transitions only, read through enter()
    CtxCaps caps;
    Life life;
    // last launch
    double l_now = 0, l_tte = 0;
    int32_t l_E = 0;
    bool l_purge_only = false;  // fb_purge_launch: orphans reported, not dispatched
    bool next_purge_only = false;
    int64_t l_T = 0, l_head = 0, l_Qn = 0;
    int l_R = 64;
    int32_t maxc_hint = 1;
    int reruns = 0;
    fb_tick_result last{};
    // timing
    bool timing = false;
    std::vector<TimedLaunch> tl;
    std::vector<hipEvent_t> ev_pool;
    // fb_timing_gate: a host-mapped word {open sequence, timed out} the gate kernel polls,
    // the gate's end and the batch's end
    uint32_t *gate_h = nullptr, *gate_d = nullptr;
    uint32_t gate_seq = 0;
    hipEvent_t gate_a = nullptr, gate_b = nullptr;
    int gate_state = 0;  // 1 held, 2 released (span readable)
    std::string err;
    // sharding (fb_create_sharded): this rank owns global slots [slot_base, slot_base + W)
    int shard = 0, rank = 0, world = 1;
    int32_t slot_base = 0, W_global = 0, Wq_cap = 0;  // Wq_cap: LRU queue capacity (global slots)
    int64_t head_local = 0, l_head_local = 0;
    uint32_t *lseq = nullptr;                         // global sequence of each local log entry
    uint32_t *ocnt = nullptr, *osegcnt = nullptr;
    uint32_t *xg_acc = nullptr, *xg_tk = nullptr, *ogrp = nullptr;  // exchanged group rows (phase 1 -> 2)
    uint32_t *xs_tk = nullptr;                        // k_xscan's ticket
    void *lc_mem = nullptr;                           // fb_log_compact's scratch (lc_plan's regions; made on first use)
    size_t lc_cap = 0;
    // fb_log_compact_shard_mark's notes for its apply (life.marked): the exchange bitmap, the
    // log it was made of and the rank's live count (the scratch's local regions hold the rest)
    void *lcs_buf = nullptr;
    int64_t lcs_head = 0, lcs_head_local = 0, lcs_live = 0;
    void *ps_mem = nullptr;                           // fb_pool_stats' scratch (ps_plan's regions; made on first use)
    size_t ps_cap = 0;
    int64_t *ps_out = nullptr, *ps_out_dev = nullptr; // ... and its folded record, host-mapped (kPsCols words)
    int full_assign = 0;                              // fb_set_full_assign: phase 2 writes the whole task -> slot array
    bool l_full = false;                              // ... and the last launch did
    int32_t *assign_all = nullptr;                    // (its own allocation, grown as ticks need)
    int64_t assign_cap = 0;
    int64_t *opre = nullptr, *oA = nullptr;
    uint8_t *xbuf = nullptr;                          // bound exchange buffer (device)
    int64_t xcap = 0;
    // the exchange records' copy the next phase 1 writes (two, by exchange parity: a phase 2
    // with block rows zeroes the other and flips it -- a collective step, so every rank
    // agrees), and whether that copy is known zero (then an idle tick's phase 1 needs no memset)
    int xpar = 0;
    bool xz_ok = false;
    int shard_R = 0;                                  // > 0: round rows a relaunch asked for (FB_ERERUN)
    // contexts without deferred clears (sharded, deque, one GPU past kLdsBitmapSlots): results
    // clear their log entries in place at launch; the entries a launch cleared (per message,
    // tagged per fb_tick_launch: fb_tick_wait's reruns write under the same tag) are named
    // again -- log_undo -- by the next launch, or by a reader of the committed state once the
    // launch's wait has failed, unless the tick was committed in between
    int64_t *undo_idx = nullptr;
    unsigned long long *undo_key = nullptr;
    uint32_t undo_tag = 0;                            // the last host launch's tag (never 0)
    hipStream_t own_s = nullptr;                      // the context's own stream (fb_set_stream may borrow another)
};

namespace {

int fail(fb_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((ctx), FB_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                        __FILE__, __LINE__);                                                      \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

template <typename T>
int dalloc(fb_ctx *c, T **p, size_t n) {
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess) return fail(c, FB_ENOMEM, "hipMalloc(%zu B) failed: %s", n * sizeof(T), hipGetErrorString(e));
    return FB_OK;
}

// One device allocation for every fixed-size buffer: random per-slot gathers then
// stay within large, contiguous mappings (fewer GPU TLB misses than many small
// hipMalloc regions).
struct ArenaPlan {
    std::vector<std::pair<void **, size_t>> req;
    template <typename T>
    void add(T **p, size_t n) {
        req.push_back({(void **)p, std::max<size_t>(n, 1) * sizeof(T)});
    }
};

// Buffer i starts (i mod 16) x 4.25 KB after the end of buffer i - 1, so arrays read by
// position side by side (c_arr, c_hb, queue, qfree, qhb: power-of-two sizes at 1 M
// workers) do not start at the same offset modulo the memory channel interleave
size_t arena_skew(int i) { return (size_t)(i % 16) * 4352; }

// The host's wait for the context stream: polled (a tick is tens of microseconds; a
// blocking wait's wake-up was measured at ~20 us per tick, tools/stream_timeline.sh)
static hipError_t stream_wait(fb_ctx *c) {
    for (;;) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e != hipErrorNotReady) return e;
    }
}

int arena_commit(fb_ctx *c, ArenaPlan &ap) {
    size_t total = 0;
    int i = 0;
    for (auto &r : ap.req) total += ((r.second + 255) & ~(size_t)255) + arena_skew(i++);
    total = (total + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    hipError_t e = hipMalloc(&c->arena, total);
    if (e != hipSuccess) return fail(c, FB_ENOMEM, "hipMalloc(arena %zu B) failed: %s", total, hipGetErrorString(e));
    c->arena_bytes = total;
    // Every byte written once: some kernels load words no tick has written yet (a
    // round table's rows past the fill level, tail padding) and discard them; zeroing
    // makes those loads deterministic.
    e = hipMemset(c->arena, 0, total);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(c, FB_EHIP, "hipMemset(arena) failed: %s", hipGetErrorString(e));
    char *p = (char *)c->arena;
    i = 0;
    for (auto &r : ap.req) {
        p += arena_skew(i++);
        *r.first = p;
        p += (r.second + 255) & ~(size_t)255;
    }
    return FB_OK;
}

hipEvent_t pool_event(fb_ctx *c) {
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

// Per-kernel device time: the events ride in the dispatch packets of the timed
// launches (start of the first, end of the last), so they bracket kernel
// execution only -- the same interval rocprofv3's kernel trace reports.
struct Timer {
    fb_ctx *c;
    const char *name;
    hipEvent_t a = nullptr, b = nullptr;
    Timer(fb_ctx *c_, const char *n) : c(c_), name(n) {
        if (c->timing) {
            a = pool_event(c);
            b = pool_event(c);
        }
    }
    Stream st() const { return Stream(c->stream, a, b); }
    Stream first() const { return Stream(c->stream, a, nullptr); }
    Stream mid() const { return Stream(c->stream); }
    Stream last() const { return Stream(c->stream, nullptr, b); }
    ~Timer() {
        if (c->timing) c->tl.push_back({name, a, b});
    }
};

static_assert(kMaxR == FB_MAX_ROUNDS && kShardMaxR == FB_MAX_ROUNDS, "the round range include/faasbal.h states");
static_assert(kEvLeave == FB_EV_LEAVE && kEvDrain == FB_EV_DRAIN && kDrainBias == FB_DRAIN_BIAS &&
                  kDrainBelow == FB_DRAIN_BELOW && is_draining(FB_DRAIN_BELOW - 1) == FB_IS_DRAINING(FB_DRAIN_BELOW - 1) &&
                  is_draining(FB_DRAIN_BELOW) == FB_IS_DRAINING(FB_DRAIN_BELOW),
              "the kinds and the drain mark include/faasbal.h states");

int ensure_table(fb_ctx *c, int R, int nbq) {
    size_t need = (size_t)R * (size_t)nbq;
    if (need > c->table_cap) {
        size_t cap = std::max(need, c->table_cap * 2);
        if (cap > ((size_t)1 << 31))
            return fail(c, FB_ERANGE, "round table of %zu entries (R=%d rows x %d blocks) exceeds the limit", need, R, nbq);
        HIPCHK(c, stream_wait(c));
        if (c->table_owned) {
            hipFree(c->qcnt);
            hipFree(c->qpre);
        }
        c->qcnt = nullptr;
        c->qpre = nullptr;
        int rc;
        if ((rc = dalloc(c, &c->qcnt, cap)) || (rc = dalloc(c, &c->qpre, cap))) return rc;
        HIPCHK(c, hipMemset(c->qcnt, 0, cap * sizeof(uint32_t)));
        HIPCHK(c, hipMemset(c->qpre, 0, cap * sizeof(int64_t)));
        c->table_cap = cap;
        c->table_owned = true;
    }
    if (R > c->R_cap) {
        HIPCHK(c, stream_wait(c));
        if (c->A_owned) hipFree(c->A);
        c->A = nullptr;
        int rc;
        if ((rc = dalloc(c, &c->A, (size_t)R))) return rc;
        c->R_cap = R;
        c->A_owned = true;
    }
    // per-segment round counts (4 rows per block) and, sharded, this rank's tables: the
    // arena holds them for 128 rows; wider sharded tables get their own, grown the same way
    if (c->shard && need > c->seg_cap) {
        const size_t cap = std::max(need, c->seg_cap * 2);
        HIPCHK(c, stream_wait(c));
        if (c->seg_owned) {
            hipFree(c->segcnt);
            hipFree(c->osegcnt);
            hipFree(c->ocnt);
            hipFree(c->opre);
        }
        c->segcnt = c->osegcnt = c->ocnt = nullptr;
        c->opre = nullptr;
        int rc;
        if ((rc = dalloc(c, &c->segcnt, 4 * cap))) return rc;
        if (c->shard && ((rc = dalloc(c, &c->osegcnt, 4 * cap)) || (rc = dalloc(c, &c->ocnt, cap)) ||
                         (rc = dalloc(c, &c->opre, cap))))
            return rc;
        c->seg_cap = cap;
        c->seg_owned = true;
    }
    if (c->shard && R > c->oA_cap) {
        HIPCHK(c, stream_wait(c));
        if (c->oA_owned) hipFree(c->oA);
        c->oA = nullptr;
        int rc;
        if ((rc = dalloc(c, &c->oA, (size_t)R))) return rc;
        c->oA_cap = R;
        c->oA_owned = true;
    }
    return FB_OK;
}

// The committed window [qoff, qoff + Qn) without its tombstones: slots, free counts and
// (h non-null) heartbeats on the host.  The stream must be idle.
int win_read(fb_ctx *c, std::vector<int32_t> &q, std::vector<int32_t> &f, std::vector<double> *h, int64_t &n) {
    const size_t Qn = (size_t)c->Qn;
    std::vector<int32_t> q0(Qn), f0(Qn);
    std::vector<double> h0(h ? Qn : 0);
    if (Qn) {
        HIPCHK(c, hipMemcpy(q0.data(), c->queue[c->qcur] + c->qoff, Qn * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(f0.data(), c->qfree[c->qcur] + c->qoff, Qn * 4, hipMemcpyDeviceToHost));
        if (h) HIPCHK(c, hipMemcpy(h0.data(), c->qhb[c->qcur] + c->qoff, Qn * 8, hipMemcpyDeviceToHost));
    }
    q.clear();
    f.clear();
    if (h) h->clear();
    for (size_t i = 0; i < Qn; ++i)
        if (f0[i] != kTomb) {
            q.push_back(q0[i]);
            f.push_back(f0[i]);
            if (h) h->push_back(h0[i]);
        }
    n = (int64_t)q.size();
    if (n != c->Qtrue) return fail(c, FB_EHIP, "window holds %lld live entries, the queue %lld", (long long)n, (long long)c->Qtrue);
    return FB_OK;
}

// Rewrite the committed window densely from position 0 of the other buffers (the state a
// general tick leaves): for readers of the device view.
int win_normalize(fb_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    std::vector<int32_t> q, f;
    std::vector<double> h;
    int64_t n = 0;
    if (int rc = win_read(c, q, f, &h, n)) return rc;
    const int o = c->qcur ^ 1;
    if (n) {
        HIPCHK(c, hipMemcpy(c->queue[o], q.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->qfree[o], f.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->qhb[o], h.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    }
    if (c->W) {
        std::vector<int32_t> pos((size_t)c->W, 0);
        for (int64_t i = 0; i < n; ++i) pos[q[i]] = (int32_t)i;
        HIPCHK(c, hipMemcpy(c->pos_of[o], pos.data(), (size_t)c->W * 4, hipMemcpyHostToDevice));
    }
    c->qcur = o;
    c->qoff = 0;
    c->Qn = n;
    c->pos_ok = true;
    return FB_OK;
}

// Window buffers for a context created without them (fb_set_window): one allocation,
// the committed queue copied over.
int win_alloc(fb_ctx *c) {
    if (c->win_cap) return FB_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    const size_t W = (size_t)c->W_cap, E = (size_t)c->E_cap, Wq = (size_t)c->Wq_cap;
    const size_t qcap = 2 * Wq + 2 * E + 4096;
    auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t bytes = 2 * (r256(qcap * 4) * 2 + r256(qcap * 8) + r256(W * 4)) + r256(2 * E * 4) +
                         r256(kWinMaxCh * 8) +
                         r256(256) + r256(1024 * 4) + r256(256) + r256(64 * 32 * 4);
    void *m = nullptr;
    hipError_t e = hipMalloc(&m, bytes);
    if (e != hipSuccess) return fail(c, FB_ENOMEM, "hipMalloc(window buffers %zu B) failed: %s", bytes, hipGetErrorString(e));
    HIPCHK(c, hipMemset(m, 0, bytes));
    char *p = (char *)m;
    auto take = [&](size_t b) { char *r = p; p += r256(b); return r; };
    int32_t *nq[2], *nf[2];
    double *nh[2];
    for (int i = 0; i < 2; ++i) {
        nq[i] = (int32_t *)take(qcap * 4);
        nf[i] = (int32_t *)take(qcap * 4);
        nh[i] = (double *)take(qcap * 8);
        c->pos_of[i] = (int32_t *)take(W * 4);
    }
    c->tomb = (int32_t *)take(2 * E * 4);
    c->wlb = (unsigned long long *)take(kWinMaxCh * 8);
    c->wticket = (uint32_t *)take(256);
    c->lpart = (uint32_t *)take(1024 * 4);
    c->died_tag = (uint32_t *)take(256);
    c->wpart = (uint32_t *)take(64 * 32 * 4);
    const int k = c->qcur;
    if (c->Qn) {
        HIPCHK(c, hipMemcpy(nq[0], c->queue[k], (size_t)c->Qn * 4, hipMemcpyDeviceToDevice));
        HIPCHK(c, hipMemcpy(nf[0], c->qfree[k], (size_t)c->Qn * 4, hipMemcpyDeviceToDevice));
        HIPCHK(c, hipMemcpy(nh[0], c->qhb[k], (size_t)c->Qn * 8, hipMemcpyDeviceToDevice));
    }
    for (int i = 0; i < 2; ++i) {
        c->queue[i] = nq[i];
        c->qfree[i] = nf[i];
        c->qhb[i] = nh[i];
    }
    c->qcur = 0;
    c->qoff = 0;
    c->qcap = (int64_t)qcap;
    c->win_mem = m;
    c->win_owned = true;
    c->win_cap = true;
    c->pos_ok = true;
    if (c->W && c->Qn) {
        std::vector<int32_t> q((size_t)c->Qn), pos((size_t)c->W, 0);
        HIPCHK(c, hipMemcpy(q.data(), c->queue[0], (size_t)c->Qn * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < c->Qn; ++i) pos[q[i]] = (int32_t)i;
        HIPCHK(c, hipMemcpy(c->pos_of[0], pos.data(), (size_t)c->W * 4, hipMemcpyHostToDevice));
    }
    return FB_OK;
}

// The deferred commit of the last tick as its own launch (when no k_ev_link takes it).
int flush_commit(fb_ctx *c) {
    if (!c->life.cm_pending) return FB_OK;
    life_commit_ran(c->life);
    HIPCHK(c, hipSetDevice(c->device));
    Timer t(c, "commit");
    launch_commit(c->cm, t.st());
    HIPCHK(c, hipGetLastError());
    return FB_OK;
}

// Lazy clears (round 6): on one-GPU heartbeat contexts a commit leaves the log entries it
// redistributed; an entry naming slot s is live only if s holds a record and the entry is
// not older than s's registration (epoch), which every kernel that reads the log tests once
// such entries may exist (live_chk).  (configs[3]: the fold's ~380 K scattered clears cost
// 2.9 µs of the committed tick; configs[2]'s 24.6 K, ~0.5 µs.)
bool lazy_ctx(const fb_ctx *c) { return c->paths.lazy_on && c->caps.lists; }

// Before a state read hands out the log: the deferred clears, all at once (k_log_normalize),
// after the last commit.
int log_settle(fb_ctx *c) {
    if (!life_settle_due(c->life)) return FB_OK;
    if (int rc_ = flush_commit(c)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->head > 0) {  // (an empty log launches nothing: no events to time)
        Timer t(c, "settle");
        launch_log_normalize(c->log_slot, c->head, c->reg, c->epoch, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    life_settled(c->life);
    return FB_OK;
}

// The in-place clears of a launch that was never committed, taken back: the log entries its
// results completed are in flight again.  (life_gate says when: before the next launch, and
// before anything reads the committed log once the launch's wait has failed; between a
// successful wait and the commit the clears stay: the commit relies on them.)
int log_undo(fb_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    {
        Timer t(c, "log_undo");
        launch_log_undo(c->log_slot, c->undo_idx, c->undo_key, c->undo_tag, c->life.undo_E, t.st());
    }
    HIPCHK(c, hipGetLastError());
    life_undone(c->life);
    return FB_OK;
}

// The top of every entry point: life_gate's refusal, or the duties it names, in order.
int enter(fb_ctx *c, Call call) {
    const Gate g = life_gate(c->life, c->caps, call);
    if (g.duties & kFlush)
        if (int rc_ = flush_commit(c)) return rc_;
    if (g.refuse) return fail(c, FB_ESTATE, "%s", g.refuse);
    if (g.duties & kUndo)
        if (int rc_ = log_undo(c)) return rc_;
    if (g.duties & kUndoSync) HIPCHK(c, stream_wait(c));
    return FB_OK;
}

// Whether the tick about to launch (c->l_*) runs as a window tick: plan_window's rules on
// this context's state; c->l_nchW, the window chunks it scans.
bool win_plan(fb_ctx *c) {
    WindowIn w{};
    w.win_cap = c->win_cap;
    w.mode = c->win;
    w.lists = c->caps.lists;
    w.ev_ll = c->paths.ev_ll != 0;
    w.compact = c->compact != 0;
    w.purge_only = c->l_purge_only;
    w.deque = c->deque != 0;
    w.shard = c->shard != 0;
    w.E = c->l_E;
    w.W = c->W;
    w.max_lds = c->max_lds;
    w.last_L = c->last_L;
    w.T = c->l_T;
    w.last_O = c->last_O;
    w.win_slack = c->win_slack;
    w.Qn = c->Qn;
    w.qoff = c->qoff;
    w.qcap = c->qcap;
    return plan_window(w, c->l_nchW);
}

// What plan_tick reads of the tick described by c->l_*.
PlanIn plan_input(const fb_ctx *c) {
    PlanIn in;
    in.shard = c->shard;
    in.phase = life_phase(c->life);
    in.world = c->world;
    in.deque = c->deque;
    in.heartbeat = c->caps.clears == Clears::deferred;
    in.lists = c->caps.lists;
    in.qaos = c->qaos;
    in.compact = c->compact;
    in.cout = c->cout_slot != nullptr;
    in.cout_cap = c->cout_cap;
    in.cout_ecap = c->cout_ecap;
    in.cout_ocap = c->cout_ocap;
    in.W = c->W;
    in.W_global = c->W_global;
    in.E = c->l_E;
    in.R = c->l_R;
    in.head = c->l_head;
    in.head_local = c->l_head_local;
    in.Qn = c->l_Qn;
    in.T = c->l_T;
    in.ncu = c->ncu;
    in.max_lds = c->max_lds;
    in.win_occ = c->win_occ;
    in.l_win = c->life.win;
    in.l_nchW = c->l_nchW;
    in.pos_ok = c->pos_ok;
    in.l_resort = c->l_resort;
    in.l_purge_only = c->l_purge_only;
    in.stale_any = c->life.stale;
    in.cm_pending = c->life.cm_pending;
    in.cm_E = c->cm.E;
    in.cm_win = c->cm.win;
    in.cm_n_clr = c->cm.n_clr;
    in.cm_shard = c->cm.shard;
    in.cm_oseg = c->cm.oseg != nullptr;
    in.cm_oseg_tiles = c->cm.oseg_tiles;
    in.cm_n_orph = c->cm.n_orph;
    in.knobs = c->paths;
    return in;
}

// The message lists and status bytes of the tick: the context's own, or (sharded) the
// regions of the bound exchange buffer.
struct EvLists {
    int32_t *front, *back;
    uint8_t *evs;
};

// The arguments of the message kernels, linked lists or sort (c->link and c->lstamp are
// this launch's).
EvArgs fill_ev_args(const fb_ctx *c, const TickPlan &p, const TickArgs &a, const EvLists &l) {
    const int cur = c->cur, nxt = 1 - cur;
    const bool defer = c->caps.clears == Clears::deferred;  // one-GPU heartbeat context
    EvArgs ea{};
    ea.E = a.E;
    ea.W = a.W;
    ea.tick = c->tick;
    ea.tte = c->l_tte;
    ea.head_in = a.head_in;
    ea.ev_kind = c->ev_kind;
    ea.ev_val = c->ev_val;
    ea.ev_ts = c->ev_ts;
    ea.ev_seq = c->ev_seq;
    ea.ev_status = l.evs;
    ea.reg = c->reg;
    ea.free_in = c->free_[cur];
    ea.hb = c->hb;
    ea.epoch = c->epoch;
    ea.live_chk = a.live_chk;
    ea.log_slot = c->log_slot;
    ea.post = c->post;
    ea.post_rf = c->post_rf;
    ea.touched = c->touched;
    ea.tbits = c->tbits;
    ea.front_list = l.front;
    ea.back_list = l.back;
    // (the budget arrays exist together: all null without them)
    ea.defer_clr = defer ? 1 : 0;
    ea.ev_clr = c->ev_clr;
    ea.ctag = c->ctag;
    ea.lstamp = defer ? c->lstamp : 0;
    ea.bud = c->bud;
    ea.post_infl = c->post_infl;
    ea.undo_idx = c->undo_idx;
    ea.undo_key = c->undo_key;
    ea.undo_tag = c->undo_tag;
    if (p.grouping == Grouping::sort) {
        ea.deque = c->deque;
        ea.tokcnt_in = c->tokcnt[cur];
        ea.front_rank = c->front_rank;
        ea.back_rank = c->back_rank;
        ea.post_tok = c->post_tok;
        ea.post_nf = c->post_nf;
        ea.shard = c->shard;
        ea.slot_base = c->slot_base;
        ea.head_local = c->l_head_local;
        ea.lseq = c->lseq;
        // the last pass's output
        ea.skeys = c->keys[(p.passes - 1) & 1];
        ea.svals = c->vals[(p.passes - 1) & 1];
        return ea;
    }
    ea.tbits_words = c->caps.lists ? (int)cdiv(a.W, 32) : 0;
    ea.ev_slot = c->ev_slot;
    ea.ev_head = c->ev_head;
    ea.ev_next = c->ev_next;
    ea.check_ev = c->l_chk[0] != nullptr;
#ifdef FAASBAL_STAMPS
    ea.dbg = c->dbg;
#endif
    ea.bad_min = c->bad_min;
    ea.link = c->link;
    ea.hout = c->hout_dev;
    ea.lstamp = c->lstamp;
    ea.bud_next = c->bud_next;
    ea.orph_grp = a.f_emit ? 1 : 0;
    if (p.commit == CommitPlan::in_ev_link) {  // the previous tick's commit rides in this launch
        ea.cm = c->cm;
        ea.cm_blocks = commit_layout(c->cm).grid();
    }
    // the slot purge (k_scan's W role) runs in k_ev_apply_ll's launch
    ea.nbw = a.nbw;
    ea.wtiles = p.ev_wtiles;
    ea.now = c->l_now;
    ea.st = c->st;
    ea.free_out = c->free_[nxt];
    ea.dmask = (!a.slots_in_scan || a.f_sep || a.f_emit || a.win) ? c->dmask : nullptr;
    if (a.win) {  // k_emit_win's look-back granules and ticket start from zero
        ea.wpart = c->wpart;
        ea.died_tag = c->died_tag;
        ea.wlb = c->wlb;
        ea.wlb_n = emit_win_layout(a).grid();
        ea.wticket = c->wticket;
        ea.cw = c->cw;
    }
    ea.wcnt = c->wcnt;
    ea.grp = a.grp_on ? a.grp : nullptr;
    ea.ngrp = a.ngrp;
    ea.gstride = a.gstride;
    ea.R = a.R;
    return ea;
}

// The buffers and scalars of the tick kernels around the flags plan_tick chose (group rows
// and, stamps builds, c->dbg are the driver's: they move state).
void fill_tick_args(const fb_ctx *c, const TickPlan &p, const EvLists &l, TickArgs &a) {
    const int cur = c->cur, nxt = 1 - cur;
    a.epoch = c->epoch;
    a.fault_qlen = -1;
    a.q_cap = c->Wq_cap;
    a.tokcnt_in = c->tokcnt[cur];
    a.xw_in = c->xw[cur];
    a.kl_in = c->kl[cur];
    a.qrank_in = c->qrank[cur];
    a.front_rank = c->front_rank;
    a.back_rank = c->back_rank;
    a.post_tok = c->post_tok;
    a.post_nf = c->post_nf;
    a.c_tok = c->c_tok;
    a.tokcnt_out = c->tokcnt[nxt];
    a.xw_out = c->xw[nxt];
    a.kl_out = c->kl[nxt];
    a.qrank_out = c->qrank[nxt];
    if (c->caps.clears == Clears::deferred) {  // one-GPU heartbeat context
        a.bud = c->bud;
        a.bud_next = c->bud_next;
        a.post_infl = c->post_infl;
        a.ctag = c->ctag;
        a.lstamp = c->lstamp;
    }
    a.tick = c->tick;
    a.now = c->l_now;
    a.tte = c->l_tte;
    a.log_cap = c->log_cap;
    a.reg = c->reg;
    a.hb = c->hb;
    a.free_in = c->free_[cur];
    // the committed queue: the window [qoff, qoff + Qn) of the current queue buffers
    const int qc = c->qcur, qn = c->qcur ^ 1;
    a.queue_in = c->queue[qc] + c->qoff;
    a.qfree_in = c->qfree[qc] ? c->qfree[qc] + c->qoff : nullptr;
    a.qhb_in = c->qhb[qc] ? c->qhb[qc] + c->qoff : nullptr;
    a.touched = c->touched;
    a.tbits = c->tbits;
    a.post = c->post;
    a.post_rf = c->post_rf;
    a.front_list = l.front;
    a.back_list = l.back;
    a.st = c->st;
    a.dmask = c->dmask;
    a.c_arr = c->c_arr;
    a.ofl = c->ofl;
    a.wcnt = c->wcnt;
    a.fcnt = c->fcnt;
    a.qcnt = c->qcnt;
    a.segcnt = c->segcnt;
    a.qbmax = c->qbmax;
    a.qbm_raw = c->qbm_raw;
    a.csum = c->csum;
    a.fpre = c->fpre;
    a.wpre = c->wpre;
    a.qpre = c->qpre;
    a.A = c->A;
    a.P = c->P;
    a.A_rep = c->A_rep;
    a.P_rep = c->P_rep;
    a.trash = c->trash;
    if (p.l_compact) {
        a.rb_slot = c->rb_slot;
        a.rb_c = c->rb_c;
    }
    if (p.l_cout) {
        a.rb_slot = c->cout_slot;
        a.rb_c = c->cout_c;
    }
    a.arena = (char *)c->arena;
    a.arena32 = c->arena_bytes < ((size_t)1 << 32) ? 1 : 0;
    a.log_slot = c->log_slot;
    a.free_out = c->free_[nxt];
    a.queue_out = c->queue[qn];
    a.qfree_out = c->qfree[qn];
    a.qhb_out = c->qhb[qn];
    a.c_hb = c->c_hb;
    a.orphans = c->orphans;
    // (registered pinned outputs: the evicted slots straight into the caller's array)
    a.evicted = p.l_cout ? c->cout_ev : c->evicted;
    a.hout = c->hout_dev;
    if (c->shard) {
        a.slot_base = c->slot_base;
        a.rank = c->rank;
        a.world = c->world;
        a.head_local = c->l_head_local;
        a.lseq = c->lseq;
        a.lseq_out = c->lseq;
        a.xc8 = c->xbuf + p.xl.c8;
        // this tick's copy of the records; phase 2 with block rows zeroes the other
        const size_t xrw = (size_t)c->world * kXRecWords;
        a.xrec = (unsigned long long *)(c->xbuf + p.xl.rec) + (size_t)c->xpar * xrw;
        a.xrows = p.xrb ? c->xbuf + p.xl.rows : nullptr;
        if (c->l_full && life_phase(c->life) == 2) a.assign_all = c->assign_all;
        if (a.xplan) {
            // k_xscan's outputs in the plan tables (unused on this path): per-block prefixes in
            // qpre's words, the chunk prefixes and totals in opre's
            a.xpre = reinterpret_cast<uint32_t *>(c->qpre);
            a.xct = reinterpret_cast<uint32_t *>(c->opre);
            a.xA = a.xct + (size_t)xscan_layout(a).grid() * 2 * a.R;
            a.xtk = c->xs_tk;
        }
        a.xgrows = p.xgb ? c->xbuf + p.xl.grows : nullptr;
        a.xg_acc = c->xg_acc;
        a.xg_tk = c->xg_tk;
        a.ogrp = c->ogrp;
        if ((p.xrb || a.xplan) && life_phase(c->life) == 2) {
            a.xz = (unsigned long long *)(c->xbuf + p.xl.rec) + (size_t)(c->xpar ^ 1) * xrw;
            a.xz_words = (int)xrw;
        }
        a.ocnt = c->ocnt;
        a.osegcnt = c->osegcnt;
        a.opre = c->opre;
        a.oA = c->oA;
    }
    if (a.win) {
        a.wq_off = c->qoff;
        a.wq_tail = c->qoff + a.Qn;
        a.wq_cap = c->qcap;
        a.q_cap = c->Wq_cap;  // the next window (tombstones included) must fit the general path
        a.wq_buf = c->queue[qc];
        a.wqf_buf = c->qfree[qc];
        a.wqh_buf = c->qhb[qc];
        a.wlb = c->wlb;
        a.wticket = c->wticket;
        a.cw = c->cw;
        a.cw_tag = c->link;
        a.wpart = c->wpart;
        a.pos_in = c->pos_of[qc];
        a.tomb = c->tomb;
        a.lstamp = c->lstamp;
        // (a test's injected length goes to the device, which checks what an eager commit reads)
        a.fault_qlen = c->paths.fault_qlen;
        a.lpart = c->lpart;
        a.died_tag = c->died_tag;
    }
}

// A stage that launches the same way in every tick kind: the window's position rebuild, the
// last tick's commit as its own launch, the message grouping (ps: the sort pass, counted
// here), k_slots, k_scan and k_logscan.
int launch_common_stage(fb_ctx *c, const TickPlan &p, const TickArgs &a, const EvArgs &ea, Stage s, int &ps) {
    switch (s) {
    case Stage::pos_rebuild:
        // the first window tick after general ticks: every queued slot's position, once
        launch_pos_rebuild(c->pos_of[c->qcur], c->queue[c->qcur], c->qfree[c->qcur], c->qoff, c->l_Qn,
                           Stream(c->stream));
        c->pos_ok = true;
        return FB_OK;
    case Stage::commit:
        return flush_commit(c);
    case Stage::ev_link: {
        Timer t(c, "ev_link");
        launch_ev_link(ea, t.st());
        return FB_OK;
    }
    case Stage::ev_apply: {
        Timer t(c, "ev_apply");
        if (p.grouping == Grouping::lists) launch_ev_apply_ll(ea, t.st());
        else launch_ev_apply(ea, t.st());
        return FB_OK;
    }
    case Stage::rs_sort: {
        Timer t(c, "rs_sort");
        RsPass r{};
        r.kin = ps == 0 ? (const uint32_t *)c->ev_slot : c->keys[(ps - 1) & 1];
        r.vin = ps == 0 ? nullptr : c->vals[(ps - 1) & 1];
        r.kout = c->keys[ps & 1];
        r.vout = c->vals[ps & 1];
        r.n = ea.E;
        r.shift = p.db * ps;
        r.db = p.db;
        r.nblk = p.rs_blocks;
        r.hist = c->rs_hist[0];
        r.identity_vals = ps == 0 ? 1 : 0;
        if (ps == 0 && !c->shard) {
            // pass 0 also clears the one-GPU front / back lists (sharded: zeroed with the
            // exchange buffer) and the touched bitmap
            r.zero0 = ea.front_list;
            r.zero1 = ea.back_list;
            r.zbits = c->tbits;
            r.zwords = c->caps.lists ? (int)cdiv(ea.W, 32) : 0;
        }
        launch_rs_pass(r, t.first(), t.last());
        ++ps;
        return FB_OK;
    }
    case Stage::slots: {
        Timer t(c, "slots");
        launch_slots(a, t.st());
        return FB_OK;
    }
    case Stage::scan: {
        Timer t(c, "scan");
        launch_scan(a, t.st());
        return FB_OK;
    }
    case Stage::logscan: {
        Timer t(c, "logscan");
        launch_logscan(a, p.ls_grid, t.st());
        return FB_OK;
    }
    default:
        return fail(c, FB_EHIP, "launch plan: stage %s has no place in this tick", stage_name(s));
    }
}

int launch_window_tick(fb_ctx *c, const TickPlan &p, const TickArgs &a, const EvArgs &ea) {
    int ps = 0;
    for (int i = 0; i < p.n_stages; ++i) {
        if (p.stages[i] == Stage::emit) {
            Timer t(c, "emit");
            // an eager commit follows: the launch's own completion signal is the event the
            // host waits for (a separate event record between the two kernels cost ~6 us)
            c->tick_ev_set = !c->timing && c->eager && c->reruns == 0;
            launch_emit_win(a, c->tick_ev_set ? Stream(c->stream, nullptr, c->tick_ev) : t.st());
        } else if (int rc = launch_common_stage(c, p, a, ea, p.stages[i], ps)) {
            return rc;
        }
    }
    HIPCHK(c, hipGetLastError());
    return FB_OK;
}

// Phase 1: own slots' purge, orphan flags and free counts into the exchange buffer.
int launch_shard_phase1(fb_ctx *c, const TickPlan &p, const TickArgs &a, const EvArgs &ea) {
    int ps = 0;
    for (int i = 0; i < p.n_stages; ++i)
        if (int rc = launch_common_stage(c, p, a, ea, p.stages[i], ps)) return rc;
    HIPCHK(c, hipGetLastError());
    return FB_OK;
}

int launch_shard_phase2(fb_ctx *c, const TickPlan &p, const TickArgs &a, const EvArgs &ea) {
    // with exchanged block rows k_emit_shard also zeroes the other records copy, which the
    // next tick's phase 1 writes; else the next phase 1 clears the records
    const bool rows = a.xrows || a.xplan;
    if (!rows) c->xz_ok = false;
    int ps = 0;
    for (int i = 0; i < p.n_stages; ++i) {
        const Stage s = p.stages[i];
        if (s == Stage::scan2) {
            Timer t(c, "scan2");
            launch_scan(a, t.st());
        } else if (s == Stage::plan) {
            Timer t(c, "plan");
            if (a.xplan) launch_xscan(a, t.st());
            else launch_plan(a, t.st());
        } else if (s == Stage::emit) {
            Timer t(c, "emit");
            launch_emit_shard(a, t.st());
        } else if (int rc = launch_common_stage(c, p, a, ea, s, ps)) {
            return rc;
        }
    }
    HIPCHK(c, hipGetLastError());
    if (rows) {
        c->xpar ^= 1;
        c->xz_ok = true;
    }
    return FB_OK;
}

int launch_local_tick(fb_ctx *c, const TickPlan &p, const TickArgs &a, const EvArgs &ea) {
    int ps = 0;
    for (int i = 0; i < p.n_stages; ++i) {
        const Stage s = p.stages[i];
        if (s == Stage::plan) {
            Timer t(c, "plan");
            launch_plan(a, t.st());
        } else if (s == Stage::emit) {
            Timer t(c, "emit");
            if (a.segw) launch_emit2(a, t.st());
            else launch_emit(a, t.st());
        } else if (s == Stage::orph_gather) {
            launch_orph_gather(c->cout_orph, c->orphans, c->fcnt, c->l_nbf, Stream(c->stream));
        } else if (int rc = launch_common_stage(c, p, a, ea, s, ps)) {
            return rc;
        }
    }
    HIPCHK(c, hipGetLastError());
    return FB_OK;
}

// Enqueue every kernel of the tick described by c->l_* (events already on device): the
// plan (plan_tick: every rule that picks the launches), the state the launch moves, the
// kernels' arguments, then the tick kind's launch sequence.
int enqueue_tick(fb_ctx *c) {
    int rc;
    TickArgs a{};
    TickPlan p;
    plan_tick(plan_input(c), a, p);
    if ((rc = ensure_table(c, a.R, a.nbq))) return rc;
    if (p.err == PlanError::group_rows)
        return fail(c, FB_ERANGE, "group rows (%d x %d words) exceed the reservation", a.ngrp, a.gstride);
    if (p.err == PlanError::sort_passes) return fail(c, FB_ERANGE, "event sort of %d passes", p.passes);
    if (p.err == PlanError::shard_rows)
        return fail(c, FB_ERANGE, "sharded tick: round table of %d rows (limit %d)", a.R, kShardMaxR);

    EvLists l{c->front_list, c->back_list, c->ev_status};
    if (c->shard) {
        if (!c->xbuf || c->xcap < (int64_t)p.xl.total)
            return fail(c, FB_ESTATE, "sharded tick needs an exchange buffer of %zu bytes (bound: %lld)", p.xl.total,
                        (long long)c->xcap);
        l.front = (int32_t *)(c->xbuf + p.xl.front);
        l.back = (int32_t *)(c->xbuf + p.xl.back);
        l.evs = c->xbuf + p.xl.evs;
        // (an idle tick whose records the last phase 2 zeroed has nothing else to clear)
        if (life_phase(c->life) != 2 && !(a.E == 0 && c->xz_ok)) HIPCHK(c, hipMemsetAsync(c->xbuf, 0, p.xl.c8, c->stream));
    }
    if (a.grp_on) {
        c->gpar ^= 1;
        a.grp = c->grp[c->gpar];  // zero: its last user's k_emit2 cleared it
        a.grp_zero = c->grp[c->gpar ^ 1];
        a.zero_words = c->gdirty[c->gpar ^ 1];
        c->gdirty[c->gpar ^ 1] = 0;
        c->gdirty[c->gpar] = a.ngrp * a.gstride;
    }
    if (++c->lstamp == 0) c->lstamp = 1;  // every launch (reruns included) stamps its own
    c->l_oseg = p.l_oseg;
    c->l_nbf = p.nbf;
    c->evict_ok = false;
    c->dense_ok = false;
    c->l_used_ll = p.grouping == Grouping::lists;
    if (c->l_used_ll && ++c->link == 0) c->link = 1;  // a fresh stamp per k_ev_link launch, reruns included
    c->l_compact = p.l_compact;
    c->l_cout = p.l_cout;
    if (c->shard) {
        c->l_full = c->full_assign != 0;
        if (c->l_full && life_phase(c->life) == 2) {
            // the whole tick's assignments: at most its pending tasks plus every in-flight entry
            const int64_t need = std::max<int64_t>(1, c->l_T + c->l_head);
            if (need > c->assign_cap) {
                const int64_t cap = std::max(need, 2 * c->assign_cap);
                HIPCHK(c, stream_wait(c));
                hipFree(c->assign_all);
                c->assign_all = nullptr;
                c->assign_cap = 0;
                if ((rc = dalloc(c, &c->assign_all, (size_t)cap))) return rc;
                c->assign_cap = cap;
            }
        }
    }
#ifdef FAASBAL_STAMPS
    {
        // diagnostic stamp rows (stamps builds only); grown geometrically -- hipFree
        // synchronises the device
        // (k_emit_win stamps rows from 8192 on, one per chunk)
        const size_t need = std::max((size_t)4 * (a.nbw + c->l_nbf + a.nbq) * 16 + 16, (size_t)(8192 + kWinMaxCh) * 16);
        if (need > c->dbg_n) {
            HIPCHK(c, stream_wait(c));
            hipFree(c->dbg);
            c->dbg = nullptr;
            const size_t cap = std::max(need, 2 * c->dbg_n);
            if ((rc = dalloc(c, &c->dbg, cap))) return rc;
            c->dbg_n = cap;
        }
        a.dbg = c->dbg;
    }
#endif
    fill_tick_args(c, p, l, a);
    const EvArgs ea = p.grouping == Grouping::none ? EvArgs{} : fill_ev_args(c, p, a, l);
    // the last tick's commit, when this tick's first kernel runs it
    if (p.commit == CommitPlan::in_ev_link || p.commit == CommitPlan::in_scan) life_commit_ran(c->life);
    switch (p.kind) {
    case TickKind::window: return launch_window_tick(c, p, a, ea);
    case TickKind::shard_phase1: return launch_shard_phase1(c, p, a, ea);
    case TickKind::shard_phase2: return launch_shard_phase2(c, p, a, ea);
    default: return launch_local_tick(c, p, a, ea);
    }
}

}  // namespace

extern "C" {

const char *fb_last_error(const fb_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

}  // extern "C"

namespace {
int create_ctx(fb_ctx **out, int32_t max_workers, int64_t max_log, int32_t max_events, int device, int shard,
               int rank, int world, int32_t n_workers_global, int64_t max_tokens = 0) {
    if (!out) return FB_EINVAL;
    *out = nullptr;
    if (max_workers < 1 || max_log < 1 || max_events < 0 || max_log >= ((int64_t)1 << 31) ||
        max_workers >= (1 << 30) || max_events >= (1 << 28))
        return FB_EINVAL;
    if (shard && (world < 1 || rank < 0 || rank >= world || n_workers_global < max_workers ||
                  n_workers_global >= (1 << 30)))
        return FB_EINVAL;
    fb_ctx *c = new fb_ctx();
    c->device = device;
    c->shard = shard;
    c->rank = shard ? rank : 0;
    c->world = shard ? world : 1;
    c->W_global = shard ? n_workers_global : max_workers;
    c->deque = max_tokens > 0 ? 1 : 0;
    c->Wq_cap = c->deque ? (int32_t)max_tokens : c->W_global;
    c->W_cap = max_workers;
    c->E_cap = std::max(max_events, 1);
    c->log_cap = max_log;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own_s, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return FB_EHIP;
    }
    c->stream = c->own_s;
    const size_t W = (size_t)max_workers, E = (size_t)c->E_cap, F = (size_t)max_log;
    const size_t Wq = (size_t)c->Wq_cap;  // queue entries are global slots
    const size_t Qlog = Wq + 2 * E;
    // the context kind (faasbal_life.h): message lists on one-GPU heartbeat contexts; in-flight
    // counts and deferred clears only where the fused tick can use them (the died bitmap of the
    // log workgroups fits in LDS), larger tables keep k_logscan and in-place clears
    c->caps.sharded = shard != 0;
    c->caps.deque = c->deque != 0;
    c->caps.lists = !shard && !c->deque;
    c->caps.clears = c->caps.lists && W <= (size_t)kLdsBitmapSlots ? Clears::deferred : Clears::in_place;
    const bool deferred = c->caps.clears == Clears::deferred;
    // window-capable contexts (one GPU, heartbeat loop): each queue buffer holds a window
    // that slides right by the served prefix and grows at its tail (<= 2 E + tasks per tick)
    // (large tables; fb_set_window allocates them later for others)
    c->win_cap = c->caps.lists && !deferred;
    c->qcap = c->win_cap ? (int64_t)(2 * Wq + 2 * E + 4096) : (int64_t)Wq;
    const size_t Wqb = (size_t)c->qcap;
    ArenaPlan ap;
    for (int i = 0; i < 2; ++i) {
        ap.add(&c->free_[i], W);
        ap.add(&c->queue[i], Wqb);
        if (!shard) {
            ap.add(&c->qfree[i], Wqb);
            ap.add(&c->qhb[i], Wqb);
        }
        if (c->win_cap) ap.add(&c->pos_of[i], W);
    }
    if (c->win_cap) {
        ap.add(&c->tomb, 2 * E);
        ap.add(&c->wlb, (size_t)kWinMaxCh);
        ap.add(&c->wticket, (size_t)64);
        ap.add(&c->lpart, (size_t)1024);
        ap.add(&c->died_tag, (size_t)64);
        ap.add(&c->wpart, (size_t)64 * 32);
    }
    ap.add(&c->reg, W);
    ap.add(&c->hb, W);
    ap.add(&c->epoch, W);
    ap.add(&c->touched, W);
    if (c->caps.lists) {
        ap.add(&c->tbitsb[0], (W + 31) / 32);
        ap.add(&c->tbitsb[1], (W + 31) / 32);
    }
    ap.add(&c->post_rf, W);
    ap.add(&c->st, W);
    ap.add(&c->trash, (size_t)kTrashRows * kBS);
    ap.add(&c->dmask, (W + 63) / 64);
    ap.add(&c->cw, (size_t)8);
    ap.add(&c->bad_min, (size_t)64);
    ap.add(&c->post, W);
    ap.add(&c->ev_status, E);
    for (int i = 0; i < 2; ++i) {
        ap.add(&c->evk[i], E);
        ap.add(&c->evv[i], E);
        ap.add(&c->evsl[i], E);
        ap.add(&c->evt[i], E);
        ap.add(&c->evq[i], E);
    }
    for (int i = 0; i < 2; ++i) {
        ap.add(&c->keys[i], E);
        ap.add(&c->vals[i], E);
    }
    // 8-bit passes: 256 x blocks; wide passes (a tick of <= kRsWideMaxBlocks blocks): 2048 x blocks
    ap.add(&c->rs_hist[0], std::max((size_t)256 * (cdiv(E, kRsTile) + 1),
                                        (size_t)2048 * (size_t)(std::min<int64_t>((int64_t)cdiv(E, kRsTile), kRsWideMaxBlocks) + 1)));
    ap.add(&c->front_list, E);
    ap.add(&c->back_list, E);
    if (c->caps.lists) {
        ap.add(&c->ev_head, W);
        ap.add(&c->ev_next, E);
    }
    ap.add(&c->c_arr, Qlog);
    if (!shard) {
        ap.add(&c->rb_slot, Qlog);
        ap.add(&c->rb_c, Qlog);
    }
    if (!shard) {
        ap.add(&c->c_hb, Qlog);
    }
    ap.add(&c->qbmax, (size_t)cdiv(Qlog, kBS));
    ap.add(&c->qbm_raw, (size_t)cdiv(Qlog, kBS));
    ap.add(&c->csum, (size_t)cdiv(Qlog, kBS));
    ap.add(&c->ofl, (size_t)cdiv(F, kFTile) * kBS);
    ap.add(&c->fcnt, (size_t)cdiv(F, kFTile));
    ap.add(&c->fpre, (size_t)cdiv(F, kFTile));
    ap.add(&c->wcnt, (size_t)cdiv(W, kBS));
    ap.add(&c->wpre, (size_t)cdiv(W, kBS));
    ap.add(&c->evicted, W);
    ap.add(&c->P, 1);
    const size_t tab = (size_t)128 * (size_t)cdiv(Qlog, kBS);
    ap.add(&c->qcnt, tab);
    ap.add(&c->segcnt, 4 * tab);
    ap.add(&c->grp[0], kGrpWords);
    ap.add(&c->grp[1], kGrpWords);
    ap.add(&c->qpre, tab);
    ap.add(&c->A, 128);
    ap.add(&c->A_rep, (size_t)64 * kRFused);
    ap.add(&c->P_rep, 64);
    ap.add(&c->log_slot, F);
    ap.add(&c->orphans, (size_t)cdiv(F, kFTile) * kFTile);  // whole tiles: f_emit's per-tile segments
    if (c->deque) {
        for (int i = 0; i < 2; ++i) {
            ap.add(&c->tokcnt[i], W);
            ap.add(&c->xw[i], W);
            ap.add(&c->kl[i], W);
            ap.add(&c->qrank[i], Wq);
        }
        ap.add(&c->front_rank, E);
        ap.add(&c->back_rank, E);
        ap.add(&c->post_tok, W);
        ap.add(&c->post_nf, W);
        ap.add(&c->c_tok, Qlog);
    }
    if (deferred) {
        ap.add(&c->bud, W);
        ap.add(&c->bud_next, W);
        ap.add(&c->post_infl, W);
        ap.add(&c->ev_clr, E);
        ap.add(&c->ctag, F);
        ap.add(&c->orph_dense, F);
    }
    // window ticks leave their orphans in per-tile segments too (gathered when read)
    if (c->win_cap) ap.add(&c->orph_dense, F);
    if (shard) {
        ap.add(&c->lseq, F);
        ap.add(&c->ocnt, tab);
        ap.add(&c->osegcnt, 4 * tab);
        ap.add(&c->opre, tab);
        ap.add(&c->oA, 128);
        // exchanged group rows: per group the running sums and ticket (zero between ticks:
        // the arena is zeroed, each group's last block resets them) and this rank's row
        const size_t ng = (size_t)kXRowsMaxBlocks / kXGroupBlocks;
        ap.add(&c->xg_acc, ng * kXgAccStride);
        ap.add(&c->xg_tk, ng);
        ap.add(&c->xs_tk, (size_t)64);  // k_xscan's ticket (zero: the arena is zeroed, the last workgroup resets it)
        ap.add(&c->ogrp, ng * kXGroupR);
    }
    // every context that clears in place (no bud / ctag above) notes its clears (k_log_undo)
    if (!deferred) {
        ap.add(&c->undo_idx, E);
        ap.add(&c->undo_key, E);
    }
    int rc = arena_commit(c, ap);
    if (!rc && hipMemset(c->bad_min, 0x7f, 4) != hipSuccess) rc = fail(c, FB_EHIP, "hipMemset(bad_min) failed");
    if (!rc) {
        c->table_cap = tab;
        c->R_cap = 128;
        c->seg_cap = tab;
        c->oA_cap = 128;
    }
    if (!rc && hipHostMalloc((void **)&c->hout, sizeof(HostOut), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        rc = FB_ENOMEM;
    if (!rc && hipHostGetDevicePointer((void **)&c->hout_dev, c->hout, 0) != hipSuccess) rc = FB_EHIP;
    if (!rc) memset(c->hout, 0, sizeof(HostOut));
    if (!rc && (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
                hipDeviceGetAttribute(&c->max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess))
        rc = FB_EHIP;
    if (!rc) c->win_occ = emit_win_resident_per_cu();
    if (!rc && hipHostMalloc(&c->h_stage, (size_t)E * 32 * 2, hipHostMallocDefault) != hipSuccess) rc = FB_ENOMEM;
    for (int h = 0; h < 2 && !rc; ++h)
        if (hipEventCreateWithFlags(&c->stage_ev[h], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->use_ev[h], hipEventDisableTiming) != hipSuccess)
            rc = FB_EHIP;
    if (!rc && hipStreamCreateWithFlags(&c->cp_s, hipStreamNonBlocking) != hipSuccess) rc = FB_EHIP;
    if (!rc && hipEventCreateWithFlags(&c->tick_ev, hipEventDisableTiming) != hipSuccess) rc = FB_EHIP;
    if (!rc) {
        int nt = getenv("FAASBAL_STAGE_THREADS") ? atoi(getenv("FAASBAL_STAGE_THREADS")) : 8;
        nt = std::max(1, std::min(nt, 16));
        if (nt > 1 && E >= kStagePar) c->pool = new HostPool(nt);
    }
    if (!rc) {
        c->ev_kind = c->evk[0];
        c->ev_slot = c->evsl[0];
        c->ev_val = c->evv[0];
        c->ev_ts = c->evt[0];
        c->ev_seq = c->evq[0];
    }
    if (!rc && hipMemset(c->touched, 0, W * 4) != hipSuccess) rc = FB_EHIP;
    for (int p = 0; p < 2 && !rc; ++p)
        if (c->caps.lists && hipMemset(c->tbitsb[p], 0, (W + 31) / 32 * 4) != hipSuccess) rc = FB_EHIP;
    if (!rc) c->tbits = c->tbitsb[c->tick & 1];
    for (int p = 0; p < 2 && !rc; ++p)
        if (hipMemset(c->grp[p], 0, kGrpWords * 4) != hipSuccess) rc = FB_EHIP;
    if (!rc && hipMemset(c->reg, 0, W) != hipSuccess) rc = FB_EHIP;
    if (!rc && c->caps.lists && hipMemset(c->ev_head, 0, W * 8) != hipSuccess) rc = FB_EHIP;  // stamp 0: never a launch's
    if (rc) {
        fb_destroy(c);
        return rc;
    }
    *out = c;
    return FB_OK;
}

static_assert(sizeof(LoadPair) == sizeof(int2), "free_[] holds {free_processes, queued} pairs");

// fb_load_state / fb_load_shard behind their gates: faasbal_load.h's check (all of it before the
// first wait or copy: a rejected load changes nothing), its image onto the device, and every
// host field that describes the committed state.
int load_install(fb_ctx *c, const LoadIn &in) {
    const LoadKind k{c->deque != 0, c->shard != 0, c->caps.clears == Clears::deferred, c->win_cap,
                     c->W_cap, c->W_global, c->Wq_cap, c->log_cap};
    std::string msg;
    if (int rc = load_check(k, in, msg)) return fail(c, rc, "%s", msg.c_str());
    const LoadImage m = load_image(k, in);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
#define FB_UP(dst, src, n)                                                                        \
    if (n) HIPCHK(c, hipMemcpy((dst), (src), (size_t)(n) * sizeof *(dst), hipMemcpyHostToDevice))
    const size_t W = (size_t)in.n_workers;
    FB_UP(c->pos_of[0], m.pos.data(), m.pos.size());
    FB_UP(c->reg, m.reg.data(), W);
    FB_UP(c->free_[0], (const int2 *)m.fq.data(), W);
    FB_UP(c->hb, m.hb.data(), W);
    FB_UP(c->epoch, m.epoch.data(), W);
    FB_UP(c->queue[0], in.queue, in.queue_len);
    FB_UP(c->qfree[0], m.qfree.data(), m.qfree.size());
    FB_UP(c->qhb[0], m.qhb.data(), m.qhb.size());
    FB_UP(c->tokcnt[0], m.tokcnt.data(), m.tokcnt.size());
    if (c->deque && W) {  // no token served yet: qrank is each token's place among its slot's
        HIPCHK(c, hipMemset(c->xw[0], 0, W * 4));
        HIPCHK(c, hipMemset(c->kl[0], 0, W * 4));
    }
    FB_UP(c->qrank[0], m.qrank.data(), m.qrank.size());
    FB_UP(c->log_slot, m.log.data(), m.log.size());
    FB_UP(c->lseq, in.log_seq, c->shard ? in.log_len : 0);
    FB_UP(c->bud, m.bud.data(), m.bud.size());
#undef FB_UP
    // the committed buffers are the ones just written, the queue a dense one from position 0
    c->cur = 0;
    c->qcur = 0;
    c->qoff = 0;
    c->slot_base = in.slot_base;
    c->W = in.n_workers;
    c->Qn = in.queue_len;
    c->head = in.log_head;
    c->head_local = c->shard ? in.log_len : 0;  // (one GPU: the log is [0, head), this stays 0)
    c->tick += 1;
    // what only some kinds read; a load writes each all the same, with the value that kind keeps:
    c->pos_ok = c->win_cap;      // window contexts: pos_of[0] above is exact (others: always false)
    c->qaos = c->caps.lists;     // one-GPU heartbeat: qfree / qhb above describe the queue (others: always false)
    c->Qtrue = in.queue_len;     // read by window and one-GPU code only (a shard's commits write it, nothing reads it)
    c->last_L = -1;              // plan_window's inputs: it answers "no" for a shard or a deque
    c->last_O = 0;               // before it reads them
    c->shard_R = 0;              // sharded: a wide table kept for the replaced state's fill level, or
                                 // asked by its relaunch (one GPU: always 0, read behind c->shard only)
    // the first tick's round table.  Sharded: from what every rank knows alike (the exchange
    // layout depends on it): its events' values and fb_set_round_hint (the loaded state's global
    // max free count, which the caller knows from the global state); the rank's own max (m.maxc)
    // would differ between ranks.  A fill level beyond it relaunches wider.
    c->maxc_hint = c->shard ? 1 : m.maxc;
    life_replaced(c->life);
    return FB_OK;
}
}  // namespace

extern "C" {

int fb_create(fb_ctx **out, int32_t max_workers, int64_t max_log, int32_t max_events, int device) {
    return create_ctx(out, max_workers, max_log, max_events, device, 0, 0, 1, max_workers);
}

int fb_create_deque(fb_ctx **out, int32_t max_workers, int64_t max_tokens, int64_t max_log, int32_t max_events,
                    int device) {
    if (max_tokens < 1 || max_tokens >= (1 << 30)) return FB_EINVAL;
    return create_ctx(out, max_workers, max_log, max_events, device, 0, 0, 1, max_workers, max_tokens);
}

int fb_create_sharded(fb_ctx **out, int32_t max_workers_local, int32_t n_workers_global, int64_t max_log_local,
                      int32_t max_events, int device, int32_t rank, int32_t world) {
    return create_ctx(out, max_workers_local, max_log_local, max_events, device, 1, rank, world, n_workers_global);
}

int fb_destroy(fb_ctx *c) {
    if (!c) return FB_OK;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->table_owned) {
        hipFree(c->qcnt);
        hipFree(c->qpre);
    }
    if (c->A_owned) hipFree(c->A);
    if (c->seg_owned) {
        hipFree(c->segcnt);
        hipFree(c->osegcnt);
        hipFree(c->ocnt);
        hipFree(c->opre);
    }
    if (c->oA_owned) hipFree(c->oA);
    if (c->assign_all) hipFree(c->assign_all);
    if (c->win_owned) hipFree(c->win_mem);
    if (c->lc_mem) hipFree(c->lc_mem);
    if (c->ps_mem) hipFree(c->ps_mem);
    if (c->ps_out) hipHostFree(c->ps_out);
    if (c->dbg) hipFree(c->dbg);
    if (c->arena) hipFree(c->arena);
    if (c->hout) hipHostFree(c->hout);
    if (c->h_stage) hipHostFree(c->h_stage);
    delete c->pool;
    delete c->xpool;
    if (c->cp_s) hipStreamSynchronize(c->cp_s);
    for (int h = 0; h < 2; ++h) {
        if (c->stage_ev[h]) hipEventDestroy(c->stage_ev[h]);
        if (c->use_ev[h]) hipEventDestroy(c->use_ev[h]);
    }
    if (c->tick_ev) hipEventDestroy(c->tick_ev);
    if (c->gate_h) hipHostFree(c->gate_h);
    if (c->gate_a) hipEventDestroy(c->gate_a);
    if (c->gate_b) hipEventDestroy(c->gate_b);
    if (c->cp_s) hipStreamDestroy(c->cp_s);
    for (auto &t : c->tl) {
        hipEventDestroy(t.a);
        hipEventDestroy(t.b);
    }
    for (auto e : c->ev_pool) hipEventDestroy(e);
    if (c->own_s) hipStreamDestroy(c->own_s);
    delete c;
    return FB_OK;
}

int fb_load_state(fb_ctx *c, int32_t n_workers, const uint8_t *registered, const int32_t *free_processes,
                  const double *last_heartbeat, const uint32_t *epoch, const int32_t *queue, int64_t queue_len,
                  const int32_t *log_slot, int64_t log_len) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::load_state)) return rc_;
    // the shard case with slot_base = 0, the entry's index for its sequence and log_head = log_len
    return load_install(c, LoadIn{0, n_workers, registered, free_processes, last_heartbeat, epoch, queue, queue_len,
                                  log_slot, nullptr, log_len, log_len});
}

int fb_read_state(fb_ctx *c, uint8_t *registered, int32_t *free_processes, double *last_heartbeat, uint32_t *epoch,
                  int32_t *queue, int64_t *queue_len, int32_t *log_slot, int64_t *log_len) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::read_state)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    const size_t W = (size_t)c->W;
    if (W) {
        if (registered) HIPCHK(c, hipMemcpy(registered, c->reg, W, hipMemcpyDeviceToHost));
        if (free_processes) {
            std::vector<int2> fq(W);
            HIPCHK(c, hipMemcpy(fq.data(), c->free_[c->cur], W * sizeof(int2), hipMemcpyDeviceToHost));
            for (size_t s = 0; s < W; ++s) free_processes[s] = fq[s].x;
        }
        if (last_heartbeat) HIPCHK(c, hipMemcpy(last_heartbeat, c->hb, W * sizeof(double), hipMemcpyDeviceToHost));
        if (epoch) HIPCHK(c, hipMemcpy(epoch, c->epoch, W * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (c->win_cap) {
        // the window without its tombstones
        std::vector<int32_t> q, f;
        int64_t n = 0;
        if (int rc = win_read(c, q, f, nullptr, n)) return rc;
        if (queue && n) memcpy(queue, q.data(), (size_t)n * 4);
        if (queue_len) *queue_len = n;
    } else {
        if (queue && c->Qn) HIPCHK(c, hipMemcpy(queue, c->queue[c->qcur], (size_t)c->Qn * 4, hipMemcpyDeviceToHost));
        if (queue_len) *queue_len = c->Qn;
    }
    const int64_t nlog = c->shard ? c->head_local : c->head;
    if (log_slot && nlog) {
        if (int rc_ = log_settle(c)) return rc_;
        HIPCHK(c, hipMemcpy(log_slot, c->log_slot, (size_t)nlog * 4, hipMemcpyDeviceToHost));
    }
    if (log_len) *log_len = nlog;
    return FB_OK;
}

int fb_load_shard(fb_ctx *c, int32_t slot_base, int32_t n_workers, const uint8_t *registered,
                  const int32_t *free_processes, const double *last_heartbeat, const uint32_t *epoch,
                  const int32_t *queue, int64_t queue_len, const int32_t *log_slot, const uint32_t *log_seq,
                  int64_t log_len, int64_t log_head) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::load_shard)) return rc_;
    return load_install(c, LoadIn{slot_base, n_workers, registered, free_processes, last_heartbeat, epoch, queue,
                                  queue_len, log_slot, log_seq, log_len, log_head});
}

int fb_read_inflight(fb_ctx *c, uint32_t *inflight) {
    if (!c || !inflight) return FB_EINVAL;
    if (int rc_ = enter(c, Call::read_inflight)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    const size_t W = (size_t)c->W;
    if (!W) return FB_OK;
    std::vector<int32_t> bud(W);
    std::vector<int2> fq(W);
    std::vector<uint8_t> reg(W);
    HIPCHK(c, hipMemcpy(bud.data(), c->bud, W * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(fq.data(), c->free_[c->cur], W * sizeof(int2), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(reg.data(), c->reg, W, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < W; ++s) inflight[s] = reg[s] ? (uint32_t)bud[s] - (uint32_t)fq[s].x : 0u;
    return FB_OK;
}

// A maintenance call's device scratch (`what`, for the messages), made on first use: sized for
// this state (`need` bytes), doubling, never beyond a full one (`full`); `keep` bytes of the
// old one survive a growth.  The stream is idle before the old one goes.
static int scratch_grow(fb_ctx *c, const char *what, void *&mem, size_t &cap, size_t need, size_t full, size_t keep) {
    if (need <= cap) return FB_OK;
    const size_t want = std::max(need, std::min(2 * cap, full));
    HIPCHK(c, stream_wait(c));
    void *m = nullptr;
    const hipError_t e = hipMalloc(&m, want);
    if (e != hipSuccess) return fail(c, FB_ENOMEM, "hipMalloc(%s %zu B) failed: %s", what, want, hipGetErrorString(e));
    if (mem) {
        if (keep) {
            const hipError_t ce = hipMemcpy(m, mem, keep, hipMemcpyDeviceToDevice);
            if (ce != hipSuccess) {
                hipFree(m);
                return fail(c, FB_EHIP, "hipMemcpy(%s) failed: %s", what, hipGetErrorString(ce));
            }
        }
        hipFree(mem);
    }
    mem = m;
    cap = want;
    return FB_OK;
}
// The compactions' scratch, one allocation for fb_log_compact, a shard group's
// two halves (`keep`: a mark's local table) and the reclaims.
static int lc_scratch(fb_ctx *c, size_t need, size_t full, size_t keep) {
    return scratch_grow(c, "compaction scratch", c->lc_mem, c->lc_cap, need, full, keep);
}
static LcTable lc_table(char *base, const LcTableAt &t, int nt) {
    return LcTable{(unsigned long long *)(base + t.bits), (uint32_t *)(base + t.wrel), (uint32_t *)(base + t.tcnt),
                   (uint32_t *)(base + t.tpre), nt};
}
// A count the device wrote (after stream_wait), checked before it is used or handed out: FB_EHIP
// when it is beyond `bound`, which `of` names.
static int read_count(fb_ctx *c, const uint32_t *dev, const char *noun, int64_t bound, const char *of, uint32_t *n) {
    HIPCHK(c, hipMemcpy(n, dev, 4, hipMemcpyDeviceToHost));
    if ((int64_t)*n > bound)
        return fail(c, FB_EHIP, "device-reported %s %u outside [0, %lld] (%s)", noun, *n, (long long)bound, of);
    return FB_OK;
}

// The kernels' arguments over the scratch as p lays it out.  A shard's global bitmap is the
// caller's exchange buffer; on one GPU the log's index is its sequence, and the tables are one.
static LcArgs lc_args(fb_ctx *c, const LcPlan &p, bool want_kept) {
    char *const base = (char *)c->lc_mem;
    LcArgs a{};
    a.log = c->log_slot;
    a.seq = c->shard ? c->lseq : nullptr;
    a.head = c->head;
    a.n = c->shard ? c->head_local : c->head;
    a.W = c->W;
    a.slot_base = c->shard ? c->slot_base : 0;
    // (no sharded context commits lazily today: the test is kept for the day one does)
    a.live_chk = c->life.stale ? 1 : 0;
    a.want_kept = want_kept ? 1 : 0;
    a.reg = c->reg;
    a.epoch = c->epoch;
    a.loc = lc_table(base, p.loc, p.ntl);
    a.glob = lc_table(base, p.glob, p.ntg);
    if (c->shard) a.glob.bits = (unsigned long long *)c->lcs_buf;
    a.dst = (int32_t *)(base + p.dst);
    a.dseq = c->shard ? (uint32_t *)(base + p.dseq) : nullptr;
    a.kept = want_kept ? (int64_t *)(base + p.kept) : nullptr;
    return a;
}

// The log renumbered densely on the device: count first
// (k_lc_flag, k_lc_scan write only the scratch), synchronise, check, and only then move.
int fb_log_compact(fb_ctx *c, int64_t expect_kept, int64_t *kept_seq, int64_t cap, int64_t *n_kept) {
    if (!c) return FB_EINVAL;
    if (kept_seq && cap < 0) return fail(c, FB_EINVAL, "cap %lld < 0", (long long)cap);
    // (a discarded tick's results completed nothing: its clears are taken back before the count)
    if (int rc_ = enter(c, Call::log_compact)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    const LcPlan p = lc_plan(c->head, c->W, kept_seq != nullptr);
    if (int rc_ = lc_scratch(c, p.bytes, lc_plan(c->log_cap, c->W_cap, true).bytes, 0)) return rc_;
    const LcArgs a = lc_args(c, p, kept_seq != nullptr);
    if (p.flag_grid > 0) {
        Timer t(c, "lc_flag");
        launch_lc_flag(a, false, t.st());
    }
    {
        Timer t(c, "lc_scan");
        launch_lc_scan(a.loc, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    uint32_t live = 0;
    if (int rc_ = read_count(c, a.loc.tpre + p.ntl, "live entries", c->head, "log head", &live)) return rc_;
    if (expect_kept >= 0 && expect_kept != (int64_t)live)
        return fail(c, FB_ESTATE, "the log holds %u live entries, the caller expected %lld", live, (long long)expect_kept);
    if (kept_seq && cap < (int64_t)live)
        return fail(c, FB_EINVAL, "kept_seq holds %lld entries, the log %u live ones", (long long)cap, live);
    if (p.move.grid() > 0) {
        Timer t(c, "lc_move");
        launch_lc_move(a, false, t.st());
    }
    if (live) {
        Timer t(c, "lc_copy");
        launch_copy_words((uint32_t *)c->log_slot, (const uint32_t *)a.dst, (int64_t)live, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    if (kept_seq && live) HIPCHK(c, hipMemcpy(kept_seq, a.kept, (size_t)live * 8, hipMemcpyDeviceToHost));
    c->head = (int64_t)live;
    life_replaced(c->life);  // (with it the discarded FB_ENOSPC tick)
    if (n_kept) *n_kept = (int64_t)live;
    return FB_OK;
}

// A shard group's compaction, this rank's two halves.
// (the scratch of a full log: lc_scratch's bound, for the compaction's halves and for
// fb_log_reclaim_shard, which shares the allocation)
static size_t lcs_full_bytes(const fb_ctx *c) {
    return std::max(lcs_plan(std::max<int64_t>(c->head, (int64_t)c->log_cap * c->world), c->log_cap, c->W_cap, true).bytes,
                    lrs_plan(c->log_cap, c->W_cap).bytes);
}

int fb_log_compact_shard_bytes(fb_ctx *c, int64_t *bytes) {
    if (!c || !bytes) return FB_EINVAL;
    if (!c->shard) return fail(c, FB_ESTATE, "fb_log_compact_shard_bytes on a one-GPU context: use fb_log_compact");
    // (the committed head: a mark's, while one stands)
    *bytes = lcs_plan(c->head, 0, 0, false).xbytes;
    return FB_OK;
}

int fb_log_compact_shard_mark(fb_ctx *c, void *device_buffer, int64_t bytes, int64_t *n_live_local) {
    if (!c) return FB_EINVAL;
    // (the refusals before the gate's duties: a refused call changes nothing, a flush aside)
    if (c->shard && !c->life.marked) {
        const int64_t need = lcs_plan(c->head, 0, 0, false).xbytes;
        if (bytes < need || (need && !device_buffer) || ((uintptr_t)device_buffer & 7))
            return fail(c, FB_EINVAL, "exchange bitmap: %lld bytes at %p, the log needs %lld, 8-byte aligned", (long long)bytes,
                        device_buffer, (long long)need);
    }
    if (int rc_ = enter(c, Call::log_compact_shard_mark)) return rc_;  // (an uncommitted tick's clears are taken back here)
    HIPCHK(c, hipSetDevice(c->device));
    const LcPlan p = lcs_plan(c->head, c->head_local, c->W, false);
    if (int rc_ = lc_scratch(c, p.bytes, lcs_full_bytes(c), 0)) return rc_;
    c->lcs_buf = device_buffer;
    const LcArgs a = lc_args(c, p, false);
    if (p.flag_grid > 0) {
        Timer t(c, "lcs_flag");
        launch_lc_flag(a, true, t.st());
    }
    {
        Timer t(c, "lc_scan");
        launch_lc_scan(a.loc, t.st());
    }
    if (p.mark_grid > 0) {
        Timer t(c, "lcs_mark");
        launch_lcs_mark(a, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    uint32_t live = 0;
    if (int rc_ = read_count(c, a.loc.tpre + p.ntl, "live entries", c->head_local, "the log shard's entries", &live)) return rc_;
    c->lcs_head = c->head;
    c->lcs_head_local = c->head_local;
    c->lcs_live = (int64_t)live;
    life_lcs_marked(c->life);  // (with it the tick that was never committed)
    if (n_live_local) *n_live_local = (int64_t)live;
    return FB_OK;
}

int fb_log_compact_shard_apply(fb_ctx *c, int64_t n_live_global, int64_t *kept_seq, int64_t cap, int64_t *n_kept_local) {
    if (!c) return FB_EINVAL;
    if (kept_seq && cap < 0) return fail(c, FB_EINVAL, "cap %lld < 0", (long long)cap);
    if (int rc_ = enter(c, Call::log_compact_shard_apply)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->head != c->lcs_head || c->head_local != c->lcs_head_local) {  // (the gates keep the log as the mark saw it)
        life_lcs_unmarked(c->life);
        return fail(c, FB_ESTATE, "the log changed under a marked compaction");
    }
    const bool want_kept = kept_seq != nullptr;
    const LcPlan p = lcs_plan(c->head, c->head_local, c->W, want_kept);
    if (int rc_ = lc_scratch(c, p.bytes, lcs_full_bytes(c), p.keep)) return rc_;
    const LcArgs a = lc_args(c, p, want_kept);
    if (p.count_grid > 0) {
        Timer t(c, "lcs_count");
        launch_lcs_count(a, t.st());
    }
    {
        Timer t(c, "lc_scan");
        launch_lc_scan(a.glob, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    uint32_t total = 0;  // (no bound here: the comparison below refuses a wrong count its own way, and unmarks)
    if (int rc_ = read_count(c, a.glob.tpre + p.ntg, "live entries", UINT32_MAX, "a 32-bit count", &total)) return rc_;
    if ((int64_t)total != n_live_global || n_live_global > c->head || n_live_global < c->lcs_live) {
        life_lcs_unmarked(c->life);
        return fail(c, FB_ESTATE, "the reduced bitmap holds %u live entries, the group agreed on %lld (this rank: %lld of %lld)",
                    total, (long long)n_live_global, (long long)c->lcs_live, (long long)c->head);
    }
    if (kept_seq && cap < n_live_global)  // (the mark stays: the caller may apply again)
        return fail(c, FB_EINVAL, "kept_seq holds %lld entries, the group's log %lld live ones", (long long)cap,
                    (long long)n_live_global);
    const int64_t live = c->lcs_live;
    if (p.move.grid() > 0) {
        Timer t(c, "lcs_move");
        launch_lc_move(a, true, t.st());
    }
    if (live) {
        Timer t(c, "lc_copy");
        launch_copy_words((uint32_t *)c->log_slot, (const uint32_t *)a.dst, live, t.st());
    }
    if (live) {
        Timer t(c, "lc_copy");
        launch_copy_words(c->lseq, a.dseq, live, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    if (kept_seq && n_live_global)
        HIPCHK(c, hipMemcpy(kept_seq, a.kept, (size_t)n_live_global * 8, hipMemcpyDeviceToHost));
    c->head = n_live_global;
    c->head_local = live;
    c->lcs_buf = nullptr;
    life_replaced(c->life);
    if (n_kept_local) *n_kept_local = live;
    return FB_OK;
}

int fb_log_compact_shard_cancel(fb_ctx *c) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::log_compact_shard_cancel)) return rc_;  // (open in every state, no duties)
    c->lcs_buf = nullptr;
    life_lcs_unmarked(c->life);
    return FB_OK;
}

// Live entries of workers that stay registered completed on the device: count
// first (k_lr_flag, k_lc_scan write only the scratch), synchronise, check the caller's room,
// and only then take.  Nothing of the Life changes: the ticks after it make the launches they
// would have made without it.
// shard: a rank's part of its group's reclaim (§5g, "A shard group's reclaim").  Whether a local
// entry goes depends on its own sequence against the bound and on its slot's record, epoch and
// mask byte, all of which this rank holds -- so there is no exchange, and the call is the same
// over the shard.  The group agrees (every rank counts, cap = 0) before any rank takes.
static int log_reclaim_run(fb_ctx *c, bool shard, int64_t below_seq, const uint8_t *slot_mask, int64_t *seq_out,
                           int32_t *slot_out, int64_t cap, int64_t *n_reclaimed) {
    if (!c) return FB_EINVAL;
    if (below_seq < 0) return fail(c, FB_EINVAL, "below_seq %lld < 0", (long long)below_seq);
    if ((seq_out || slot_out) && cap < 0) return fail(c, FB_EINVAL, "cap %lld < 0", (long long)cap);
    // (a dropped launch's in-place clears are taken back here: what its results named is live)
    if (int rc_ = enter(c, shard ? Call::log_reclaim_shard : Call::log_reclaim)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    const LrPlan p = shard ? lrs_plan(c->head_local, c->W) : lr_plan(c->head, below_seq, c->W);
    if (p.nt == 0 || c->W == 0) {  // (nothing to walk, or no slot to hold a record: nothing is launched)
        if (n_reclaimed) *n_reclaimed = 0;
        return FB_OK;
    }
    const size_t full = shard ? lcs_full_bytes(c)
                              : std::max(lc_plan(c->log_cap, c->W_cap, true).bytes,
                                         lr_plan(c->log_cap, c->log_cap, c->W_cap).bytes);
    if (int rc_ = lc_scratch(c, p.bytes, full, 0)) return rc_;
    char *const base = (char *)c->lc_mem;
    // (the scratch is idle: every call that uses it waits for its launches before it returns,
    // and no mark stands)
    if (slot_mask) HIPCHK(c, hipMemcpy(base + p.mask, slot_mask, (size_t)c->W, hipMemcpyHostToDevice));
    LrArgs a{};
    a.log = c->log_slot;
    a.B = shard ? std::min(below_seq, c->head) : p.B;  // (a shard's bounds sequences, not entries)
    a.W = c->W;
    // (no sharded context commits lazily today: the test is kept for the day one does)
    a.live_chk = c->life.stale ? 1 : 0;
    a.reg = c->reg;
    a.epoch = c->epoch;
    a.mask = slot_mask ? (const uint8_t *)(base + p.mask) : nullptr;
    a.t = lc_table(base, p.tab, p.nt);
    a.seq_out = seq_out ? (int64_t *)(base + p.seq) : nullptr;
    a.slot_out = slot_out ? (int32_t *)(base + p.slot) : nullptr;
    // (sharded contexts keep no per-slot budget)
    a.bud = !shard && c->caps.clears == Clears::deferred ? c->bud : nullptr;
    if (shard) {
        a.seq = c->lseq;
        a.n = c->head_local;
        a.slot_base = c->slot_base;
    }
    {
        Timer t(c, "lr_flag");
        launch_lr_flag(a, shard, t.st());
    }
    {
        Timer t(c, "lc_scan");
        launch_lc_scan(a.t, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    uint32_t n = 0;
    if (int rc_ = read_count(c, a.t.tpre + p.nt, "reclaimed entries", shard ? c->head_local : p.B,
                             shard ? "the log shard's entries" : "the prefix", &n))
        return rc_;
    if (n_reclaimed) *n_reclaimed = (int64_t)n;
    if ((seq_out || slot_out) && cap < (int64_t)n)
        return fail(c, FB_EINVAL, "the outputs hold %lld entries, the call reclaims %u", (long long)cap, n);
    if (!n) return FB_OK;
    {
        Timer t(c, "lr_take");
        launch_lr_take(a, shard, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    if (seq_out) HIPCHK(c, hipMemcpy(seq_out, a.seq_out, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (slot_out) HIPCHK(c, hipMemcpy(slot_out, a.slot_out, (size_t)n * 4, hipMemcpyDeviceToHost));
    return FB_OK;
}
int fb_log_reclaim(fb_ctx *c, int64_t below_seq, const uint8_t *slot_mask, int64_t *seq_out, int32_t *slot_out, int64_t cap,
                   int64_t *n_reclaimed) {
    return log_reclaim_run(c, false, below_seq, slot_mask, seq_out, slot_out, cap, n_reclaimed);
}
int fb_log_reclaim_shard(fb_ctx *c, int64_t below_seq, const uint8_t *slot_mask, int64_t *seq_out, int32_t *slot_out,
                         int64_t cap, int64_t *n_reclaimed) {
    return log_reclaim_run(c, true, below_seq, slot_mask, seq_out, slot_out, cap, n_reclaimed);
}

// The committed pool summarised on the device.  The three launches write only
// the scratch and the host-mapped record; nothing here settles the log or normalises a window,
// so the ticks after it make the launches they would have made without it.
// shard: a rank's part for fb_pool_stats_shard (its own slots and log shard, the replicated
// queue's positions on its slots; *queue_len the queue's length).
static int pool_stats_run(fb_ctx *c, bool shard, double now, double tte, const double *age_edges, int32_t n_edges,
                          fb_pool_summary *out, int64_t *queue_len) {
    if (!c) return FB_EINVAL;
    if (!out) return fail(c, FB_EINVAL, "%s: out is null", shard ? "fb_pool_stats_shard" : "fb_pool_stats");
    if (shard && !queue_len) return fail(c, FB_EINVAL, "fb_pool_stats_shard: queue_len is null");
    if (n_edges < 0 || n_edges > FB_PS_MAX_EDGES)
        return fail(c, FB_EINVAL, "n_edges %d outside [0, %d]", n_edges, FB_PS_MAX_EDGES);
    const bool hbc = !c->deque;  // liveness exists
    if (hbc) {
        if (n_edges > 0 && !age_edges) return fail(c, FB_EINVAL, "age_edges is null with n_edges %d", n_edges);
        for (int i = 0; i < n_edges; ++i)
            if (!std::isfinite(age_edges[i]) || (i && !(age_edges[i] > age_edges[i - 1])))
                return fail(c, FB_EINVAL, "age_edges[%d] = %g: the edges must be finite and strictly ascending", i,
                            age_edges[i]);
        if (!std::isfinite(now) || !std::isfinite(tte))
            return fail(c, FB_EINVAL, "now %g / tte %g must be finite", now, tte);
    }
    // (its flush: observably an immediate commit)
    if (int rc_ = enter(c, shard ? Call::pool_stats_shard : Call::pool_stats)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->ps_out) {
        if (hipHostMalloc((void **)&c->ps_out, kPsCols * sizeof(int64_t), hipHostMallocMapped | hipHostMallocCoherent) !=
            hipSuccess) {
            c->ps_out = nullptr;
            return fail(c, FB_ENOMEM, "hipHostMalloc(pool summary record) failed");
        }
        HIPCHK(c, hipHostGetDevicePointer((void **)&c->ps_out_dev, c->ps_out, 0));
    }
    const int64_t head = shard ? c->head_local : c->head;  // the entries this context's log holds
    const PsPlan p = ps_plan(c->W, c->Qn, head);
    // (never beyond a full table, queue and log)
    if (int rc_ = scratch_grow(c, "pool summary scratch", c->ps_mem, c->ps_cap, p.bytes,
                               ps_plan(c->W_cap, std::max<int64_t>(c->qcap, c->Wq_cap), c->log_cap).bytes, 0))
        return rc_;
    char *const base = (char *)c->ps_mem;
    PsArgs a{};
    a.now = hbc ? now : 0.0;
    a.tte = hbc ? tte : 0.0;
    a.n_edges = hbc ? n_edges : 0;
    for (int i = 0; i < a.n_edges; ++i) a.edge[i] = age_edges[i];
    a.W = c->W;
    a.nt = p.nt;
    a.hb_chk = hbc ? 1 : 0;
    a.tomb_chk = c->win_cap ? 1 : 0;
    // (a sharded Life is never stale: only contexts with message lists commit lazily,
    // fb_tick_commit, and a sharded context has none -- its entries are completed in place)
    a.live_chk = c->life.stale ? 1 : 0;
    a.slot_base = shard ? c->slot_base : 0;
    a.Qn = c->Qn;
    a.qoff = c->qoff;
    a.head = head;
    a.reg = c->reg;
    a.free_ = c->free_[c->cur];
    a.hb = c->hb;
    a.bud = c->bud;
    a.epoch = c->epoch;
    a.queue = c->queue[c->qcur];
    a.qfree = c->qfree[c->qcur];
    a.log = c->log_slot;
    a.xbits = (unsigned long long *)(base + p.xbits);
    a.srow = (int64_t *)(base + p.srow);
    a.qrow = (int64_t *)(base + p.qrow);
    a.lrow = (int64_t *)(base + p.lrow);
    a.out = c->ps_out_dev;
    if (p.slots.grid() > 0) {
        Timer t(c, "ps_slots");
        shard ? launch_ps_slots_shard(a, t.st()) : launch_ps_slots(a, t.st());
    }
    if (p.log_grid > 0) {
        Timer t(c, "ps_log");
        shard ? launch_ps_log_shard(a, t.st()) : launch_ps_log(a, t.st());
    }
    {
        Timer t(c, "ps_fold");
        launch_ps_fold(a, t.st());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, stream_wait(c));
    const int64_t *r = c->ps_out;
    const int64_t W = c->W, n_reg = r[kPsReg], n_exp = r[kPsExp];
    // device-reported numbers are checked before they are handed out
    if (n_reg < 0 || n_reg > W)
        return fail(c, FB_EHIP, "device-reported registered slots %lld outside [0, %lld] (slots)", (long long)n_reg, (long long)W);
    if (n_exp < 0 || n_exp > n_reg)
        return fail(c, FB_EHIP, "device-reported expired slots %lld outside [0, %lld] (registered)", (long long)n_exp,
                    (long long)n_reg);
    if (shard && (r[kPsQ] < 0 || r[kPsQExp] < 0 || r[kPsQ] + r[kPsQExp] > c->Qn))
        return fail(c, FB_EHIP, "device-reported queue positions %lld + %lld outside [0, %lld] (the queue's length)",
                    (long long)r[kPsQ], (long long)r[kPsQExp], (long long)c->Qn);
    if (!shard && (r[kPsQ] < 0 || r[kPsQExp] < 0 || r[kPsQ] + r[kPsQExp] != c->Qtrue))
        return fail(c, FB_EHIP, "device-reported queue positions %lld + %lld differ from the queue's %lld", (long long)r[kPsQ],
                    (long long)r[kPsQExp], (long long)c->Qtrue);
    if (r[kPsLive] < 0 || r[kPsLiveExp] < 0 || r[kPsLive] + r[kPsLiveExp] > head)
        return fail(c, FB_EHIP, "device-reported live entries %lld + %lld outside [0, %lld] (%s)", (long long)r[kPsLive],
                    (long long)r[kPsLiveExp], (long long)head, shard ? "the log shard's entries" : "log head");
    int64_t fsum = 0, asum = 0;
    for (int i = 0; i < FB_PS_FREE_BINS; ++i) fsum += r[kPsFreeHist + i];
    for (int i = 0; i <= FB_PS_MAX_EDGES; ++i) asum += r[kPsAgeHist + i];
    if (fsum != n_reg - n_exp)
        return fail(c, FB_EHIP, "device-reported free histogram holds %lld slots, not %lld (registered, not expired)",
                    (long long)fsum, (long long)(n_reg - n_exp));
    if (asum != (hbc ? n_reg : 0))
        return fail(c, FB_EHIP, "device-reported age histogram holds %lld slots, not %lld (registered)", (long long)asum,
                    (long long)(hbc ? n_reg : 0));
    fb_pool_summary s{};
    s.n_slots = W;
    s.n_registered = n_reg;
    s.n_expired = n_exp;
    s.n_queued = r[kPsQ];
    s.n_queued_expired = r[kPsQExp];
    s.dispatchable = hbc ? r[kPsDisp] : -1;
    s.free_total = r[kPsFree];
    s.log_head = c->head;
    s.inflight = r[kPsLive];
    s.inflight_expired = r[kPsLiveExp];
    s.inflight_max = c->caps.clears == Clears::deferred ? r[kPsInflMax] : -1;
    const bool any_hb = hbc && r[kPsHbN] > 0;
    memcpy(&s.oldest_hb, &r[kPsHbMin], 8);
    memcpy(&s.newest_hb, &r[kPsHbMax], 8);
    if (!any_hb) s.oldest_hb = s.newest_hb = __builtin_nan("");
    for (int i = 0; i < FB_PS_FREE_BINS; ++i) s.free_hist[i] = r[kPsFreeHist + i];
    for (int i = 0; i <= FB_PS_MAX_EDGES; ++i) s.age_hist[i] = r[kPsAgeHist + i];
    *out = s;
    if (queue_len) *queue_len = c->Qn;
    return FB_OK;
}

int fb_pool_stats(fb_ctx *c, double now, double tte, const double *age_edges, int32_t n_edges, fb_pool_summary *out) {
    return pool_stats_run(c, false, now, tte, age_edges, n_edges, out, nullptr);
}

int fb_pool_stats_shard(fb_ctx *c, double now, double tte, const double *age_edges, int32_t n_edges,
                        fb_pool_summary *part, int64_t *queue_len) {
    return pool_stats_run(c, true, now, tte, age_edges, n_edges, part, queue_len);
}

// The ranks' parts folded into the group's summary: host arithmetic only (no device, no
// lifecycle: the parts are the caller's).
int fb_pool_merge(fb_ctx *c, const fb_pool_summary *parts, const int64_t *queue_lens, int32_t n_parts,
                  fb_pool_summary *out) {
    if (n_parts < 1) return fail(c, FB_EINVAL, "fb_pool_merge: n_parts %d < 1", n_parts);
    if (!parts || !queue_lens || !out) return fail(c, FB_EINVAL, "fb_pool_merge: a null pointer");
    fb_pool_summary s{};
    s.log_head = parts[0].log_head;
    s.oldest_hb = s.newest_hb = __builtin_nan("");
    bool no_counts = false;
    for (int p = 0; p < n_parts; ++p) {
        const fb_pool_summary &x = parts[p];
        if (x.log_head != s.log_head)
            return fail(c, FB_EINVAL, "fb_pool_merge: part %d has log head %lld, part 0 %lld", p, (long long)x.log_head,
                        (long long)s.log_head);
        if (queue_lens[p] != queue_lens[0])
            return fail(c, FB_EINVAL, "fb_pool_merge: part %d has queue length %lld, part 0 %lld", p,
                        (long long)queue_lens[p], (long long)queue_lens[0]);
        s.n_slots += x.n_slots;
        s.n_registered += x.n_registered;
        s.n_expired += x.n_expired;
        s.n_queued += x.n_queued;
        s.n_queued_expired += x.n_queued_expired;
        s.dispatchable += x.dispatchable;
        s.free_total += x.free_total;
        s.inflight += x.inflight;
        s.inflight_expired += x.inflight_expired;
        no_counts = no_counts || x.inflight_max < 0;
        s.inflight_max = std::max(s.inflight_max, x.inflight_max);
        // (NaN: a part without a heartbeat; the comparisons skip it)
        if (x.oldest_hb == x.oldest_hb && !(s.oldest_hb <= x.oldest_hb)) s.oldest_hb = x.oldest_hb;
        if (x.newest_hb == x.newest_hb && !(s.newest_hb >= x.newest_hb)) s.newest_hb = x.newest_hb;
        for (int i = 0; i < FB_PS_FREE_BINS; ++i) s.free_hist[i] += x.free_hist[i];
        for (int i = 0; i <= FB_PS_MAX_EDGES; ++i) s.age_hist[i] += x.age_hist[i];
    }
    if (no_counts) s.inflight_max = -1;
    if (s.n_queued + s.n_queued_expired != queue_lens[0])
        return fail(c, FB_EINVAL, "fb_pool_merge: the parts hold %lld + %lld queue positions, the queue %lld",
                    (long long)s.n_queued, (long long)s.n_queued_expired, (long long)queue_lens[0]);
    *out = s;
    return FB_OK;
}

int fb_read_shard_log(fb_ctx *c, uint32_t *log_seq, int64_t *log_len, int64_t *log_head) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::read_shard_log)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    if (log_seq && c->head_local)
        HIPCHK(c, hipMemcpy(log_seq, c->lseq, (size_t)c->head_local * 4, hipMemcpyDeviceToHost));
    if (log_len) *log_len = c->head_local;
    if (log_head) *log_head = c->head;
    return FB_OK;
}

int fb_bind_exchange(fb_ctx *c, void *device_buffer, int64_t bytes) {
    if (!c) return FB_EINVAL;
    if (!c->shard) return fail(c, FB_ESTATE, "fb_bind_exchange on a one-GPU context");
    if (bytes < 0 || (bytes && !device_buffer)) return fail(c, FB_EINVAL, "exchange buffer");
    HIPCHK(c, stream_wait(c));
    c->xbuf = (uint8_t *)device_buffer;
    c->xcap = bytes;
    c->xpar = 0;
    c->xz_ok = false;
    return FB_OK;
}

int fb_exchange_bytes(fb_ctx *c, int32_t n_events, int64_t *bytes) {
    if (!c || !bytes) return FB_EINVAL;
    if (int rc_ = enter(c, Call::exchange_bytes)) return rc_;
    const bool launched = life_launched(c->life);
    const int64_t E = n_events < 0 ? c->E_cap : n_events;
    const int64_t Qn = n_events < 0 ? c->Wq_cap : (launched ? c->l_Qn : c->Qn);
    // the maximum: room for the wide form or for the block rows of a <= kRFused-row table,
    // whichever is larger; a launched tick: its own width and rows
    const int64_t Qlog = Qn + 2 * E;
    if (n_events < 0) {
        // the largest of: the wide form at the largest queue; a queue of at most
        // kXRowsMaxBlocks blocks with a 128-row table's block rows (the one-launch form; a
        // 32-row table's block + group rows are smaller); the largest queue with a 32-row
        // table's block rows (the k_xscan form)
        const int64_t Qr = std::min<int64_t>(Qlog, (int64_t)kXRowsMaxBlocks * kBS);
        *bytes = (int64_t)std::max({xlayout(c->world, E, Qlog, 2).total,
                                    xlayout(c->world, E, Qr, 1, xrows_bytes(c->world, kRFused, Qr)).total,
                                    xlayout(c->world, E, Qlog, 1, xrows_bytes(c->world, kXGroupR, Qlog),
                                            xgrows_bytes(c->world, kXGroupR, Qlog)).total});
    } else {
        const int R = launched ? c->l_R : kRFused;
        const XRows xr = exchange_rows(c->paths, c->world, R, Qlog);
        *bytes = (int64_t)xlayout(c->world, E, Qlog, xc_width(R), xr.rows, xr.grows).total;
    }
    return FB_OK;
}

int fb_set_stream(fb_ctx *c, void *stream) {
    if (!c) return FB_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    c->stream = stream ? (hipStream_t)stream : c->own_s;
    return FB_OK;
}

int fb_tick_continue(fb_ctx *c) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::tick_continue)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    life_continue(c->life);
    return enqueue_tick(c);
}

// H2D copies of a staged batch into device half `half` on the copy stream, after the
// last tick that read that half; the launch waits for stage_ev[half].
static int stage_copies(fb_ctx *c, int half, const void *sk, const void *ss, const void *sv, const void *st,
                        const void *sq, int E) {
    if (c->use_rec[half]) HIPCHK(c, hipStreamWaitEvent(c->cp_s, c->use_ev[half], 0));
    HIPCHK(c, hipMemcpyAsync(c->evk[half], sk, E, hipMemcpyHostToDevice, c->cp_s));
    HIPCHK(c, hipMemcpyAsync(c->evsl[half], ss, (size_t)E * 4, hipMemcpyHostToDevice, c->cp_s));
    HIPCHK(c, hipMemcpyAsync(c->evv[half], sv, (size_t)E * 4, hipMemcpyHostToDevice, c->cp_s));
    HIPCHK(c, hipMemcpyAsync(c->evt[half], st, (size_t)E * 8, hipMemcpyHostToDevice, c->cp_s));
    if (sq)
        HIPCHK(c, hipMemcpyAsync(c->evq[half], sq, (size_t)E * 8, hipMemcpyHostToDevice, c->cp_s));
    else
        HIPCHK(c, hipMemsetAsync(c->evq[half], 0xff, (size_t)E * 8, c->cp_s));  // -1 for every event
    HIPCHK(c, hipEventRecord(c->stage_ev[half], c->cp_s));
    c->stage_rec[half] = true;
    return FB_OK;
}

// Validate a tick's events and stage them into the pinned half the next launch
// copies from.  Two halves: staging tick t+1 on the host overlaps tick t on the
// device (the half's previous copies were enqueued two launches ago; its event
// is waited for, not the stream).
int fb_tick_stage(fb_ctx *c, double now, int32_t n_events, const uint8_t *kind, const int32_t *slot,
                  const int32_t *val, const double *ts, const int64_t *seq) {
    if (!c) return FB_EINVAL;
    if (n_events < 0 || n_events > c->E_cap) return fail(c, FB_EINVAL, "n_events %d outside [0, %d]", n_events, c->E_cap);
    if (n_events && (!kind || !slot || !val || !ts))
        return fail(c, FB_EINVAL, "event arrays must be non-NULL");
    if (int rc_ = enter(c, Call::stage)) return rc_;
    const int E = n_events;
    const int half = c->stage_half ^ 1;
    // One pass over the caller's arrays: validate (branch-free; the per-event loop
    // below runs only to name the first offending event) while staging them into
    // pinned memory; fb_tick_launch_staged issues one async copy per array.
    const uint32_t Wv = (uint32_t)(c->shard ? c->W_global : c->W);
    int32_t vmax = 0;
    // Zero-copy: when the caller's arrays are pinned host memory (fb_host_alloc, e.g. a
    // dispatcher that parses messages straight into them) the pass only validates, and
    // the H2D copies read the caller's arrays; they must stay unchanged until the tick
    // that uses them has been waited for.
    bool direct = E > 0, resident = E > 0;
    if (direct) {
        const void *ptrs[5] = {kind, slot, val, ts, seq};
        int nhost = 0, ndev = 0, n = 0;
        for (int j = 0; j < 5; ++j) {
            if (!ptrs[j]) continue;  // seq may be NULL: filled with -1 on the device
            ++n;
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, ptrs[j]) != hipSuccess) {
                (void)hipGetLastError();
            } else if (at.type == hipMemoryTypeHost) {
                ++nhost;
            } else if (at.type == hipMemoryTypeDevice) {
                if (at.device != c->device)
                    return fail(c, FB_EINVAL, "event array %d is in the memory of GPU %d, the context's is GPU %d", j,
                                at.device, c->device);
                ++ndev;
            }
        }
        direct = nhost == n;
        resident = ndev == n;
        if (ndev && !resident) return fail(c, FB_EINVAL, "event arrays mix this GPU's memory with other memory");
    }
    if (resident) {
        // a batch already in this GPU's memory (e.g. parsed there, or staged ahead): the
        // tick reads it in place and its first kernel checks it (an invalid message is
        // overwritten with a harmless one and fb_tick_wait names it); no host pass
        if (!(c->caps.lists && c->paths.ev_ll))
            return fail(c, FB_EINVAL, "device-resident messages need a one-GPU heartbeat context");
        c->st_dev[0] = kind;
        c->st_dev[1] = slot;
        c->st_dev[2] = val;
        c->st_dev[3] = ts;
        c->st_dev[4] = seq;
        c->st_res = true;
        c->st_chk[0] = c->st_chk[1] = c->st_chk[2] = kind;  // device-checked (names come from bad_min)
        life_stage(c->life, true);
        c->st_E = E;
        c->st_vmax = 0;
        c->st_now = now;
        return FB_OK;
    }
    c->st_res = false;
    // pinned inputs: their H2D copies go out first and overlap the validation below (a
    // batch that fails validation is never launched, so copying it first is harmless)
    bool copied = false;
    if (E && direct) {
        if (int rc = stage_copies(c, half, kind, slot, val, ts, seq, E)) return rc;
        copied = true;
    }
    if (E) {
        const size_t ecap = (size_t)c->E_cap;
        char *h = (char *)c->h_stage + (size_t)half * ecap * 32;
        uint8_t *hk = (uint8_t *)h;
        int32_t *hs = (int32_t *)(h + ecap);
        int32_t *hv = (int32_t *)(h + ecap * 5);
        double *ht = (double *)(h + ecap * 9);
        int64_t *hq = (int64_t *)(h + ecap * 17);
        HIPCHK(c, hipSetDevice(c->device));
        if (!direct && c->stage_rec[half]) HIPCHK(c, hipEventSynchronize(c->stage_ev[half]));  // staging buffer reuse
        // parts of the batch on the pool's workers when it is large (the pass reads and
        // writes ~25 B per event, mostly cold caller memory: memory-latency bound)
        const int np = (c->pool && E >= kStagePar) ? c->pool->size() : 1;
        uint32_t pbad[16] = {0};
        int32_t pvmax[16] = {0};
        // pinned batches of contexts whose first launch is k_ev_link are checked there
        // (slots, kinds, timestamps; fb_tick_wait names the first offending event and the
        // tick commits nothing): the host does not read them at all.  The round table is
        // then sized from the last tick's free counts (a wider one is a rerun away).
        const bool dev_chk = direct && c->caps.lists && c->paths.ev_ll;
        const bool dq = c->deque;
        auto part = [&](int pi) {
            if (dev_chk) {
                pbad[pi] = 0;
                pvmax[pi] = 0;
                return;
            }
            const int lo = (int)((int64_t)E * pi / np), hi = (int)((int64_t)E * (pi + 1) / np);
            uint32_t bad = 0;
            int32_t vm = 0;
            double prev = ts[lo > 0 ? lo - 1 : 0];
            for (int i = lo; i < hi; ++i) {
                const uint8_t k = kind[i];
                const int32_t sl = slot[i], v = val[i];
                const double t = ts[i];
                // (a deque context, which never deletes a record, refuses a leave)
                bad |= (uint32_t)((uint32_t)sl >= Wv) | (uint32_t)!ev_kind_valid(k, dq) | (uint32_t)!(t <= now) |
                       (uint32_t)(t < prev);
                prev = t;
                vm = std::max(vm, k <= FB_EV_RECONNECT ? v : 0);
                if (!direct) {
                    hk[i] = k;
                    hs[i] = sl;
                    hv[i] = v;
                    ht[i] = t;
                    hq[i] = seq ? seq[i] : -1;
                }
            }
            pbad[pi] = bad;
            pvmax[pi] = vm;
        };
        if (np > 1 && !dev_chk) c->pool->run(part);
        else part(0);
        uint32_t bad = 0;
        for (int pi = 0; pi < np; ++pi) {
            bad |= pbad[pi];
            vmax = std::max(vmax, pvmax[pi]);
        }
        for (int i = 0; bad && i < E; ++i) {
            life_stage(c->life, false);
            c->stage_rec[half] = false;  // nothing was copied out of this half
            if ((uint32_t)slot[i] >= Wv) return fail(c, FB_EINVAL, "event %d: slot %d outside [0, %u)", i, slot[i], Wv);
            if (!ev_kind_valid(kind[i], false)) return fail(c, FB_EINVAL, "event %d: unknown kind %d", i, kind[i]);
            if (c->deque && kind[i] == FB_EV_LEAVE) return fail(c, FB_EINVAL, "event %d: leave on a deque context", i);
            if (c->deque && kind[i] == FB_EV_DRAIN) return fail(c, FB_EINVAL, "event %d: drain on a deque context", i);
            if (!(ts[i] <= now) || (i && ts[i] < ts[i - 1]))
                return fail(c, FB_EINVAL, "event %d: timestamps must be non-decreasing and <= now", i);
        }
        if (dev_chk) {  // checked by k_ev_link (fb_tick_wait reports)
            c->st_chk[0] = kind;
            c->st_chk[1] = slot;
            c->st_chk[2] = ts;
        } else {
            c->st_chk[0] = nullptr;
        }
    }
    if (E && !copied) {
        const size_t ecap = (size_t)c->E_cap;
        char *h = (char *)c->h_stage + (size_t)half * ecap * 32;
        if (int rc = stage_copies(c, half, h, h + ecap, h + ecap * 5, h + ecap * 9, h + ecap * 17, E)) return rc;
    }
    life_stage(c->life, true);
    c->st_E = E;
    c->st_vmax = vmax;
    c->st_now = now;
    return FB_OK;
}

static CommitArgs commit_args(fb_ctx *c, bool eager);

int fb_tick_launch_staged(fb_ctx *c, double tte, int64_t n_pending) {
    if (!c) return FB_EINVAL;
    if (n_pending < 0) return fail(c, FB_EINVAL, "n_pending < 0");
    if (int rc_ = enter(c, Call::launch)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    const int E = c->st_E;
    const int half = c->stage_half ^ 1;
    c->l_res = E && c->st_res;
    if (c->l_res) {
        c->ev_kind = (uint8_t *)c->st_dev[0];
        c->ev_slot = (int32_t *)c->st_dev[1];
        c->ev_val = (int32_t *)c->st_dev[2];
        c->ev_ts = (double *)c->st_dev[3];
        c->ev_seq = (int64_t *)c->st_dev[4];
        if (!c->ev_seq) {  // -1 for every message
            HIPCHK(c, hipMemsetAsync(c->evq[half], 0xff, (size_t)E * 8, c->stream));
            c->ev_seq = c->evq[half];
        }
    } else {
        if (E) HIPCHK(c, hipStreamWaitEvent(c->stream, c->stage_ev[half], 0));  // the staged copies
        c->ev_kind = c->evk[half];
        c->ev_slot = c->evsl[half];
        c->ev_val = c->evv[half];
        c->ev_ts = c->evt[half];
        c->ev_seq = c->evq[half];
    }
    c->stage_half = half;
    const double now = c->st_now;
    c->l_now = now;
    c->l_tte = c->deque ? __builtin_inf() : tte;  // start() has no liveness: nobody ever expires
    c->l_E = E;
    c->l_T = n_pending;
    c->l_head = c->head;
    c->l_head_local = c->head_local;
    c->l_Qn = c->Qn;
    c->l_qoff = c->qoff;
    c->tick += 1;  // per-launch stamp: a relaunch with other messages never sees this launch's marks
    if (c->caps.lists) c->tbits = c->tbitsb[c->tick & 1];  // the last tick's bits stay for its deferred commit
    c->l_R = choose_R(std::max(c->maxc_hint, c->st_vmax));
    // sharded: the round table starts at <= 128 rows (one byte per exchanged c: every
    // round below the table is exact, 255 > 128); a fill level reaching the table makes
    // fb_tick_wait ask for a relaunch, which gets a wider table (two bytes per c)
    if (c->shard) c->l_R = std::min(c->shard_R > 0 ? c->shard_R : std::min(c->l_R, kRFused), kShardMaxR);
    c->reruns = 0;
    c->l_resort = false;
    c->l_purge_only = c->next_purge_only;
    c->next_purge_only = false;
    life_launch(c->life, c->caps, E, win_plan(c));
    for (int j = 0; j < 3; ++j) c->l_chk[j] = E ? c->st_chk[j] : nullptr;
    c->hout->bad_ev = 0;  // set by k_ev_link when it finds an invalid message
    // lengths every finished tick writes: a value left unwritten reads back as -1 and fails
    // check_lengths instead of becoming a copy size (a relaunch overwrites them again)
    c->hout->new_qlen = -1;
    c->hout->win_head = -1;
    c->hout->win_qlen = -1;
    // one tag per host launch: the notes of fb_tick_wait's reruns and of a sharded
    // tick's phase 2 belong to this launch too (notes under older tags are never applied)
    if (c->caps.clears == Clears::in_place && ++c->undo_tag == 0) c->undo_tag = 1;
    const int rc = enqueue_tick(c);
    if (rc) return rc;
    if (c->eager && c->life.win) {
        // eager: the window tick's commit right behind it on the stream; it commits only
        // if the tick finished as a window tick (fb_tick_wait reruns it otherwise)
        const CommitArgs a = commit_args(c, true);
        if (!c->tick_ev_set) HIPCHK(c, hipEventRecord(c->tick_ev, c->stream));  // fb_tick_wait waits for the tick, not its commit
        Timer t(c, "commit");
        launch_commit(a, t.st());
        HIPCHK(c, hipGetLastError());
        life_eager_enqueued(c->life);
    }
    if (E && !c->l_res) {  // (a device-resident batch used no half)
        // the next copy into this device half waits for the tick's reads (a rerun in
        // fb_tick_wait reads it again, but no stage can target this half before then)
        HIPCHK(c, hipEventRecord(c->use_ev[half], c->stream));
        c->use_rec[half] = true;
    }
    return FB_OK;
}

int fb_tick_launch(fb_ctx *c, double now, double tte, int32_t n_events, const uint8_t *kind, const int32_t *slot,
                   const int32_t *val, const double *ts, const int64_t *seq, int64_t n_pending) {
    if (!c) return FB_EINVAL;
    if (n_pending < 0) return fail(c, FB_EINVAL, "n_pending < 0");
    int rc = fb_tick_stage(c, now, n_events, kind, slot, val, ts, seq);
    if (rc) return rc;
    return fb_tick_launch_staged(c, tte, n_pending);
}

int fb_purge_launch(fb_ctx *c, double now, double tte) {
    if (!c) return FB_EINVAL;
    // a tick without messages or pending tasks whose orphans are reported, not dispatched
    int rc = fb_tick_stage(c, now, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    c->next_purge_only = true;
    return fb_tick_launch_staged(c, tte, 0);
}

// Every length a finished tick reports becomes a copy size or a kernel bound later
// (fb_read_state's queue copy, the commit's grids, the readbacks): a value outside its
// buffer is a device fault, reported here with both numbers, before anything uses it.
// (task_dispatcher.py:327: the queue new_qlen describes.)
static int check_lengths(fb_ctx *c) {
    const HostOut &p = *c->hout;
    const int64_t O = p.O, N = p.N_eff;
    if (O < 0 || O > c->l_head)
        return fail(c, FB_EHIP, "device-reported orphans %lld outside [0, %lld] (log head)", (long long)O,
                    (long long)c->l_head);
    if (c->shard && (p.O_local < 0 || p.O_local > c->l_head_local || p.O_local > O))
        return fail(c, FB_EHIP, "device-reported local orphans %lld outside [0, %lld] (local log head)",
                    (long long)p.O_local, (long long)std::min<int64_t>(c->l_head_local, O));
    if (p.n_evicted < 0 || p.n_evicted > c->W)
        return fail(c, FB_EHIP, "device-reported evictions %lld outside [0, %d] (slots)", (long long)p.n_evicted, c->W);
    if (N < 0 || N > c->l_T + O)
        return fail(c, FB_EHIP, "device-reported dispatches %lld outside [0, %lld] (pending + orphans)", (long long)N,
                    (long long)(c->l_T + O));
    if (c->shard && (p.n_local < 0 || p.n_local > N))
        return fail(c, FB_EHIP, "device-reported local dispatches %lld outside [0, %lld]", (long long)p.n_local,
                    (long long)N);
    if (c->life.win) {
        if (p.win_head < c->l_qoff || p.new_qlen < 0 || p.win_head > c->qcap || p.new_qlen > c->qcap - p.win_head)
            return fail(c, FB_EHIP, "device-reported window [%lld, +%lld) outside the queue buffer [%lld, %lld)",
                        (long long)p.win_head, (long long)p.new_qlen, (long long)c->l_qoff, (long long)c->qcap);
        if (p.win_qlen < 0 || p.win_qlen > p.new_qlen || p.win_qlen > c->Wq_cap)
            return fail(c, FB_EHIP, "device-reported queue length %lld outside [0, %lld] (window length)",
                        (long long)p.win_qlen, (long long)std::min<int64_t>(p.new_qlen, c->Wq_cap));
    } else if (p.new_qlen < 0 || (!c->deque && p.new_qlen > c->qcap)) {
        // (deque contexts: a length past the token capacity is FB_ENOSPC below)
        return fail(c, FB_EHIP, "device-reported queue length %lld outside [0, %lld] (queue buffer)",
                    (long long)p.new_qlen, (long long)c->qcap);
    }
    return FB_OK;
}

static int tick_wait(fb_ctx *c, fb_tick_result *res, Wait &o);

int fb_tick_wait(fb_ctx *c, fb_tick_result *res) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::wait)) return rc_;
    for (;;) {
        // the one place a wait's outcome moves the tick on.  Whatever failed, the launch never
        // commits: a reader of the committed state takes its in-place clears back (life_gate)
        // without waiting for the next launch
        Wait o = Wait::other;
        int rc = tick_wait(c, res, o);
        life_wait_done(c->life, o);
        if (o != Wait::rerun && o != Wait::rerun_general) return rc;
        // the same functional tick again (a rerun cancels an eager commit: its kernel found the
        // tick unfinished and committed nothing; the rerun's commit is the ordinary one)
        c->reruns++;
        if ((rc = enqueue_tick(c))) {
            life_wait_done(c->life, Wait::other);
            return rc;
        }
    }
}

// One round: wait for the launched tick and say what it left (o).  A rerun is set up here and
// enqueued by the caller.
static int tick_wait(fb_ctx *c, fb_tick_result *res, Wait &o) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->life.eager) {
        // the tick's results are final when its last kernel is: the host goes on while
        // the eager commit runs (the next launch queues behind it)
        hipError_t e;
        while ((e = hipEventQuery(c->tick_ev)) == hipErrorNotReady) {
        }
        HIPCHK(c, e);
    } else {
        HIPCHK(c, stream_wait(c));
    }
    if (c->l_chk[0] && c->hout->bad_ev) {
        // the batch was left to the device's check: name the first offending event; the
        // tick is not committed (its launch read only committed state)
        o = Wait::invalid_message;
        // the first offending message's index (k_ev_link atomicMins it for every checked
        // batch): read, and reset for the next checked batch whatever its kind
        int32_t bi = 0x7f7f7f7f;
        const int32_t none = 0x7f7f7f7f;
        HIPCHK(c, hipMemcpy(&bi, c->bad_min, 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->bad_min, &none, 4, hipMemcpyHostToDevice));
        if (c->l_res) {
            // a device-resident batch: the index from the device
            return fail(c, FB_EINVAL, "event %d: invalid message (slot outside [0, %d), unknown kind, or a "
                        "timestamp decreasing or past now)", bi, c->W);
        }
        const uint8_t *k = (const uint8_t *)c->l_chk[0];
        const int32_t *sl = (const int32_t *)c->l_chk[1];
        const double *ts = (const double *)c->l_chk[2];
        for (int i = 0; i < c->l_E; ++i) {
            if ((uint32_t)sl[i] >= (uint32_t)c->W) return fail(c, FB_EINVAL, "event %d: slot %d outside [0, %d)", i, sl[i], c->W);
            if (!ev_kind_valid(k[i], false)) return fail(c, FB_EINVAL, "event %d: unknown kind %d", i, k[i]);
            if (!(ts[i] <= c->l_now) || (i && ts[i] < ts[i - 1]))
                return fail(c, FB_EINVAL, "event %d: timestamps must be non-decreasing and <= now", i);
        }
        return fail(c, FB_EINVAL, "invalid message in the batch");
    }
    if (c->l_used_ll && c->hout->resort) {
        // a slot got more messages than k_ev_apply_ll sorts in registers: the same
        // functional tick again, grouped by the radix sort
        if (c->reruns > 4) return fail(c, FB_EHIP, "event regrouping did not converge");
        c->l_resort = true;
        o = Wait::rerun_general;  // the sorted path purges in k_scan: a general tick
        return FB_OK;
    }
    if (c->life.win && (c->hout->status == 3 || c->hout->win_ovf)) {
        // the window tick could not finish inside its window (a fill level above 0, an
        // unserved front, a first unserved element past the scanned prefix, no room at
        // the tail): the same functional tick on the general path
        if (c->hout->status == 3 && (int64_t)c->l_nchW * kWinCh < c->l_Qn)  // the scanned prefix was short
            c->win_slack = std::min<int64_t>(2 * c->win_slack, 1 << 24);
        c->win_fallbacks++;
        o = Wait::rerun_general;
        return FB_OK;
    }
    if (c->hout->status == 2) {
        o = Wait::log_full;
        return fail(c, FB_ENOSPC, "in-flight log full: %lld entries + this tick's dispatches exceed %lld",
                    (long long)c->l_head, (long long)c->log_cap);
    }
    // the queue holds free counts beyond the round table: widen and rerun
    if (c->hout->status != 0 && c->shard) {
        // the exchange runs between the phases, so the caller relaunches: the same tick
        // with a table sized by the max free count seen (the ranks' records carry the true one)
        const int R = choose_R(c->hout->maxc, kShardMaxR);
        o = Wait::too_narrow;
        if (c->l_R >= kShardMaxR || R <= c->l_R)
            return fail(c, FB_ERANGE, "sharded tick: fill level beyond a %d-round table (max free %d)", c->l_R,
                        c->hout->maxc);
        c->shard_R = std::min(R, kShardMaxR);
        o = Wait::relaunch_wanted;
        return fail(c, FB_ERERUN, "sharded tick: the fill level reaches the %d-round table; relaunch (%d rows)",
                    c->l_R, c->shard_R);
    }
    if (c->hout->status != 0) {
        const int R = choose_R(c->hout->maxc);
        o = Wait::too_narrow;
        if (R <= c->l_R || c->reruns > 4)
            return fail(c, FB_ERANGE, "fill level beyond the round table (maxc %d, R %d)", c->hout->maxc, c->l_R);
        c->l_R = R;
        o = Wait::rerun;
        return FB_OK;
    }
    if (c->paths.fault_qlen >= 0) {
        // (a window tick reported the injected length from the device already)
        c->hout->new_qlen = c->paths.fault_qlen;
        c->hout->win_qlen = c->paths.fault_qlen;
        c->paths.fault_qlen = -1;
    }
    if (int rc_ = check_lengths(c)) {
        o = Wait::lengths_rejected;  // the tick is not committed (its launch read only committed state)
        return rc_;
    }
    const HostOut &p = *c->hout;
    if (c->deque && p.new_qlen > c->Wq_cap)
        return fail(c, FB_ENOSPC, "deque of %lld tokens exceeds the context's capacity %d", (long long)p.new_qlen,
                    c->Wq_cap);
    fb_tick_result r{};
    r.n_assigned = p.N_eff;
    r.n_orphans = p.O;
    r.queue_len = c->life.win ? p.win_qlen : (int64_t)p.new_qlen;
    r.log_head = c->l_head + p.N_eff;
    r.n_evicted = (int32_t)p.n_evicted;
    r.fill_level = p.L;
    r.max_free = p.maxc;
    r.reruns = c->reruns;
    r.n_local = c->shard ? p.n_local : p.N_eff;
    r.n_orphans_local = c->shard ? p.O_local : p.O;
    c->last = r;
    o = Wait::ok;
    if (res) *res = r;
    return FB_OK;
}

// The commit of the launched tick.  eager: built at launch, before the tick's results
// exist -- the window's head and appended positions are read by the kernel from the
// tick's results, and every orphan tile and appended position gets blocks (grid-stride).
static CommitArgs commit_args(fb_ctx *c, bool eager) {
    // lazy clears: the redistributed entries stay in the log (dead to every later tick)
    const bool lazy = lazy_ctx(c);
    const int64_t n_orph = (eager || lazy) ? 0 : c->last.n_orphans_local;
    CommitArgs a{};
    a.W = c->W;
    a.nbw = (int)cdiv(c->W, kBS);
    a.tick = c->tick;
    a.st = c->st;
    a.touched = c->touched;
    a.post = c->post;
    a.tbits = c->tbits;
    a.E = c->l_E;
    a.reg = c->reg;
    a.hb = c->hb;
    a.epoch = c->epoch;
    a.n_orph = n_orph;
    a.orphans = c->orphans;
    a.log_slot = c->log_slot;
    a.lseq = c->lseq;
    a.head_local = c->l_head_local;
    a.shard = c->shard;
    a.nbo = (int)cdiv(n_orph, kBS);
    if (!lazy && c->l_oseg && (n_orph > 0 || eager)) {  // per-tile segments: a wave per log tile
        a.oseg = c->fcnt;
        a.oseg_tiles = c->l_nbf;
        a.nbo = (int)cdiv(c->l_nbf, kWaves);
    }
    a.n_clr = c->caps.clears == Clears::deferred ? c->l_E : 0;  // one-GPU heartbeat: the results' completed entries
    a.ev_clr = c->ev_clr;
    a.bud = c->bud;
    a.bud_next = c->bud_next;
    if (c->life.win) {
        // the window moves: positions of slots that left become tombstones, kept slots that
        // got messages take their post-message counts, appended slots their positions
        a.win = 1;
        a.wq_tail = c->l_qoff + c->l_Qn;
        if (eager) {
            a.eager = c->cw;
            a.cw_tag = c->link;
            a.nbap = (int)std::min<int64_t>(1024, cdiv(2 * (int64_t)c->l_E + c->l_T, kBS) + 1);
        } else {
            const HostOut &p = *c->hout;
            a.wq_head = p.win_head;
            a.napp = p.win_head + p.new_qlen - a.wq_tail;
            a.nbap = (int)cdiv(a.napp, kBS);
        }
        a.wq_buf = c->queue[c->qcur];
        a.wqf = c->qfree[c->qcur];
        a.wqh = c->qhb[c->qcur];
        a.pos = c->pos_of[c->qcur];
        a.tomb = c->tomb;
        a.n_tomb = 2 * c->l_E;
        a.post_rf = c->post_rf;
    }
    return a;
}

int fb_tick_commit(fb_ctx *c) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::commit)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n_orph = c->last.n_orphans_local;
    bool deferred = false;
    if (c->life.eager) {
        // the device committed the tick right behind it (fb_tick_launch_staged)
    } else if (c->W > 0 || n_orph > 0 || (c->caps.clears == Clears::deferred && c->l_E > 0)) {
        const CommitArgs a = commit_args(c, false);
        deferred = c->caps.lists && c->paths.ev_ll && !c->life.win;
        if (deferred) {  // (by default a window tick's commit runs at once)
            // deferred: the next launch's k_ev_link runs it (or flush_commit)
            c->cm = a;
        } else {
            Timer t(c, "commit");
            launch_commit(a, t.st());
            HIPCHK(c, hipGetLastError());
        }
    }
    c->cur = 1 - c->cur;
    // sharded: a tick that needed a wide table keeps it for the next one while the fill
    // level stays beyond the narrow table (no relaunch per tick)
    if (c->shard) c->shard_R = c->last.fill_level + 2 > kRFused ? c->l_R : 0;
    c->head = c->last.log_head;
    c->head_local += c->shard ? c->last.n_local : 0;
    c->Qtrue = c->last.queue_len;
    c->last_L = c->last.fill_level;
    c->last_O = c->last.n_orphans;
    if (c->life.win) {
        // the queue stays in its buffers: the window slid and grew
        c->qoff = c->hout->win_head;
        c->Qn = c->hout->new_qlen;
        c->win_ticks++;
        // the scanned prefix saw only part of the queue: keep the larger hint
        c->maxc_hint = std::max(c->maxc_hint, std::max(1, c->last.max_free));
    } else {
        c->qcur ^= 1;
        c->qoff = 0;
        c->pos_ok = false;  // the new queue's positions are rebuilt by the next window tick
        c->Qn = c->last.queue_len;
        c->maxc_hint = std::max(1, c->last.max_free);
    }
    life_commit(c->life, deferred, lazy_ctx(c) && c->last.n_orphans > 0);  // (lazy: its orphans stay in the log)
    return FB_OK;
}

int fb_get_local_assignments(fb_ctx *c, int64_t first, int64_t n, int64_t *task, int32_t *slot) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::get_local_assignments)) return rc_;
    if (first < 0 || n < 0 || first + n > c->last.n_local) return fail(c, FB_EINVAL, "assignment range");
    if (!n) return FB_OK;
    const int64_t base = c->shard ? c->l_head_local : c->l_head;
    if (slot) HIPCHK(c, hipMemcpy(slot, c->log_slot + base + first, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (task) {
        if (c->shard) {
            std::vector<uint32_t> q((size_t)n);
            HIPCHK(c, hipMemcpy(q.data(), c->lseq + base + first, (size_t)n * 4, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < n; ++i) task[i] = (int64_t)q[i] - c->l_head;
        } else {
            for (int64_t i = 0; i < n; ++i) task[i] = first + i;
        }
    }
    return FB_OK;
}

// Device -> host copy enqueued on the context stream: into pinned host memory by a
// copy kernel whose stores cross PCIe directly (the DMA engine path measured 137 to
// 344 us for 4 MB on different boxes, the kernel path is not tied to it), else by
// hipMemcpyAsync (pageable memory: the runtime stages it).
static int d2h(fb_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!bytes) return FB_OK;
    if ((bytes & 3) == 0) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, dst) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) {
            launch_copy_words((uint32_t *)at.devicePointer, (const uint32_t *)src, (int64_t)(bytes / 4), Stream(c->stream));
            HIPCHK(c, hipGetLastError());
            return FB_OK;
        }
        (void)hipGetLastError();
    }
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return FB_OK;
}
// Device pointer of the waited tick's dense orphan list: an f_emit tick left per-tile
// segments, gathered into orph_dense here (once per tick).
static int64_t *orph_dense_dev(fb_ctx *c) {
    if (!c->l_oseg) return c->orphans;
    if (!c->dense_ok) {
        launch_orph_gather(c->orph_dense, c->orphans, c->fcnt, c->l_nbf, Stream(c->stream));
        c->dense_ok = true;
    }
    return c->orph_dense;
}
// n orphans of the waited tick into dst; the whole list of segments goes straight into
// pinned host memory by the gather kernel
static int orph_out(fb_ctx *c, int64_t *dst, int64_t n) {
    if (!n) return FB_OK;
    if (c->l_oseg && n == c->last.n_orphans_local) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, dst) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) {
            launch_orph_gather((int64_t *)at.devicePointer, c->orphans, c->fcnt, c->l_nbf, Stream(c->stream));
            HIPCHK(c, hipGetLastError());
            return FB_OK;
        }
        (void)hipGetLastError();
    }
    return d2h(c, dst, orph_dense_dev(c), (size_t)n * 8);
}
// A window tick leaves its evicted slots to the per-slot status bytes: the ascending list
// is built (once per tick) when something reads it.
static int evict_ready(fb_ctx *c) {
    if (!c->life.win || c->evict_ok || !c->last.n_evicted) return FB_OK;
    launch_evict_gather(c->evicted, c->st, c->wcnt, c->wpre, c->W, Stream(c->stream));
    HIPCHK(c, hipGetLastError());
    c->evict_ok = true;
    return FB_OK;
}
static int copy_out(fb_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!bytes) return FB_OK;
    if (int rc = d2h(c, dst, src, bytes)) return rc;
    HIPCHK(c, stream_wait(c));
    return FB_OK;
}

int fb_get_assignments(fb_ctx *c, int64_t first, int64_t n, int32_t *dst) {
    if (!c || !dst) return FB_EINVAL;
    if (int rc_ = enter(c, Call::get_assignments)) return rc_;
    if (c->shard && !c->l_full)
        return fail(c, FB_ESTATE, "sharded context: use fb_get_local_assignments (or fb_set_full_assign)");
    if (first < 0 || n < 0 || first + n > c->last.n_assigned) return fail(c, FB_EINVAL, "assignment range");
    if (c->shard) return copy_out(c, dst, c->assign_all + first, (size_t)n * 4);
    return copy_out(c, dst, c->log_slot + c->l_head + first, (size_t)n * 4);
}

int fb_get_orphans(fb_ctx *c, int64_t n, int64_t *dst) {
    if (!c || !dst) return FB_EINVAL;
    if (int rc_ = enter(c, Call::get_orphans)) return rc_;
    if (n < 0 || n > c->last.n_orphans_local) return fail(c, FB_EINVAL, "orphan count");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = orph_out(c, dst, n)) return rc;
    HIPCHK(c, stream_wait(c));
    return FB_OK;
}

int fb_get_evicted(fb_ctx *c, int32_t n, int32_t *dst) {
    if (!c || !dst) return FB_EINVAL;
    if (int rc_ = enter(c, Call::get_evicted)) return rc_;
    if (n < 0 || n > c->last.n_evicted) return fail(c, FB_EINVAL, "evicted count");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->l_cout) {  // the tick wrote them into the registered pinned buffer
        if (n && dst != c->cout_host[3]) memcpy(dst, c->cout_host[3], (size_t)n * 4);
        return FB_OK;
    }
    if (int rc = evict_ready(c)) return rc;
    return copy_out(c, dst, c->evicted, (size_t)n * 4);
}

int fb_get_outputs(fb_ctx *c, int32_t *assign, int64_t *orphans, int32_t *evicted) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::get_outputs)) return rc_;
    if (assign && c->shard) return fail(c, FB_ESTATE, "sharded context: use fb_get_local_assignments");
    HIPCHK(c, hipSetDevice(c->device));
    // the three copies back to back on the stream, one synchronisation
    int rc;
    if (assign && c->last.n_assigned && (rc = d2h(c, assign, c->log_slot + c->l_head, (size_t)c->last.n_assigned * 4)))
        return rc;
    if (orphans && (rc = orph_out(c, orphans, c->last.n_orphans_local))) return rc;
    if (evicted && (rc = evict_ready(c))) return rc;
    if (evicted && c->last.n_evicted && c->l_cout) {
        if (evicted != c->cout_host[3]) memcpy(evicted, c->cout_host[3], (size_t)c->last.n_evicted * 4);
    } else if (evicted && c->last.n_evicted && (rc = d2h(c, evicted, c->evicted, (size_t)c->last.n_evicted * 4))) {
        return rc;
    }
    HIPCHK(c, stream_wait(c));
    return FB_OK;
}

int fb_set_window(fb_ctx *c, int mode) {
    if (!c) return FB_EINVAL;
    if (mode < -1 || mode > 1) return fail(c, FB_EINVAL, "window mode %d (-1 auto, 0 off, 1 on)", mode);
    if (int rc_ = enter(c, Call::set_window)) return rc_;
    if (mode > 0) {
        if (int rc = win_alloc(c)) return rc;
    }
    c->win = mode;
    return FB_OK;
}

int fb_set_eager_commit(fb_ctx *c, int enable) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::set_eager_commit)) return rc_;
    c->eager = enable ? 1 : 0;
    return FB_OK;
}

int fb_window_stats(fb_ctx *c, int64_t *window_ticks, int64_t *fallbacks) {
    if (!c) return FB_EINVAL;
    if (window_ticks) *window_ticks = c->win_ticks;
    if (fallbacks) *fallbacks = c->win_fallbacks;
    return FB_OK;
}

int fb_set_compact_out(fb_ctx *c, int32_t *slot, uint8_t *cnt, int64_t cap, int64_t *orphans, int64_t ocap,
                       int32_t *evicted, int64_t ecap) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::set_compact_out)) return rc_;
    if (!slot) {  // unregister
        c->cout_slot = nullptr;
        return FB_OK;
    }
    if (!cnt || !orphans || !evicted || cap < 0 || ocap < 0 || ecap < 0) return FB_EINVAL;
    void *dv[4];
    const void *hp[4] = {slot, cnt, orphans, evicted};
    for (int j = 0; j < 4; ++j) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, hp[j]) != hipSuccess || at.type != hipMemoryTypeHost || !at.devicePointer) {
            (void)hipGetLastError();
            return fail(c, FB_EINVAL, "compact output buffers must be pinned host memory (fb_host_alloc)");
        }
        dv[j] = at.devicePointer;
        c->cout_host[j] = hp[j];
    }
    c->cout_slot = (int32_t *)dv[0];
    c->cout_c = (uint8_t *)dv[1];
    c->cout_orph = (int64_t *)dv[2];
    c->cout_ev = (int32_t *)dv[3];
    c->cout_cap = cap;
    c->cout_ocap = ocap;
    c->cout_ecap = ecap;
    c->compact = 1;
    return FB_OK;
}

int fb_set_compact(fb_ctx *c, int enable) {
    if (!c) return FB_EINVAL;
    if (c->shard) return fail(c, FB_ESTATE, "compact assignments exist on one-GPU contexts only");
    c->compact = enable != 0;
    return FB_OK;
}

int fb_get_outputs_compact(fb_ctx *c, int32_t *slot, uint8_t *cnt, int64_t cap, int64_t *n_pos, int64_t *orphans,
                           int32_t *evicted) {
    if (!c || !n_pos) return FB_EINVAL;
    if (int rc_ = enter(c, Call::get_outputs_compact)) return rc_;
    if (!c->l_compact) return fail(c, FB_ESTATE, "the tick was launched without fb_set_compact");
    if (c->last.fill_level + 1 > 255)
        return fail(c, FB_ERANGE, "fill level %d: rounds beyond a byte, read fb_get_outputs", c->last.fill_level);
    const int64_t n = c->l_Qn + 2 * (int64_t)c->l_E;
    *n_pos = n;
    // the tick wrote into the registered buffers: nothing left to copy into those
    if (c->l_cout && (!slot || slot == c->cout_host[0]) && (!cnt || cnt == c->cout_host[1]) &&
        (!orphans || orphans == c->cout_host[2]) && (!evicted || evicted == c->cout_host[3]))
        return FB_OK;
    if ((slot || cnt) && cap < n) return fail(c, FB_EINVAL, "compact buffers of %lld < %lld positions", (long long)cap,
                                              (long long)n);
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    // into pinned memory: the word copies in one kernel (and the orphan segments gathered
    // straight into their buffer), else one transfer per array
    CopyMulti m{};
    auto mapped = [](void *p) -> uint32_t * {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer)
            return (uint32_t *)at.devicePointer;
        (void)hipGetLastError();
        return nullptr;
    };
    auto add = [&](void *dst, const void *src, int64_t bytes) -> bool {
        uint32_t *d = (bytes & 3) == 0 ? mapped(dst) : nullptr;
        if (!d) return false;
        const int b0 = m.n ? m.blk0[m.n - 1] + copy_blocks(m.words[m.n - 1]) : 0;
        m.dst[m.n] = d;
        m.src[m.n] = (const uint32_t *)src;
        m.words[m.n] = bytes / 4;
        m.blk0[m.n] = b0;
        m.n++;
        return true;
    };
    // the c bytes travel as whole words when the caller's buffer has room for the padding
    const int64_t cw = (n + 3) & ~(int64_t)3;
    if (c->l_cout) {  // the tick wrote the compact form into the registered buffers
        if (slot && n && slot != c->cout_host[0]) memcpy(slot, c->cout_host[0], (size_t)n * 4);
        if (cnt && n && cnt != c->cout_host[1]) memcpy(cnt, c->cout_host[1], (size_t)n);
    } else {
        if (slot && n && !add(slot, c->rb_slot, n * 4) && (rc = d2h(c, slot, c->rb_slot, (size_t)n * 4))) return rc;
        if (cnt && n && !(cw <= cap && add(cnt, c->rb_c, cw)) && (rc = d2h(c, cnt, c->rb_c, (size_t)n))) return rc;
    }
    if (evicted && c->last.n_evicted && c->l_cout) {
        if (evicted != c->cout_host[3]) memcpy(evicted, c->cout_host[3], (size_t)c->last.n_evicted * 4);
    } else if (evicted && c->last.n_evicted && !add(evicted, c->evicted, (int64_t)c->last.n_evicted * 4) &&
               (rc = d2h(c, evicted, c->evicted, (size_t)c->last.n_evicted * 4))) {
        return rc;
    }
    // the orphans' segments gathered by the same launch when they go to pinned memory
    bool orph_done = false;
    if (orphans && c->l_oseg && c->last.n_orphans_local) {
        if (int64_t *od = (int64_t *)mapped(orphans)) {
            m.odst = od;
            m.osrc = c->orphans;
            m.ocnt = c->fcnt;
            m.otiles = c->l_nbf;
            orph_done = true;
        }
    }
    launch_copy_multi(m, Stream(c->stream));
    HIPCHK(c, hipGetLastError());
    if (orphans && !orph_done && (rc = orph_out(c, orphans, c->last.n_orphans_local))) return rc;
    HIPCHK(c, stream_wait(c));
    return FB_OK;
}

// Host: every task's slot from the compact form of the waited tick.  Round r <= L
// serves the positions with c > r in LRU order, task S(r) + j going to the j-th of
// them; S(r) = sum of min(c, r).  The rounds are independent ranges of the output,
// so they are expanded in parallel (FAASBAL_EXPAND_THREADS workers, default 8).
int fb_expand_compact(fb_ctx *c, const int32_t *slot, const uint8_t *cnt, int64_t n_pos, int32_t *assign) {
    if (!c || (n_pos && (!slot || !cnt)) || (!assign && c->last.n_assigned)) return FB_EINVAL;
    if (int rc_ = enter(c, Call::expand_compact)) return rc_;
    const int L = c->last.fill_level;
    const int64_t N = c->last.n_assigned;
    if (L + 1 > 255) return fail(c, FB_ERANGE, "fill level %d beyond the compact form", L);
    // A(r) = #{c > r}, S(r + 1) = S(r) + A(r), r <= L
    std::vector<int64_t> hist(L + 3, 0), S(L + 2, 0);
    for (int64_t i = 0; i < n_pos; ++i) hist[std::min<int>(cnt[i], L + 2)]++;
    int64_t above = 0;
    std::vector<int64_t> A(L + 2, 0);
    for (int r = L + 1; r >= 0; --r) {
        above += hist[r + 1];
        A[r] = above;
    }
    for (int r = 0; r <= L; ++r) S[r + 1] = S[r] + A[r];
    if (S[L] > N || N > S[L + 1]) return fail(c, FB_EINVAL, "compact form does not match the waited tick");
    if (!c->xpool) {
        const char *e = getenv("FAASBAL_EXPAND_THREADS");
        c->xpool = new HostPool(std::max(1, std::min(e ? atoi(e) : 8, 64)));
    }
    const int np = c->xpool->size();
    c->xpool->run([&](int t) {
        for (int r = t; r <= L; r += np) {
            int32_t *o = assign + S[r];
            const int64_t lim = std::min<int64_t>(A[r], N - S[r]);
            int64_t k = 0;
            for (int64_t i = 0; i < n_pos && k < lim; ++i)
                if (cnt[i] > r) o[k++] = slot[i];
        }
    });
    return FB_OK;
}

int fb_host_alloc(fb_ctx *c, int64_t bytes, void **ptr) {
    if (!c || !ptr || bytes < 0) return FB_EINVAL;
    *ptr = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    if (hipHostMalloc(ptr, (size_t)std::max<int64_t>(bytes, 1), hipHostMallocDefault) != hipSuccess)
        return fail(c, FB_ENOMEM, "hipHostMalloc(%lld B) failed", (long long)bytes);
    return FB_OK;
}

int fb_host_free(fb_ctx *c, void *ptr) {
    // pinned host memory belongs to the process, not to the context: ctx may be NULL
    // (a buffer that outlives its context is freed when its last user lets it go)
    if (!c) return (!ptr || hipHostFree(ptr) == hipSuccess) ? FB_OK : FB_EHIP;
    if (ptr) HIPCHK(c, hipHostFree(ptr));
    return FB_OK;
}

int fb_get_event_status(fb_ctx *c, int32_t n, uint8_t *dst) {
    if (!c || !dst) return FB_EINVAL;
    if (int rc_ = enter(c, Call::get_event_status)) return rc_;
    if (n < 0 || n > c->l_E) return fail(c, FB_EINVAL, "event count");
    const uint8_t *src = c->shard ? c->xbuf + xlayout(c->world, c->l_E, c->l_Qn + 2 * (int64_t)c->l_E).evs : c->ev_status;
    if (n) HIPCHK(c, hipMemcpy(dst, src, (size_t)n, hipMemcpyDeviceToHost));
    return FB_OK;
}

namespace {
// wait for the launched tick, copy the requested outputs, commit
int finish_tick(fb_ctx *c, int32_t n_events, fb_tick_result *res, uint8_t *ev_status, int32_t *assign,
                int64_t *orphans, int32_t *evicted) {
    int rc;
    fb_tick_result r;
    if ((rc = fb_tick_wait(c, &r))) return rc;
    if (ev_status && (rc = fb_get_event_status(c, n_events, ev_status))) return rc;
    if (assign && (rc = fb_get_assignments(c, 0, r.n_assigned, assign))) return rc;
    if (orphans && (rc = fb_get_orphans(c, r.n_orphans, orphans))) return rc;
    if (evicted && (rc = fb_get_evicted(c, r.n_evicted, evicted))) return rc;
    if (res) *res = r;
    return fb_tick_commit(c);
}
}  // namespace

int fb_apply_events(fb_ctx *c, double tte, int32_t n_events, const uint8_t *kind, const int32_t *slot,
                    const int32_t *val, const double *ts, const int64_t *seq, fb_tick_result *res,
                    uint8_t *ev_status, int64_t *orphans, int32_t *evicted) {
    if (!c) return FB_EINVAL;
    if (c->shard) return fail(c, FB_ESTATE, "fb_apply_events on a sharded context (use the two-phase tick)");
    if (n_events < 0 || (n_events && !ts)) return fail(c, FB_EINVAL, "event arrays");
    if (res) *res = fb_tick_result{};
    if (!n_events) return FB_OK;
    // the messages, each after the purge at its own clock, then the purge that follows
    // the last one (:390) at that clock; nothing dispatched, orphans reported
    int rc = fb_tick_stage(c, ts[n_events - 1], n_events, kind, slot, val, ts, seq);
    if (rc) return rc;
    c->next_purge_only = true;
    if ((rc = fb_tick_launch_staged(c, tte, 0))) return rc;
    return finish_tick(c, n_events, res, ev_status, nullptr, orphans, evicted);
}

int fb_purge(fb_ctx *c, double now, double tte, fb_tick_result *res, int64_t *orphans, int32_t *evicted) {
    if (!c) return FB_EINVAL;
    if (c->shard) return fail(c, FB_ESTATE, "fb_purge on a sharded context (fb_purge_launch + exchange)");
    int rc = fb_purge_launch(c, now, tte);
    if (rc) return rc;
    return finish_tick(c, 0, res, nullptr, nullptr, orphans, evicted);
}

int fb_assign(fb_ctx *c, double now, double tte, int64_t n_tasks, fb_tick_result *res, int32_t *assign,
              int64_t *orphans, int32_t *evicted) {
    if (!c) return FB_EINVAL;
    if (c->shard) return fail(c, FB_ESTATE, "fb_assign on a sharded context (use the two-phase tick)");
    int rc = fb_tick_launch(c, now, tte, 0, nullptr, nullptr, nullptr, nullptr, nullptr, n_tasks);
    if (rc) return rc;
    return finish_tick(c, 0, res, nullptr, assign, orphans, evicted);
}

int fb_tick(fb_ctx *c, double now, double tte, int32_t n_events, const uint8_t *kind, const int32_t *slot,
            const int32_t *val, const double *ts, const int64_t *seq, int64_t n_pending, fb_tick_result *res,
            uint8_t *ev_status, int32_t *assign, int64_t *orphans, int32_t *evicted) {
    int rc = fb_tick_launch(c, now, tte, n_events, kind, slot, val, ts, seq, n_pending);
    if (rc) return rc;
    fb_tick_result r;
    if ((rc = fb_tick_wait(c, &r))) return rc;
    if (ev_status && (rc = fb_get_event_status(c, n_events, ev_status))) return rc;
    if (assign && (rc = fb_get_assignments(c, 0, r.n_assigned, assign))) return rc;
    if (orphans && (rc = fb_get_orphans(c, r.n_orphans, orphans))) return rc;
    if (evicted && (rc = fb_get_evicted(c, r.n_evicted, evicted))) return rc;
    if (res) *res = r;
    return fb_tick_commit(c);
}

int fb_device_view_get(fb_ctx *c, fb_device_view *v) {
    if (!c || !v) return FB_EINVAL;
    if (int rc_ = enter(c, Call::device_view)) return rc_;
    v->free_processes = &c->free_[c->cur]->x;
    v->free_processes_stride = (int32_t)sizeof(int2);
    v->last_heartbeat = c->hb;
    v->last_heartbeat_stride = (int32_t)sizeof(double);
    v->registered = c->reg;
    if (c->win_cap && (c->qoff != 0 || c->Qn != c->Qtrue)) {
        if (int rc = win_normalize(c)) return rc;
    }
    v->queue = c->queue[c->qcur];
    if (int rc_ = log_settle(c)) return rc_;
    v->log_slot = c->log_slot;
    v->orphans = orph_dense_dev(c);
    if (life_waited(c->life)) {
        if (int rc = evict_ready(c)) return rc;
        HIPCHK(c, stream_wait(c));
    }
    v->evicted = c->l_cout ? c->cout_ev : c->evicted;
    v->n_workers = c->W;
    v->queue_len = c->Qn;
    v->log_head = c->head;
    return FB_OK;
}

int fb_set_full_assign(fb_ctx *c, int on) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::set_full_assign)) return rc_;
    c->full_assign = on ? 1 : 0;
    return FB_OK;
}

int fb_set_round_hint(fb_ctx *c, int32_t max_free) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::set_round_hint)) return rc_;
    c->maxc_hint = std::max<int32_t>(1, max_free);
    return FB_OK;
}

int fb_set_path(fb_ctx *c, const char *name, int value) {
    if (!c || !name) return FB_EINVAL;
    if (int rc_ = enter(c, Call::set_path)) return rc_;
    for (const PathKnob &k : kPathKnobs) {
        if (strcmp(name, k.name) || !knob_allows(k, value)) continue;
        // "lazy" off: the entries left so far leave the log first
        if (k.member == &PathKnobs::lazy_on && !value)
            if (int rc_ = log_settle(c)) return rc_;
        c->paths.*k.member = value;
        return FB_OK;
    }
    return fail(c, FB_EINVAL, "fb_set_path(\"%s\", %d): unknown path or value", name, value);
}

int fb_timing_enable(fb_ctx *c, int enable) {
    if (!c) return FB_EINVAL;
    c->timing = enable != 0;
    return FB_OK;
}

int fb_timing_gate(fb_ctx *c, int hold) {
    if (!c) return FB_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (hold) {
        if (c->gate_state == 1) return fail(c, FB_ESTATE, "fb_timing_gate: the gate is already held");
        if (!c->gate_h) {
            if (hipHostMalloc((void **)&c->gate_h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
                return fail(c, FB_ENOMEM, "fb_timing_gate: hipHostMalloc failed");
            memset(c->gate_h, 0, 64);
            HIPCHK(c, hipHostGetDevicePointer((void **)&c->gate_d, c->gate_h, 0));
            HIPCHK(c, hipEventCreate(&c->gate_a));
            HIPCHK(c, hipEventCreate(&c->gate_b));
        }
        // (a pending deferred commit stays pending: it rides in the next gated launch as usual)
        if (++c->gate_seq == 0) c->gate_seq = 1;
        __atomic_store_n(&c->gate_h[1], 0u, __ATOMIC_RELEASE);
        // the gate opens by itself after 0.5 s (5e7 ticks of the 100 MHz counter)
        launch_gate(c->gate_d, c->gate_seq, 50000000ull, Stream(c->stream, nullptr, c->gate_a));
        HIPCHK(c, hipGetLastError());
        c->gate_state = 1;
        return FB_OK;
    }
    if (c->gate_state != 1) return fail(c, FB_ESTATE, "fb_timing_gate(0) without a held gate");
    HIPCHK(c, hipEventRecord(c->gate_b, c->stream));
    __atomic_store_n(&c->gate_h[0], c->gate_seq, __ATOMIC_RELEASE);
    c->gate_state = 2;
    return FB_OK;
}

int fb_timing_mark(fb_ctx *c) {
    if (!c) return FB_EINVAL;
    if (c->gate_state == 1) return fail(c, FB_ESTATE, "fb_timing_mark while the gate is held");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->gate_h) {
        // (the gate's word, so the mark finds it open)
        if (int rc_ = fb_timing_gate(c, 1)) return rc_;
        return fb_timing_gate(c, 0);
    }
    launch_gate(c->gate_d, c->gate_seq, 50000000ull, Stream(c->stream));
    HIPCHK(c, hipGetLastError());
    return FB_OK;
}

int fb_timing_span(fb_ctx *c, double *ms, int32_t *timed_out) {
    if (!c) return FB_EINVAL;
    if (c->gate_state != 2) return fail(c, FB_ESTATE, "fb_timing_span without a released gate");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    float f = 0;
    HIPCHK(c, hipEventElapsedTime(&f, c->gate_a, c->gate_b));
    if (ms) *ms = f;
    if (timed_out) *timed_out = (int32_t)__atomic_load_n(&c->gate_h[1], __ATOMIC_ACQUIRE);
    return FB_OK;
}

int fb_timing_read(fb_ctx *c, int32_t max_kernels, const char **names, double *total_ms, int64_t *launches,
                   int32_t *n_kernels) {
    if (!c) return FB_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    std::vector<const char *> nm;
    std::vector<double> ms;
    std::vector<int64_t> cnt;
    for (auto &t : c->tl) {
        float f = 0;
        HIPCHK(c, hipEventElapsedTime(&f, t.a, t.b));
        size_t k = 0;
        while (k < nm.size() && strcmp(nm[k], t.name)) ++k;
        if (k == nm.size()) {
            nm.push_back(t.name);
            ms.push_back(0);
            cnt.push_back(0);
        }
        ms[k] += f;
        cnt[k] += 1;
        c->ev_pool.push_back(t.a);
        c->ev_pool.push_back(t.b);
    }
    c->tl.clear();
    const int n = (int)std::min<size_t>(nm.size(), (size_t)std::max(max_kernels, 0));
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = nm[i];
        if (total_ms) total_ms[i] = ms[i];
        if (launches) launches[i] = cnt[i];
    }
    if (n_kernels) *n_kernels = n;
    return FB_OK;
}

// Device self-test of the wave/block primitives (DPP scans); *errors = mismatches.
int fb_selftest(fb_ctx *c, int32_t *errors) {
    if (!c || !errors) return FB_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t *d = nullptr;
    int rc = dalloc(c, &d, 1);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(d, 0, 4, c->stream));
    for (uint32_t seed = 1; seed <= 8; ++seed) launch_selftest(d, seed * 7919u, c->stream);
    uint32_t h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, stream_wait(c));
    hipFree(d);
    *errors = (int32_t)h;
    return FB_OK;
}

// Diagnostic: copy the stamp buffer (meaningful only in FAASBAL_STAMPS builds).
int fb_debug_read(fb_ctx *c, unsigned long long *dst, int64_t n, int64_t *n_total) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::debug_read)) return rc_;
    HIPCHK(c, stream_wait(c));
    if (n_total) *n_total = (int64_t)c->dbg_n;
    if (dst && n > 0) HIPCHK(c, hipMemcpy(dst, c->dbg, (size_t)std::min<int64_t>(n, c->dbg_n) * 8, hipMemcpyDeviceToHost));
    return FB_OK;
}

int fb_sync(fb_ctx *c) {
    if (!c) return FB_EINVAL;
    if (int rc_ = enter(c, Call::sync)) return rc_;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, stream_wait(c));
    return FB_OK;
}

}  // extern "C"
