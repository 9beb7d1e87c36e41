// faasbal_fill.h -- internal, host and device: the water-filling closed form, stated once.
//
// With c = max(free, 1) per live queued worker, A(r) = #{c > r} and S(r) = sum_{q < r} A(q)
// (= sum min(c, r)), a tick of N tasks ends at the fill level L, the largest r with
// S(r) <= N: rounds r < L are served in full, round L to its first p = N - S(L) workers
// (LRU order), and the next queue is round L's unserved workers followed by the served
// ones that still have a free process (round L + 1).  Every emission kernel finds L, S(L)
// and A(L) from the round table its own way (faasbal_kernels.hip: fill_scan in wave
// registers, k_emit through LDS, k_emit_shard_wide chunk by chunk) and takes everything
// else from here; tests/test_fill_cases.py runs these functions on the CPU
// (tests/fill_probe.cpp).  No HIP runtime call.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#define FB_HD __host__ __device__ __forceinline__

namespace fb {

// ---- the tick's demand.  A table of R rows knows A(r) for r < rlim only; with a worker
// beyond it (max c > R) the capacity sum of c is unknown and nothing caps N.
struct FillDemand {
    int rlim;       // rounds of the table that count: min(max c, R)
    int64_t cap;    // sum of c over the live queued workers (INT64_MAX: beyond the table)
    int64_t N_eff;  // tasks dispatched: min(N, cap)
};
FB_HD FillDemand fill_demand(int maxc, int R, int64_t cap, int64_t O, int64_t T, bool redist) {
    if (maxc > R) cap = INT64_MAX;
    const int64_t N = (redist ? O : 0) + T;  // purge-only ticks report orphans, dispatch none
    return {maxc < R ? maxc : R, cap, N < cap ? N : cap};
}

// ---- the verdict on a fill level found in a table of R rows.  The emission reads rounds L
// and L + 1, so with a worker beyond the table the level is exact while L <= R - 2; from
// L = R - 1 on the tick asks for a wider table (status 1).  Status 1 (every rank of a shard
// group sees it, all relaunch) comes before status 2 (this rank's log is full), whose
// N_eff is exact only once the table is wide enough -- so the ranks never split between a
// relaunch and a failure, and the log is never written past its end.
struct FillVerdict {
    int status;  // HostOut::status: 0, 1 = table too narrow, 2 = in-flight log full
    int64_t p;   // tasks of the partial round L
    int64_t AL;  // |A_L| (0: every worker saturated below L)
};
FB_HD FillVerdict fill_verdict(int maxc, int R, int rlim, int L, int64_t S_L, int64_t A_at_L, int64_t N_eff,
                               int64_t head, int64_t log_cap) {
    const int status = (maxc > R && L >= R - 1) ? 1 : (head + N_eff > log_cap ? 2 : 0);
    // (A_at_L: the table's row L, read only where it exists; rlim <= max c)
    return {status, N_eff - S_L, L < rlim ? A_at_L : 0};
}

// ---- the next state of a queue position with c > 0: rankL its rank in A_L (meaningful
// when c > L), exL1 its rank in A_{L+1} (when c > L + 1).
struct FillNext {
    int64_t n_q;     // tasks it takes this tick
    int64_t np;      // its index in the next queue (-1: it leaves the queue)
    bool takes_L;    // served in the partial round L
    bool sets_qlen;  // the one position of rank p in A_L: it knows the next queue's length
    int64_t qlen;    // ... which is this
};
FB_HD FillNext fill_next(int c, int L, int64_t rankL, int64_t p, int64_t AL, int64_t exL1) {
    const bool inL = c > L, takes_L = inL && rankL < p;
    const int64_t qlen = (AL - p) + exL1;
    int64_t np = -1;
    if (inL && !takes_L) np = rankL - p;
    else if (c > L + 1) np = qlen;
    return {(int64_t)(c < L ? c : L) + (takes_L ? 1 : 0), np, takes_L, inL && rankL == p, qlen};
}

}  // namespace fb

#undef FB_HD
