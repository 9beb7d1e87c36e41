// fill_probe -- the water-filling closed form (csrc/faasbal_fill.h) from the command line, no GPU.
//
// Reads one tick per line on stdin:
//   R maxc cap O T redist head log_cap  nA A[0] .. A[nA-1]  nq c[0] .. c[nq-1]
// A: the round table's rows that count (nA = min(maxc, R), A[r] = positions with c > r); c: the
// logical queue in LRU order (0 = no live worker at the position).  The fill level comes from a
// plain sequential search of the table, everything else from fill_demand, fill_verdict and --
// for a tick without a status, as the kernels return early with one -- fill_next of every
// position with its ranks in A_L and A_{L+1} (the live positions before it with c > L, c > L + 1).
// Answers one line of key=value words; next = the next queue as positions of c, qlen = the
// length the one position of rank p reported (-1: nobody did).
// Built by tests/test_fill_cases.py; it makes no HIP runtime call.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "faasbal_fill.h"

using namespace fb;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        long long R, maxc, cap, O, T, redist, head, log_cap, nA, nq;
        if (!(in >> R >> maxc >> cap >> O >> T >> redist >> head >> log_cap >> nA)) {
            std::puts("error=header");
            continue;
        }
        std::vector<long long> A(nA);
        for (auto &x : A) in >> x;
        in >> nq;
        std::vector<long long> c(in ? nq : 0);
        for (auto &x : c) in >> x;
        const FillDemand d = fill_demand((int)maxc, (int)R, cap, O, T, redist != 0);
        if (!in || d.rlim != nA) {
            std::puts("error=table");
            continue;
        }
        int L = 0;
        int64_t S_L = 0;
        while (L < d.rlim && S_L + A[L] <= d.N_eff) S_L += A[L++];
        const FillVerdict v =
            fill_verdict((int)maxc, (int)R, d.rlim, L, S_L, L < d.rlim ? A[L] : 0, d.N_eff, head, log_cap);
        std::printf("L=%d S_L=%lld rlim=%d cap=%lld N_eff=%lld status=%d p=%lld AL=%lld", L, (long long)S_L, d.rlim,
                    (long long)d.cap, (long long)d.N_eff, v.status, (long long)v.p, (long long)v.AL);
        if (v.status) {
            std::puts("");
            continue;
        }
        long long rL = 0, rL1 = 0, served = 0, qlen = -1, setters = 0, partial = 0;
        std::vector<long long> next(nq, -1);
        bool ok = true;
        for (long long pos = 0; pos < nq; ++pos) {
            if (c[pos] <= 0) continue;
            const FillNext nx = fill_next((int)c[pos], L, rL, v.p, v.AL, rL1);
            served += nx.n_q;
            partial += nx.takes_L;
            if (nx.sets_qlen) {
                qlen = nx.qlen;
                ++setters;
            }
            if (nx.np >= 0) {
                if (nx.np >= nq || next[nx.np] >= 0) ok = false;  // outside the queue, or taken twice
                else next[nx.np] = pos;
            }
            rL += c[pos] > L;
            rL1 += c[pos] > L + 1;
        }
        long long placed = 0;
        for (long long i = 0; i < nq; ++i) placed += next[i] >= 0;
        for (long long i = 0; i < placed; ++i) ok = ok && next[i] >= 0;  // no hole: indices 0 .. placed - 1
        std::printf(" served=%lld partial=%lld qlen=%lld setters=%lld ok=%d next=", served, partial, qlen, setters, ok);
        for (long long i = 0; i < placed && next[i] >= 0; ++i) std::printf(i ? ",%lld" : "%lld", next[i]);
        std::puts("");
    }
    return 0;
}
