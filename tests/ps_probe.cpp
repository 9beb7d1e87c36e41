// ps_probe -- fb_pool_stats' launch plan (ps_plan, csrc/faasbal_layout.h) from the command
// line, no GPU.
//
// Reads "W Qn qoff head" per line on stdin and answers each with one line of key=value
// words: the plan's numbers, then the walk of its grids as the kernels index them --
//   slots.cover  1: k_ps_slots' slot workgroups (through role_at; kPsTiles tiles of kBS
//                slots, slot = workgroup * kPsSpan + tile * kBS + thread) gave every slot
//                below W exactly once and nothing else
//   queue.cover  1: its queue workgroups gave every position of the window
//                [qoff, qoff + Qn) exactly once and nothing else
//   xbits.cover  1: the bitmap words the slot workgroups' waves write (one per wave and tile,
//                those that begin below W) are the words [0, nxw), each once
//   log.cover    1: k_ps_log's waves (tile = workgroup * kWaves + wave, entries
//                [tile * kLcTile, ...) below head) gave every log entry exactly once
//   rows.cover   1: every workgroup of the three roles owns one row of its region, below the
//                region's row count
// Built by tests/test_pool_stats_host.py; it makes no HIP runtime call.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "faasbal_plan.h"

using namespace fb;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        long long W = 0, Qn = 0, qoff = 0, head = 0;
        if (!(ss >> W >> Qn >> qoff >> head)) continue;
        const PsPlan p = ps_plan((int)W, Qn, head);
        bool slots = true, queue = true, xbits = true, rows = true;
        {
            std::vector<unsigned char> seen((size_t)W, 0), qseen((size_t)(qoff + Qn), 0), wseen((size_t)p.nxw, 0);
            std::vector<unsigned char> srow((size_t)p.slots.count(kPsSlotsSlots), 0), qrow((size_t)p.slots.count(kPsSlotsQueue), 0);
            for (int blk = 0; blk < p.slots.grid(); ++blk) {
                const Role r = role_at(p.slots, blk);
                if (r.role == kPsSlotsSlots) {
                    slots = slots && r.idx == blk;  // (the kernel reads its slots from blockIdx.x)
                    rows = rows && r.idx < (int)srow.size() && ++srow[(size_t)r.idx] == 1;
                    for (int k = 0; k < kPsTiles; ++k) {
                        for (int t = 0; t < kBS; ++t) {
                            const long long s = (long long)r.idx * kPsSpan + k * kBS + t;
                            if (s < W) slots = slots && ++seen[(size_t)s] == 1;
                        }
                        for (int w = 0; w < kWaves; ++w) {
                            const long long word = ((long long)r.idx * kPsSpan + k * kBS + w * 64) >> 6;
                            if (word * 64 < W) xbits = xbits && word < p.nxw && ++wseen[(size_t)word] == 1;
                        }
                    }
                } else if (r.role == kPsSlotsQueue) {
                    queue = queue && r.idx == p.slots.rel(kPsSlotsQueue, blk);
                    rows = rows && r.idx < (int)qrow.size() && ++qrow[(size_t)r.idx] == 1;
                    for (int k = 0; k < kPsTiles; ++k)
                        for (int t = 0; t < kBS; ++t) {
                            const long long pos = (long long)r.idx * kPsSpan + k * kBS + t;
                            // the kernel's masked positions: queue[qoff + pos] for pos < Qn
                            if (pos < Qn) queue = queue && ++qseen[(size_t)(qoff + pos)] == 1;
                        }
                } else {
                    slots = queue = false;
                }
            }
            for (unsigned char c : seen) slots = slots && c == 1;
            for (size_t i = 0; i < qseen.size(); ++i) queue = queue && qseen[i] == (i >= (size_t)qoff ? 1 : 0);
            for (unsigned char c : wseen) xbits = xbits && c == 1;
            for (unsigned char c : srow) rows = rows && c == 1;
            for (unsigned char c : qrow) rows = rows && c == 1;
        }
        bool log = true;
        {
            std::vector<unsigned char> seen((size_t)head, 0);
            for (int blk = 0; blk < p.log_grid; ++blk)
                for (int w = 0; w < kWaves; ++w) {
                    const int tile = blk * kWaves + w;
                    if (tile >= p.nt) continue;
                    for (int64_t q = (int64_t)tile * kLcTile; q < (int64_t)(tile + 1) * kLcTile && q < head; ++q)
                        log = log && ++seen[(size_t)q] == 1;
                }
            for (unsigned char c : seen) log = log && c == 1;
        }
        std::printf("W=%lld Qn=%lld qoff=%lld head=%lld nt=%d nxw=%lld span=%d tile=%d cols=%d qcols=%d lcols=%d used=%d"
                    " slot_wgs=%d queue_wgs=%d slots_grid=%d log_grid=%d fold_grid=%d fold_threads=%d"
                    " xbits=%zu srow=%zu qrow=%zu lrow=%zu bytes=%zu"
                    " slots.cover=%d queue.cover=%d xbits.cover=%d log.cover=%d rows.cover=%d\n",
                    W, Qn, qoff, head, p.nt, (long long)p.nxw, kPsSpan, kLcTile, kPsCols, kPsQCols, kPsLCols, (int)kPsUsed,
                    p.slots.count(kPsSlotsSlots), p.slots.count(kPsSlotsQueue), p.slots.grid(), p.log_grid, p.fold_grid,
                    kPsFoldBS, p.xbits, p.srow, p.qrow, p.lrow, p.bytes, (int)slots, (int)queue, (int)xbits, (int)log,
                    (int)rows);
    }
    return 0;
}
