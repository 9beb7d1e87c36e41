// lr_probe -- fb_log_reclaim's launch plan (lr_plan, csrc/faasbal_layout.h) from the command
// line, no GPU.
//
// Reads "head below_seq W" per line on stdin and answers each with one line of key=value
// words: the plan's numbers, then the walk of its grids as the kernels index them --
//   flag.cover / take.cover  1: the tile workgroups' waves (tile = workgroup * kWaves + wave,
//                            entries [tile * kLcTile, ...) below B) gave every entry of the
//                            prefix exactly once and nothing at or past B
//   words.cover              1: every bitmap word a tile's wave writes (tile * kLcWords + lane,
//                            lane < kLcWords) is below nw, each once
// Built by tests/test_log_reclaim_host.py; it makes no HIP runtime call.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "faasbal_plan.h"

using namespace fb;

namespace {

bool tiles_cover(int grid, int nt, int64_t B) {
    std::vector<unsigned char> seen((size_t)B, 0);
    bool ok = true;
    for (int blk = 0; blk < grid; ++blk)
        for (int w = 0; w < kWaves; ++w) {
            const int tile = blk * kWaves + w;
            if (tile >= nt) continue;
            for (int64_t q = (int64_t)tile * kLcTile; q < (int64_t)(tile + 1) * kLcTile && q < B; ++q)
                ok = ok && ++seen[(size_t)q] == 1;
        }
    for (unsigned char c : seen) ok = ok && c == 1;
    return ok;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        long long head = 0, below = 0, W = 0;
        if (!(ss >> head >> below >> W)) continue;
        const LrPlan p = lr_plan(head, below, (int)W);
        bool words = true;
        {
            std::vector<unsigned char> seen((size_t)p.nw, 0);
            for (int t = 0; t < p.nt; ++t)
                for (int l = 0; l < kLcWords; ++l) {
                    const int64_t w = (int64_t)t * kLcWords + l;
                    words = words && w < p.nw && ++seen[(size_t)w] == 1;
                }
            for (unsigned char c : seen) words = words && c == 1;
        }
        std::printf("head=%lld below=%lld W=%lld B=%lld nt=%d nw=%lld tile=%d words_per_tile=%d flag_grid=%d scan_grid=%d"
                    " take_grid=%d bitmap=%zu wrel=%zu tcnt=%zu tpre=%zu mask=%zu seq=%zu slot=%zu bytes=%zu"
                    " flag.cover=%d take.cover=%d words.cover=%d\n",
                    head, below, W, (long long)p.B, p.nt, (long long)p.nw, kLcTile, kLcWords, p.flag_grid, p.scan_grid,
                    p.take_grid, p.tab.bits, p.tab.wrel, p.tab.tcnt, p.tab.tpre, p.mask, p.seq, p.slot, p.bytes,
                    (int)tiles_cover(p.flag_grid, p.nt, p.B), (int)tiles_cover(p.take_grid, p.nt, p.B), (int)words);
    }
    return 0;
}
