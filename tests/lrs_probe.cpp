// lrs_probe -- fb_log_reclaim_shard's launch plan (lrs_plan, csrc/faasbal_layout.h) from the
// command line, no GPU.
//
// Reads "head_local W" per line on stdin and answers each with one line of key=value words:
// the plan's numbers, then the walk of its grids as the kernels index them --
//   flag.cover / take.cover  1: the tile workgroups' waves (tile = workgroup * kWaves + wave,
//                            entries [tile * kLcTile, ...) below head_local) gave every local
//                            entry exactly once and nothing past the shard
//   words.cover              1: every bitmap word a tile's wave writes (tile * kLcWords + lane,
//                            lane < kLcWords) is below nw, each once
//   lists                    the entries each of the two lists holds (the count's bound)
//   regions.ok               1: the regions, in the order table / mask / seq / slot, each hold
//                            what the passes touch, are 256-byte aligned, do not overlap and
//                            end inside `bytes`
// Built by tests/test_log_reclaim_shard_host.py; it makes no HIP runtime call.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "faasbal_plan.h"

using namespace fb;

namespace {

bool tiles_cover(int grid, int nt, int64_t n) {
    std::vector<unsigned char> seen((size_t)n, 0);
    bool ok = true;
    for (int blk = 0; blk < grid; ++blk)
        for (int w = 0; w < kWaves; ++w) {
            const int tile = blk * kWaves + w;
            if (tile >= nt) continue;
            for (int64_t q = (int64_t)tile * kLcTile; q < (int64_t)(tile + 1) * kLcTile && q < n; ++q)
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
        long long hl = 0, W = 0;
        if (!(ss >> hl >> W)) continue;
        const LrPlan p = lrs_plan(hl, (int)W);
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
        // the regions front to back: what each pass touches of them
        const size_t at[] = {p.tab.bits, p.tab.wrel, p.tab.tcnt, p.tab.tpre, p.mask, p.seq, p.slot};
        const size_t need[] = {(size_t)p.nw * 8, (size_t)p.nw * 4, (size_t)p.nt * 4, ((size_t)p.nt + 1) * 4,
                               (size_t)(W > 0 ? W : 0), (size_t)hl * 8, (size_t)hl * 4};
        bool regions = true;
        size_t end = 0;
        for (int i = 0; i < 7; ++i) {
            regions = regions && at[i] >= end && at[i] % 256 == 0;
            end = at[i] + need[i];
        }
        regions = regions && end <= p.bytes;
        std::printf("head_local=%lld W=%lld lists=%lld nt=%d nw=%lld tile=%d words_per_tile=%d flag_grid=%d scan_grid=%d"
                    " take_grid=%d bitmap=%zu wrel=%zu tcnt=%zu tpre=%zu mask=%zu seq=%zu slot=%zu bytes=%zu"
                    " flag.cover=%d take.cover=%d words.cover=%d regions.ok=%d\n",
                    hl, W, (long long)p.B, p.nt, (long long)p.nw, kLcTile, kLcWords, p.flag_grid, p.scan_grid, p.take_grid,
                    p.tab.bits, p.tab.wrel, p.tab.tcnt, p.tab.tpre, p.mask, p.seq, p.slot, p.bytes,
                    (int)tiles_cover(p.flag_grid, p.nt, hl), (int)tiles_cover(p.take_grid, p.nt, hl), (int)words,
                    (int)regions);
    }
    return 0;
}
