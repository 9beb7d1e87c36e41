// lc_probe -- fb_log_compact's launch plan (lc_plan, csrc/faasbal_layout.h) from the command
// line, no GPU.
//
// Reads "head W want_kept" per line on stdin and answers each with one line of key=value
// words: the plan's numbers, then the walk of its grids as the kernels index them --
//   flag.cover / move.cover  1: the tile workgroups' waves (tile = workgroup * kWaves + wave,
//                            entries [tile * kLcTile, ...) below head) gave every entry of the
//                            log exactly once and nothing else
//   slots.cover              1: k_lc_move's slot workgroups (through role_at) gave every slot
//                            exactly once
//   words.cover              1: every bitmap word a tile's wave writes (tile * kLcWords + lane,
//                            lane < kLcWords) is below nwl, each once
// Built by tests/test_log_compact_host.py; it makes no HIP runtime call.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "faasbal_plan.h"

using namespace fb;

namespace {

// the entries the waves of `grid` tile workgroups visit, counted per entry
bool tiles_cover(int grid, int nt, int64_t head) {
    std::vector<unsigned char> seen((size_t)head, 0);
    bool ok = true;
    for (int blk = 0; blk < grid; ++blk)
        for (int w = 0; w < kWaves; ++w) {
            const int tile = blk * kWaves + w;
            if (tile >= nt) continue;
            for (int64_t q = (int64_t)tile * kLcTile; q < (int64_t)(tile + 1) * kLcTile && q < head; ++q)
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
        long long head = 0, W = 0, want = 0;
        if (!(ss >> head >> W >> want)) continue;
        const LcPlan p = lc_plan(head, (int)W, want != 0);
        bool words = true;
        {
            std::vector<unsigned char> seen((size_t)p.nwl, 0);
            for (int t = 0; t < p.ntl; ++t)
                for (int l = 0; l < kLcWords; ++l) {
                    const int64_t w = (int64_t)t * kLcWords + l;
                    words = words && w < p.nwl && ++seen[(size_t)w] == 1;
                }
            for (unsigned char c : seen) words = words && c == 1;
        }
        bool slots = true;
        int tile_wgs = 0;
        {
            std::vector<unsigned char> seen((size_t)W, 0);
            for (int blk = 0; blk < p.move.grid(); ++blk) {
                const Role r = role_at(p.move, blk);
                if (r.role == kLcMoveTiles) {
                    slots = slots && r.idx == blk;  // (the kernel reads its tiles from blockIdx.x)
                    ++tile_wgs;
                } else if (r.role == kLcMoveSlots) {
                    slots = slots && r.idx == p.move.rel(kLcMoveSlots, blk);
                    for (int t = 0; t < kBS; ++t) {
                        const long long s = (long long)r.idx * kBS + t;
                        if (s < W) slots = slots && ++seen[(size_t)s] == 1;
                    }
                } else {
                    slots = false;
                }
            }
            for (unsigned char c : seen) slots = slots && c == 1;
        }
        std::printf("head=%lld W=%lld nt=%d nw=%lld tile=%d words_per_tile=%d flag_grid=%d scan_grid=%d move_grid=%d"
                    " move_tiles=%d move_slots=%d bitmap=%zu wrel=%zu tcnt=%zu tpre=%zu dst=%zu kept=%zu bytes=%zu"
                    " flag.cover=%d move.cover=%d slots.cover=%d words.cover=%d\n",
                    head, W, p.ntl, (long long)p.nwl, kLcTile, kLcWords, p.flag_grid, p.scan_grid, p.move.grid(),
                    p.move.count(kLcMoveTiles), p.move.count(kLcMoveSlots), p.loc.bits, p.loc.wrel, p.loc.tcnt, p.loc.tpre, p.dst,
                    p.kept, p.bytes, (int)tiles_cover(p.flag_grid, p.ntl, head),
                    (int)(tile_wgs == p.move.count(kLcMoveTiles) && tiles_cover(tile_wgs, p.ntl, head)), (int)slots,
                    (int)words);
    }
    return 0;
}
