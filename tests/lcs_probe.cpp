// lcs_probe -- a shard group compaction's launch plan (lcs_plan, csrc/faasbal_layout.h) from
// the command line, no GPU.
//
// Reads "head head_local W want_kept" per line on stdin and answers each with one line of
// key=value words: the plan's numbers, then the walk of its grids as the kernels index them --
//   flag.cover / move.cover  1: the local tile workgroups' waves (tile = workgroup * kWaves +
//                            wave) gave every entry of the shard exactly once and nothing else
//   mark.cover               1: k_lcs_mark's threads (word = workgroup * kBS + thread) gave
//                            every word of the exchange bitmap exactly once
//   count.cover / kept.cover 1: the global tile workgroups' waves and their lanes < kLcWords
//                            gave every word of the exchange bitmap exactly once (kept: through
//                            role_at; without want_kept: no such workgroup)
//   slots.cover              1: k_lc_move's slot workgroups (through role_at) gave every slot
//                            exactly once
// Built by tests/test_log_compact_shard_host.py; it makes no HIP runtime call.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "faasbal_plan.h"

using namespace fb;

namespace {

// the entries the waves of `grid` tile workgroups visit, counted per entry
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

// the bitmap words the waves of `grid` tile workgroups visit (lane < kLcWords), counted per word
bool words_cover(int grid, int nt, int64_t nw) {
    std::vector<unsigned char> seen((size_t)nw, 0);
    bool ok = true;
    for (int blk = 0; blk < grid; ++blk)
        for (int w = 0; w < kWaves; ++w) {
            const int tile = blk * kWaves + w;
            if (tile >= nt) continue;
            for (int l = 0; l < kLcWords; ++l) {
                const int64_t x = (int64_t)tile * kLcWords + l;
                ok = ok && x < nw && ++seen[(size_t)x] == 1;
            }
        }
    for (unsigned char c : seen) ok = ok && c == 1;
    return ok;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        long long head = 0, hl = 0, W = 0, want = 0;
        if (!(ss >> head >> hl >> W >> want)) continue;
        const LcPlan p = lcs_plan(head, hl, (int)W, want != 0);
        bool mark = true;
        {
            std::vector<unsigned char> seen((size_t)p.nwg, 0);
            for (int blk = 0; blk < p.mark_grid; ++blk)
                for (int t = 0; t < kBS; ++t) {
                    const int64_t w = (int64_t)blk * kBS + t;
                    if (w < p.nwg) mark = mark && ++seen[(size_t)w] == 1;
                }
            for (unsigned char c : seen) mark = mark && c == 1;
        }
        bool slots = true, order = true;
        int tile_wgs = 0, kept_wgs = 0;
        {
            std::vector<unsigned char> seen((size_t)W, 0);
            for (int blk = 0; blk < p.move.grid(); ++blk) {
                const Role r = role_at(p.move, blk);
                if (r.role == kLcMoveTiles) {
                    order = order && r.idx == blk;  // (the kernel reads its local tiles from blockIdx.x)
                    ++tile_wgs;
                } else if (r.role == kLcMoveSlots) {
                    order = order && r.idx == p.move.rel(kLcMoveSlots, blk);
                    for (int t = 0; t < kBS; ++t) {
                        const long long s = (long long)r.idx * kBS + t;
                        if (s < W) slots = slots && ++seen[(size_t)s] == 1;
                    }
                } else if (r.role == kLcMoveKept) {
                    order = order && r.idx == p.move.rel(kLcMoveKept, blk) && r.idx == kept_wgs;
                    ++kept_wgs;
                } else {
                    order = false;
                }
            }
            for (unsigned char c : seen) slots = slots && c == 1;
        }
        const bool kept = want ? (kept_wgs == p.move.count(kLcMoveKept) && words_cover(kept_wgs, p.ntg, p.nwg)) : kept_wgs == 0;
        std::printf("head=%lld head_local=%lld W=%lld ntl=%d ntg=%d nwl=%lld nwg=%lld tile=%d words_per_tile=%d"
                    " flag_grid=%d mark_grid=%d count_grid=%d scan_grid=%d move_grid=%d move_tiles=%d move_slots=%d"
                    " move_kept=%d lbitmap=%zu lwrel=%zu ltcnt=%zu ltpre=%zu keep=%zu gwrel=%zu gtcnt=%zu gtpre=%zu"
                    " dst=%zu dseq=%zu kept=%zu bytes=%zu xbytes=%lld"
                    " flag.cover=%d move.cover=%d mark.cover=%d count.cover=%d kept.cover=%d slots.cover=%d order=%d\n",
                    head, hl, W, p.ntl, p.ntg, (long long)p.nwl, (long long)p.nwg, kLcTile, kLcWords, p.flag_grid,
                    p.mark_grid, p.count_grid, p.scan_grid, p.move.grid(), p.move.count(kLcMoveTiles),
                    p.move.count(kLcMoveSlots), p.move.count(kLcMoveKept), p.loc.bits, p.loc.wrel, p.loc.tcnt,
                    p.loc.tpre, p.keep, p.glob.wrel, p.glob.tcnt, p.glob.tpre, p.dst, p.dseq, p.kept, p.bytes, (long long)p.xbytes,
                    (int)(tiles_cover(p.flag_grid, p.ntl, hl) && words_cover(p.flag_grid, p.ntl, p.nwl)),
                    (int)(tile_wgs == p.move.count(kLcMoveTiles) && tiles_cover(tile_wgs, p.ntl, hl)), (int)mark,
                    (int)words_cover(p.count_grid, p.ntg, p.nwg), (int)kept, (int)slots, (int)order);
    }
    return 0;
}
