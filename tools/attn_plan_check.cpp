// The attention kernels' launch policy (csrc/attn_plan.h) on the host, with the tuning structure the library reads (cswin_tuning(),
// so CSWIN_ATTN_FWD_QSPLIT and CSWIN_ATTN_BWD_TWO_PASS act here as they do there).  Reads one request per line from stdin,
//   B reso C nbranch heads[nbranch] idx[nbranch] split
// and prints one line for each: `refused <name>` (a refusal of the geometry, or window_tokens: no forward instantiation), or
//   N nt nwg hd thin | family NT QS threads grid lds | path NT|nblk slab_rows ds_stride vs_floats lds lds_reserved grids... |
//   ws_bytes slab offsets... delta offset
// (family fwd3 / fwd; path bwd3 with its NT and one grid, or two_pass with nblk and four grids; sizes in bytes, offsets in floats).
// tests/test_attn_plan_host.py compares the Python transcription of tests/test_gpu_attn_shapes.py with this output.
//   c++ -O1 -std=c++17 -I cswin_unet_amd/csrc tools/attn_plan_check.cpp -o attn_plan_check
#include <cstdio>
#include <iostream>

#include "attn_plan.h"

int main() {
    std::ios::sync_with_stdio(false);
    const CswinTuning& t = cswin_tuning();
    int B, reso, C, nbranch;
    while (std::cin >> B >> reso >> C >> nbranch) {
        int heads[ap::MAX_BRANCH] = {}, idx[ap::MAX_BRANCH] = {}, split;
        const int n = nbranch == 2 ? 2 : 1;           // any other count is refused below; one value each is still read
        for (int i = 0; i < n; ++i) std::cin >> heads[i];
        for (int i = 0; i < n; ++i) std::cin >> idx[i];
        if (!(std::cin >> split)) {
            std::fprintf(stderr, "attn_plan_check: bad request\n");
            return 1;
        }
        const ap::Geometry g = ap::geometry(B, reso, C, nbranch, heads, idx, split);
        if (g.refusal != ap::Refusal::none) {
            std::printf("refused %s\n", ap::refusal_name(g.refusal));
            continue;
        }
        const ap::FwdPlan f = ap::fwd_plan(t, g);
        if (f.refusal != ap::Refusal::none) {
            std::printf("refused %s\n", ap::refusal_name(f.refusal));
            continue;
        }
        const ap::BwdPlan b = ap::bwd_plan(t, g, B, reso, nbranch);
        std::printf("%d %d %d %d %d | %s %d %d %d %d %zu |", g.N, g.nt, g.nwg, g.hd, (int)g.thin, f.family == ap::Family::fwd3 ? "fwd3" : "fwd",
                    f.NT, f.QS, f.threads, f.grid, f.lds);
        if (b.path == ap::BwdPath::bwd3)
            std::printf(" bwd3 %d %d %d %d %zu %zu %u |", b.NT, b.slab_rows, b.ds_stride, b.vs_floats, b.lds, b.lds_reserved, b.grid[0]);
        else
            std::printf(" two_pass %d %d %d %d %zu %zu %u %u %u %u |", b.nblk, b.slab_rows, b.ds_stride, b.vs_floats, b.lds, b.lds_reserved,
                        b.grid[0], b.grid[1], b.grid[2], b.grid[3]);
        std::printf(" %zu", b.ws_bytes);
        for (int i = 0; i < nbranch; ++i) std::printf(" %zu", b.slab_off[i]);
        std::printf(" %zu\n", b.delta_off);
    }
    return 0;
}
