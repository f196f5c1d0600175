// The CARAFE kernels' launch policy (csrc/carafe_plan.h) on the host, with the tuning structure the library reads (cswin_tuning(),
// so CSWIN_CARAFE_GENERIC acts here as it does there).  Reads one request per line from stdin and prints one line for each:
//   tok B H W Cz S            ->  tok lpr groups grid                      (cswin_carafe_fwd)
//   planes B H W Cz C S       ->  planes ppb grid                          (cswin_carafe_fwd_nchw)
//   bwd B H W Cz S            ->  bwd route lpr groups chunks grid_e grid_z colsum_lanes colsum_rgroups colsum_grid
//                                 tiles_x tiles_y grid_fused part_rows ws_bytes          (cswin_carafe_bwd and its workspace query)
//   bwd_planes B H W Cz C S   ->  the same record, as cswin_carafe_bwd_nchw launches it (the tuning flag does not apply)
//   colsum rows C             ->  colsum lanes rgroups grid                (colsum_partial_kernel wherever it is launched)
//   limits                    ->  limits threads grid_clamp colsum_clamp colsum_rows bias_in_e_cz e_chunks e_stage_chunk_floats
//                                 e_stage_bytes fused_threads fused_tile fused_lds_bytes lds_plain
// or `refused <name>` where the entry point returns an error code.  route: fused, bias_in_e or colsum; fields of a route that is
// not taken are 0.  tests/test_carafe_plan_host.py compares the Python transcription of tests/test_gpu_carafe_shapes.py with this.
//   c++ -O1 -std=c++17 -I cswin_unet_amd/csrc tools/carafe_plan_check.cpp -o carafe_plan_check
#include <cstdio>
#include <iostream>
#include <string>

#include "carafe_plan.h"
#include "tuning.h"

static void print_bwd(const cp::BwdPlan& p, size_t ws_bytes) {
    std::printf("bwd %s %d %d %d %d %d %d %d %d %d %d %d %d %zu\n", cp::route_name(p.route), p.lpr, p.groups, p.chunks, p.grid_e, p.grid_z,
                p.colsum.lanes, p.colsum.rgroups, p.colsum.grid, p.tiles_x, p.tiles_y, p.grid_fused, p.part_rows, ws_bytes);
}

int main() {
    std::ios::sync_with_stdio(false);
    const bool generic_only = cswin_tuning().carafe_generic != 0;
    std::string tag;
    while (std::cin >> tag) {
        int B = 0, H = 0, W = 0, Cz = 0, C = 0, S = 0;
        long rows = 0;
        cp::Refusal r = cp::Refusal::none;
        if (tag == "limits") {
            std::printf("limits %d %d %d %d %d %d %d %zu %d %d %zu %zu\n", cp::THREADS, cp::GRID_CLAMP, cp::COLSUM_CLAMP, cp::COLSUM_ROWS, cp::BIAS_IN_E_CZ,
                        cp::E_CHUNKS, cp::e_stage_chunk_floats(), cp::e_stage_floats() * sizeof(float), cp::F_THREADS, cp::F_TILE,
                        cp::fused_lds_bytes(), cp::LDS_PLAIN);
            continue;
        }
        const bool planes = tag == "planes" || tag == "bwd_planes";
        if (tag == "colsum") std::cin >> rows >> C;
        else if (planes) std::cin >> B >> H >> W >> Cz >> C >> S;
        else if (tag == "tok" || tag == "bwd") std::cin >> B >> H >> W >> Cz >> S;
        else std::cin.setstate(std::ios::failbit);
        if (!std::cin || (tag == "colsum" && C <= 0)) {
            std::fprintf(stderr, "carafe_plan_check: bad request\n");
            return 1;
        }
        if (tag == "tok" || tag == "bwd") r = cp::refusal(B, H, W, Cz, S);
        else if (tag == "planes") r = cp::planes_refusal(B, H, W, Cz, C, S);
        else if (tag == "bwd_planes") r = cp::bwd_planes_refusal(B, H, W, Cz, C, S);
        if (r != cp::Refusal::none) {
            std::printf("refused %s\n", cp::refusal_name(r));
        } else if (tag == "tok") {
            const cp::FwdTokens f = cp::fwd_tokens(B, H, W, Cz, S);
            std::printf("tok %d %d %d\n", f.lpr, f.groups, f.grid);
        } else if (tag == "planes") {
            const cp::FwdPlanes f = cp::fwd_planes(B, H, W, S);
            std::printf("planes %d %d\n", f.ppb, f.grid);
        } else if (tag == "colsum") {
            const cp::Colsum c = cp::colsum_plan(rows, C);
            std::printf("colsum %d %d %d\n", c.lanes, c.rgroups, c.grid);
        } else {
            print_bwd(cp::bwd_plan(tag == "bwd" && generic_only, B, H, W, Cz, S), cp::bwd_workspace(B, H, W, Cz, S));
        }
    }
    return 0;
}
