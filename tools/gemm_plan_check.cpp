// The GEMM family's launch policy (csrc/gemm_plan.h) on the host, with the tuning structure the library reads (cswin_tuning(), so the
// CSWIN_* tuning variables act here as they do there).  Reads one request per line from stdin and prints the plan of each in
// the vocabulary of tests/test_gpu_gemm_shapes.py's plan_str, the kernel's name first; tests/test_gemm_plan_host.py compares the
// Python transcription of that file with this output.  Alignment flags are 1 = every such operand starts 16-B aligned.
//   fwd   M N K k_split precision io_bf16 loads outs           cswin_linear_fwd (k_split 0: no concat input)
//   dgrad M N K k_split add precision io_bf16 loads outs       cswin_linear_bwd_data (k_split: the dx | dx2 seam; add 0 / 1)
//   dw    M N K k_split precision loads x2 workspace           the stand-alone cswin_linear_bwd_weight
//   tiled Mo No R splits rows wgrad precision                  a raw configuration of the tiled family (the convolutions): tile only
//   batch n precision  n x (M N K io_bf16 rows_per_sample mask loads workspace ws_bytes)  dgrad tM tN tK tloads tdx order njobs
//         cswin_linear_bwd_weight_batch / cswin_linear_bwd_tail and their masked / skip forms.  rows_per_sample 0: no row scale;
//         ws_bytes -1: what cswin_linear_bwd_weight_workspace says; dgrad 0: no data gradient (the next six fields are still read).
//         Prints the problems' plans and the data gradient's (or "-"), " | " between them, then " ; " and the route.
//   c++ -O1 -std=c++17 -I cswin_unet_amd/csrc tools/gemm_plan_check.cpp -o gemm_plan_check
#include <cstdio>
#include <iostream>
#include <string>

#include "gemm_plan.h"

static std::string slabs(const gp::Plan& p) {
    return " " + std::to_string(p.splits) + "x" + std::to_string(p.rows) + "(" + std::to_string(p.last) + ")";
}
static std::string tile_str(const gp::Plan& p) {
    return std::to_string(p.bm) + "x" + std::to_string(p.bn) + "x" + std::to_string(p.bk) + " KW" + std::to_string(p.kw);
}
static std::string plan_str(const gp::Plan& p) {
    switch (p.kernel) {
        case gp::Kernel::gemm16:
            return "gemm16 " + std::to_string(p.bm) + "x64 S" + std::to_string(p.stages) + " last" + std::to_string(p.last_step);
        case gp::Kernel::wgrad16: return std::string(p.dma ? "wgrad16 dma" : "wgrad16 reg") + slabs(p);
        default: break;
    }
    const char* name = p.kernel == gp::Kernel::batch ? "batch " : p.kernel == gp::Kernel::tail ? "tail " : "tiled ";
    std::string s = name + tile_str(p) + " V" + std::to_string(p.vec) + " E" + std::to_string(p.store);
    return p.kernel != gp::Kernel::tiled || p.wgrad ? s + slabs(p) : s;
}

int main() {
    std::ios::sync_with_stdio(false);
    const CswinTuning& t = cswin_tuning();
    static const char* const routes[] = {"separate", "wgrad16", "plain", "masked", "tail", "tail_masked", "tail_order"};
    std::string what;
    while (std::cin >> what) {
        int M, N, K, ks, prec, io, a, b, c;
        if (what == "fwd" && std::cin >> M >> N >> K >> ks >> prec >> io >> a >> b) {
            std::puts(plan_str(gp::linear_fwd_plan(t, M, N, K, ks, prec, io, a, b)).c_str());
        } else if (what == "dgrad" && std::cin >> M >> N >> K >> ks >> c >> prec >> io >> a >> b) {
            std::puts(plan_str(gp::linear_dgrad_plan(t, M, N, K, ks, c, prec, io, a, b)).c_str());
        } else if (what == "dw" && std::cin >> M >> N >> K >> ks >> prec >> a >> b >> c) {
            gp::WgradProblem p = {};
            p.M = M; p.N = N; p.K = K;
            p.loads_aligned = a; p.ws_aligned = c;
            p.ws_bytes = gp::wgrad_workspace_bytes(t, M, N, K);
            std::puts(plan_str(gp::linear_wgrad_plan(t, p, ks, prec, b)).c_str());
        } else if (what == "tiled" && std::cin >> M >> N >> K >> a >> b >> c >> prec) {
            gp::Plan p = {};
            const gp::Tile tile = gp::choose_tile(t, M, N, K, a, b, c, prec);
            p.bm = tile.bm; p.bn = tile.bn; p.bk = tile.bk; p.kw = tile.kw;
            std::puts(tile_str(p).c_str());
        } else if (what == "batch" && std::cin >> a >> prec && a >= 1 && a <= gp::WGRAD_BATCH) {
            gp::WgradProblem p[gp::WGRAD_BATCH] = {};
            for (int i = 0; i < a; ++i) {
                long long ws;
                int mask, loads, wsa;
                if (!(std::cin >> p[i].M >> p[i].N >> p[i].K >> p[i].io_bf16 >> p[i].rows_per_sample >> mask >> loads >> wsa >> ws)) return 1;
                p[i].has_scale = p[i].rows_per_sample > 0;
                p[i].has_mask = mask; p[i].loads_aligned = loads; p[i].ws_aligned = wsa;
                p[i].ws_bytes = ws < 0 ? gp::wgrad_workspace_bytes(t, p[i].M, p[i].N, p[i].K) : (size_t)ws;
            }
            gp::TailRequest x = {};
            int dgrad, loads, dx, order;
            if (!(std::cin >> dgrad >> x.M >> x.N >> x.K >> loads >> dx >> order >> x.njobs)) return 1;
            x.dgrad = dgrad; x.loads_aligned = loads; x.dx_aligned = dx; x.order = order;
            const gp::BatchRoute r = gp::batch_route(t, p, a, prec, x);
            std::string s;
            for (int i = 0; i < a; ++i) s += plan_str(r.problem[i]) + " | ";
            s += x.dgrad ? plan_str(r.dgrad) : "-";
            s += std::string(" ; ") + routes[(int)r.kernel] + (r.dgrad_first ? " dgrad_first" : "") + (r.jobs_first ? " jobs_first" : "") +
                 (r.jobs_ride ? " jobs_ride" : "");
            std::puts(s.c_str());
        } else {
            std::fprintf(stderr, "gemm_plan_check: bad request '%s'\n", what.c_str());
            return 1;
        }
    }
    return 0;
}
