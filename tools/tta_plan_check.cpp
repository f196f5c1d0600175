// The views and launch policy of the test-time-augmentation kernels (csrc/tta_plan.h) on the host.  Reads request lines from
// stdin and answers each with one line:
//   "pos c h w"                   -> the h * w pairs "i j" of tta_view_pos(c, r, s, h, w), r-major, on one line
//   "views h w V c0 .. c(V-1)"    -> "refusal bad packed any_transposed" of tta_pack_views
//   "plan V B nsel h w"           -> "general gx gy gz threads lds_bytes | vx vy vz view_threads" of tta_plan and tta_view_grid
// tests/test_tta_plan_host.py holds the first to numpy and the others to what the kernels and the hardware need.
//   c++ -O1 -std=c++17 -I cswin_unet_amd/csrc tools/tta_plan_check.cpp -o tta_plan_check
#include <cstdio>
#include <cstring>

#include "tta_plan.h"

int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "pos")) {
            int c, h, w;
            if (std::scanf("%d %d %d", &c, &h, &w) != 3) return 1;
            for (int r = 0; r < h; ++r)
                for (int s = 0; s < w; ++s) {
                    const TtaPos q = tta_view_pos(c, r, s, h, w);
                    std::printf("%d %d ", q.i, q.j);
                }
            std::printf("\n");
        } else if (!std::strcmp(what, "views")) {
            int h, w, V, views[16] = {0};
            if (std::scanf("%d %d %d", &h, &w, &V) != 3 || V < 0 || V > 16) return 1;
            for (int v = 0; v < V; ++v)
                if (std::scanf("%d", &views[v]) != 1) return 1;
            const TtaViews p = tta_pack_views(views, V, h, w);
            std::printf("%d %d %u %d\n", (int)p.refusal, p.bad, p.packed, (int)p.any_transposed);
        } else if (!std::strcmp(what, "plan")) {
            int V, B, nsel, h, w;
            if (std::scanf("%d %d %d %d %d", &V, &B, &nsel, &h, &w) != 5) return 1;
            if (!tta_dim_ok(B) || !tta_dim_ok(h) || !tta_dim_ok(w) || nsel < 1 || nsel > TTA_MAX_CLS || V < 1 || V > TTA_MAX_VIEWS) {
                std::fprintf(stderr, "tta_plan_check: V=%d B=%d nsel=%d h=%d w=%d outside what the entry points plan for\n", V, B, nsel, h, w);
                return 1;
            }
            const TtaPlan p = tta_plan(B, nsel, h, w);
            const TtaGrid g = tta_view_grid(V, B, h, w);
            std::printf("%d %d %d %d %d %ld | %d %d %d %d\n", (int)p.general, p.grid.x, p.grid.y, p.grid.z, p.threads, p.lds_bytes, g.x, g.y,
                        g.z, TTA_VIEW_THREADS);
        } else {
            std::fprintf(stderr, "tta_plan_check: unknown request %s\n", what);
            return 1;
        }
    }
    return 0;
}
