// The blur's tile plan (csrc/blur_plan.h) on the host: reads "H W r vec" lines from stdin and prints
// "TR cw_log2 budget_index lds_bytes" for each (budget_index -1 and TR 0: no plan).  tests/test_blur_host.py compares the
// Python transcription of tests/blur_cases.py with this output.
//   c++ -O1 -std=c++17 -I cswin_unet_amd/csrc tools/blur_plan_check.cpp -o blur_plan_check
#include <cstdio>

#include "blur_plan.h"

int main() {
    int H, W, r, vec;
    while (std::scanf("%d %d %d %d", &H, &W, &r, &vec) == 4) {
        if (!bl_dim_ok(H) || !bl_dim_ok(W) || r < 0 || r > BL_MAX_RADIUS || (vec != 1 && vec != 2)) {
            std::fprintf(stderr, "blur_plan_check: H=%d W=%d r=%d vec=%d outside what cswin_gaussian_blur plans for\n", H, W, r, vec);
            return 1;
        }
        const BlurPlan p = bl_plan(H, W, r, vec);
        std::printf("%d %d %d %ld\n", p.TR, p.cw_log2, p.budget, bl_lds_bytes(p, W, r));
    }
    return 0;
}
