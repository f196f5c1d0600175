// The signed distance maps' launch policy (csrc/sdm_plan.h) on the host: reads "B ncls H W" lines from stdin and prints
// "ok TX col_tiles row_blocks col_blocks lds_bytes workspace_bytes" for each (ok 0 and zeros: the call is refused and nothing is
// launched).  tests/test_sdm_plan_host.py checks the invariants on this output.
//   c++ -O1 -std=c++17 -I cswin_unet_amd/csrc tools/sdm_plan_check.cpp -o sdm_plan_check
#include <cstdio>

#include "sdm_plan.h"

int main() {
    int B, ncls, H, W;
    while (std::scanf("%d %d %d %d", &B, &ncls, &H, &W) == 4) {
        const SdmPlan p = sdm_plan(B, ncls, H, W);
        std::printf("%d %d %d %ld %ld %ld %zu\n", p.ok, p.TX, p.col_tiles, p.row_blocks, p.col_blocks, p.lds_bytes,
                    p.ok ? sdm_workspace_bytes(B, ncls, H, W) : (size_t)0);
    }
    return 0;
}
