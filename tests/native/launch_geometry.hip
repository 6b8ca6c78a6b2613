// Stand-alone host program: prints the launch geometry of protein_redesign_amd/csrc/prd_launch.h for tests/test_launch_cpu.py, which
// compares it with the formulas the launch sites spelled out before the header existed.  No HIP call is made; runs without a GPU.
//   g <tasks> <per_wg> <cap> <grid_for>
//   r <rows_total> <H> <rows per head> <... rounded for the XCDs> <... with the rounding switched off>
#include "../../protein_redesign_amd/csrc/prd_launch.h"
#include <cstdio>

int main() {
    const int pairs[][2] = {{1, 2048}, {256, 2048}, {256, 4096}, {4, 1024}, {4, 2048}, {4, 256}, {4, 512}, {8, 256}};   // per_wg, cap of the sources
    const long big[] = {4201, 65536, 1000000, 8388608, 2147483647L, 2147483653L, 1L << 40};
    for (const auto& p : pairs) {
        for (long t = 0; t <= 4200; ++t) printf("g %ld %d %d %d\n", t, p[0], p[1], grid_for(t, p[0], p[1]));
        for (long t : big) printf("g %ld %d %d %d\n", t, p[0], p[1], grid_for(t, p[0], p[1]));
    }
    for (int H = 1; H <= 8; ++H)
        for (long rows = 1; rows <= 4200; ++rows)
            printf("r %ld %d %ld %ld %ld\n", rows, H, prd_rows_per_head(rows, 256 / H), prd_rows_per_head_xcd8(rows, 256 / H),
                   prd_rows_per_head_xcd8(rows, 256 / H, false));
    return 0;
}
