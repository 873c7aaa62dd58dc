// Host-only check of the head backward's weight-gradient plan (csrc/nlspn_heads_bwd_plan.h):
// no device, no HIP header.  Without arguments: sweeps shapes and prints a JSON report of the
// violations of
//   * every (image, row, band) lies in exactly one unit, and every unit in exactly one slice;
//   * the slices are in order (slice i holds units [i ups, (i + 1) ups));
//   * the bands tile the width, none wider than kHbBW;
//   * slabs, VALU partials and bias partials lie inside the workspace, in that order, disjoint;
//   * the LDS bytes are within a CU's 160 KB;
//   * the plan is a function of the shape alone (planned twice: the same fields).
// With B C H W nout: prints that shape's plan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nlspn_heads_bwd_plan.h"

using namespace nlspn;

static long long g_bad = 0;
static std::string g_first;
static void bad(const char *what, int B, int C, int H, int W, int nout) {
    if (g_bad++ < 5) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "%s\"%s at B=%d C=%d H=%d W=%d nout=%d\"", g_first.empty() ? "" : ", ", what, B, C, H, W, nout);
        g_first += buf;
    }
}

static long long check(int B, int C, int H, int W, int nout) {
    const HbPlan p = hb_plan(B, C, H, W, nout), q = hb_plan(B, C, H, W, nout);
    if (std::memcmp(&p, &q, sizeof p) != 0) bad("plan differs between two calls", B, C, H, W, nout);
    if (!p.fits) bad("does not fit", B, C, H, W, nout);
    if (p.R != nout + 2 || p.mtiles * kHbMT < p.R || (p.mtiles - 1) * kHbMT >= p.R) bad("row tiles", B, C, H, W, nout);
    if (p.ntiles * kHbNT < 2 * C || (p.ntiles - 1) * kHbNT >= 2 * C) bad("channel tiles", B, C, H, W, nout);
    if (p.bw < 1 || p.bw > kHbBW || p.nbands * p.bw < W || (p.nbands - 1) * p.bw >= W) bad("bands", B, C, H, W, nout);
    if (p.units != B * H * p.nbands) bad("units", B, C, H, W, nout);
    // every (image, row, band) in exactly one unit, every unit in exactly one slice, slices in order
    std::vector<int> hits((size_t)p.units, 0);
    int prev = -1;
    for (int sl = 0; sl < p.nsl; ++sl) {
        const int u0 = sl * p.ups, u1 = p.units < u0 + p.ups ? p.units : u0 + p.ups;
        if (u0 >= u1) bad("empty slice", B, C, H, W, nout);
        for (int u = u0; u < u1; ++u) {
            if (u != prev + 1) bad("slices out of order", B, C, H, W, nout);
            prev = u;
            const int band = u % p.nbands, row = u / p.nbands, b = row / H, y = row - b * H;
            if (b < 0 || b >= B || y < 0 || y >= H || band * p.bw >= W) bad("unit outside the tensor", B, C, H, W, nout);
            ++hits[(size_t)((b * H + y) * p.nbands + band)];
        }
    }
    for (int h : hits)
        if (h != 1) {
            bad("a unit not hit exactly once", B, C, H, W, nout);
            break;
        }
    const long long tiles = (long long)p.mtiles * p.ntiles;
    if (tiles * p.nsl > 2 * kHbTargetWgs + tiles) bad("far more workgroups than the target", B, C, H, W, nout);
    if (p.slab != tiles * kHbMT * kHbNT * 9 || p.vec_off != p.slab * p.nsl) bad("slabs", B, C, H, W, nout);
    if (p.nvs < 1 || p.nvs > kHbMaxVecSlices || p.bias_off != p.vec_off + (long long)p.nvs * 2 * C * 9) bad("VALU partials", B, C, H, W, nout);
    if (p.nsb < 1 || p.nsb > kHbMaxBiasSlices || p.floats != p.bias_off + (long long)p.nsb * p.R) bad("bias partials", B, C, H, W, nout);
    if (kHbLdsBytes > kHbLdsBudget || kHbLdsBytes != 4 * (kHbMT * kHbGP + kHbNT * 3 * kHbXRP)) bad("LDS", B, C, H, W, nout);
    return p.units;
}

int main(int argc, char **argv) {
    if (argc == 6) {
        const int B = std::atoi(argv[1]), C = std::atoi(argv[2]), H = std::atoi(argv[3]), W = std::atoi(argv[4]), nout = std::atoi(argv[5]);
        const HbPlan p = hb_plan(B, C, H, W, nout);
        std::printf("{\"R\": %d, \"mtiles\": %d, \"ntiles\": %d, \"nbands\": %d, \"bw\": %d, \"units\": %d, \"ups\": %d, \"nsl\": %d, "
                    "\"nvs\": %d, \"nsb\": %d, \"slab\": %lld, \"vec_off\": %lld, \"bias_off\": %lld, \"floats\": %lld, \"fits\": %d, "
                    "\"lds\": %d}\n",
                    p.R, p.mtiles, p.ntiles, p.nbands, p.bw, p.units, p.ups, p.nsl, p.nvs, p.nsb, p.slab, p.vec_off, p.bias_off,
                    p.floats, (int)p.fits, kHbLdsBytes);
        return 0;
    }
    long long grids = 0, units = 0;
    const int BH[][2] = {{1, 1}, {1, 7}, {2, 5}, {3, 37}, {8, 228}};
    const int CS[] = {16, 32, 64, 80}, NOUT[] = {1, 8, 24, 30, 31, 48, 72, 144, 158};
    for (const auto &bh : BH)
        for (int W = 1; W <= 330; ++W)
            for (int C : CS)
                for (int nout : NOUT) {
                    if (bh[0] == 8 && (W % 19 != 0 || C != 64)) continue;  // the large grid at a few widths
                    units += check(bh[0], C, bh[1], W, nout);
                    ++grids;
                }
    std::printf("{\"violations\": %lld, \"first\": [%s], \"grids\": %lld, \"units\": %lld, \"lds\": %d, \"lds_budget\": %d, "
                "\"target_wgs\": %d, \"band_max\": %d}\n",
                g_bad, g_first.c_str(), grids, units, kHbLdsBytes, kHbLdsBudget, kHbTargetWgs, kHbBW);
    return g_bad ? 1 : 0;
}
