// Plan of the head epilogue's weight gradient (nlspn_heads_bwd.h) as pure arithmetic: the row
// tiles, channel tiles, column bands, units, K slices, the VALU companion's slices, the bias
// slices and the workspace floats of a shape.  No HIP header and no runtime call, so a host-only
// program can include it and check the plan over every grid (tests/heads_bwd_plan_check.cpp,
// tests/test_heads_bwd_cpu.py).  The launcher calls this very function; the shape rules that
// refuse a call stay with it (nlspn_seam.hip).
#pragma once

#ifndef NLSPN_HD
#if defined(__HIPCC__)
#define NLSPN_HD __host__ __device__
#else
#define NLSPN_HD
#endif
#endif

namespace nlspn {
#pragma GCC visibility push(hidden)

constexpr int kHbMT = 32;   // rows of gpre per tile: the forward's M-block
constexpr int kHbNT = 64;   // channels of [fd_oa | fe1] per tile: four waves of 16
constexpr int kHbBW = 64;   // pixels per unit at most (a multiple of 4)
constexpr int kHbNTHR = 256;
// K slices x tiles aimed at (a constant, not the device's CU count: the summation order, hence
// the bits, is the same on every device)
constexpr int kHbTargetWgs = 512;
constexpr int kHbMaxVecSlices = 64;   // slices of the one-row (id / cf decoder half) VALU sums at most
constexpr int kHbMaxBiasSlices = 64;  // slices of the bias gradient's partial sums at most
constexpr int kHbVecPixels = 16384;   // (image, pixel) elements per VALU / bias slice aimed at
// LDS: gpre rows [kHbMT] at pitch kHbGP, the window [kHbNT][3 rows] at row pitch kHbXRP; both
// channel pitches = 2 (mod 32): the bank rule of nlspn_gconv_bwd.h
constexpr int kHbGP = 66, kHbXRP = 86, kHbXCP = 3 * kHbXRP;
static_assert(kHbGP % 32 == 2 && kHbXCP % 32 == 2 && kHbGP >= kHbBW && kHbXRP >= kHbBW + 2, "bank rule, window fits");
constexpr int kHbLdsBytes = 4 * (kHbMT * kHbGP + kHbNT * kHbXCP);
constexpr int kHbLdsBudget = 160 * 1024;
static_assert(kHbLdsBytes <= kHbLdsBudget, "LDS of a CU");

// A unit is (image, row of the image, column band); K slice i is units [i ups, (i + 1) ups) and
// writes slab floats [mtiles kHbMT][ntiles kHbNT][9] at i * slab.  The VALU partials
// [nvs][2 heads][C][9] follow at vec_off, the bias partials [nsb][R] at bias_off.  fits: every
// count an int can hold (otherwise only floats is meaningful, as an upper bound's order).
struct HbPlan {
    int R, mtiles, ntiles, nbands, bw, units, ups, nsl, nvs, nsb;
    long long slab, vec_off, bias_off, floats;
    bool fits;
};
NLSPN_HD inline HbPlan hb_plan(int B, int C, int H, int W, int nout) {
    HbPlan p{};
    p.R = nout + 2;
    p.mtiles = (p.R + kHbMT - 1) / kHbMT;
    p.ntiles = (2 * C + kHbNT - 1) / kHbNT;
    p.nbands = (W + kHbBW - 1) / kHbBW;
    p.bw = (W + p.nbands - 1) / p.nbands;
    const long long units = (long long)B * H * p.nbands;
    const long long tiles = (long long)p.mtiles * p.ntiles;
    long long nsl = (kHbTargetWgs + tiles - 1) / tiles;
    nsl = nsl < units ? nsl : units;
    nsl = nsl > 1 ? nsl : 1;
    const long long ups = (units + nsl - 1) / nsl;
    nsl = (units + ups - 1) / ups;
    const long long n = (long long)B * H * W, per = (n + kHbVecPixels - 1) / kHbVecPixels;
    p.nvs = (int)(per < 1 ? 1 : per > kHbMaxVecSlices ? kHbMaxVecSlices : per);
    p.nsb = (int)(per < 1 ? 1 : per > kHbMaxBiasSlices ? kHbMaxBiasSlices : per);
    p.slab = tiles * kHbMT * kHbNT * 9;
    p.vec_off = p.slab * nsl;
    p.bias_off = p.vec_off + (long long)p.nvs * 2 * C * 9;
    p.floats = p.bias_off + (long long)p.nsb * p.R;
    p.fits = units <= 0x3fffffffLL && tiles * nsl <= 0x7fffffffLL;
    p.units = p.fits ? (int)units : 0;
    p.ups = p.fits ? (int)ups : 0;
    p.nsl = p.fits ? (int)nsl : 0;
    return p;
}

#pragma GCC visibility pop
}  // namespace nlspn
