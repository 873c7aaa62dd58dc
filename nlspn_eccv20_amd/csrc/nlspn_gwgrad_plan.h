// Plan of a weight-gradient call (nlspn_gconv_bwd.h, nlspn_gwgrad16.h) as pure arithmetic: the
// channel tiles, column bands, units, K slices, bias slices and workspace floats of a shape
// (gw_split, which the f32 plan below and gw16_plan of nlspn_gwgrad16_plan.h both call), and
// the f32 kernels' tiling choice (gw_choose).  No HIP header and no runtime call, so a
// host-only program can include it and check the plan over every grid
// (tests/gwgrad16_plan_check.cpp, tests/test_gwgrad16_plan_cpu.py).  The launcher calls these
// very functions; the shape rules that refuse a call stay with it (nlspn_gconv_host.hip).
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

constexpr int kGwBW = 64;            // f32 kernels: pixels per unit at most (a multiple of 4)
// K slices x tiles aimed at by the f32 kernels (a constant, not the device's CU count: the
// summation order, hence the bits, is the same on every device)
constexpr int kGwTargetWgs = 512;
// Slices of the bias gradient's partial sums at most, for the f32 and the split-bf16 entry
// alike: both run the same bias launches on the same slices, so their bias gradients are
// bit-equal.
constexpr int kGwMaxBiasSlices = 64;

// What a shape fixes of a call under tiles of mt small x nt large channels, bands of at most
// bwmax pixels and about target_wgs workgroups: a unit is (image, small row, column band), a
// K slice ups consecutive units; slice i writes slab floats [mtiles mt][ntiles nt][9] at
// i * slab, the nsb bias partials of max(Cs, Cl) channels follow at bias_off.
struct GwSplit {
    int mtiles, ntiles, nbands, bw, units, ups, nsl, nsb;
    long long slab, bias_off, floats;  // slab floats; the bias partials' offset; the workspace's floats
};
// (the shape is validated by the caller)
NLSPN_HD inline GwSplit gw_split(int mt, int nt, int bwmax, int target_wgs, int Cs, int Cl, int B, int Hs, int Ws,
                                 int Hl, int Wl) {
    GwSplit p{};
    p.mtiles = (Cs + mt - 1) / mt;
    p.ntiles = (Cl + nt - 1) / nt;
    p.nbands = (Ws + bwmax - 1) / bwmax;
    p.bw = (Ws + p.nbands - 1) / p.nbands;
    p.units = B * Hs * p.nbands;
    const int tiles = p.mtiles * p.ntiles;
    int nsl = (target_wgs + tiles - 1) / tiles;
    nsl = nsl < p.units ? nsl : p.units;
    nsl = nsl > 1 ? nsl : 1;
    p.ups = (p.units + nsl - 1) / nsl;
    p.nsl = (p.units + p.ups - 1) / p.ups;
    p.slab = (long long)p.mtiles * mt * p.ntiles * nt * 9;
    const long long nb = ((long long)B * Hl * Wl + 16383) / 16384;
    p.nsb = (int)(nb < 1 ? 1 : nb > kGwMaxBiasSlices ? kGwMaxBiasSlices : nb);
    p.bias_off = p.slab * p.nsl;
    p.floats = p.bias_off + (long long)p.nsb * (Cs > Cl ? Cs : Cl);
    return p;
}

// The f32 tilings (NLSPN_GW_CONFIGS of nlspn_gconv_bwd.h): a workgroup of wgm x wgn waves, a
// wave wm x 9 16x16 blocks, owns mt small channels x nt large channels x 9 taps.
struct GwGeo {
    int S, wm, wgm, wgn;
    NLSPN_HD constexpr int mt() const { return 16 * wm * wgm; }
    NLSPN_HD constexpr int nt() const { return 16 * wgn; }
    NLSPN_HD constexpr int nthr() const { return 64 * wgm * wgn; }
};
// 64 x 32 channels for the wide layers; 128 x 16 when the large tensor has at most 16 channels;
// one wave (16 x 16) for the narrow layers (1 / 9 -> 16, 16 -> 8)
NLSPN_HD constexpr GwGeo gw_choose(int stride, int Cs, int Cl) {
    return stride == 1 ? GwGeo{1, 2, 2, 2} : Cl > 16 ? GwGeo{2, 2, 2, 2} : Cs > 16 ? GwGeo{2, 2, 4, 1} : GwGeo{2, 1, 1, 1};
}

// ---- the f32 plan of one call, a pure function of the shape
struct GwPlan : GwSplit {
    GwGeo g;
};
NLSPN_HD inline GwPlan gw_plan(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    const GwGeo g = gw_choose(stride, Cs, Cl);
    return GwPlan{gw_split(g.mt(), g.nt(), kGwBW, kGwTargetWgs, Cs, Cl, B, Hs, Ws, Hl, Wl), g};
}

#pragma GCC visibility pop
}  // namespace nlspn
