// Plan and LDS addressing of the split-bf16 weight gradient (nlspn_gwgrad16.h) as pure
// arithmetic: the tiling choice, bands, units, K slices and workspace floats of a call, where
// staging writes cell (channel, row, column copy, part, pixel) of a stage, which staging item
// fills it from which tensor element, and where k-step / lane group / tap reads.  No HIP header
// and no runtime call, so a host-only program can include it and walk every read of every unit
// (tests/gwgrad16_plan_check.cpp, tests/test_gwgrad16_plan_cpu.py).  The kernel and the
// launcher call these very functions.
#pragma once

#include "nlspn_gwgrad_plan.h"  // NLSPN_HD; gw_split and the bias slices both entries share

namespace nlspn {
#pragma GCC visibility push(hidden)

// One unit = (image, small row, column band of at most kGw16BW pixels) = one or two k-steps of
// 32 pixels.  A stage holds bf16 elements:
//   A (small row):    [c < MT][part 2][kGw16BW pixels]                 channel pitch kGw16AP
//   B (large window): [c < NT][ky 3][kx 3][part 2][kGw16BW pixels]     channel pitch kGw16BP
// part 0 = hi, 1 = lo.  B keeps one column-shifted copy of the window row per kx: element p of
// copy kx is the large tensor's column S (bx0 + p) - 1 + kx, so a lane's fragment (eight
// consecutive pixels of one channel at one tap) is eight consecutive elements starting at a
// multiple of eight: one 16-byte read, aligned, for every kx and both strides (at stride 2
// copies 0 / 2 are the window's even columns and the same shifted by one, copy 1 its odd ones).
// Both channel pitches are 32 (mod 64) bytes: see the bank note in nlspn_gwgrad16.h.
constexpr int kGw16BW = 64;                      // pixels per unit at most = elements per LDS row
constexpr int kGw16KS = 32;                      // pixels per k-step
constexpr int kGw16AP = 2 * kGw16BW + 16;        // 144 elements = 288 bytes
constexpr int kGw16BP = 18 * kGw16BW + 16;       // 1168 elements = 2336 bytes
constexpr int kGw16LdsBudget = 160 * 1024;
#ifndef NLSPN_GW16_TARGET_WGS  // (A/B builds: make EXTRA=-DNLSPN_GW16_TARGET_WGS=...)
#define NLSPN_GW16_TARGET_WGS 256
#endif
constexpr int kGw16TargetWgs = NLSPN_GW16_TARGET_WGS;  // K slices x tiles aimed at (a constant, not the device's CU count)
static_assert((kGw16AP * 2) % 64 == 32 && (kGw16BP * 2) % 64 == 32, "bank rule");
static_assert(kGw16AP % 8 == 0 && kGw16BP % 8 == 0 && kGw16BW % 8 == 0, "16-byte fragments");

enum { kGw16F32 = -1, kGw16S1 = 0, kGw16S2Wide = 1, kGw16S2Narrow = 2 };

// The tilings: a workgroup of wgm x wgn waves, a wave wm x 9 16x16 blocks, owns mt small
// channels x nt large channels x 9 taps.  All three cases run the 128 x 16 tile of four waves
// (two stages of a 64 x 32 tile with the three window copies would need 182 KB of LDS).
struct Gw16Geo {
    int S, wm, wgm, wgn;
    NLSPN_HD constexpr int mt() const { return 16 * wm * wgm; }
    NLSPN_HD constexpr int nt() const { return 16 * wgn; }
    NLSPN_HD constexpr int nthr() const { return 64 * wgm * wgn; }
    NLSPN_HD constexpr int stage_elems() const { return mt() * kGw16AP + nt() * kGw16BP; }
    NLSPN_HD constexpr int lds_bytes() const { return 2 * stage_elems() * 2; }  // two stages of bf16
};
NLSPN_HD constexpr Gw16Geo gw16_geo(int tiling) {
    return tiling == kGw16S1 ? Gw16Geo{1, 2, 4, 1} : Gw16Geo{2, 2, 4, 1};
}
// kGw16F32: both channel counts <= 16 (1 / 9 -> 16, 16 -> 8): the one-wave f32 kernel
NLSPN_HD constexpr int gw16_choose(int stride, int Cs, int Cl) {
    return Cs <= 16 && Cl <= 16 ? kGw16F32 : stride == 1 ? kGw16S1 : Cl > 16 ? kGw16S2Wide : kGw16S2Narrow;
}

// ---- LDS addressing (element offsets inside a stage)
NLSPN_HD constexpr int gw16_a_off(int c, int part, int px) { return c * kGw16AP + part * kGw16BW + px; }
NLSPN_HD constexpr int gw16_b_off(int mt, int c, int ky, int kx, int part, int px) {
    return mt * kGw16AP + c * kGw16BP + ((ky * 3 + kx) * 2 + part) * kGw16BW + px;
}
// the first of the eight elements lane group lg reads in k-step ks
NLSPN_HD constexpr int gw16_frag_px(int ks, int lg) { return kGw16KS * ks + 8 * lg; }

// ---- staging items.  An item fills two adjacent pixels (2 pp, 2 pp + 1) of one row: both parts
// of one A row, or both parts of the three copies of one B row.  Item i of a stage region is
// pixel pair i % 32 of row i / 32; an A row is a channel, B row r is channel r % nt at ky = r / nt.
// Thread tid of nthr takes the items tid + k nthr (pass k): consecutive lanes, consecutive pixel
// pairs of a row; its row in pass k is tid / 32 + k gw16_pass_rows(nthr), so with the rows of a pass
// dividing nt a pass has ONE ky and channel step for all threads (gw16_b_pass_ky / _c): the
// kernel adds those to a uniform base address and keeps one per-thread offset for all passes.
NLSPN_HD constexpr int gw16_a_items(int mt) { return mt * (kGw16BW / 2); }
NLSPN_HD constexpr int gw16_b_items(int nt) { return nt * 3 * (kGw16BW / 2); }
NLSPN_HD inline void gw16_a_item(int i, int &c, int &pp) {
    pp = i % (kGw16BW / 2);
    c = i / (kGw16BW / 2);
}
NLSPN_HD inline void gw16_b_item(int i, int nt, int &c, int &ky, int &pp) {
    pp = i % (kGw16BW / 2);
    const int r = i / (kGw16BW / 2);
    c = r % nt;
    ky = r / nt;
}
NLSPN_HD constexpr int gw16_pass_rows(int nthr) { return nthr / (kGw16BW / 2); }
NLSPN_HD constexpr int gw16_b_pass_c(int nt, int nthr, int k) { return gw16_pass_rows(nthr) * k % nt; }
NLSPN_HD constexpr int gw16_b_pass_ky(int nt, int nthr, int k) { return gw16_pass_rows(nthr) * k / nt; }
// a B item loads the S + 3 window columns wc = 2 S pp + j (column wc of the window is the large
// tensor's column S bx0 - 1 + wc); copy kx takes loads j = kx (pixel 2 pp) and kx + S (2 pp + 1)
NLSPN_HD constexpr int gw16_b_loads(int S) { return S + 3; }
NLSPN_HD constexpr int gw16_b_wc(int S, int pp, int j) { return 2 * S * pp + j; }
// the window columns a band of bwi pixels reads: the rest is stored as zeros
NLSPN_HD constexpr int gw16_ncol(int S, int bwi) { return S * (bwi - 1) + 3; }

// ---- units
struct Gw16Unit {
    int b, sy, bx0, bwi, nks;  // image, small row, band's first column and width, k-steps
};
NLSPN_HD inline Gw16Unit gw16_unit(int u, int nbands, int bw, int Hs, int Ws) {
    Gw16Unit n{};
    const int band = u % nbands, row = u / nbands;
    n.b = row / Hs;
    n.sy = row - n.b * Hs;
    n.bx0 = band * bw;
    n.bwi = bw < Ws - n.bx0 ? bw : Ws - n.bx0;
    n.nks = (n.bwi + kGw16KS - 1) / kGw16KS;
    return n;
}

// ---- the plan of one call, a pure function of the shape (the shape is validated by the caller)
struct Gw16Plan : GwSplit {
    int tiling;
    Gw16Geo g;
};
NLSPN_HD inline Gw16Plan gw16_plan(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    const int tiling = gw16_choose(stride, Cs, Cl);
    const Gw16Geo g = gw16_geo(tiling);
    return Gw16Plan{gw_split(g.mt(), g.nt(), kGw16BW, kGw16TargetWgs, Cs, Cl, B, Hs, Ws, Hl, Wl), tiling, g};
}

#pragma GCC visibility pop
}  // namespace nlspn
