// Tiling of the GRU-mode convolutions (nlspn_gconv.h) as pure arithmetic: the preset table,
// the geometry a preset's template arguments fix, the pixel tiling of a launch (gc_tile), the
// input window of one tile (gc_window) and GRU1's workgroup map (gc_gru1_map).  No HIP header
// and no runtime call, so a host-only program can include it and check the contract between
// planner and kernel over every grid (tests/gconv_plan_check.cpp, tests/test_gconv_plan_cpu.py).
// The kernel and the launcher call these very functions.
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

constexpr int kGcNT = 256;  // threads per workgroup (4 waves)
constexpr int kGcCP = 16;   // packed input channels: a multiple of this (every chunk size CC divides it)
enum { kGcS1 = 0, kGcS2 = 1, kGcT2 = 2 };         // 3x3 pad 1 stride 1 / stride 2; transposed stride 2 (pad 1, output pad 1)
// kGcEpiDact: the data-gradient epilogue (nlspn_gconv_bwd.h): no bias; the sum times the
// activation derivative of the saved forward output at the same element, times a scalar
enum { kGcEpiAct = 0, kGcEpiGru1 = 1, kGcEpiGru2 = 2, kGcEpiAff = 3, kGcEpiDact = 4 };
enum { kGcActNone = 0, kGcActRelu = 1, kGcActTanh = 2 };

// The instantiated configurations: X(id, MODE, WM, WN, WGM, WGN, XR, XP, CC, EPI).  Ids 0..5, 23 and 24
// are the presets NLSPN_GC_* of include/nlspn_prop.h (23 / 24: NLSPN_GC_S2 / NLSPN_GC_GRU2 on
// 32-pixel tiles, which nlspn_gconv picks for small grids; 25: NLSPN_GC_T2_C16 with the affinity
// normalisation in its epilogue, nlspn_gconv_affnorm); the other ids >= 16 are alternative tilings of the same
// layer kinds, selectable through nlspn_gconv's layer argument for A/B timing
// (tools/gc_bench.py) and bit-compatible with the preset of their kind in layout (the packed
// weights depend only on the kind's output-channel tile, which a variant must keep).
#define NLSPN_GC_CONFIGS(X)                                        \
    X(0, kGcS2, 4, 1, 1, 4, 12, 40, 4, kGcEpiAct)                  \
    X(1, kGcS2, 1, 1, 1, 4, 10, 72, 8, kGcEpiAct)                  \
    X(2, kGcS1, 2, 2, 2, 2, 6, 40, 4, kGcEpiGru1)                  \
    X(3, kGcS1, 2, 2, 2, 2, 8, 40, 8, kGcEpiGru2)                  \
    X(4, kGcT2, 4, 1, 1, 4, 6, 40, 8, kGcEpiAct)                   \
    X(5, kGcT2, 1, 4, 1, 4, 6, 80, 8, kGcEpiAct)                   \
    X(16, kGcS1, 2, 2, 2, 2, 8, 40, 8, kGcEpiGru1)                 \
    X(17, kGcS1, 2, 2, 2, 2, 6, 40, 4, kGcEpiGru2)                 \
    X(18, kGcS1, 2, 4, 2, 2, 8, 40, 8, kGcEpiGru1)                 \
    X(20, kGcS2, 4, 1, 1, 4, 12, 40, 8, kGcEpiAct)                 \
    X(21, kGcT2, 4, 1, 1, 4, 6, 40, 4, kGcEpiAct)                  \
    X(22, kGcT2, 1, 4, 1, 4, 6, 80, 4, kGcEpiAct)                  \
    X(23, kGcS2, 2, 1, 2, 2, 8, 40, 4, kGcEpiAct)                  \
    X(24, kGcS1, 2, 1, 2, 2, 6, 40, 8, kGcEpiGru2)                 \
    X(25, kGcT2, 1, 4, 1, 4, 6, 80, 8, kGcEpiAff)

// The data-gradient presets NLSPN_GC_DG_* (nlspn_gconv_dgrad): the forward tilings of the adjoint
// layer kind with the kGcEpiDact epilogue, and a stride-1 convolution with a plain epilogue (the
// ConvGRU's adjoints).  Instantiated in nlspn_kern_gconv_bwd.hip.
#define NLSPN_GC_DG_CONFIGS(X)                                     \
    X(32, kGcT2, 4, 1, 1, 4, 6, 40, 8, kGcEpiDact)                 \
    X(33, kGcT2, 1, 4, 1, 4, 6, 80, 8, kGcEpiDact)                 \
    X(34, kGcS2, 4, 1, 1, 4, 12, 40, 4, kGcEpiDact)                \
    X(35, kGcS2, 1, 1, 1, 4, 10, 72, 8, kGcEpiDact)                \
    X(36, kGcS1, 2, 2, 2, 2, 8, 40, 8, kGcEpiDact)

// The f16-operand family (nlspn_gconv16.h, presets NLSPN_GC16_* of include/nlspn_prop.h):
// X(id, MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI).  XP counts 16-byte cells (eight channels of one
// pixel) and CCB the 8-channel blocks of a chunk (4: one k-step of the 16x16x32 MFMA per tap).
// The pixel tiling is gc_tile / gc_window's, unchanged.  Instantiated in nlspn_kern_gconv16.hip.
#define NLSPN_GC16_CONFIGS(X)                                      \
    X(48, kGcS2, 2, 2, 2, 2, 12, 40, 4, kGcEpiAct)                 \
    X(49, kGcS1, 2, 2, 2, 2, 6, 40, 4, kGcEpiGru1)                 \
    X(50, kGcS1, 2, 2, 2, 2, 6, 40, 4, kGcEpiGru2)                 \
    X(51, kGcT2, 2, 2, 2, 2, 6, 40, 4, kGcEpiAct)                  \
    X(52, kGcT2, 1, 2, 1, 4, 6, 80, 4, kGcEpiAct)

// The LDS bytes of an f16 preset: two stages of a chunk's weights [CCB][taps][WGCO] and window
// [CCB][XR][XP], in 16-byte cells, each region rounded up to whole LDS-DMA rounds of the
// workgroup (one cell per lane).  Gc16Cfg (nlspn_gconv16.h) uses these very functions.
constexpr int kGc16LdsBudget = 160 * 1024;
NLSPN_HD constexpr int gc16_round(int v, int m) { return (v + m - 1) / m * m; }
NLSPN_HD constexpr int gc16_wst(int mode, int wgco, int ccb) { return gc16_round(ccb * (mode == kGcT2 ? 4 : 9) * wgco, kGcNT); }
NLSPN_HD constexpr int gc16_xst(int xr, int xp, int ccb) { return gc16_round(ccb * xr * xp, kGcNT); }
NLSPN_HD constexpr int gc16_lds_bytes(int mode, int wgco, int xr, int xp, int ccb) {
    return 2 * (gc16_wst(mode, wgco, ccb) + gc16_xst(xr, xp, ccb)) * 16;
}

// The split-bf16 family (nlspn_gconv_x3.h, presets NLSPN_GCX3_* of include/nlspn_prop.h), one
// preset per kind of the f16 family with its tiling: X(id, MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI).
// XP counts 16-byte cells and CCB the cell blocks of a chunk; a cell block is one part (hi or
// lo) of eight channels, so CCB = 4 is a 16-channel chunk (hi0, lo0, hi1, lo1): one k-step of a
// K = 32 and a K = 16 MFMA per tap.  Instantiated in nlspn_kern_gconv_x3.hip.
#define NLSPN_GCX3_CONFIGS(X)                                      \
    X(64, kGcS2, 2, 2, 2, 2, 12, 40, 4, kGcEpiAct)                 \
    X(65, kGcS1, 2, 2, 2, 2, 6, 40, 4, kGcEpiGru1)                 \
    X(66, kGcS1, 2, 2, 2, 2, 6, 40, 4, kGcEpiGru2)                 \
    X(67, kGcT2, 2, 2, 2, 2, 6, 40, 4, kGcEpiAct)                  \
    X(68, kGcT2, 1, 2, 1, 4, 6, 80, 4, kGcEpiAct)

// The split-bf16 data-gradient presets NLSPN_GCX3_DG_* (nlspn_gconv_x3_dgrad): the tiling of the
// forward preset of the adjoint layer kind (80: of 67, 81: of 68, 82: of 64; 83: GRU2's tile, 66,
// as a plain stride-1 convolution) with the kGcEpiDact epilogue.  Instantiated in
// nlspn_kern_gconv_x3_dg.hip.
#define NLSPN_GCX3_DG_CONFIGS(X)                                   \
    X(80, kGcT2, 2, 2, 2, 2, 6, 40, 4, kGcEpiDact)                 \
    X(81, kGcT2, 1, 2, 1, 4, 6, 80, 4, kGcEpiDact)                 \
    X(82, kGcS2, 2, 2, 2, 2, 12, 40, 4, kGcEpiDact)                \
    X(83, kGcS1, 2, 2, 2, 2, 6, 40, 4, kGcEpiDact)

// The LDS bytes of a split-bf16 preset: two stages of a chunk's weights [CCB][taps][WGCO] and
// window [CCB][XR][XP] in 16-byte cells, each region rounded up to whole LDS-DMA rounds of the
// workgroup.  A hi and a lo cell per eight channels: a 16-channel chunk (CCB 4) has the bytes of
// the f16 family's 32-channel chunk; a 32-channel chunk (CCB 8) would be 208 KB in the GRU
// presets.  GcX3Cfg (nlspn_gconv_x3.h) uses these very functions.
constexpr int kGcX3LdsBudget = 160 * 1024;
NLSPN_HD constexpr int gcx3_chunk_channels(int ccb) { return 8 * (ccb / 2); }
NLSPN_HD constexpr int gcx3_wst(int mode, int wgco, int ccb) { return gc16_round(ccb * (mode == kGcT2 ? 4 : 9) * wgco, kGcNT); }
NLSPN_HD constexpr int gcx3_xst(int xr, int xp, int ccb) { return gc16_round(ccb * xr * xp, kGcNT); }
NLSPN_HD constexpr int gcx3_lds_bytes(int mode, int wgco, int xr, int xp, int ccb) {
    return 2 * (gcx3_wst(mode, wgco, ccb) + gcx3_xst(xr, xp, ccb)) * 16;
}
#define NLSPN_GCX3_BUDGET(id, MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI) \
    static_assert(gcx3_lds_bytes(MODE, 16 * WM * WGM, XR, XP, CCB) <= kGcX3LdsBudget, "split-bf16 preset " #id ": LDS budget");
NLSPN_GCX3_CONFIGS(NLSPN_GCX3_BUDGET)
NLSPN_GCX3_DG_CONFIGS(NLSPN_GCX3_BUDGET)
#undef NLSPN_GCX3_BUDGET
static_assert(gcx3_lds_bytes(kGcS1, 64, 6, 40, 8) > kGcX3LdsBudget, "a 32-channel chunk does not fit the GRU presets");

// What a configuration's template arguments fix of the tiling: a workgroup of WGM x WGN waves,
// each WM x WN 16x16 blocks, owns WGCO output channels x NPX pixels; its LDS input window has
// XR rows of pitch XP words.
template <int MODE, int WM, int WN, int WGM, int WGN, int XR_, int XP_>
struct GcGeom {
    static constexpr int WGCO = 16 * WM * WGM, NPX = 16 * WN * WGN, XR = XR_, XP = XP_;
};
struct GcGeo {  // the same as run-time values
    int mode, wgco, npx, xr, xp;
};

// The pixel tiling of a launch: the gh x gw grid (convolutions: the output; transposed: one
// output phase's grid = the input) in nbands column bands of width bw (the last one narrower
// when bw does not divide gw), a band in tpb flat row-major runs of npx pixels (tpb: of the
// widest band; a narrower band's surplus tiles are empty).
struct GcTiling {
    int gh, gw, bw, nbands, tpb, npx;
};

// the widest band whose window columns fit the LDS pitch
NLSPN_HD constexpr int gc_bwmax(int mode, int xp) { return mode == kGcS1 ? xp - 2 : mode == kGcS2 ? (xp - 3) / 2 + 1 : xp - 1; }
// the window rows of a run of npx pixels in a band of width w: the run starts anywhere in a
// row, so it spans at most (npx + w - 2) / w row steps
NLSPN_HD constexpr int gc_rows_of(int mode, int npx, int w) {
    return mode == kGcS1 ? (npx + w - 2) / w + 3 : mode == kGcS2 ? 2 * ((npx + w - 2) / w) + 3 : (npx + w - 2) / w + 2;
}

// The tiling of a gh x gw grid under a preset's geometry; false: no tile of any size fits the
// window rows (the launcher refuses the shape, NLSPN_EUNSUPPORTED).
NLSPN_HD inline bool gc_tile(const GcGeo &p, int gh, int gw, GcTiling &t) {
    t.gh = gh;
    t.gw = gw;
    // column bands: the window's columns within the LDS pitch
    const int bwmax = gc_bwmax(p.mode, p.xp);
    t.nbands = (gw + bwmax - 1) / bwmax;
    t.bw = (gw + t.nbands - 1) / t.nbands;
    // the rows a tile of npx pixels spans, within the window's XR rows: narrow bands take
    // fewer pixels per tile.  The kernel cuts EVERY band into runs of the same npx, and a run
    // in a narrower band spans more rows, so the bound must hold for the narrowest band cut:
    // the last one, of width gw - (nbands - 1) bw <= bw (equal when bw divides gw: the plan
    // is then the widest band's).  Sizing npx by bw alone let a last band one column
    // narrower (20 | 19) read one row past the staged window.
    const int bwl = gw - (t.nbands - 1) * t.bw;
    t.npx = p.npx;
    while (t.npx > 1 && gc_rows_of(p.mode, t.npx, bwl) > p.xr) --t.npx;
    t.tpb = (gh * t.bw + t.npx - 1) / t.npx;
    return gc_rows_of(p.mode, t.npx, bwl) <= p.xr;
}

// One tile's pixels and input window, as gconv_body computes them: band `band`'s columns
// bx0 .. bx0 + bwi - 1, the flat pixels f0 .. f0 + npx - 1 of its gh x bwi pixels (grid rows
// ra .. rb), and the input rows iy0 .. iy0 + nrows - 1 / columns ix0 .. ix0 + ncols - 1 their
// taps reach.  empty: the tile lies past the band's last pixel (nothing else is set then
// but bx0 / bwi / f0).
struct GcWindow {
    int bx0, bwi, f0, ra, rb, iy0, ix0, nrows, ncols;
    bool empty;
};
NLSPN_HD inline GcWindow gc_window(int mode, int gh, int gw, int bw, int npx, int band, int tile) {
    GcWindow w{};
    const int S = mode == kGcS2 ? 2 : 1;
    w.bx0 = band * bw;
    w.bwi = bw < gw - w.bx0 ? bw : gw - w.bx0;
    w.f0 = tile * npx;
    w.empty = w.f0 >= gh * w.bwi;  // (the narrower last band has fewer tiles)
    if (w.empty) return w;
    const int rl = (w.f0 + npx - 1) / w.bwi;
    w.ra = w.f0 / w.bwi;
    w.rb = gh - 1 < rl ? gh - 1 : rl;
    w.iy0 = mode == kGcT2 ? w.ra : S * w.ra - 1;
    w.ix0 = mode == kGcT2 ? w.bx0 : S * w.bx0 - 1;
    w.nrows = mode == kGcT2 ? w.rb - w.ra + 2 : S * (w.rb - w.ra) + 3;
    w.ncols = mode == kGcT2 ? w.bwi + 1 : S * (w.bwi - 1) + 3;
    return w;
}

// GRU1's output-channel tiles differ in cost: z and r run K over h and x, qx over x alone (half).
// One workgroup per (co tile, pixel tile) left the CUs unevenly loaded (every workgroup is
// resident at once, so a CU's finish time is its summed work: 3.5 heavy-tile units on the most
// loaded CUs against 2.8 on average).  A qx workgroup takes TWO consecutive pixel tiles instead,
// so every workgroup costs the same.  (The pixel tiles of a GRU1 launch: gc_rest_count.)
NLSPN_HD constexpr int gc_gru1_heavy_cots(int hc, int wgco) { return (2 * hc) / wgco; }
NLSPN_HD constexpr int gc_rest_count(int B, int nbands, int tpb) { return B * nbands * tpb; }
NLSPN_HD constexpr int gc_gru1_wgs(int hc, int wgco, int co_tiles, int nr) {
    return gc_gru1_heavy_cots(hc, wgco) * nr + (co_tiles - gc_gru1_heavy_cots(hc, wgco)) * ((nr + 1) / 2);
}
// workgroup wg of a GRU1 launch -> its co tile and its one or two pixel tiles r0, r1 (of
// gc_rest_count; r1 = -1: one tile).  gconv_body's flat index of (cot, r) is cot + r * co_tiles.
NLSPN_HD inline void gc_gru1_map(int wg, int nh, int nr, int co_tiles, int &cot, int &r0, int &r1) {
    if (wg < nh * nr) {  // z / r: one pixel tile
        cot = wg % nh;
        r0 = wg / nh;
        r1 = -1;
    } else {             // qx: two pixel tiles in turn
        const int w = wg - nh * nr, nl = co_tiles - nh;
        cot = nh + w % nl;
        r0 = 2 * (w / nl);
        r1 = r0 + 1 < nr ? r0 + 1 : -1;
    }
}

#pragma GCC visibility pop
}  // namespace nlspn
