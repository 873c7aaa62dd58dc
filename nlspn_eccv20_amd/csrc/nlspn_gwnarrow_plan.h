// Plan and index arithmetic of the streaming weight gradient of the narrow stride-2 layers
// (nlspn_gwnarrow.h: both channel counts <= 16): which shapes it covers, the units, slices, slab
// and workspace of a call, the chunks a staged row is loaded in and the LDS offsets of the
// staging stores and the k-loop reads.  No HIP header and no runtime call: the kernel, the
// launcher (nlspn_gconv_host.hip) and the host-only check (tests/gwnarrow_plan_check.cpp) call
// these very functions.  Every count is a constant or a function of the shape, never of the
// device: the same shape sums in the same order, hence gives the same bits, everywhere.
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

constexpr int kGwnR = 4;             // small rows per unit = waves per workgroup (a wave per row)
constexpr int kGwnNW = kGwnR;
constexpr int kGwnNTHR = 64 * kGwnNW;
constexpr int kGwnBW = 64;           // small pixels per band at most (a multiple of 4)
constexpr int kGwnTargetWgs = 512;   // slices aimed at (a constant, not the device's CU count)
constexpr int kGwnGP = 66;           // small row pitch per channel (>= kGwnBW, = 2 mod 32)
constexpr int kGwnHALF = 80;         // offset of a window row's odd columns (>= kGwnBW + 1, = 16 mod 32)
constexpr int kGwnXRP = 150;         // window row pitch (>= kGwnHALF + kGwnBW)
constexpr int kGwnXCP = (2 * kGwnR + 1) * kGwnXRP;  // window channel pitch: 2R + 1 rows
constexpr int kGwnRedLanes = 16;     // the reduce: slice lanes of its first level
constexpr int kGwnLdsBudget = 160 * 1024;
static_assert(kGwnBW % 4 == 0 && kGwnGP >= kGwnBW && kGwnHALF >= kGwnBW + 1 && kGwnXRP >= kGwnHALF + kGwnBW, "rows fit");

// stride 2, one source, both channel counts within one 16-wide block
NLSPN_HD constexpr bool gwn_covers(int stride, int Cs, int c0, int c1) {
    return stride == 2 && Cs >= 1 && Cs <= 16 && c0 >= 1 && c0 <= 16 && c1 == 0;
}

// N is (large channel, tap) flattened: entry n = 9 cl + 3 ky + kx, in 16-wide blocks
NLSPN_HD constexpr int gwn_blocks(int Cl) { return (9 * Cl + 15) / 16; }
// the most large channels a kernel of nb blocks serves (its window's channels in LDS)
NLSPN_HD constexpr int gwn_clmax(int nb) { return 16 * nb / 9; }
// LDS floats of the kernel of nb blocks: the stage (small rows [R][16][GP], window
// [clmax][2R + 1][XRP]), reused for the waves' accumulators and bias partials, then the bias
// accumulators of the large side
NLSPN_HD constexpr int gwn_stage_floats(int nb) { return kGwnR * 16 * kGwnGP + gwn_clmax(nb) * kGwnXCP; }
NLSPN_HD constexpr int gwn_red_floats(int nb) { return kGwnNW * (nb * 256 + 64); }
NLSPN_HD constexpr int gwn_lds_floats(int nb) {
    return (gwn_stage_floats(nb) > gwn_red_floats(nb) ? gwn_stage_floats(nb) : gwn_red_floats(nb)) + 16;
}

// A unit is (image, group of R small rows, column band); a slice is ups consecutive units and
// writes one slab: nb blocks of [4 registers][64 lanes] accumulator floats, then 16 bias sums.
struct GwnPlan {
    int nb, nbands, bw, ngroups, units, ups, nsl, lds_bytes;
    long long slab, floats;
};
// (the shape is validated by the caller)
NLSPN_HD inline GwnPlan gwn_plan(int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    (void)Cs; (void)Hl; (void)Wl;
    GwnPlan p{};
    p.nb = gwn_blocks(Cl);
    p.nbands = (Ws + kGwnBW - 1) / kGwnBW;
    p.bw = (Ws + p.nbands - 1) / p.nbands;
    p.ngroups = (Hs + kGwnR - 1) / kGwnR;
    p.units = B * p.ngroups * p.nbands;
    int nsl = kGwnTargetWgs < p.units ? kGwnTargetWgs : p.units;
    p.ups = (p.units + nsl - 1) / nsl;
    p.nsl = (p.units + p.ups - 1) / p.ups;
    p.lds_bytes = gwn_lds_floats(p.nb) * 4;
    p.slab = (long long)p.nb * 256 + 16;
    p.floats = p.slab * p.nsl;
    return p;
}

struct GwnUnit {
    int b, sy0, nrows, bx0, bwi, k4;
};
NLSPN_HD inline GwnUnit gwn_unit(int u, int nbands, int bw, int ngroups, int Hs, int Ws) {
    GwnUnit n{};
    const int band = u % nbands, g = u / nbands;
    n.b = g / ngroups;
    n.sy0 = (g - n.b * ngroups) * kGwnR;
    n.nrows = Hs - n.sy0 < kGwnR ? Hs - n.sy0 : kGwnR;
    n.bx0 = band * bw;
    n.bwi = bw < Ws - n.bx0 ? bw : Ws - n.bx0;
    n.k4 = (n.bwi + 3) & ~3;
    return n;
}

// The staging lines of a unit of nrows small rows: the Cs x nrows small rows, then the Cl x
// (2 nrows + 1) window rows; line li is (channel c, small row / window row rj).
struct GwnLine {
    int window, c, rj;
};
NLSPN_HD constexpr int gwn_lines(int Cs, int Cl, int nrows) { return Cs * nrows + Cl * (2 * nrows + 1); }
NLSPN_HD inline GwnLine gwn_line(int li, int Cs, int nrows) {
    const int nsm = Cs * nrows, nwr = 2 * nrows + 1;
    if (li < nsm) {
        const int cs = li / nrows;
        return GwnLine{0, cs, li - cs * nrows};
    }
    const int k = li - nsm, cl = k / nwr;
    return GwnLine{1, cl, k - cl * nwr};
}

// A staged row: columns [xf, xf + cnt) of a tensor row whose column 0 sits a0 floats (mod 4) past
// a 16-byte boundary, loaded in nch chunks of four columns from column xs <= xf on: every
// chunk's address is then a multiple of 16 bytes.  (xf may be negative: -1 at the left edge.)
struct GwnChunks {
    int xs, nch;
};
NLSPN_HD inline GwnChunks gwn_chunks(int a0, int xf, int cnt) {
    const int m = (a0 + xf) & 3;
    return GwnChunks{xf - m, (m + cnt + 3) >> 2};
}

// LDS offsets.  The small rows: [row r][channel][pixel]; the window: [channel][row j][parity of
// the window column wc][wc / 2] (a tap's pixels are then consecutive words).
NLSPN_HD constexpr int gwn_a_off(int r, int cs, int p) { return (r * 16 + cs) * kGwnGP + p; }
NLSPN_HD constexpr int gwn_b_off(int cl, int j, int wc) {
    return kGwnR * 16 * kGwnGP + cl * kGwnXCP + j * kGwnXRP + (wc & 1) * kGwnHALF + (wc >> 1);
}
// the k-loop's reads of small row r at pixel p: small channel cs; entry n of N
NLSPN_HD constexpr int gwn_a_read(int cs, int r, int p) { return gwn_a_off(r, cs, p); }
NLSPN_HD constexpr int gwn_b_read(int n, int r, int p) { return gwn_b_off(n / 9, 2 * r + (n % 9) / 3, 2 * p + n % 3); }
// where a slab keeps dW[cs][entry n]: block n / 16, register cs % 4, lane 16 (cs / 4) + n % 16
NLSPN_HD constexpr int gwn_slab_off(int cs, int n) { return ((n >> 4) * 4 + (cs & 3)) * 64 + (cs >> 2) * 16 + (n & 15); }

#pragma GCC visibility pop
}  // namespace nlspn
