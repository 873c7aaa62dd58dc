// Launch planning of the resident kernels: the part grid, the launch form and the build of
// the forward resident launch (res_plan) and the part grid of the resident backward
// (br_plan), as pure arithmetic.  No HIP runtime call and no environment read: the CU
// count and the A/B switches are arguments, so a host-only program can include this
// header and print the plans (tests/planner_dump.cpp, tests/test_planner_cpu.py).  The
// geometry constants the kernels share with the planners live here too.
#pragma once

#include <algorithm>
#include <cstddef>

#if defined(__HIPCC__)
#define NLSPN_HD __host__ __device__
#else
#define NLSPN_HD
#endif

namespace nlspn {
#pragma GCC visibility push(hidden)  // host helpers: not part of the library's exported symbols

// ------------------------------------------------------------------ A/B switches
// The forward resident path's A/B switches, read from the environment on every call
// (read_switches, nlspn_host.hip: the tests and the A/B tools flip them inside one process).
// The defaults are the product's.
struct Switches {
    bool resident = true;      // NLSPN_RESIDENT=0: the per-iteration step launches
    bool res_first = true;     // NLSPN_RES_FIRST=0: step 1 stays in front of the resident launches
    int res_split = 1;         // NLSPN_RES_SPLIT=0 / 2: a thread per quad / two threads per quad
    bool res_merge = true;     // NLSPN_RES_MERGE=0: one launch per image group
    bool res_l2 = true;        // NLSPN_RES_L2=0: every hand-off line exported (write-through)
    bool res_offcopy = true;   // NLSPN_RES_OFFCOPY=0: step 1 writes the inserted offsets
    bool res_helper = true;    // NLSPN_RES_HELPER=0: the main waves copy them in the loop, no helper wave
    int res_gy = 0, res_gx = 0;  // NLSPN_RES_GRID="gy,gx": the part grid (same images per launch)
    unsigned res_dbg = 0;      // NLSPN_RES_DBG (experiments build only, nlspn_common.h kExperiments)
};

// ------------------------------------------------- forward resident kernel: geometry
constexpr int kResMaxNT = 768;                  // launch bound (threads per part)
constexpr int kResRY = 8, kResRXQ = 2;           // fallback window halo (3x3): rows, quad columns
// the fallback halo of a kh x kw geometry: the 3x3 one plus the taps' wider base reach
NLSPN_HD constexpr int res_ry(int kh) { return kResRY + (kh > 3 ? (kh - 3) / 2 : 0); }
NLSPN_HD constexpr int res_rxq(int kw) { return kResRXQ + (kw > 3 ? ((kw - 3) / 2 + 3) / 4 : 0); }
// pixels per thread of a kh x kw geometry (a quad's 4 pixels as 1, 2 or 4 threads): the tap
// geometry of K x PX tap-pixels lives in registers (2 per tap-pixel + half a packed index), so
// PX shrinks as K grows — 3x3 (K = 8): 4; 1x17 (K = 16): 2; 5x5 (K = 24): 1; 0: not resident
// (7x7, K = 48: 4 x 48 registers of tap geometry alone pass the 168-VGPR cap)
NLSPN_HD constexpr int res_px(int kh, int kw) {
    return (kh == 3 && kw == 3) ? 4 : (kh == 1 && kw == 17) ? 2 : (kh == 5 && kw == 5) ? 1 : 0;
}
// bytes of a thread's LDS rows: the K affinities, 1 - sum, conf', dep of its PX pixels
NLSPN_HD constexpr int res_row_bytes(int K, int px) { return (K + 3) * px * 4; }
constexpr int kResPadX = 4;                      // zero columns either side of the window (keeps 16-B rows)
// The export list (per-line write-through, nlspn_resident.h): at most kResNC foreign windows
// per part (the parts on another XCC whose windows reach this part's 128-B lines), two words each
constexpr int kResNC = 28;
constexpr int kResCtl = 8 + 2 * kResNC;          // LDS control words ahead of the window
constexpr int kResAS = 11;                       // float4 per thread (3x3): K = 8 affinities, 1 - sum, conf', dep
constexpr int kResLds = 160 * 1024;              // LDS per CU

// LDS cells per copy of the f window for nt threads: what the per-thread rows leave,
// a multiple of 4 (16-B aligned copies), both copies addressable by 16-bit indices.
// (A PITCH build's copies stay within 16-bit byte addresses: at most 8,184 cells.)
NLSPN_HD constexpr int res_win_cells(int nt, int row_bytes = 16 * kResAS, int cap = 32764) {
    return ((kResLds - 4 * kResCtl - row_bytes * nt) / 8 / 4 * 4) < cap
               ? ((kResLds - 4 * kResCtl - row_bytes * nt) / 8 / 4 * 4)
               : cap;
}

// the compile-time window pitch of a fixed-thread-count build (0: the pitch is the window's
// width, a run-time value): 128 cells for 576 threads, whose two window copies span
// 2 * 7,740 cells = 61.9 KB of byte addresses (below 64 KB: 16-bit)
NLSPN_HD constexpr int res_pitch(int ntc) { return ntc == 576 ? 128 : 0; }
// the window cells per copy of a build (threads ntc, 0: nt at run time) and geometry
NLSPN_HD constexpr int res_build_cells(int ntc, int nt, int K, int px) {
    return res_win_cells(ntc ? ntc : nt, res_row_bytes(K, px), res_pitch(ntc) ? 8184 : 32764);
}
static_assert(4 * (kResCtl + 2 * res_win_cells(576)) < 65536, "576-thread window byte addresses need 16 bits");
static_assert(kResCtl % 4 == 0, "the window starts 16-B aligned");

// The sync workspace: one 128-B line per word group — [0] the abort word, [1] the count of
// parts that have finished, then per part i (blockIdx) the line kResLine * (1 + i) holding
// (word + 1) its tagged XCC id.  No two parts share a line, so a line is only ever written
// from one XCD.  The words are zero when a launch starts and zero again when it ends: the
// last part to finish (the count) clears them (res_finish), so a plan's launches need no
// clearing pass (the host clears a workspace once, before its first resident launch).
constexpr int kResLine = 32;
// the abort word's line and one 128-B line per part, up to 512 parts (nlspn_workspace_bytes)
constexpr size_t kSyncBytes = (1 + 512) * 4 * kResLine;
constexpr int kResMaxGroups = 64;  // image groups (back-to-back resident launches) per section

// ------------------------------------------------ forward resident kernel: the plan
// The part grid of a resident launch: Bg images per launch, each cut into gy row
// bands x gx quad-column bands (one workgroup per part, Bg*gy*gx <= CUs), nt threads
// (one per quad of the largest part), win_cells LDS cells per window copy.
struct ResShape {
    int Bg = 0, gy = 0, gx = 0, nt = 0, win_cells = 0;
};

// The most images per launch (fewest launches) whose parts fit one workgroup and
// whose fixed-halo window fits LDS; among the part grids of that image count, the
// one with the least estimated work per iteration: the largest part's quads plus a
// fifth per quad of its window rim restaged every iteration (a rim of ~9 px: the
// 3x3 taps at N(0,2^2) offsets).  Measured weights: C2 taps 2.4 us for 542 quads,
// staging 1.2 us for ~1350 quads.  Every CU may hold a part: with the
// poisoned-plane hand-off (a part waits only for the cells it stages) a B=1 NYU image
// in 247 parts runs 6 % faster than in 32 (same box, 222.0 k vs 209.2 k iters/s,
// profiles/r04/ab_grid_nyu_b1_r04.txt) — round 2's cap of cus / 8 parts per image (fewer
// neighbours to wait for under the flag hand-off) is gone.
inline bool res_shape(int B, int H, int W, int kh, int kw, int cus, ResShape &S) {
    const int W4 = W / 4, K = kh * kw - 1, px = res_px(kh, kw), tpq = 4 / px;
    const int ry = res_ry(kh), rxq = res_rxq(kw);
    const long long Q = (long long)H * W4;
    // the rim's reach: ~9 px for 3x3, plus the wider geometries' tap reach (1x17: 8 x 16)
    const double Ry = 9.0 + (kh - 3) / 2, Rx = 9.0 + (kw - 3) / 2;
    const auto search = [&](int Bg) {  // the best part grid for Bg images per launch
        const int gmax = (int)std::min<long long>(cus / Bg, std::max<long long>(1, Q / 64));
        double best = 1e300;
        for (int g = gmax; g >= std::max(1, gmax * 3 / 4); --g) {
            for (int gy = 1; gy <= g; ++gy) {
                if (g % gy) continue;
                const int gx = g / gy;
                if (gy > H || gx > W4) continue;
                const int ph = (H + gy - 1) / gy, pq = (W4 + gx - 1) / gx;
                const int nq = ph * pq, nt = (nq * tpq + 63) / 64 * 64;
                if (nt > kResMaxNT) continue;
                const long long cells = res_win_cells(nt, res_row_bytes(K, px));
                const long long fb = (long long)(ph + 2 * ry) * (4 * (pq + 2 * rxq) + 2 * kResPadX);
                if (cells < fb) continue;
                const double rim = ((ph + 2 * Ry) * (4.0 * pq + 2 * Rx) - 4.0 * nq) / 4.0;
                const double cost = nq + 0.2 * rim;
                if (cost < best) {
                    best = cost;
                    S.Bg = Bg; S.gy = gy; S.gx = gx; S.nt = nt; S.win_cells = (int)cells;
                }
            }
        }
        return best < 1e300;
    };
    for (int Bg = std::min(B, cus); Bg >= 1; --Bg) {
        if (!search(Bg)) continue;
        // the same number of launches with the images spread evenly: smaller parts (C5, 16
        // images: 4 groups of 4 in parts of 286 quads, not 3 of 5 and 1 of 1 in parts of 363)
        const int ng = (B + Bg - 1) / Bg, Be = (B + ng - 1) / ng;
        if (Be < Bg) search(Be);  // (feasible: more parts per image, each smaller)
        return true;
    }
    return false;
}

// The plan of a section's resident launches: what the planner needs to know of the call
// (set by the caller), then what res_plan decides.  The build of a launch is
// prop_resident_kernel<T, KH, KW, kResMaxNT, kResSMax, NTC, GROUPS, FIRST, PXO, COPY> with NTC = ntc
// (ntc_merged for a merged launch 0, GROUPS = true), FIRST = first, PXO = split;
// nlspn_prop_fwd.hip maps it to the kernel's address, and picks COPY per launch (false: the
// build without the loop's copy code, for main waves that copy nothing).
struct ResPlanRec {
    int es;  // bytes per element (2 or 4)
    int B, H, W, kh, kw, T;
    bool ptrs_ok;   // workspace and learned offsets given, every plane 16-B aligned
    bool first_ok;  // the caller can run the prologue in the launch: raw inputs and prologue
                    // outputs given and 16-B aligned, raw offset layout
    ResShape S;        // (nt and win_cells: of the split build when split != 0)
    int split = 0;     // split quads: pixels per thread (1 or 2), 0: a thread per quad
    int row_bytes = 0;
    bool pitch_ok = false;  // the largest part's fixed-halo window fits the 576-thread builds' pitch
    bool first = false;     // the prologue and iteration 1 run inside the launches
    // launch 0 runs the nfull full image groups in turn; a partial last group keeps a launch of
    // its own (its grid differs), so a merged plan has one or two launches
    bool merged = false;
    int ngroups = 0, nfull = 0;  // image groups; those of S.Bg images
    unsigned grid[kResMaxGroups] = {};  // parts per image group
    size_t lds = 0, sync_bytes = 0;
    int ntc = 0, ntc_merged = 0;  // compile-time thread counts of the builds (0: run time)
};

// Step 1 of the plan, the shape: res_shape's part grid, NLSPN_RES_GRID's instead when it
// fits, and the split-quad choice.
// Split quads: 3x3 parts of at most two waves in one image group (C1: 247 parts of 72
// quads) run four threads per quad (320 threads) or two (192), cutting each thread's
// latency-bound chain of tap-pixel slots from 32 to 8 or 16; NLSPN_RES_SPLIT=0 / 2 (A/B)
// keeps a thread per quad / forces two
inline bool res_plan_shape(int cus, const Switches &sw, ResPlanRec &R) {
    const ResPlanRec &q = R;
    const int K = q.kh * q.kw - 1, px = res_px(q.kh, q.kw), tpq = 4 / px, ry = res_ry(q.kh), rxq = res_rxq(q.kw);
    ResShape &S = R.S;
    R.row_bytes = res_row_bytes(K, px);
    if (!res_shape(q.B, q.H, q.W, q.kh, q.kw, cus, S)) return false;
    const auto window = [&](int ph, int pq) { return (long long)(ph + 2 * ry) * (4 * (pq + 2 * rxq) + 2 * kResPadX); };
    if (sw.res_gy >= 1 && sw.res_gx >= 1 && sw.res_gy <= q.H && sw.res_gx <= q.W / 4 &&
        S.Bg * sw.res_gy * sw.res_gx <= cus) {  // A/B only
        const int ph = (q.H + sw.res_gy - 1) / sw.res_gy, pq = (q.W / 4 + sw.res_gx - 1) / sw.res_gx;
        const int nt = (ph * pq * tpq + 63) / 64 * 64;
        if (nt <= kResMaxNT && window(ph, pq) <= res_win_cells(nt, R.row_bytes)) {
            S.gy = sw.res_gy; S.gx = sw.res_gx; S.nt = nt; S.win_cells = res_win_cells(nt, R.row_bytes);
        }
    }
    const int php = (q.H + S.gy - 1) / S.gy, pqp = (q.W / 4 + S.gx - 1) / S.gx;  // the largest part
    R.pitch_ok = 4 * (pqp + 2 * rxq) + 2 * kResPadX <= res_pitch(576) &&
                 (php + 2 * ry) * res_pitch(576) <= res_build_cells(576, 576, K, px);
    if (q.kh == 3 && S.nt <= 128 && q.B <= S.Bg) {
        for (int sp = sw.res_split; sp >= 1 && sp <= 2 && !R.split; ++sp) {
            const int ntc = sp == 1 ? 320 : 192, nts = (php * pqp * (4 / sp) + 63) / 64 * 64;
            const int rbs = res_row_bytes(K, sp), cells = res_win_cells(ntc, rbs);
            if (nts <= ntc && window(php, pqp) <= cells) {
                R.split = sp;
                S.nt = ntc;
                S.win_cells = cells;
                R.row_bytes = rbs;
            }
        }
    }
    return true;
}

// Step 2, the form: whether the forward prologue and iteration 1 run inside the resident
// launches (kResFirst: no step-1 launch) or step 1 stays in front of them.  `small`: the
// parts have at most two waves at a thread per quad; `want_merge`: several full image groups
// would run in one launch.
inline bool res_plan_first(const ResPlanRec &R, bool small, bool want_merge) {
    // the caller has no raw inputs for it, they are not 16-B aligned, the offsets come in the
    // inserted layout, or NLSPN_RES_FIRST=0 (A/B)
    const bool unavailable = !R.first_ok;
    // Parts of two waves (a B=1 NYU image in 247 parts of 72 quads, C1): the prologue's
    // setup work (27 raw planes, the normalisation's tanh / divisions) runs on two waves per
    // CU, slower than step 1 across the whole chip: 93.5 vs 91.6 us per section same-process
    // (profiles/r05/ab_first_r5f.json); C2 102.97 vs 107.52, C3 219.05 vs 227.37 the other
    // way.  (The four-thread split build of such parts has a prologue form and uses it.)
    const bool two_waves = small && R.split != 1;
    // The wider geometries (two or one pixel per thread) load their raw planes in 4-B (fp16
    // pairs) or smaller pieces: the prologue's loads from HBM take C5's setup 14.2 us per
    // image group where step 1's L2-hot outputs take 4.8 (traces), 690 vs 662 us per section
    // same-process (profiles/r05/ab_first_c5_r5.json): step 1 stays in front of them
    const bool narrow_loads = res_px(R.kh, R.kw) < 4;
    // the run-time-thread-count GROUPS build of the prologue form holds scratch reloads in its
    // iteration loop (tests/test_resource_usage_cpu.py): a merged multi-group launch of such a
    // shape keeps step 1 (C3's 576-thread shape has the compile-time build)
    const bool merged_run_time_nt = want_merge && !(R.S.nt == 576 && R.pitch_ok);
    return !unavailable && !two_waves && !narrow_loads && !merged_run_time_nt;
}

// The compile-time thread count of a launch's build.  The 576-thread builds have a compile-time window pitch
// (res_pitch): only when the part's fixed-halo window fits it, otherwise the run-time-width
// build.  The 128-thread build: 3x3, C1's small parts, one image group.  5x5: the
// run-time-thread-count single-group build only.  The split-quad builds: 2 pixels per thread
// at 192 threads, 1 at 320.
inline int res_ntc(const ResPlanRec &R, bool groups) {
    if (R.split) return R.split == 1 ? 320 : 192;
    return R.kh == 5 ? 0 : (R.S.nt == 576 && R.pitch_ok) ? 576 : (R.kh == 3 && R.S.nt == 128 && !groups) ? 128 : 0;
}

// Completes R and returns true when the resident kernel applies (iterations 2..T).
inline bool res_plan(int cus, const Switches &sw, ResPlanRec &R) {
    const ResPlanRec &q = R;
    if (!sw.resident) return false;  // A/B: force the per-iteration launches
    if (!q.ptrs_ok || res_px(q.kh, q.kw) == 0 || q.T < 2 || q.W % 4 != 0 || cus < 1) return false;
    const int K = q.kh * q.kw - 1;
    if ((long long)q.H * q.W * 2 * (K + 1) * q.es > 0x7fffffffLL) return false;  // 32-bit buffer offsets into an item
    if (!res_plan_shape(cus, sw, R)) return false;
    const ResShape &S = R.S;
    R.ngroups = (q.B + S.Bg - 1) / S.Bg;
    R.nfull = q.B / S.Bg;
    if (R.ngroups > kResMaxGroups) return false;
    const unsigned G = (unsigned)(S.Bg * S.gy * S.gx);
    R.sync_bytes = (size_t)(G + 1) * 4 * kResLine;
    if (R.sync_bytes > kSyncBytes) return false;
    // The full image groups run in turn inside ONE launch (ResArgs::ngroups): no launch
    // boundary between them, so a part sets up its next group while others finish the
    // current one.  NLSPN_RES_MERGE=0 (A/B) or a trace (dbg 8, one record per part) keeps
    // one launch per group.  (5x5 has no GROUPS build: one launch per image group)
    const bool want_merge = R.nfull >= 2 && sw.res_merge && q.kh != 5;
    R.first = res_plan_first(R, R.split || S.nt <= 128, want_merge);
    R.merged = want_merge && !(sw.res_dbg & 8u);
    // more than half a CU's LDS, so one workgroup per CU (a small part's window, capped at
    // res_win_cells, may need less: the request is padded)
    R.lds = std::max<size_t>(4 * kResCtl + (size_t)S.win_cells * 8 + (size_t)R.row_bytes * S.nt, 80 * 1024 + 16);
    if (R.lds > (size_t)kResLds) return false;
    for (int k = 0; k < R.ngroups; ++k)
        R.grid[k] = (unsigned)(std::min<long long>(S.Bg, q.B - (long long)k * S.Bg) * S.gy * S.gx);
    R.ntc = res_ntc(R, false);
    R.ntc_merged = res_ntc(R, true);
    return true;
}

// ------------------------------------------------------ resident backward: the plan
constexpr int kBrNT = 1024;        // threads per part
constexpr int kBrPX = 3;           // pixels per thread, at most
constexpr int kBrR = 8;            // LDS window halo (the step form's RY = RX = 8)
constexpr int kBrMaxParts = 256;   // parts per launch (one per CU)
constexpr int kBrMaxCells = 8192;  // LDS window cells (64 KiB of fixed-point sums)
constexpr int kBrLdsBytes = 150 * 1024;  // dynamic LDS: window (8 B per cell) + affinities (32 B per pixel)

// Resident pass 1 of the two-pass backward (nlspn_bwd_resident.h).
// Parts: images of one launch x (py x px) rectangles of PR x PC pixels, at most one part per CU
// (every part co-resident), PR * PC <= kBrNT * kBrPX pixels, the LDS window within kBrMaxCells.
// The most images per launch (fewest launches), then the most parts, then the shortest
// perimeter (the halo flush is the window's rim).
struct BrPlan {
    int Bl = 0, py = 0, px = 0, PR = 0, PC = 0;
};

inline bool br_plan(int B, int H, int W, int cus, BrPlan &P) {
    const int cap = std::min(cus, kBrMaxParts);
    for (int Bl = std::min(B, cap); Bl >= 1; --Bl) {
        const int ppi_max = cap / Bl;
        BrPlan best;
        long long best_n = 0, best_per = 0;
        for (int py = 1; py <= std::min(H, ppi_max); ++py) {
            const int PR = (H + py - 1) / py;
            if ((long long)(py - 1) * PR >= H) continue;  // no empty part row
            for (int px = 1; px <= std::min(W, ppi_max / py); ++px) {
                const int PC = (W + px - 1) / px;
                if ((long long)(px - 1) * PC >= W) continue;
                if ((long long)PR * PC > (long long)kBrNT * kBrPX) continue;
                const long long cells = (long long)(PR + 2 * kBrR) * (PC + 2 * kBrR);
                if (cells > kBrMaxCells || (cells + 1) * 8 + (long long)PR * PC * 32 > kBrLdsBytes) continue;
                const long long n = (long long)py * px, per = PR + PC;
                if (n > best_n || (n == best_n && per < best_per)) {
                    best_n = n; best_per = per;
                    best.Bl = Bl; best.py = py; best.px = px; best.PR = PR; best.PC = PC;
                }
            }
        }
        if (best_n > 0) { P = best; return true; }
    }
    return false;
}

#pragma GCC visibility pop
}  // namespace nlspn
