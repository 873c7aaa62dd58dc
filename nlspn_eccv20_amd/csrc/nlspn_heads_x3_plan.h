// LDS addressing and packed sizes of the split-bf16 head epilogue (nlspn_heads_x3.h) as pure
// arithmetic: where staging writes window cell (part, channel half, row, column), which staging
// item fills it from which image element, where lane (l32, h) reads its B fragment of a tap and
// its A fragment of an M-block, and the packed weights' offsets and sizes.  No HIP header and no
// runtime call, so a host-only program can include it and walk every read of every tile
// (tests/heads_x3_plan_check.cpp, tests/test_heads_x3_cpu.py).  The kernel, the pack kernel and
// the launcher call these very functions.
#pragma once

#include "nlspn_gwgrad_plan.h"  // NLSPN_HD

namespace nlspn {
#pragma GCC visibility push(hidden)

// The tile is the f32 kernel's: 8 rows x 32 columns, 256 threads (4 waves x 2 rows), rounds of
// 16 channels.  A cell is 16 bytes = 8 bf16: one part (0 = hi, 1 = lo) of 8 consecutive channels
// (half kh of the round: channels 8 kh .. 8 kh + 7) of one window pixel; element j of a cell is
// channel 8 kh + j.  The window holds rows y0 - 1 .. y0 + 8 and columns x0 - 1 .. x0 + 32:
//   X image:  [part 2][kh 2][row 10][column 34] cells
// A lane's B fragment of tap (dy, dx) and tile row yl is cell (part, h, yl + dy, l32 + dx): the
// 32 lanes of a half read 32 consecutive cells, the halves a whole plane apart, so every 16-lane
// group of a ds_read_b128 covers 256 consecutive bytes (no bank conflict); staging writes
// consecutive cells from consecutive lanes likewise.
constexpr int kHx3TH = 8, kHx3TW = 32, kHx3NT = 256, kHx3CC = 16;
constexpr int kHx3Rows = kHx3TH + 2, kHx3Cols = kHx3TW + 2;
#ifndef NLSPN_HX3_PITCH  // (the addressing check builds a shifted pitch to see itself fail)
#define NLSPN_HX3_PITCH (kHx3TW + 2)
#endif
constexpr int kHx3Pitch = NLSPN_HX3_PITCH;           // cells per window row, as the fragment reads take it
constexpr int kHx3Plane = kHx3Rows * kHx3Cols;       // cells of one (part, kh) plane
constexpr int kHx3XCells = 4 * kHx3Plane;            // cells of a round's window (1360 = 21760 bytes)
constexpr int kHx3XItems = 2 * kHx3Plane;            // staging items: one pixel of one channel half, both parts
constexpr int kHx3XR = (kHx3XItems + kHx3NT - 1) / kHx3NT;  // per thread (3)

NLSPN_HD constexpr int hx3_x_cell(int part, int kh, int row, int col) {
    return ((part * 2 + kh) * kHx3Rows + row) * kHx3Cols + col;
}
// item i: channels 8 kh .. 8 kh + 7 of window pixel (row, col) = image (y0 - 1 + row, x0 - 1 + col);
// consecutive items are consecutive columns of a row (coalesced loads, conflict-free cell stores)
NLSPN_HD inline void hx3_x_item(int i, int &kh, int &row, int &col) {
    kh = i / kHx3Plane;
    const int rem = i - kh * kHx3Plane;
    row = rem / kHx3Cols;
    col = rem - row * kHx3Cols;
}
// the B fragment of lane (l32, h): tile row yl = 0..7, tap (dy, dx)
NLSPN_HD constexpr int hx3_b_cell(int part, int h, int yl, int dy, int l32, int dx) {
    return ((part * 2 + h) * kHx3Rows + yl + dy) * kHx3Pitch + l32 + dx;
}

// Packed weights, in exact fragment order: per round (source s, 16-channel chunk) the cells
//   [tap 9][M-block MB][part 2][lane 64]
// lane (l32, h) of M-block m holding output channel 32 m + l32, channels 8 h + j of the round.
// A round is contiguous in the packed array and is staged cell for cell, so the A fragment read
// is 64 consecutive cells.
NLSPN_HD constexpr int hx3_mb(int nout) {  // M-blocks of nout + 2 columns: 1, 2, 3 or 5 (-1: past 158)
    return (nout + 2 + 31) / 32 <= 3 ? (nout + 2 + 31) / 32 : ((nout + 2 + 31) / 32 <= 5 ? 5 : -1);
}
NLSPN_HD constexpr int hx3_w_cells(int mb) { return 9 * mb * 2 * 64; }  // of one round
NLSPN_HD constexpr int hx3_a_cell(int mb, int t, int m, int part, int lane) {
    return ((t * mb + m) * 2 + part) * 64 + lane;
}
NLSPN_HD constexpr long long hx3_w_round(int C, int s, int chunk) { return (long long)s * (C / kHx3CC) + chunk; }
NLSPN_HD constexpr long long hx3_wm_elems(int C, int mb) { return 2LL * (C / kHx3CC) * hx3_w_cells(mb) * 8; }
NLSPN_HD constexpr long long hx3_wv_floats(int C) { return 2LL * C * 9; }
NLSPN_HD constexpr long long hx3_bias_floats(int mb) { return 32LL * mb; }
// bf16 element e of the packed array -> (source, input channel of the source, tap, column, part)
struct Hx3WElem {
    int s, c, t, co, part;
};
NLSPN_HD inline Hx3WElem hx3_w_elem(long long e, int C, int mb) {
    const int j = (int)(e & 7);
    long long cell = e >> 3;
    const int lane = (int)(cell & 63);
    cell >>= 6;
    const int part = (int)(cell & 1);
    cell >>= 1;
    const int m = (int)(cell % mb);
    cell /= mb;
    const int t = (int)(cell % 9);
    const long long round = cell / 9;
    const int nch = C / kHx3CC;
    const int s = (int)(round / nch), chunk = (int)(round - (long long)s * nch);
    return Hx3WElem{s, chunk * kHx3CC + 8 * (lane >> 5) + j, t, 32 * m + (lane & 31), part};
}

// LDS bytes of a workgroup: the window, the round's weights, then the f32 kernel's VALU window
// (16 channels x 416 floats), its two sum planes and the VALU weights of all rounds
constexpr int kHx3LdsBudget = 160 * 1024;
NLSPN_HD constexpr int hx3_lds_bytes(int mb, int C) {
    return 16 * (kHx3XCells + hx3_w_cells(mb)) + 4 * (16 * 416 + 2 * kHx3NT + 2 * C * 9);
}

#pragma GCC visibility pop
}  // namespace nlspn
