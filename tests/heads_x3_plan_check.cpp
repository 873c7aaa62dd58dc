// Host-only check of the split-bf16 head epilogue's LDS addressing (csrc/nlspn_heads_x3_plan.h):
// replays the staging of a round with the kernel's own item functions into a tagged LDS image,
// then walks every A and B fragment read of the k-loop.  Each read must be 16-byte aligned,
// inside what the round staged, and hold the intended (channel, row, column) element of the
// window (or a zero where the convolution pads) / the intended (column, channel, tap, part)
// weight.  Grid: MB in {1, 2, 3, 5} x W = 1..80 x H in {1, 7, 8, 9, 17}, every tile.
// Prints "violations N" and exits 1 if N > 0.  Built with -DNLSPN_HX3_PITCH=35 (a shifted read
// pitch) it must report violations (tests/test_heads_x3_cpu.py).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "nlspn_heads_x3_plan.h"

using namespace nlspn;

namespace {

// a staged bf16 element: what it is, not its value
struct Tag {
    int16_t kind;  // 0 never written, 1 window element, 2 zero padding, 3 weight
    int16_t part, c, t;
    int32_t y, x;  // window: image row / column; weight: output column in y
};

long long violations = 0;
void bad(const char *what, int mb, int H, int W, int a, int b, int c) {
    if (violations++ < 10) std::printf("violation: %s (MB %d, H %d, W %d: %d %d %d)\n", what, mb, H, W, a, b, c);
}

void check_window(int mb, int H, int W) {
    const int tiles_x = (W + kHx3TW - 1) / kHx3TW, tiles_y = (H + kHx3TH - 1) / kHx3TH;
    std::vector<Tag> lds((size_t)kHx3XCells * 8);
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) {
            const int y0 = ty * kHx3TH, x0 = tx * kHx3TW;
            for (auto &e : lds) e = Tag{};
            // staging, as Hx3Win: thread tid takes items tid + k 256; both parts of 8 channels
            for (int tid = 0; tid < kHx3NT; ++tid)
                for (int k = 0; k < kHx3XR; ++k) {
                    const int it = tid + k * kHx3NT;
                    if (it >= kHx3XItems) continue;
                    int kh, row, col;
                    hx3_x_item(it, kh, row, col);
                    const int y = y0 - 1 + row, x = x0 - 1 + col;
                    const bool in = y >= 0 && y < H && x >= 0 && x < W;
                    // the load's clamped address is in the image
                    const int yc = y < 0 ? 0 : (y > H - 1 ? H - 1 : y), xc = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
                    if (yc < 0 || yc >= H || xc < 0 || xc >= W) bad("load outside the image", mb, H, W, it, yc, xc);
                    for (int part = 0; part < 2; ++part) {
                        const int cell = hx3_x_cell(part, kh, row, col);
                        if (cell < 0 || cell >= kHx3XCells) {
                            bad("store outside the window image", mb, H, W, it, part, cell);
                            continue;
                        }
                        for (int j = 0; j < 8; ++j) {
                            Tag &e = lds[(size_t)cell * 8 + j];
                            if (e.kind != 0) bad("cell stored twice", mb, H, W, it, part, cell);
                            e = Tag{(int16_t)(in ? 1 : 2), (int16_t)part, (int16_t)(8 * kh + j), 0, y, x};
                        }
                    }
                }
            // B fragment reads: wave wv, row n, tap t, part, lane
            for (int wv = 0; wv < 4; ++wv)
                for (int n = 0; n < 2; ++n)
                    for (int t = 0; t < 9; ++t)
                        for (int part = 0; part < 2; ++part)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int h = lane >> 5, l32 = lane & 31, yl = 2 * wv + n, dy = t / 3, dx = t % 3;
                                const long long byte = 16LL * hx3_b_cell(part, h, yl, dy, l32, dx);
                                if (byte % 16) bad("B read not 16-byte aligned", mb, H, W, t, lane, (int)byte);
                                if (byte < 0 || byte + 16 > 16LL * kHx3XCells) {
                                    bad("B read outside the staged window", mb, H, W, t, lane, (int)byte);
                                    continue;
                                }
                                const int y = y0 + yl + dy - 1, x = x0 + l32 + dx - 1;
                                const bool in = y >= 0 && y < H && x >= 0 && x < W;
                                for (int j = 0; j < 8; ++j) {
                                    const Tag &e = lds[(size_t)(byte / 2) + j];
                                    const bool ok = e.kind == (in ? 1 : 2) && e.part == part && e.c == 8 * h + j &&
                                                    e.y == y && e.x == x;
                                    if (!ok) bad("B read holds another element", mb, H, W, t, lane, j);
                                }
                            }
        }
}

void check_weights(int mb, int C) {
    const int wc = hx3_w_cells(mb);
    const long long elems = hx3_wm_elems(C, mb);
    if (elems != 2LL * C * 9 * 32 * mb * 2) bad("packed size", mb, 0, 0, C, 0, 0);
    // every packed element names one (source, channel, tap, column, part), each exactly once
    std::vector<char> seen((size_t)elems, 0);
    for (long long e = 0; e < elems; ++e) {
        const Hx3WElem w = hx3_w_elem(e, C, mb);
        if (w.s < 0 || w.s > 1 || w.c < 0 || w.c >= C || w.t < 0 || w.t > 8 || w.co < 0 || w.co >= 32 * mb || w.part < 0 ||
            w.part > 1) {
            bad("packed element out of range", mb, 0, 0, C, (int)e, 0);
            continue;
        }
        const long long id = ((((long long)w.s * C + w.c) * 9 + w.t) * 32 * mb + w.co) * 2 + w.part;
        if (seen[(size_t)id]++) bad("packed element named twice", mb, 0, 0, C, (int)e, 0);
    }
    // a round staged cell for cell; A fragment reads of (tap, M-block, part, lane)
    for (int s = 0; s < 2; ++s)
        for (int ck = 0; ck < C / kHx3CC; ++ck) {
            const long long base = hx3_w_round(C, s, ck) * wc;  // cells
            if (base < 0 || (base + wc) * 8 > elems) bad("round outside the packed array", mb, 0, 0, C, s, ck);
            for (int t = 0; t < 9; ++t)
                for (int m = 0; m < mb; ++m)
                    for (int part = 0; part < 2; ++part)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int cell = hx3_a_cell(mb, t, m, part, lane);
                            if (cell < 0 || cell >= wc) {
                                bad("A read outside the staged weights", mb, 0, 0, t, m, lane);
                                continue;
                            }
                            for (int j = 0; j < 8; ++j) {
                                const Hx3WElem w = hx3_w_elem((base + cell) * 8 + j, C, mb);
                                const bool ok = w.s == s && w.c == ck * kHx3CC + 8 * (lane >> 5) + j && w.t == t &&
                                                w.co == 32 * m + (lane & 31) && w.part == part;
                                if (!ok) bad("A read holds another weight", mb, 0, 0, t, lane, j);
                            }
                        }
        }
}

}  // namespace

int main() {
    const int mbs[] = {1, 2, 3, 5}, hs[] = {1, 7, 8, 9, 17};
    long long tiles = 0;
    for (int mb : mbs) {
        if (hx3_lds_bytes(mb, 64) > kHx3LdsBudget) bad("LDS budget", mb, 0, 0, hx3_lds_bytes(mb, 64), 0, 0);
        for (int C : {16, 64}) check_weights(mb, C);
        for (int H : hs)
            for (int W = 1; W <= 80; ++W) {
                check_window(mb, H, W);
                tiles += ((W + kHx3TW - 1) / kHx3TW) * ((H + kHx3TH - 1) / kHx3TH);
            }
    }
    const int nouts[] = {1, 24, 30, 31, 62, 63, 94, 95, 158, 159};
    const int want[] = {1, 1, 1, 2, 2, 3, 3, 5, 5, -1};
    for (int i = 0; i < 10; ++i)
        if (hx3_mb(nouts[i]) != want[i]) bad("hx3_mb", want[i], 0, 0, nouts[i], hx3_mb(nouts[i]), 0);
    std::printf("tiles %lld\nviolations %lld\n", tiles, violations);
    return violations ? 1 : 0;
}
