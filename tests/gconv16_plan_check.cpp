// Host-only check of the tiling contract of the f16-operand GRU-mode convolutions
// (csrc/nlspn_gconv16.h): no device, no HIP header.  For every preset of NLSPN_GC16_CONFIGS and
// every grid gh 1..64 x gw 1..400 it plans with gc_tile (the launcher's function) and, for every
// non-empty tile gc_window (the kernel's function) cuts, walks EVERY pixel of the tile and EVERY
// tap of that pixel and requires the cell the kernel reads to lie inside the staged window: its
// row within nrows <= XR, its column within ncols <= XP, and, for the stride-2 presets, its
// even / odd-split cell inside the row's XP cells and equal to the cell the staging writes that
// column to.  (The property the 20 | 19 band defect of the f32 family violated.)  Also: the tiles
// of a band partition its pixels, each preset's LDS bytes are within the 160 KB budget, and
// GRU1's workgroup map hits every (co tile, pixel tile) pair once.
// Prints one JSON object.  With arguments <preset> <gh> <gw> [npx]: that grid only (npx forces
// the tile size, to show that the check sees an oversized tile).  tests/test_gconv16_plan_cpu.py
// builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nlspn_gconv_plan.h"

using namespace nlspn;

namespace {
struct Preset {
    int id, epi, ccb, lds;
    GcGeo g;
};
template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CCB, int EPI>
Preset preset(int id) {
    using G = GcGeom<MODE, WM, WN, WGM, WGN, XR, XP>;
    return Preset{id, EPI, CCB, gc16_lds_bytes(MODE, G::WGCO, XR, XP, CCB), GcGeo{MODE, G::WGCO, G::NPX, G::XR, G::XP}};
}

long long n_viol = 0, n_taps = 0;
std::vector<std::string> shown;

void violation(const Preset &p, const GcTiling &t, int band, int tile, const char *detail) {
    char buf[512];
    std::snprintf(buf, sizeof buf,
                  "{\"preset\": %d, \"gh\": %d, \"gw\": %d, \"bw\": %d, \"nbands\": %d, \"npx\": %d, \"tpb\": %d, "
                  "\"band\": %d, \"tile\": %d, \"detail\": \"%s\"}",
                  p.id, t.gh, t.gw, t.bw, t.nbands, t.npx, t.tpb, band, tile, detail);
    if (n_viol < 40) shown.push_back(buf);
    ++n_viol;
}

bool check_grid(const Preset &p, int gh, int gw, int force_npx = 0) {
    GcTiling t;
    if (!gc_tile(p.g, gh, gw, t)) return false;
    if (force_npx > 0) {
        t.npx = force_npx;
        t.tpb = (gh * t.bw + t.npx - 1) / t.npx;
    }
    char d[200];
    if (t.npx < 1 || (force_npx == 0 && t.npx > p.g.npx) || (long long)t.tpb * t.npx < (long long)gh * t.bw ||
        (long long)t.nbands * t.bw < gw || (long long)(t.nbands - 1) * t.bw >= gw) {
        violation(p, t, -1, -1, "bands or tiles do not cover the grid");
        return true;
    }
    const int S = p.g.mode == kGcS2 ? 2 : 1, XP = p.g.xp, XPH = (XP + 1) / 2;
    const int nside = p.g.mode == kGcT2 ? 2 : 3, ntap = nside * nside;  // conv 3 x 3; transposed: the phases' union {0, 1}^2
    for (int band = 0; band < t.nbands; ++band) {
        long long covered = 0, total = -1;
        for (int tile = 0; tile < t.tpb; ++tile) {
            const GcWindow w = gc_window(p.g.mode, t.gh, t.gw, t.bw, t.npx, band, tile);
            total = (long long)gh * w.bwi;
            if (w.empty) {
                if (covered != total) violation(p, t, band, tile, "an empty tile before the band's last pixel");
                continue;
            }
            if (w.f0 != covered) violation(p, t, band, tile, "tiles do not partition the band");
            const long long end = w.f0 + t.npx < total ? w.f0 + t.npx : total;
            covered = end;
            if (w.nrows > p.g.xr || w.ncols > XP || w.nrows < 1 || w.ncols < 1) {
                std::snprintf(d, sizeof d, "window %d rows x %d columns, LDS %d x %d", w.nrows, w.ncols, p.g.xr, XP);
                violation(p, t, band, tile, d);
                continue;
            }
            // every tap of every pixel, addressed as gconv16_body addresses it.  A tap (dy, dx) lies
            // inside the window iff its row (a function of dy alone, increasing) and its column (of dx
            // alone) do, so a pixel's taps are checked as its first and last row and each of its columns.
            int gy = (int)(w.f0 / w.bwi), cx = (int)(w.f0 - (long long)gy * w.bwi);
            for (long long f = w.f0; f < end; ++f) {
                const int ry = gy - w.ra;
                n_taps += ntap;
                const int row0 = S * ry, row1 = S * ry + nside - 1;
                bool bad = row0 < 0 || row1 >= w.nrows || row1 >= p.g.xr;
                for (int x = 0; x < nside; ++x) {
                    const int col = S * cx + x;
                    // the cell the kernel reads, and the cell the staging puts column `col` at
                    const int rd = S == 2 ? cx + (x == 1 ? XPH : x / 2) : cx + x;
                    const int st = S == 2 ? (col & 1) * XPH + col / 2 : col;
                    bad = bad || col >= w.ncols || rd != st || rd >= XP || (S == 2 && !(col & 1) && rd >= XPH);
                }
                // the input cell the pixel's first tap stands for is the convolution's own (the others follow: linear)
                const int gx = w.bx0 + cx;
                const int wy = p.g.mode == kGcT2 ? gy : S * gy - 1, wx = p.g.mode == kGcT2 ? gx : S * gx - 1;
                bad = bad || w.iy0 + row0 != wy || w.ix0 + S * cx != wx;
                if (bad) {
                    std::snprintf(d, sizeof d, "pixel (%d, %d): a tap outside the window: rows %d..%d of %d, columns from %d of %d",
                                  gy, gx, row0, row1, w.nrows, S * cx, w.ncols);
                    violation(p, t, band, tile, d);
                }
                if (++cx == w.bwi) { cx = 0; ++gy; }
            }
        }
        if (covered != total) violation(p, t, band, t.tpb, "the band's pixels are not all covered");
    }
    return true;
}

void check_gru1_map(const Preset &p, int hc, int nr, std::vector<unsigned char> &seen) {
    const int co_tiles = 3 * hc / p.g.wgco, nh = gc_gru1_heavy_cots(hc, p.g.wgco);
    const int nwg = gc_gru1_wgs(hc, p.g.wgco, co_tiles, nr);
    seen.assign((size_t)co_tiles * nr, 0);
    bool bad = nh < 1 || nh >= co_tiles || (3 * hc) % p.g.wgco != 0 || (2 * hc) % p.g.wgco != 0;
    for (int wg = 0; wg < nwg && !bad; ++wg) {
        int cot, r[2];
        gc_gru1_map(wg, nh, nr, co_tiles, cot, r[0], r[1]);
        for (int k = 0; k < 2; ++k) {
            if (r[k] < 0 && k == 1) continue;
            if (cot < 0 || cot >= co_tiles || r[k] < 0 || r[k] >= nr || seen[(size_t)cot * nr + r[k]]++) bad = true;
        }
    }
    for (size_t i = 0; i < seen.size() && !bad; ++i) bad = seen[i] != 1;
    GcTiling t{0, 0, 0, hc, nr, 0};
    if (bad) violation(p, t, -1, -1, "GRU1 workgroups do not hit every (co tile, pixel tile) pair once");
}
}  // namespace

int main(int argc, char **argv) {
    std::vector<Preset> presets;
#define NLSPN_GC16_ROW(id, ...) presets.push_back(preset<__VA_ARGS__>(id));
    NLSPN_GC16_CONFIGS(NLSPN_GC16_ROW)
    if (argc >= 4) {
        for (const Preset &p : presets)
            if (p.id == std::atoi(argv[1])) check_grid(p, std::atoi(argv[2]), std::atoi(argv[3]), argc > 4 ? std::atoi(argv[4]) : 0);
        std::printf("[");
        for (size_t i = 0; i < shown.size(); ++i) std::printf("%s\n %s", i ? "," : "", shown[i].c_str());
        std::printf("]\n");
        return 0;
    }
    long long grids = 0, refused = 0, gru_maps = 0;
    std::vector<unsigned char> seen;
    for (const Preset &p : presets) {
        for (int gh = 1; gh <= 64; ++gh)
            for (int gw = 1; gw <= 400; ++gw) {
                ++grids;
                if (!check_grid(p, gh, gw)) ++refused;
            }
        if (p.epi != kGcEpiGru1) continue;
        for (int hc = 128; hc <= 256; hc += 128)
            for (int nr = 1; nr <= 512; ++nr, ++gru_maps) check_gru1_map(p, hc, nr, seen);
    }
    std::printf("{\"grids\": %lld, \"refused\": %lld, \"taps\": %lld, \"gru1_maps\": %lld, \"violations\": %lld,\n \"first\": [",
                grids, refused, n_taps, gru_maps, n_viol);
    for (size_t i = 0; i < shown.size(); ++i) std::printf("%s\n  %s", i ? "," : "", shown[i].c_str());
    std::printf("],\n \"presets\": [");
    for (size_t i = 0; i < presets.size(); ++i) {
        const Preset &p = presets[i];
        std::printf("%s\n  {\"id\": %d, \"mode\": %d, \"wgco\": %d, \"npx\": %d, \"xr\": %d, \"xp\": %d, \"ccb\": %d, \"lds\": %d}",
                    i ? "," : "", p.id, p.g.mode, p.g.wgco, p.g.npx, p.g.xr, p.g.xp, p.ccb, p.lds);
    }
    std::printf("],\n \"lds_budget\": %d}\n", kGc16LdsBudget);
    return 0;
}
