// Host-only check of the tiling contract of the split-bf16 GRU-mode convolutions
// (csrc/nlspn_gconv_x3.h): no device, no HIP header.  For every preset of NLSPN_GCX3_CONFIGS and
// every grid (several heights x widths 1..400 x several batch sizes) it plans with gc_tile (the
// launcher's function) and, for every non-empty tile gc_window (the kernel's function) cuts,
//   - stages the window as gconvx3_body does: LDS cell p of a chunk holds (cell block, input row,
//     input column) or nothing, the stride-2 rows with the even columns first;
//   - walks every pixel, every tap and every lane group g = 0..3 and requires the K = 32 B
//     fragment's cell to be one the staging wrote, holding cell block g (part g & 1 of channel
//     block g >> 1) of the convolution's own input pixel; the K = 16 B fragment (8 bytes, half
//     g & 1 of a cell) to come from the hi cell block g & 2 of that same pixel; and the two A
//     fragments to lie inside the chunk's staged weights and hold the hi part (16 bytes) and
//     half g & 1 of the lo part (8 bytes) of that same channel block (hi and lo of the same
//     channels meet in one MFMA);
//   - every 16-byte read is a whole cell inside the stage (ds_read_b128 aligned), every 8-byte
//     read a half of one (ds_read_b64 aligned).
// Also: the tiles of a band partition its pixels (every pixel covered once), each preset's LDS
// bytes are within the 160 KB budget, and GRU1's workgroup map hits every (co tile, pixel tile)
// pair once for the pixel-tile counts the batch sizes give.
// Prints one JSON object.  With arguments <preset> <gh> <gw> [bw [shift]]: that grid only, with
// the band width forced to bw (0: the planner's) and the pitch the reads use shifted by `shift`
// cells against the pitch the staging uses (to show that the check sees both defects).
// tests/test_gconv_x3_plan_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nlspn_gconv_plan.h"

using namespace nlspn;

namespace {
struct Preset {
    int id, epi, ccb, lds, wst, xst;
    GcGeo g;
};
template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CCB, int EPI>
Preset preset(int id) {
    using G = GcGeom<MODE, WM, WN, WGM, WGN, XR, XP>;
    return Preset{id, EPI, CCB, gcx3_lds_bytes(MODE, G::WGCO, XR, XP, CCB), gcx3_wst(MODE, G::WGCO, CCB),
                  gcx3_xst(XR, XP, CCB), GcGeo{MODE, G::WGCO, G::NPX, G::XR, G::XP}};
}

long long n_viol = 0, n_reads = 0, n_staged = 0;
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

struct Cell {
    int blk, row, col;  // blk < 0: nothing staged (reads as zero or as the pad)
};

bool check_grid(const Preset &p, int gh, int gw, int force_bw = 0, int shift = 0) {
    GcTiling t;
    if (!gc_tile(p.g, gh, gw, t)) return false;
    if (force_bw > 0) {
        t.bw = force_bw;
        t.nbands = (gw + t.bw - 1) / t.bw;
        t.tpb = (gh * t.bw + t.npx - 1) / t.npx;
    }
    char d[240];
    if (t.npx < 1 || t.npx > p.g.npx || (long long)t.tpb * t.npx < (long long)gh * t.bw ||
        (long long)t.nbands * t.bw < gw || (long long)(t.nbands - 1) * t.bw >= gw) {
        violation(p, t, -1, -1, "bands or tiles do not cover the grid");
        return true;
    }
    const int S = p.g.mode == kGcS2 ? 2 : 1, XP = p.g.xp, XR = p.g.xr, XPH = (XP + 1) / 2, XCS = XR * XP;
    const int XPr = XP + shift, XPHr = (XPr + 1) / 2;  // the pitch the reads use
    const int nside = p.g.mode == kGcT2 ? 2 : 3;       // conv 3 x 3; transposed: the phases' union {0, 1}^2
    const int ntapw = p.g.mode == kGcT2 ? 4 : 9, WCS = ntapw * p.g.wgco;
    std::vector<Cell> lds((size_t)p.xst);
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
            if (w.nrows > XR || w.ncols > XP || w.nrows < 1 || w.ncols < 1) {
                std::snprintf(d, sizeof d, "window %d rows x %d columns, LDS %d x %d", w.nrows, w.ncols, XR, XP);
                violation(p, t, band, tile, d);
                continue;
            }
            // the staging, as gconvx3_body's xoff: stage cell q <- (cell block, row, column) or nothing
            for (int q = 0; q < p.xst; ++q) {
                const int c = q / XCS, rem = q - c * XCS, row = rem / XP, pos = rem - row * XP;
                const int col = S == 2 ? (pos < XPH ? 2 * pos : 2 * (pos - XPH) + 1) : pos;
                const bool ok = c < p.ccb && row < w.nrows && col < w.ncols;
                lds[q] = ok ? Cell{c, row, col} : Cell{-1, 0, 0};
                n_staged += ok;
            }
            int gy = (int)(w.f0 / w.bwi), cx = (int)(w.f0 - (long long)gy * w.bwi);
            for (long long f = w.f0; f < end; ++f) {
                const int ry = gy - w.ra, gx = w.bx0 + cx;
                // the convolution's own first input cell of this pixel
                const int wy = p.g.mode == kGcT2 ? gy : S * gy - 1, wx = p.g.mode == kGcT2 ? gx : S * gx - 1;
                bool bad = false;
                for (int dy = 0; dy < nside && !bad; ++dy)
                    for (int dx = 0; dx < nside && !bad; ++dx)
                        for (int g = 0; g < 4; ++g) {
                            ++n_reads;
                            const int dcell = S == 2 ? (dx == 1 ? XPHr : dx / 2) : dx;
                            const long long q = (long long)g * XCS + (long long)(S * ry + dy) * XPr + cx + dcell;
                            const long long bytes = q * 16;
                            if (q < 0 || q >= p.xst || bytes % 16 != 0 || lds[(size_t)q].blk != g ||
                                w.iy0 + lds[(size_t)q].row != wy + dy || w.ix0 + lds[(size_t)q].col != wx + dx) {
                                std::snprintf(d, sizeof d, "pixel (%d, %d) tap (%d, %d) lane group %d: cell %lld is not that "
                                              "input cell of the staged window (%d rows x %d columns)", gy, gx, dy, dx, g, q,
                                              w.nrows, w.ncols);
                                violation(p, t, band, tile, d);
                                bad = true;
                                break;
                            }
                            // the K = 16 B fragment: half g & 1 of the hi cell of this lane group's channel block
                            const long long q2 = q - (long long)(g & 1) * XCS, bytes2 = q2 * 16 + 8 * (g & 1);
                            if (q2 < 0 || q2 >= p.xst || bytes2 % 8 != 0 || bytes2 + 8 > (q2 + 1) * 16 || lds[(size_t)q2].blk != (g & 2) ||
                                lds[(size_t)q2].row != lds[(size_t)q].row || lds[(size_t)q2].col != lds[(size_t)q].col) {
                                violation(p, t, band, tile, "the x_hi half-cell of the K = 16 product is not the hi part of that input cell");
                                bad = true;
                                break;
                            }
                            // the A fragments of this lane group: the weights' cell blocks (g & 2) and (g & 2) + 1
                            // = the hi and the lo part of channel block g >> 1, the block B's cell block g is a part of
                            const int ah = g & 2, al = ah + 1;
                            const bool same = (ah >> 1) == (g >> 1) && (al >> 1) == (g >> 1) && (ah & 1) == 0 && (al & 1) == 1;
                            const long long wlast = (long long)al * WCS + (ntapw - 1) * p.g.wgco + p.g.wgco - 1;
                            if (!same || wlast >= (long long)p.ccb * WCS || wlast >= p.wst) {
                                violation(p, t, band, tile, "a weight fragment outside the chunk's staged weights or of another channel block");
                                bad = true;
                                break;
                            }
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
#define NLSPN_GCX3_ROW(id, ...) presets.push_back(preset<__VA_ARGS__>(id));
    NLSPN_GCX3_CONFIGS(NLSPN_GCX3_ROW)
    if (argc >= 4) {
        for (const Preset &p : presets)
            if (p.id == std::atoi(argv[1]))
                check_grid(p, std::atoi(argv[2]), std::atoi(argv[3]), argc > 4 ? std::atoi(argv[4]) : 0,
                           argc > 5 ? std::atoi(argv[5]) : 0);
        std::printf("[");
        for (size_t i = 0; i < shown.size(); ++i) std::printf("%s\n %s", i ? "," : "", shown[i].c_str());
        std::printf("]\n");
        return 0;
    }
    const int heights[] = {1, 2, 3, 7, 17, 29}, batches[] = {1, 2, 8};
    long long grids = 0, refused = 0, gru_maps = 0;
    std::vector<unsigned char> seen;
    for (const Preset &p : presets)
        for (int gh : heights)
            for (int gw = 1; gw <= 400; ++gw) {
                ++grids;
                if (!check_grid(p, gh, gw)) {
                    ++refused;
                    continue;
                }
                if (p.epi != kGcEpiGru1) continue;
                GcTiling t;
                gc_tile(p.g, gh, gw, t);
                for (int B : batches)
                    for (int hc = 128; hc <= 256; hc += 128, ++gru_maps)
                        check_gru1_map(p, hc, gc_rest_count(B, t.nbands, t.tpb), seen);
            }
    std::printf("{\"grids\": %lld, \"refused\": %lld, \"reads\": %lld, \"staged\": %lld, \"gru1_maps\": %lld, \"violations\": %lld,\n \"first\": [",
                grids, refused, n_reads, n_staged, gru_maps, n_viol);
    for (size_t i = 0; i < shown.size(); ++i) std::printf("%s\n  %s", i ? "," : "", shown[i].c_str());
    std::printf("],\n \"presets\": [");
    for (size_t i = 0; i < presets.size(); ++i) {
        const Preset &p = presets[i];
        std::printf("%s\n  {\"id\": %d, \"mode\": %d, \"wgco\": %d, \"npx\": %d, \"xr\": %d, \"xp\": %d, \"ccb\": %d, \"lds\": %d, "
                    "\"chunk_channels\": %d}",
                    i ? "," : "", p.id, p.g.mode, p.g.wgco, p.g.npx, p.g.xr, p.g.xp, p.ccb, p.lds, gcx3_chunk_channels(p.ccb));
    }
    std::printf("],\n \"lds_budget\": %d}\n", kGcX3LdsBudget);
    return 0;
}
