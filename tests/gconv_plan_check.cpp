// Host-only check of the tiling contract between the planner and the kernel of the GRU-mode
// convolutions (csrc/nlspn_gconv_plan.h): no device, no HIP header.  For every preset of
// NLSPN_GC_CONFIGS and NLSPN_GC_DG_CONFIGS and every grid gh 1..64 x gw 1..400, plus the 1/2-,
// 1/4- and 1/8-scale grids of the real image sizes, it plans with gc_tile (the launcher's
// function) and recomputes every tile's window with gc_window (the kernel's function):
//   (a) every tile of every band, the narrower last band included, has nrows <= XR, ncols <= XP;
//   (b) the non-empty tiles of a band partition its gh * bwi pixels exactly once;
//   (c) 1 <= npx <= NPX and tpb covers the widest band;
//   (d) GRU1's workgroup -> (co tile, pixel tile) map hits every pair exactly once
//       (hc 128 and 256, odd and even pixel-tile counts);
//   (e) a shape is planned within the bounds or refused, never planned with a violated bound.
// Prints one JSON object: the counts, the first violations (at most kMaxShown, and the first
// per preset), and the plans of the benchmark grids (tests/golden/gconv_plans.json).
// tests/test_gconv_plan_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nlspn_gconv_plan.h"

using namespace nlspn;

namespace {
struct Preset {
    int id, epi;
    GcGeo g;
};
template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CC, int EPI>
Preset preset(int id) {
    using G = GcGeom<MODE, WM, WN, WGM, WGN, XR, XP>;
    return Preset{id, EPI, GcGeo{MODE, G::WGCO, G::NPX, G::XR, G::XP}};
}

constexpr int kMaxShown = 40;
long long n_viol = 0;
std::vector<std::string> shown, first_of;
int last_first_id = -1;

void violation(const Preset &p, const char *rule, const GcTiling &t, int band, int tile, const char *detail) {
    char buf[512];
    std::snprintf(buf, sizeof buf,
                  "{\"preset\": %d, \"rule\": \"%s\", \"gh\": %d, \"gw\": %d, \"bw\": %d, \"nbands\": %d, \"npx\": %d, "
                  "\"tpb\": %d, \"band\": %d, \"tile\": %d, \"detail\": \"%s\"}",
                  p.id, rule, t.gh, t.gw, t.bw, t.nbands, t.npx, t.tpb, band, tile, detail);
    if (n_viol < kMaxShown) shown.push_back(buf);
    if (p.id != last_first_id) {
        last_first_id = p.id;
        first_of.push_back(buf);
    }
    ++n_viol;
}

// (a) (b) (c) (e) on one grid; returns false when the planner refuses it
// (force_npx > 0: the tile size is that, not the planner's: what the kernel would do with it)
bool check_grid(const Preset &p, int gh, int gw, int force_npx = 0) {
    GcTiling t;
    if (!gc_tile(p.g, gh, gw, t)) return false;
    if (force_npx > 0) {
        t.npx = force_npx;
        t.tpb = (gh * t.bw + t.npx - 1) / t.npx;
    }
    char d[160];
    if (t.gh != gh || t.gw != gw || t.nbands < 1 || t.bw < 1 || (long long)t.nbands * t.bw < gw ||
        (long long)(t.nbands - 1) * t.bw >= gw) {
        std::snprintf(d, sizeof d, "the bands do not cover the %d columns with a non-empty last band", gw);
        violation(p, "c", t, -1, -1, d);
        return true;
    }
    if (t.npx < 1 || t.npx > p.g.npx || (long long)t.tpb * t.npx < (long long)gh * t.bw) {
        std::snprintf(d, sizeof d, "npx outside 1..%d or tpb * npx < %d pixels of the widest band", p.g.npx, gh * t.bw);
        violation(p, "c", t, -1, -1, d);
        return true;
    }
    for (int band = 0; band < t.nbands; ++band) {
        long long covered = 0, total = -1;
        for (int tile = 0; tile < t.tpb; ++tile) {
            const GcWindow w = gc_window(p.g.mode, t.gh, t.gw, t.bw, t.npx, band, tile);
            total = (long long)gh * w.bwi;
            if (w.empty) {
                if (covered != total) {
                    std::snprintf(d, sizeof d, "an empty tile after %lld of %lld pixels", covered, total);
                    violation(p, "b", t, band, tile, d);
                }
                continue;
            }
            if (w.f0 != covered) {
                std::snprintf(d, sizeof d, "tile starts at pixel %d, %lld covered", w.f0, covered);
                violation(p, "b", t, band, tile, d);
            }
            covered = w.f0 + t.npx < total ? w.f0 + t.npx : total;
            if (w.nrows > p.g.xr || w.ncols > p.g.xp || w.nrows < 1 || w.ncols < 1) {
                std::snprintf(d, sizeof d, "band width %d, grid rows %d..%d: window %d rows x %d columns, LDS %d x %d", w.bwi,
                              w.ra, w.rb, w.nrows, w.ncols, p.g.xr, p.g.xp);
                violation(p, "a", t, band, tile, d);
            }
        }
        if (covered != total) {
            std::snprintf(d, sizeof d, "%lld of %lld pixels covered", covered, total);
            violation(p, "b", t, band, t.tpb, d);
        }
    }
    return true;
}

// (d) for nr pixel tiles
void check_gru1_map(const Preset &p, int hc, int nr, std::vector<unsigned char> &seen) {
    const int co_tiles = 3 * hc / p.g.wgco, nh = gc_gru1_heavy_cots(hc, p.g.wgco);
    const int nwg = gc_gru1_wgs(hc, p.g.wgco, co_tiles, nr);
    seen.assign((size_t)co_tiles * nr, 0);
    GcTiling t{0, 0, 0, hc, nr, 0};  // (reported: nbands = hc, tpb = nr)
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
    if (bad) violation(p, "d", t, -1, -1, "GRU1 workgroups do not hit every (co tile, pixel tile) pair once");
}

int half(int n, int k) {
    for (; k > 0; --k) n = (n - 1) / 2 + 1;
    return n;
}
}  // namespace

int main(int argc, char **argv) {
    std::vector<Preset> presets;
#define NLSPN_GC_ROW(id, ...) presets.push_back(preset<__VA_ARGS__>(id));
    NLSPN_GC_CONFIGS(NLSPN_GC_ROW)
    NLSPN_GC_DG_CONFIGS(NLSPN_GC_ROW)
    if (argc >= 4) {  // one grid: gconv_plan_check <preset id> <gh> <gw> [npx] prints its violations
        for (const Preset &p : presets)
            if (p.id == std::atoi(argv[1]))
                check_grid(p, std::atoi(argv[2]), std::atoi(argv[3]), argc > 4 ? std::atoi(argv[4]) : 0);
        std::printf("[");
        for (size_t i = 0; i < shown.size(); ++i) std::printf("%s\n %s", i ? "," : "", shown[i].c_str());
        std::printf("]\n");
        return 0;
    }
    const int images[4][2] = {{480, 640}, {375, 1242}, {352, 1216}, {228, 304}};
    long long grids = 0, refused = 0, gru_maps = 0;
    std::vector<unsigned char> seen;
    for (const Preset &p : presets) {
        for (int gh = 1; gh <= 64; ++gh)
            for (int gw = 1; gw <= 400; ++gw) {
                ++grids;
                if (!check_grid(p, gh, gw)) ++refused;
            }
        for (const auto &im : images)
            for (int k = 1; k <= 3; ++k) {
                ++grids;
                if (!check_grid(p, half(im[0], k), half(im[1], k))) ++refused;
            }
        if (p.epi != kGcEpiGru1) continue;
        for (int hc = 128; hc <= 256; hc += 128) {
            for (int nr = 1; nr <= 512; ++nr, ++gru_maps) check_gru1_map(p, hc, nr, seen);
            // the pixel-tile counts of real launches: B = 1..3 images of the 1/8-scale grids
            for (const auto &im : images)
                for (int B = 1; B <= 3; ++B) {
                    GcTiling t;
                    if (!gc_tile(p.g, half(im[0], 3), half(im[1], 3), t)) continue;
                    check_gru1_map(p, hc, gc_rest_count(B, t.nbands, t.tpb), seen);
                    ++gru_maps;
                }
        }
    }
    // the plans of the benchmark grids (NYU 228x304 and KITTI 240x1216: the 1/8-, 1/4- and
    // 1/2-scale grids the encoders write and the decoder's layers read), every preset
    const int bench[][2] = {{29, 38}, {30, 152}, {57, 76}, {60, 304}, {58, 76}, {114, 152}, {116, 152}, {120, 608}};
    std::printf("{\"grids\": %lld, \"refused\": %lld, \"gru1_maps\": %lld, \"violations\": %lld,\n \"first\": [", grids, refused,
                gru_maps, n_viol);
    for (size_t i = 0; i < shown.size(); ++i) std::printf("%s\n  %s", i ? "," : "", shown[i].c_str());
    std::printf("],\n \"first_per_preset\": [");
    for (size_t i = 0; i < first_of.size(); ++i) std::printf("%s\n  %s", i ? "," : "", first_of[i].c_str());
    std::printf("],\n \"plans\": [");
    bool sep = false;
    for (const Preset &p : presets)
        for (const auto &g : bench) {
            GcTiling t;
            const bool ok = gc_tile(p.g, g[0], g[1], t);
            std::printf("%s\n  {\"preset\": %d, \"gh\": %d, \"gw\": %d, \"planned\": %s, \"bw\": %d, \"nbands\": %d, \"npx\": %d, "
                        "\"tpb\": %d}", sep ? "," : "", p.id, g[0], g[1], ok ? "true" : "false", t.bw, t.nbands, t.npx, t.tpb);
            sep = true;
        }
    std::printf("]}\n");
    return 0;
}
