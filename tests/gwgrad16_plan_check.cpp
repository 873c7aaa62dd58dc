// Host-only check of the plan and the LDS addressing of the split-bf16 weight gradient
// (csrc/nlspn_gwgrad16.h): no device, no HIP header.  For each of the three tilings x Ws 1..400 x
// a few (B, Hs) from 1 x 1, and at stride 2 the cropped large sizes (2 Ws - 1 x 2 Hs - 1, and 7
// short as decode_aff's last layer), it plans with gw16_plan (the launcher's function) and walks every
// unit of every slice for the last channel tile (the one with channels past the counts).  Per
// unit it replays the staging items exactly as the kernel decodes them (gw16_a_item /
// gw16_b_item / gw16_b_wc, the zero rules) into a map "LDS element -> tensor element or zero",
// then walks every read of the k-loop: k-step, lane group, element, tap, part and channel.
// Each read must start at a multiple of eight elements (16 bytes, the read's width), lie inside
// the stage and inside what the staging wrote for this unit, and hold the correlation's own
// element: A the small tensor's (row, bx0 + pixel), zero past the band and the channels; B the
// large tensor's (S sy - 1 + ky, S (bx0 + pixel) - 1 + kx), zero outside the stored size and
// past the channels (past the band, where A is zero, any staged cell).  The units of all slices
// must hit every (image, small row, band) exactly once, and a tiling's LDS stay within 160 KB.
// Prints one JSON object.  With arguments
//     <stride> <Cs> <Cl> <B> <Hs> <Ws> <Hl> <Wl> [force_bw] [read_shift]
// that shape only: its plan and its violations (force_bw: a band width the plan would not
// choose; read_shift: elements added to every read address, as a wrong pitch would), to show
// that the check is not vacuous.  tests/test_gwgrad16_plan_cpu.py builds and runs it.
//
// A first argument "f32" selects the f32 weight gradient's plan (gw_plan, csrc/nlspn_gwgrad_plan.h,
// the launcher's function; its kernels' LDS addressing is checked on the device, per element):
//     f32 <stride> <Cs> <Cl> <B> <Hs> <Ws> <Hl> <Wl>
// prints that shape's plan; "f32" alone sweeps the four f32 tilings x Ws 1..400 x the same
// (B, Hs) and cropped sizes: the band widths sum to Ws and none is wider than kGwBW, the slices
// hit every unit exactly once ((nsl - 1) ups < units <= nsl ups), the tiles cover the channels
// and floats = slab nsl + nsb max(Cs, Cl).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nlspn_gwgrad16_plan.h"

using namespace nlspn;

namespace {
struct Cell {
    int gen, ch, y, x;  // ch < 0: a stored zero
};
struct Shape {
    int stride, Cs, Cl, B, Hs, Ws, Hl, Wl;
};

long long n_viol = 0, n_reads = 0, n_units = 0, n_decode_bad = 0;
std::vector<std::string> shown;
std::vector<Cell> lds;
int gen = 0;

void violation(const Shape &s, const Gw16Plan &p, int u, const char *detail) {
    char buf[640];
    std::snprintf(buf, sizeof buf,
                  "{\"stride\": %d, \"Cs\": %d, \"Cl\": %d, \"B\": %d, \"Hs\": %d, \"Ws\": %d, \"Hl\": %d, \"Wl\": %d, "
                  "\"tiling\": %d, \"bw\": %d, \"nbands\": %d, \"unit\": %d, \"detail\": \"%s\"}",
                  s.stride, s.Cs, s.Cl, s.B, s.Hs, s.Ws, s.Hl, s.Wl, p.tiling, p.bw, p.nbands, u, detail);
    if (n_viol < 40) shown.push_back(buf);
    ++n_viol;
}

void put(int off, int ch, int y, int x) {
    if (off < 0 || off >= (int)lds.size()) return;  // (a read of it is then reported as not staged)
    lds[off] = Cell{gen, ch, y, x};
}

// the staging of unit n for the channel tiles at cs0 / cl0, as gwgrad16_kernel's load() and store()
void stage(const Shape &s, const Gw16Geo &g, const Gw16Unit &n, int cs0, int cl0) {
    const int S = g.S, MT = g.mt(), NT = g.nt();
    ++gen;
    for (int i = 0; i < gw16_a_items(MT); ++i) {
        int c, pp;
        gw16_a_item(i, c, pp);
        for (int e = 0; e < 2; ++e) {
            const int p = 2 * pp + e;
            const bool ok = cs0 + c < s.Cs && p < n.bwi;
            for (int part = 0; part < 2; ++part) put(gw16_a_off(c, part, p), ok ? cs0 + c : -1, n.sy, n.bx0 + p);
        }
    }
    const int ly0 = S * n.sy - 1, lx0 = S * n.bx0 - 1, ncol = gw16_ncol(S, n.bwi);
    for (int i = 0; i < gw16_b_items(NT); ++i) {
        int c, ky, pp;
        {   // the kernel's decode by pass is the item's
            const int nthr = g.nthr(), tid = i % nthr, k = i / nthr;
            gw16_b_item(i, NT, c, ky, pp);
            if (NT % gw16_pass_rows(nthr) != 0 || pp != tid % (kGw16BW / 2) || ky != gw16_b_pass_ky(NT, nthr, k) ||
                c != tid / (kGw16BW / 2) + gw16_b_pass_c(NT, nthr, k)) {
                ++n_decode_bad;
                continue;
            }
        }
        gw16_b_item(i, NT, c, ky, pp);
        const int ly = ly0 + ky;
        const bool rowok = cl0 + c < s.Cl && ly >= 0 && ly < s.Hl;
        int vx[8];
        bool vok[8];
        for (int j = 0; j < gw16_b_loads(S); ++j) {
            const int wc = gw16_b_wc(S, pp, j);
            vx[j] = lx0 + wc;
            vok[j] = rowok && wc < ncol && vx[j] >= 0 && vx[j] < s.Wl;
        }
        for (int kx = 0; kx < 3; ++kx)
            for (int e = 0; e < 2; ++e) {
                const int j = kx + e * S;
                for (int part = 0; part < 2; ++part)
                    put(gw16_b_off(MT, c, ky, kx, part, 2 * pp + e), vok[j] ? cl0 + c : -1, ly, vx[j]);
            }
    }
}

// every read of unit n's k-loop
void reads(const Shape &s, const Gw16Plan &p, int u, const Gw16Unit &n, int cs0, int cl0, int shift) {
    const Gw16Geo &g = p.g;
    const int S = g.S, MT = g.mt(), NT = g.nt(), stage_elems = g.stage_elems();
    char d[240];
    for (int ks = 0; ks < n.nks; ++ks)
        for (int lg = 0; lg < 4; ++lg) {
            const int px0 = gw16_frag_px(ks, lg);
            for (int part = 0; part < 2; ++part) {
                for (int c = 0; c < MT; ++c) {
                    const int off = gw16_a_off(c, part, px0) + shift;
                    ++n_reads;
                    if (off % 8 != 0 || off < 0 || off + 8 > MT * kGw16AP) {
                        std::snprintf(d, sizeof d, "A read at element %d: misaligned or outside the A region", off);
                        violation(s, p, u, d);
                        continue;
                    }
                    for (int j = 0; j < 8; ++j) {
                        const Cell &q = lds[off + j];
                        const int px = px0 + j;
                        const bool want = cs0 + c < s.Cs && px < n.bwi;
                        const bool ok = q.gen == gen && (want ? q.ch == cs0 + c && q.y == n.sy && q.x == n.bx0 + px : q.ch < 0);
                        if (!ok) {
                            std::snprintf(d, sizeof d, "A channel %d pixel %d part %d: %s", c, px, part,
                                          q.gen != gen ? "not staged for this unit" : want ? "not the small tensor's element" : "not zero past the band / the channels");
                            violation(s, p, u, d);
                        }
                    }
                }
                for (int c = 0; c < NT; ++c)
                    for (int t = 0; t < 9; ++t) {
                        const int ky = t / 3, kx = t % 3;
                        const int off = gw16_b_off(MT, c, ky, kx, part, px0) + shift;
                        ++n_reads;
                        if (off % 8 != 0 || off < MT * kGw16AP || off + 8 > stage_elems) {
                            std::snprintf(d, sizeof d, "B read at element %d: misaligned or outside the B region", off);
                            violation(s, p, u, d);
                            continue;
                        }
                        for (int j = 0; j < 8; ++j) {
                            const Cell &q = lds[off + j];
                            const int px = px0 + j;
                            const int ly = S * n.sy - 1 + ky, lx = S * (n.bx0 + px) - 1 + kx;
                            bool ok = q.gen == gen;
                            if (ok && px < n.bwi) {
                                const bool want = cl0 + c < s.Cl && ly >= 0 && ly < s.Hl && lx >= 0 && lx < s.Wl;
                                ok = want ? q.ch == cl0 + c && q.y == ly && q.x == lx : q.ch < 0;
                            }
                            if (!ok) {
                                std::snprintf(d, sizeof d, "B channel %d tap (%d, %d) pixel %d part %d: %s", c, ky, kx, px, part,
                                              q.gen != gen ? "not staged for this unit" : "not the correlation's element (or zero)");
                                violation(s, p, u, d);
                            }
                        }
                    }
            }
        }
}

Gw16Plan check_shape(const Shape &s, int force_bw = 0, int shift = 0) {
    Gw16Plan p = gw16_plan(s.stride, s.Cs, s.Cl, s.B, s.Hs, s.Ws, s.Hl, s.Wl);
    if (p.tiling == kGw16F32) return p;
    if (force_bw > 0) {
        p.bw = force_bw;
        p.nbands = (s.Ws + p.bw - 1) / p.bw;
        p.units = s.B * s.Hs * p.nbands;
        p.ups = (p.units + p.nsl - 1) / p.nsl;
        p.nsl = (p.units + p.ups - 1) / p.ups;
        p.bias_off = p.slab * p.nsl;
        p.floats = p.bias_off + (long long)p.nsb * (s.Cs > s.Cl ? s.Cs : s.Cl);
    }
    const Gw16Geo &g = p.g;
    if (g.lds_bytes() > kGw16LdsBudget) violation(s, p, -1, "LDS over the budget");
    if (p.bw < 1 || (long long)p.nbands * p.bw < s.Ws || (long long)(p.nbands - 1) * p.bw >= s.Ws || p.nsl < 1 ||
        (long long)p.nsl * p.ups < p.units || (long long)(p.nsl - 1) * p.ups >= p.units ||
        p.mtiles * g.mt() < s.Cs || p.ntiles * g.nt() < s.Cl ||
        p.floats != p.slab * p.nsl + (long long)p.nsb * (s.Cs > s.Cl ? s.Cs : s.Cl)) {
        violation(s, p, -1, "bands, slices or tiles do not cover the problem");
        return p;
    }
    lds.assign((size_t)g.stage_elems(), Cell{0, 0, 0, 0});
    gen = 0;
    const int cs0 = (p.mtiles - 1) * g.mt(), cl0 = (p.ntiles - 1) * g.nt();
    std::vector<int> hit((size_t)s.B * s.Hs * p.nbands, 0);
    for (int sl = 0; sl < p.nsl; ++sl) {
        const int u0 = sl * p.ups, u1 = p.units < u0 + p.ups ? p.units : u0 + p.ups;
        if (u0 >= u1) violation(s, p, u0, "an empty slice");
        for (int u = u0; u < u1; ++u) {
            const Gw16Unit n = gw16_unit(u, p.nbands, p.bw, s.Hs, s.Ws);
            ++n_units;
            if (n.b < 0 || n.b >= s.B || n.sy < 0 || n.sy >= s.Hs || n.bwi < 1 || n.bx0 + n.bwi > s.Ws) {
                violation(s, p, u, "a unit outside the small tensor");
                continue;
            }
            ++hit[((size_t)n.b * s.Hs + n.sy) * p.nbands + n.bx0 / p.bw];
            stage(s, g, n, cs0, cl0);
            reads(s, p, u, n, cs0, cl0, shift);
        }
    }
    if (n_decode_bad) {
        violation(s, p, -1, "a thread's B row in a pass is not its item's (gw16_b_pass_c / gw16_b_pass_ky)");
        n_decode_bad = 0;
    }
    for (size_t i = 0; i < hit.size(); ++i)
        if (hit[i] != 1) {
            violation(s, p, (int)i, "the units do not hit every (image, small row, band) exactly once");
            break;
        }
    return p;
}

// ---- the f32 plan
long long f32_grids = 0;
void f32_violation(const Shape &s, const GwPlan &p, const char *detail) {
    char buf[640];
    std::snprintf(buf, sizeof buf,
                  "{\"stride\": %d, \"Cs\": %d, \"Cl\": %d, \"B\": %d, \"Hs\": %d, \"Ws\": %d, \"Hl\": %d, \"Wl\": %d, "
                  "\"bw\": %d, \"nbands\": %d, \"units\": %d, \"ups\": %d, \"nsl\": %d, \"detail\": \"%s\"}",
                  s.stride, s.Cs, s.Cl, s.B, s.Hs, s.Ws, s.Hl, s.Wl, p.bw, p.nbands, p.units, p.ups, p.nsl, detail);
    if (n_viol < 40) shown.push_back(buf);
    ++n_viol;
}
void f32_check_shape(const Shape &s, const GwGeo &want) {
    const GwPlan p = gw_plan(s.stride, s.Cs, s.Cl, s.B, s.Hs, s.Ws, s.Hl, s.Wl);
    ++f32_grids;
    if (p.g.S != want.S || p.g.wm != want.wm || p.g.wgm != want.wgm || p.g.wgn != want.wgn)
        f32_violation(s, p, "the tiling rule picked another tiling");
    long long sum = 0;
    bool widths_ok = p.nbands >= 1 && p.bw >= 1 && p.bw <= kGwBW;
    for (int i = 0; widths_ok && i < p.nbands; ++i) {
        const int w = p.bw < s.Ws - i * p.bw ? p.bw : s.Ws - i * p.bw;  // as the kernel cuts band i
        widths_ok = w >= 1;
        sum += w;
    }
    if (!widths_ok || sum != s.Ws) f32_violation(s, p, "the band widths do not sum to Ws within kGwBW each");
    if (p.units != s.B * s.Hs * p.nbands) f32_violation(s, p, "units is not B Hs nbands");
    if (p.nsl < 1 || p.ups < 1 || (long long)(p.nsl - 1) * p.ups >= p.units || (long long)p.nsl * p.ups < p.units)
        f32_violation(s, p, "the slices do not hit every unit exactly once");
    if (p.mtiles * p.g.mt() < s.Cs || (p.mtiles - 1) * p.g.mt() >= s.Cs || p.ntiles * p.g.nt() < s.Cl ||
        (p.ntiles - 1) * p.g.nt() >= s.Cl || p.slab != (long long)p.mtiles * p.g.mt() * p.ntiles * p.g.nt() * 9)
        f32_violation(s, p, "the tiles do not cover the channels, or the slab is not theirs");
    if (p.nsb < 1 || p.nsb > kGwMaxBiasSlices || p.bias_off != p.slab * p.nsl ||
        p.floats != p.slab * p.nsl + (long long)p.nsb * (s.Cs > s.Cl ? s.Cs : s.Cl))
        f32_violation(s, p, "floats is not slab nsl + nsb max(Cs, Cl)");
}

void print_shown() {
    std::printf("[");
    for (size_t i = 0; i < shown.size(); ++i) std::printf("%s\n  %s", i ? "," : "", shown[i].c_str());
    std::printf("]");
}
}  // namespace

int f32_main(int argc, char **argv) {
    if (argc >= 10) {
        int v[8];
        for (int i = 0; i < 8; ++i) v[i] = std::atoi(argv[i + 2]);
        const GwPlan p = gw_plan(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
        std::printf("{\"S\": %d, \"wm\": %d, \"wgm\": %d, \"wgn\": %d, \"mt\": %d, \"nt\": %d, \"nthr\": %d, \"mtiles\": %d, "
                    "\"ntiles\": %d, \"bw\": %d, \"nbands\": %d, \"units\": %d, \"ups\": %d, \"nsl\": %d, \"nsb\": %d, "
                    "\"slab\": %lld, \"bias_off\": %lld, \"floats\": %lld}\n",
                    p.g.S, p.g.wm, p.g.wgm, p.g.wgn, p.g.mt(), p.g.nt(), p.g.nthr(), p.mtiles, p.ntiles, p.bw, p.nbands, p.units,
                    p.ups, p.nsl, p.nsb, p.slab, p.bias_off, p.floats);
        return 0;
    }
    // the channel counts of each tiling: a last tile with channels past the counts where the tile allows
    struct Case { GwGeo g; int stride, Cs, Cl; };
    const Case cases[] = {{{1, 2, 2, 2}, 1, 136, 40}, {{2, 2, 2, 2}, 2, 136, 40}, {{2, 2, 4, 1}, 2, 136, 9}, {{2, 1, 1, 1}, 2, 16, 9}};
    const int bh[][2] = {{1, 1}, {2, 2}};
    for (const Case &c : cases)
        for (int Ws = 1; Ws <= 400; ++Ws) {
            for (const auto &q : bh) f32_check_shape(Shape{c.stride, c.Cs, c.Cl, q[0], q[1], Ws, c.stride * q[1], c.stride * Ws}, c.g);
            if (c.stride != 2) continue;
            if (2 * Ws - 1 >= 1) f32_check_shape(Shape{2, c.Cs, c.Cl, 1, 1, Ws, 1, 2 * Ws - 1}, c.g);
            if (2 * Ws - 7 >= 1) f32_check_shape(Shape{2, c.Cs, c.Cl, 1, 4, Ws, 1, 2 * Ws - 7}, c.g);
        }
    std::printf("{\"grids\": %lld, \"violations\": %lld, \"band_max\": %d, \"target_wgs\": %d, \"bias_slices_max\": %d,\n \"first\": ",
                f32_grids, n_viol, kGwBW, kGwTargetWgs, kGwMaxBiasSlices);
    print_shown();
    std::printf("}\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "f32") return f32_main(argc, argv);
    if (argc >= 9) {
        int v[10] = {0};
        for (int i = 1; i < argc && i <= 10; ++i) v[i - 1] = std::atoi(argv[i]);
        const Shape s{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
        const Gw16Plan p = check_shape(s, v[8], v[9]);
        std::printf("{\"tiling\": %d, \"mt\": %d, \"nt\": %d, \"nthr\": %d, \"lds\": %d, \"mtiles\": %d, \"ntiles\": %d, \"bw\": %d, "
                    "\"nbands\": %d, \"units\": %d, \"ups\": %d, \"nsl\": %d, \"nsb\": %d, \"slab\": %lld, \"floats\": %lld,\n \"violations\": ",
                    p.tiling, p.g.mt(), p.g.nt(), p.g.nthr(), p.g.lds_bytes(), p.mtiles, p.ntiles, p.bw, p.nbands, p.units,
                    p.ups, p.nsl, p.nsb, p.slab, p.floats);
        print_shown();
        std::printf("}\n");
        return 0;
    }
    // the channel counts of each tiling: a last tile with channels past the counts on both sides
    struct Case { int tiling, stride, Cs, Cl; };
    const Case cases[] = {{kGw16S1, 1, 136, 40}, {kGw16S2Wide, 2, 136, 40}, {kGw16S2Narrow, 2, 136, 9}};
    const int bh[][2] = {{1, 1}, {2, 2}};
    long long grids = 0;
    for (const Case &c : cases) {
        if (gw16_choose(c.stride, c.Cs, c.Cl) != c.tiling) {
            Shape s{c.stride, c.Cs, c.Cl, 1, 1, 1, 1, 1};
            violation(s, gw16_plan(c.stride, c.Cs, c.Cl, 1, 1, 1, 1, 1), -1, "the tiling rule picked another tiling");
        }
        for (int Ws = 1; Ws <= 400; ++Ws) {
            for (const auto &q : bh) {
                if (Ws > 2 * kGw16BW + 2 && q[0] * q[1] > 1) continue;  // (past three bands: the one-row shape alone)
                check_shape(Shape{c.stride, c.Cs, c.Cl, q[0], q[1], Ws, c.stride * q[1], c.stride * Ws});
                ++grids;
            }
            if (c.stride != 2) continue;
            // the cropped large sizes: one short (one small row: its only large row), and seven short
            if (2 * Ws - 1 >= 1) {
                check_shape(Shape{2, c.Cs, c.Cl, 1, 1, Ws, 1, 2 * Ws - 1});
                ++grids;
            }
            if (2 * Ws - 7 >= 1) {
                check_shape(Shape{2, c.Cs, c.Cl, 1, 4, Ws, 1, 2 * Ws - 7});
                ++grids;
            }
        }
    }
    std::printf("{\"grids\": %lld, \"units\": %lld, \"reads\": %lld, \"violations\": %lld,\n \"first\": ", grids, n_units, n_reads, n_viol);
    print_shown();
    std::printf(",\n \"tilings\": [");
    for (int t = 0; t < 3; ++t) {
        const Gw16Geo g = gw16_geo(t);
        std::printf("%s\n  {\"tiling\": %d, \"S\": %d, \"mt\": %d, \"nt\": %d, \"nthr\": %d, \"lds\": %d}", t ? "," : "", t, g.S, g.mt(),
                    g.nt(), g.nthr(), g.lds_bytes());
    }
    std::printf("],\n \"lds_budget\": %d}\n", kGw16LdsBudget);
    return 0;
}
