// Host-only check of the plan, the staging and the LDS addressing of the streaming weight
// gradient of the narrow layers (csrc/nlspn_gwnarrow.h): no device, no HIP header.  For Cs, Cl in
// {1, 3, 8, 9, 16} x Ws 1..400 x a few (B, Hs) from 1 x 1 and the cropped large sizes (one short,
// seven short) it plans with gwn_plan (the launcher's function) and walks every unit of every
// slice.  Per unit it replays the staging exactly as the kernel decodes it (gwn_lines / gwn_line,
// gwn_chunks, the vector-or-dword rule, the zero rules, gwn_a_off / gwn_b_off) into a map "LDS
// element -> tensor element or zero": a 16-byte load must sit at a multiple of 16 bytes (the
// operand's base `mis` floats past one) and wholly inside its tensor row, a dword load inside
// the row.  Then it walks every read of the k-loop (small row, k-step, lane group, small
// channel / N entry: gwn_a_read / gwn_b_read): inside the stage, written by this unit's staging,
// and holding the correlation's own element (A: zero past the band; B: zero outside the stored
// size; past the band, where A is zero, any cell this unit staged), and the large-side bias
// reads likewise.  The units of all slices must hit every (image, small row, band) exactly
// once, the owned large pixels every stored (image, row, column) exactly once, and the LDS stay
// within 160 KB.  Prints one JSON object.  With arguments
//     <stride> <Cs> <Cl> <B> <Hs> <Ws> <Hl> <Wl> [force_bw] [read_shift]
// that shape only: its plan and its violations (force_bw: a band width the plan would not
// choose; read_shift: floats added to every k-loop read, as a wrong pitch would), to show that
// the check is not vacuous.  tests/test_gwnarrow_plan_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "nlspn_gwnarrow_plan.h"

using namespace nlspn;

namespace {
struct Cell {
    int gen, ch, y, x;  // ch < 0: a stored zero
};
struct Shape {
    int Cs, Cl, B, Hs, Ws, Hl, Wl;
};

long long n_viol = 0, n_reads = 0, n_units = 0, n_loads = 0, n_vec = 0;
std::vector<std::string> shown;
std::vector<Cell> lds;
int gen = 0;

void violation(const Shape &s, const GwnPlan &p, int u, const char *detail) {
    if (n_viol++ >= 40) return;
    char buf[640];
    std::snprintf(buf, sizeof buf,
                  "{\"Cs\": %d, \"Cl\": %d, \"B\": %d, \"Hs\": %d, \"Ws\": %d, \"Hl\": %d, \"Wl\": %d, \"bw\": %d, \"nbands\": %d, "
                  "\"unit\": %d, \"detail\": \"%s\"}",
                  s.Cs, s.Cl, s.B, s.Hs, s.Ws, s.Hl, s.Wl, p.bw, p.nbands, u, detail);
    shown.push_back(buf);
}

void put(int off, int ch, int y, int x) {
    if (off < 0 || off >= (int)lds.size()) return;  // (a read of it is then reported as not staged)
    lds[off] = Cell{gen, ch, y, x};
}

// gwn_stage_line: base = the floats from a 16-byte boundary to the row's column 0
void stage_line(const Shape &s, const GwnPlan &p, int u, bool window, long long base, bool rowok, int W, int xf, int cnt, int lo,
                int hi, int c, int rj, int y) {
    const GwnChunks ch = gwn_chunks(rowok ? (int)(base & 3) : 0, xf, cnt);
    if (ch.xs > xf || ch.xs + 4 * ch.nch < xf + cnt) violation(s, p, u, "the chunks do not cover the staged columns");
    for (int q = 0; q < ch.nch; ++q) {
        const int x4 = ch.xs + 4 * q;
        bool have[4] = {false, false, false, false};
        if (rowok) {
            if (x4 >= 0 && x4 + 4 <= W) {
                ++n_vec;
                if ((base + x4) % 4 != 0) violation(s, p, u, "a 16-byte load that is not 16-byte aligned");
                for (int e = 0; e < 4; ++e) have[e] = true;
            } else {
                for (int e = 0; e < 4; ++e)
                    if (x4 + e >= lo && x4 + e < hi) {
                        ++n_loads;
                        if (x4 + e < 0 || x4 + e >= W) violation(s, p, u, "a dword load outside the tensor row");
                        have[e] = true;
                    }
            }
        }
        for (int e = 0; e < 4; ++e) {
            const int x = x4 + e, k = x - xf;
            if (k < 0 || k >= cnt) continue;
            const bool keep = rowok && x >= lo && x < hi;  // (a row outside the tensor: zeros)
            if (keep && !have[e]) violation(s, p, u, "a kept column that was not loaded");
            put(window ? gwn_b_off(c, rj, k) : gwn_a_off(rj, c, k), keep ? c : -1, y, x);
        }
    }
}

void stage(const Shape &s, const GwnPlan &p, int u, const GwnUnit &n, int mis_s, int mis_l) {
    ++gen;
    const int nlines = gwn_lines(s.Cs, s.Cl, n.nrows);
    std::vector<int> seen((size_t)nlines, 0);
    for (int hw = 0; hw < 2 * kGwnNW; ++hw)
        for (int li = hw; li < nlines; li += 2 * kGwnNW) {
            ++seen[li];
            const GwnLine q = gwn_line(li, s.Cs, n.nrows);
            if (!q.window) {
                if (q.c < 0 || q.c >= s.Cs || q.rj < 0 || q.rj >= n.nrows) {
                    violation(s, p, u, "a small line outside the unit");
                    continue;
                }
                const int y = n.sy0 + q.rj;
                const long long base = mis_s + (((long long)n.b * s.Cs + q.c) * s.Hs + y) * s.Ws;
                stage_line(s, p, u, false, base, true, s.Ws, n.bx0, n.k4, n.bx0, n.bx0 + n.bwi, q.c, q.rj, y);
            } else {
                if (q.c < 0 || q.c >= s.Cl || q.rj < 0 || q.rj > 2 * n.nrows) {
                    violation(s, p, u, "a window line outside the unit");
                    continue;
                }
                const int ly = 2 * n.sy0 - 1 + q.rj, xf = 2 * n.bx0 - 1, cnt = 2 * n.k4 + 1;
                const bool ok = ly >= 0 && ly < s.Hl;
                const long long base = mis_l + (((long long)n.b * s.Cl + q.c) * s.Hl + ly) * s.Wl;
                stage_line(s, p, u, true, base, ok, s.Wl, xf, cnt, xf > 0 ? xf : 0, s.Wl < xf + cnt ? s.Wl : xf + cnt, q.c, q.rj, ly);
            }
        }
    for (int li = 0; li < nlines; ++li)
        if (seen[li] != 1) {
            violation(s, p, u, "a staging line taken twice or never");
            break;
        }
}

// every read of unit n's k-loop, and of its large-side bias sum
void reads(const Shape &s, const GwnPlan &p, int u, const GwnUnit &n, int shift, std::vector<int> &owned) {
    const int stage_floats = gwn_stage_floats(p.nb), nent = 9 * s.Cl;
    char d[240];
    for (int r = 0; r < n.nrows; ++r)
        for (int p0 = 0; p0 < n.k4; p0 += 4)
            for (int lg = 0; lg < 4; ++lg) {
                const int px = p0 + lg;
                for (int l16 = 0; l16 < 16; ++l16) {
                    const int cs = l16 < s.Cs ? l16 : 0;
                    const int off = gwn_a_read(cs, r, lg) + p0 + shift;
                    ++n_reads;
                    if (off < 0 || off >= kGwnR * 16 * kGwnGP) {
                        violation(s, p, u, "A read outside the small rows' region");
                        continue;
                    }
                    const Cell &q = lds[off];
                    const bool want = px < n.bwi;
                    const bool ok = q.gen == gen && (want ? q.ch == cs && q.y == n.sy0 + r && q.x == n.bx0 + px : q.ch < 0);
                    if (!ok) {
                        std::snprintf(d, sizeof d, "A channel %d row %d pixel %d: %s", cs, r, px,
                                      q.gen != gen ? "not staged for this unit" : want ? "not the small tensor's element" : "not zero past the band");
                        violation(s, p, u, d);
                    }
                }
                for (int nn = 0; nn < 16 * p.nb; ++nn) {
                    const int e = nn < nent ? nn : 0, cl = e / 9, ky = (e % 9) / 3, kx = e % 3;
                    const int off = gwn_b_read(e, r, lg) + p0 + shift;
                    ++n_reads;
                    if (off < kGwnR * 16 * kGwnGP || off >= stage_floats) {
                        violation(s, p, u, "B read outside the window's region");
                        continue;
                    }
                    const Cell &q = lds[off];
                    const int ly = 2 * (n.sy0 + r) - 1 + ky, lx = 2 * (n.bx0 + px) - 1 + kx;
                    bool ok = q.gen == gen;
                    if (ok && px < n.bwi) {
                        const bool want = ly >= 0 && ly < s.Hl && lx >= 0 && lx < s.Wl;
                        ok = want ? q.ch == cl && q.y == ly && q.x == lx : q.ch < 0;
                    }
                    if (!ok) {
                        std::snprintf(d, sizeof d, "B channel %d tap (%d, %d) row %d pixel %d: %s", cl, ky, kx, r, px,
                                      q.gen != gen ? "not staged for this unit" : "not the correlation's element (or zero)");
                        violation(s, p, u, d);
                    }
                }
            }
    // the cells the unit owns (the large-side bias gradient): window rows 1 .. 2 nrows, columns 1 .. 2 bwi
    for (int cl = 0; cl < s.Cl; ++cl)
        for (int j = 1; j <= 2 * n.nrows; ++j)
            for (int wc = 1; wc <= 2 * n.bwi; ++wc) {
                const int off = gwn_b_off(cl, j, wc);
                const int ly = 2 * n.sy0 - 1 + j, lx = 2 * n.bx0 - 1 + wc;
                const bool want = ly < s.Hl && lx < s.Wl;
                ++n_reads;
                const Cell &q = off < (int)lds.size() ? lds[off] : lds[0];
                if (off >= stage_floats || q.gen != gen || (want ? q.ch != cl || q.y != ly || q.x != lx : q.ch >= 0))
                    violation(s, p, u, "an owned window cell is not the large tensor's element (or zero past the crop)");
                if (want && cl == 0) ++owned[((size_t)n.b * s.Hl + ly) * s.Wl + lx];
            }
}

GwnPlan check_shape(const Shape &s, int force_bw = 0, int shift = 0) {
    GwnPlan p = gwn_plan(s.Cs, s.Cl, s.B, s.Hs, s.Ws, s.Hl, s.Wl);
    if (force_bw > 0) {
        p.bw = force_bw;
        p.nbands = (s.Ws + p.bw - 1) / p.bw;
        p.units = s.B * p.ngroups * p.nbands;
        p.ups = (p.units + p.nsl - 1) / p.nsl;
        p.nsl = (p.units + p.ups - 1) / p.ups;
        p.floats = p.slab * p.nsl;
    }
    if (p.lds_bytes > kGwnLdsBudget || p.lds_bytes != 4 * gwn_lds_floats(p.nb)) violation(s, p, -1, "LDS over the budget");
    if (p.nb != gwn_blocks(s.Cl) || 16 * p.nb < 9 * s.Cl || gwn_clmax(p.nb) < s.Cl || gwn_red_floats(p.nb) + 16 > gwn_lds_floats(p.nb))
        violation(s, p, -1, "the N blocks do not cover the entries, or the LDS does not hold the channels");
    if (p.bw < 1 || (force_bw == 0 && p.bw > kGwnBW) || (long long)p.nbands * p.bw < s.Ws || (long long)(p.nbands - 1) * p.bw >= s.Ws ||
        p.ngroups * kGwnR < s.Hs || (p.ngroups - 1) * kGwnR >= s.Hs || p.units != s.B * p.ngroups * p.nbands || p.nsl < 1 ||
        (long long)p.nsl * p.ups < p.units || (long long)(p.nsl - 1) * p.ups >= p.units || p.slab != (long long)p.nb * 256 + 16 ||
        p.floats != p.slab * p.nsl) {
        violation(s, p, -1, "bands, groups, slices or slabs do not cover the problem");
        return p;
    }
    lds.assign((size_t)gwn_lds_floats(p.nb), Cell{0, 0, 0, 0});
    gen = 0;
    std::vector<int> hit((size_t)s.B * s.Hs * p.nbands, 0), owned((size_t)s.B * s.Hl * s.Wl, 0);
    const int mis_s = s.Ws & 3, mis_l = (s.Ws + 1) & 3;
    for (int sl = 0; sl < p.nsl; ++sl) {
        const int u0 = sl * p.ups, u1 = p.units < u0 + p.ups ? p.units : u0 + p.ups;
        if (u0 >= u1) violation(s, p, u0, "an empty slice");
        for (int u = u0; u < u1; ++u) {
            const GwnUnit n = gwn_unit(u, p.nbands, p.bw, p.ngroups, s.Hs, s.Ws);
            ++n_units;
            if (n.b < 0 || n.b >= s.B || n.sy0 < 0 || n.nrows < 1 || n.sy0 + n.nrows > s.Hs || n.bwi < 1 || n.bx0 + n.bwi > s.Ws) {
                violation(s, p, u, "a unit outside the small tensor");
                continue;
            }
            for (int r = 0; r < n.nrows; ++r) ++hit[((size_t)n.b * s.Hs + n.sy0 + r) * p.nbands + n.bx0 / p.bw];
            stage(s, p, u, n, mis_s, mis_l);
            reads(s, p, u, n, shift, owned);
        }
    }
    for (size_t i = 0; i < hit.size(); ++i)
        if (hit[i] != 1) {
            violation(s, p, (int)i, "the units do not hit every (image, small row, band) exactly once");
            break;
        }
    for (size_t i = 0; i < owned.size(); ++i)
        if (owned[i] != 1) {
            violation(s, p, (int)i, "the owned large pixels do not hit every stored pixel exactly once");
            break;
        }
    return p;
}

void print_shown() {
    std::printf("[");
    for (size_t i = 0; i < shown.size(); ++i) std::printf("%s\n  %s", i ? "," : "", shown[i].c_str());
    std::printf("]");
}
}  // namespace

int main(int argc, char **argv) {
    if (argc >= 9) {
        int v[10] = {0};
        for (int i = 1; i < argc && i <= 10; ++i) v[i - 1] = std::atoi(argv[i]);
        const Shape s{v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
        const bool covers = gwn_covers(v[0], v[1], v[2], 0);
        GwnPlan p{};
        if (covers) p = check_shape(s, v[8], v[9]);
        std::printf("{\"covers\": %d, \"nb\": %d, \"nbands\": %d, \"bw\": %d, \"ngroups\": %d, \"units\": %d, \"ups\": %d, \"nsl\": %d, "
                    "\"lds_bytes\": %d, \"slab\": %lld, \"floats\": %lld,\n \"violations\": ",
                    covers ? 1 : 0, p.nb, p.nbands, p.bw, p.ngroups, p.units, p.ups, p.nsl, p.lds_bytes, p.slab, p.floats);
        print_shown();
        std::printf("}\n");
        return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "covers") {  // the grid of gwn_covers, one character per point
        std::printf("{\"covers\": \"");
        for (int stride = 0; stride <= 3; ++stride)
            for (int Cs = 0; Cs <= 18; ++Cs)
                for (int c0 = 0; c0 <= 18; ++c0)
                    for (int c1 = 0; c1 <= 16; c1 += 16) std::printf("%d", gwn_covers(stride, Cs, c0, c1) ? 1 : 0);
        std::printf("\"}\n");
        return 0;
    }
    const int ch[] = {1, 3, 8, 9, 16};
    const int bh[][2] = {{1, 1}, {2, 5}};
    long long grids = 0;
    for (int Cs : ch)
        for (int Cl : ch)
            for (int Ws = 1; Ws <= 400; ++Ws) {
                for (const auto &q : bh) {
                    if (Ws > 2 * kGwnBW + 2 && q[0] * q[1] > 1) continue;  // (past three bands: the one-row shape alone)
                    check_shape(Shape{Cs, Cl, q[0], q[1], Ws, 2 * q[1], 2 * Ws});
                    ++grids;
                }
                // the cropped large sizes: one short (one small row: its only large row), and seven short
                check_shape(Shape{Cs, Cl, 1, 1, Ws, 1, 2 * Ws - 1});
                ++grids;
                if (2 * Ws - 7 >= 1) {
                    const int Hs = Ws <= 2 * kGwnBW + 2 ? 6 : 1;
                    check_shape(Shape{Cs, Cl, 1, Hs, Ws, Hs == 1 ? 1 : 2 * Hs - 7, 2 * Ws - 7});
                    ++grids;
                }
            }
    std::printf("{\"grids\": %lld, \"units\": %lld, \"reads\": %lld, \"vector_loads\": %lld, \"dword_loads\": %lld, \"violations\": %lld,\n \"first\": ",
                grids, n_units, n_reads, n_vec, n_loads, n_viol);
    print_shown();
    std::printf(",\n \"kernels\": [");
    for (int nb = 1; nb <= 9; ++nb)
        std::printf("%s\n  {\"nb\": %d, \"clmax\": %d, \"lds\": %d}", nb > 1 ? "," : "", nb, gwn_clmax(nb), 4 * gwn_lds_floats(nb));
    std::printf("],\n \"rows\": %d, \"waves\": %d, \"band_max\": %d, \"target_wgs\": %d, \"lds_budget\": %d}\n", kGwnR, kGwnNW, kGwnBW,
                kGwnTargetWgs, kGwnLdsBudget);
    return 0;
}
