// Weight gradient of the GRU-mode convolutions on the bf16 matrix cores with split operands
// ("bf16x3"), opt-in (nlspn_gconv_wgrad_bf16x3; GruConvs.wgrad_precision, NLSPNModel.
// gru_wgrad_precision).  The f32 kernel (gwgrad_kernel, nlspn_gconv_bwd.h) is untouched.
//
// Numerics.  The operands are the f32 NCHW tensors gwgrad_kernel reads.  While staging, each
// value a becomes hi = rne_bf16(a) and lo = rne_bf16(a - hi) (the subtraction in f32), and per
// output element the kernel accumulates sum (s_hi l_hi + s_hi l_lo + s_lo l_hi) in the f32
// accumulators of v_mfma_f32_16x16x32_bf16; lo lo is dropped.  |a - hi - lo| <= 2^-17 |a| and
// |lo| <= 2^-8 |a|, so a term is off by at most 2^-15 |s l| before accumulation rounding.
// Nothing is clamped: non-finite inputs give non-finite outputs, not necessarily of the f32
// kernel's kind (an inf operand has lo = inf - inf = NaN).  The slabs, the fixed-order slab
// reduce, the scale factor and the bias gradient are the f32 entry's own code.
//
// GEMM: M = small channels, N = (large channel, tap), K = pixels, as gwgrad_kernel.  One k-step
// is 32 pixels of one (row, band): lane l supplies A[cs = l & 15][pixel 8 (l >> 4) + j] and
// B[pixel 8 (l >> 4) + j][cl = l & 15], j = 0..7; the C/D map is the f32 16x16 one, so the slab
// store is gwgrad_kernel's.  A unit = (image, small row, band of at most 64 pixels) is one or
// two k-steps; a workgroup of four waves owns 128 small x 16 large channels x 9 taps, a wave
// 32 x 16 x 9 (72 accumulator registers).
//
// LDS image (nlspn_gwgrad16_plan.h): per stage the small row [128][hi, lo][64 pixels] and the
// large window [16][ky][kx][hi, lo][64 pixels] with one column-shifted copy per kx, so every
// fragment is one naturally aligned ds_read_b128 at both strides.  Banks: a ds_read_b128 serves
// four groups of 16 lanes ({0-3, 12-15, 20-27}, ...) over 64 banks; the lanes l & 15 sit one
// channel pitch apart and the lane groups l >> 4 16 bytes apart, and a channel pitch of 32
// (mod 64) bytes (288 / 2336) puts the 16 lanes of every group on 16 different 16-byte slots:
// conflict-free.  The staging stores are 32-bit words (two pixels), consecutive per lane.
//
// Staging: global -> VGPR -> v_cvt_pk_bf16_f32 (hi, then lo of the f32 residual) -> LDS (LDS-DMA
// cannot convert).  A staging item is two adjacent pixels of one row; consecutive lanes take
// consecutive pixel pairs of a row, dword loads: a window starts at the odd column S bx0 - 1 and
// the rows have any width, so 4 bytes is the alignment there is in general (8-byte loads of the
// small tensor where its rows are aligned measured no faster: DESIGN.md 3.8.3).  A thread's
// addresses are a uniform base per pass plus one 32-bit offset for all passes.  The next
// unit's loads are issued before the current unit's MFMAs and converted / stored into the other
// stage after them: two stages, one barrier per unit.  Zero: outside the tensor, past the
// band's window, past the channel counts, past a partial k-step (every stage is written whole).
#pragma once

#include "nlspn_gconv_bwd.h"
#include "nlspn_gwgrad16_plan.h"

namespace nlspn {

typedef __bf16 gw16_bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 gw16_bf8 __attribute__((ext_vector_type(8)));
typedef float gw16_f2 __attribute__((ext_vector_type(2)));

// (a, b) -> packed hi and lo parts
__device__ __forceinline__ void gw16_split(float a, float b, unsigned &hi, unsigned &lo) {
    const gw16_f2 v{a, b};
    const gw16_bf2 h = __builtin_convertvector(v, gw16_bf2);
    const gw16_bf2 l = __builtin_convertvector(v - __builtin_convertvector(h, gw16_f2), gw16_bf2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}

template <int S, int WM, int WGM, int WGN>
__global__ void __launch_bounds__(64 * WGM * WGN) gwgrad16_kernel(GwgradArgs a) {
    constexpr Gw16Geo G{S, WM, WGM, WGN};
    constexpr int NTHR = G.nthr(), MT = G.mt(), NT = G.nt(), STAGE = G.stage_elems();
    constexpr int NIA = gw16_a_items(MT) / NTHR, NIB = gw16_b_items(NT) / NTHR, NLB = gw16_b_loads(S);
    static_assert(gw16_a_items(MT) % NTHR == 0 && gw16_b_items(NT) % NTHR == 0, "whole staging rounds");
    static_assert(G.lds_bytes() <= kGw16LdsBudget, "LDS budget");
    extern __shared__ __attribute__((aligned(16))) unsigned short gw16_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv % WGM, wn = wv / WGM;
    const int l16 = lane & 15, lg = lane >> 4;
    const int ntile = a.mtiles * a.ntiles;
    const int tile = (int)blockIdx.x % ntile, sl = (int)blockIdx.x / ntile;
    const int mt = tile % a.mtiles, nt = tile / a.mtiles;
    const int cs0 = mt * MT, cl0 = nt * NT;
    const long long HWs = (long long)a.Hs * a.Ws, HWl = (long long)a.Hl * a.Wl;
    const int Cl = a.c0 + a.c1;

    f32x4v acc[WM][9];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[m][t] = f32x4v{0.f, 0.f, 0.f, 0.f};

    // Staging addresses.  Thread tid takes pixel pair pp = tid % 32 of row r0 + RP k in pass k
    // (gw16_a_item / gw16_b_item): the pass's rows, the unit's image / row / band and the tile's
    // channels go into a uniform base pointer, and ONE per-thread 32-bit offset serves all passes.
    constexpr int RP = gw16_pass_rows(NTHR);
    static_assert(NT % RP == 0, "a pass of B rows has one ky");
    const int pp = tid % (kGw16BW / 2), r0 = tid / (kGw16BW / 2);
    const unsigned offa = (unsigned)(r0 * HWs) + 2u * pp;               // channel r0, pixel 2 pp of the unit's row
    const unsigned offb = (unsigned)(r0 * HWl) + (unsigned)(2 * S * pp);  // channel r0, window column 2 S pp
    // (a tile of NT = 16 large channels reads one source: c0 % 16 == 0 when there are two)
    const float *lsrc = cl0 < a.c0 ? a.l0 + (long long)cl0 * HWl : a.l1 + (long long)(cl0 - a.c0) * HWl;
    const long long limg = (cl0 < a.c0 ? a.c0 : a.c1) * HWl;
    unsigned *const wa = reinterpret_cast<unsigned *>(gw16_lds) + (gw16_a_off(r0, 0, 2 * pp) >> 1);
    unsigned *const wb = reinterpret_cast<unsigned *>(gw16_lds) + (gw16_b_off(MT, r0, 0, 0, 0, 2 * pp) >> 1);

    float ra[NIA][2], rb[NIB][NLB];
    // the global loads of unit u into registers (zeros where the unit has no element)
    auto load = [&](int u) {
        const Gw16Unit n = gw16_unit(u, a.nbands, a.bw, a.Hs, a.Ws);
        const float *pa = a.s + ((long long)n.b * a.Cs + cs0) * HWs + (long long)n.sy * a.Ws + n.bx0;
        const bool p0 = 2 * pp < n.bwi, p1 = 2 * pp + 1 < n.bwi;
#pragma unroll
        for (int k = 0; k < NIA; ++k) {
            const float *src = pa + (long long)(RP * k) * HWs;
            const bool cok = cs0 + r0 + RP * k < a.Cs;
            ra[k][0] = cok && p0 ? src[offa] : 0.f;
            ra[k][1] = cok && p1 ? src[offa + 1] : 0.f;
        }
        const int ly0 = S * n.sy - 1, lx0 = S * n.bx0 - 1, ncol = gw16_ncol(S, n.bwi);
        // (the pointer may stand before the tensor's first element: row / column -1 are never loaded)
        const float *pb = lsrc + n.b * limg + (long long)ly0 * a.Wl + lx0;
        bool colok[NLB];
#pragma unroll
        for (int j = 0; j < NLB; ++j) {
            const int wc = gw16_b_wc(S, pp, j);
            colok[j] = wc < ncol && (unsigned)(lx0 + wc) < (unsigned)a.Wl;
        }
#pragma unroll
        for (int k = 0; k < NIB; ++k) {
            const int ck = gw16_b_pass_c(NT, NTHR, k), ky = gw16_b_pass_ky(NT, NTHR, k);
            const float *src = pb + (long long)ck * HWl + (long long)ky * a.Wl;
            const bool rowok = cl0 + r0 + ck < Cl && (unsigned)(ly0 + ky) < (unsigned)a.Hl;
#pragma unroll
            for (int j = 0; j < NLB; ++j) rb[k][j] = rowok && colok[j] ? src[offb + j] : 0.f;
        }
    };
    // split the registers and write stage st whole
    auto store = [&](int st) {
        unsigned *const sa = wa + st * (STAGE / 2), *const sb = wb + st * (STAGE / 2);
#pragma unroll
        for (int k = 0; k < NIA; ++k) {
            unsigned hi, lo;
            gw16_split(ra[k][0], ra[k][1], hi, lo);
            sa[gw16_a_off(RP * k, 0, 0) >> 1] = hi;
            sa[gw16_a_off(RP * k, 1, 0) >> 1] = lo;
        }
#pragma unroll
        for (int k = 0; k < NIB; ++k) {
            const int ck = gw16_b_pass_c(NT, NTHR, k), ky = gw16_b_pass_ky(NT, NTHR, k);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                unsigned hi, lo;
                gw16_split(rb[k][kx], rb[k][kx + S], hi, lo);
                sb[(gw16_b_off(0, ck, ky, kx, 0, 0)) >> 1] = hi;
                sb[(gw16_b_off(0, ck, ky, kx, 1, 0)) >> 1] = lo;
            }
        }
    };

    const int u0 = sl * a.ups, u1 = min(a.units, u0 + a.ups);
    const int ca = wm * WM * 16 + l16, cb = wn * 16 + l16;  // this lane's A channel of block m = 0, B channel
    load(u0);
    store(0);
    __syncthreads();
    for (int u = u0; u < u1; ++u) {
        const int cur = (u - u0) & 1;
        const int nks = gw16_unit(u, a.nbands, a.bw, a.Hs, a.Ws).nks;
        if (u + 1 < u1) load(u + 1);
        const unsigned short *st = gw16_lds + cur * STAGE;
        for (int ks = 0; ks < nks; ++ks) {
            const int px = gw16_frag_px(ks, lg);
            const unsigned short *pa = st + gw16_a_off(ca, 0, px), *pb = st + gw16_b_off(MT, cb, 0, 0, 0, px);
            gw16_bf8 ah[WM], al[WM], bh[2], bl[2];
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                ah[m] = *reinterpret_cast<const gw16_bf8 *>(pa + gw16_a_off(16 * m, 0, 0));
                al[m] = *reinterpret_cast<const gw16_bf8 *>(pa + gw16_a_off(16 * m, 1, 0));
            }
            bh[0] = *reinterpret_cast<const gw16_bf8 *>(pb + gw16_b_off(0, 0, 0, 0, 0, 0));
            bl[0] = *reinterpret_cast<const gw16_bf8 *>(pb + gw16_b_off(0, 0, 0, 0, 1, 0));
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (t + 1 < 9) {  // the next tap's fragments are in flight during this tap's MFMAs
                    bh[(t + 1) & 1] = *reinterpret_cast<const gw16_bf8 *>(pb + gw16_b_off(0, 0, (t + 1) / 3, (t + 1) % 3, 0, 0));
                    bl[(t + 1) & 1] = *reinterpret_cast<const gw16_bf8 *>(pb + gw16_b_off(0, 0, (t + 1) / 3, (t + 1) % 3, 1, 0));
                }
#pragma unroll
                for (int m = 0; m < WM; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[m], bh[t & 1], acc[m][t], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < WM; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[m], bl[t & 1], acc[m][t], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < WM; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[m], bh[t & 1], acc[m][t], 0, 0, 0);
            }
        }
        if (u + 1 < u1) store(cur ^ 1);
        __syncthreads();
    }
    // lane l, register r of block (m, t): small channel 16 m + 4 (l >> 4) + r, large channel l & 15
    const int Clp = a.ntiles * NT;
    float *slab = a.ws + (long long)sl * a.mtiles * MT * Clp * 9;
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cs = cs0 + wm * WM * 16 + 16 * m + 4 * lg + r;
            float *d = slab + ((long long)cs * Clp + cl0 + wn * 16 + l16) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) d[t] = acc[m][t][r];
        }
}

// The instantiated tilings: X(S, WM, WGM, WGN) (gw16_geo)
#define NLSPN_GW16_CONFIGS(X) \
    X(1, 2, 4, 1)             \
    X(2, 2, 4, 1)

}  // namespace nlspn
