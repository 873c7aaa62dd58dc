// GRU-mode convolutions on the bf16 matrix cores with split operands ("bf16x3",
// v_mfma_f32_16x16x32_bf16), inference only, opt-in (NLSPNModel.gru_precision = "bf16x3"): the
// layers of nlspn_gconv.h as gconv16_kernel's implicit GEMM over (channel, tap), every f32
// operand carried as two bf16 parts.  The f32 and f16 families are untouched.
//
// Under gradients, opt-in as well (NLSPNModel.gru_dgrad_precision = "bf16x3"), the same body
// computes the data gradients: a forward launch of the adjoint layer kind (nlspn_gconv_bwd.h) on
// the gradient as c8x2 and the adjoint weights packed split, with the f32 family's derivative
// epilogue (kGcEpiDact; presets NLSPN_GCX3_DG_CONFIGS, entry nlspn_gconv_x3_dgrad).  The MFMA
// loop, the staging and the fragment reads are the forward's; gcx3_split_kernel brings an f32
// NCHW gradient into the layout where it enters a chain.
//
// Numerics contract (include/nlspn_prop.h):
//   - Every MFMA operand value a (f32) is the pair hi = rne_bf16(a), lo = rne_bf16(a - hi), the
//     subtraction in f32.  Weights are split once, when packed (gru.py pack_conv_x3 /
//     pack_convt_x3); activations once, from the f32 value the producing layer's epilogue holds
//     (gcx3_store4).
//   - Per output element the kernel accumulates sum (w_hi x_hi + w_hi x_lo + w_lo x_hi) in the
//     MFMAs' f32 accumulators (v_mfma_f32_16x16x32_bf16 for the first two products,
//     v_mfma_f32_16x16x16_bf16 for the third); lo lo is dropped.  bf16 x bf16 products are
//     exact in f32.
//   - |a - hi| <= 2^-8 |a| and |a - hi - lo| <= 2^-17 |a|, so a term is off by at most
//     (2^-17 + 2^-17 + 2^-16) |w x| = 2^-15 |w x| before accumulation rounding.
//   - Every epilogue (bias, ReLU, tanhf, sigmoid, the GRU blend) runs in f32 on the accumulators,
//     as the f32 family's.  The ConvGRU state h is carried in f32 beside its split copy; z and qx
//     stay f32; r*h is formed in f32 and stored split.
//   - Nothing is clamped: non-finite inputs give non-finite outputs, not necessarily of the f32
//     kernel's kind (inf has lo = inf - inf = NaN).  No atomics, no waiting between workgroups:
//     the same bits on every run.
//
// Layout "c8x2": a (B, C, H, W) activation is [B][ceil(C/8)][2][H][W][8] bf16, pad channels
// zero: per 8-channel block a hi cell plane, then a lo cell plane.  To the staging code this is
// the f16 family's c8 tensor of 2 ceil(C/8) "cell blocks" (block 2 c + s: part s of channels
// 8c .. 8c + 7), so gconv16_kernel's LDS-DMA staging, descriptors and zero padding carry over
// unchanged with every block count doubled.  Weights are packed the same way, per co tile
// [cell block][tap][co][8] bf16.
//
// A chunk is four cell blocks = 16 channels (hi0, lo0, hi1, lo1): the f16 presets' LDS bytes.
// A k-step (one tap of a chunk) is a K = 32 and a K = 16 MFMA per 16x16 block: three products of
// 16 channels in 1.5 K = 32 MFMAs' time.  Lane group g = l >> 4 supplies k = 8 g + j (K = 32) or
// k = 4 g + j (K = 16), and the k index only has to agree between A and B:
//     K = 32:  A = [w_hi0, w_hi0, w_hi1, w_hi1]   B = [x_hi0, x_lo0, x_hi1, x_lo1]     (8 channels each)
//     K = 16:  A = [w_lo0', w_lo0", w_lo1', w_lo1"]  B = [x_hi0', x_hi0", x_hi1', x_hi1"]  (' / ": channels 0-3 / 4-7)
// The K = 32 B is the natural read (lane group g reads cell block g: the f16 kernel's), its A
// the weights' cell block g & 2 (two lane groups read the same cells: a broadcast).  The K = 16
// fragments are ds_read_b64 of half (g & 1) of a cell: A from the weights' lo cell block
// (g & 2) + 1, B from the window's hi cell block g & 2 at the same pixel.  Per k-step that is
// WM + WN ds_read_b128 and WM + WN ds_read_b64 for WM WN MFMAs of each kind.  (Measured against
// a second K = 32 MFMA on the same B registers with the odd lane groups' A zeroed: DESIGN 3.8.4.)
//
// From gconv16_kernel unchanged: gc_tile / gc_window, the two LDS stages with the next chunk in
// flight by LDS-DMA, the compile-time window pitch, the even-then-odd column order of the
// stride-2 window rows, gc_gru1_map, out-of-range buffer offsets as the zero padding, and the
// f32 family's C/D epilogue indexing (co = co0 + 16 m + 4 (l >> 4) + r).
#pragma once

#include "nlspn_gconv.h"

namespace nlspn {

typedef __bf16 gx3_bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 gx3_bf4 __attribute__((ext_vector_type(4)));
typedef float gx3_f4 __attribute__((ext_vector_type(4)));
typedef short gx3_s4 __attribute__((ext_vector_type(4)));  // four bf16 as the K = 16 MFMA takes them

struct GconvX3Args {
    const void *x0, *x1;   // c8x2 inputs of c0 / c1 channels (the VALU kernel: x0 f32 NCHW)
    const void *w;         // packed weights [phase][co_tile][nbp][ntap][WGco][8] bf16 (phase: transposed only)
    const float *bias;     // [co_tiles * WGco] (zero past cout)
    __bf16 *ys;            // kGcEpiAct: c8x2 (B, ceil(cout/8), 2, ohs, ows, 8), or null
    float *y32;            // kGcEpiAct: (B, cout, ohs, ows), or null
    const float *h;        // ConvGRU: the f32 hidden state (B, hc, Ho, Wo)
    float *zb, *qxb;       // z and qx, f32
    __bf16 *rhs;           // GRU1: r*h as c8x2
    float *hout32;         // GRU2: h'
    __bf16 *houts;         // GRU2: h' as c8x2
    int c0, c1;
    int nb0, nb1, nbp;     // cell blocks (two per 8 channels) of x0 / x1; the packed weights' (a multiple of CCB)
    int B, Hi, Wi, Ho, Wo;
    int ohs, ows;
    int cout, co_tiles;
    int gh, gw, bw, nbands, tpb, npx;  // the pixel tiling (gc_tile)
    int act;
    float in_div;          // the VALU kernel only
    int hc;
    // kGcEpiDact (nlspn_gconv_x3_dgrad; the other epilogues read none of these): y32 (channels
    // [0, ysplit)) and y1 (channels [ysplit, cout)) = act'(ysave) * scale * sum (+ add / add1, laid
    // out as y32 / y1; they may be y32 / y1 themselves), all f32 NCHW as GconvArgs'; x0 is the
    // gradient as c8x2, bias is not read; ys (optional, ysplit = cout): the same value split
    const float *ysave, *add, *add1;
    float *y1;
    int ysplit;
    float scale;
};

template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CCB, int EPI>
struct GcX3Cfg {
    using Geom = GcGeom<MODE, WM, WN, WGM, WGN, XR, XP>;  // (nlspn_gconv_plan.h)
    static constexpr int WGCO = Geom::WGCO, NPX = Geom::NPX;
    static constexpr int XCS = XR * XP;  // cells of one cell block's window
    static_assert(CCB % 4 == 0, "a k-step is four cell blocks: hi and lo of two channel blocks");
    static_assert(XCS % 16 == 0, "lane groups one cell block apart must fall on the same bank slots");
    // in 16-byte cells (gcx3_lds_bytes, nlspn_gconv_plan.h, is the same arithmetic)
    static constexpr int WST = gcx3_wst(MODE, WGCO, CCB), XST = gcx3_xst(XR, XP, CCB);
    static constexpr int STAGE = WST + XST;
    static constexpr int LDS_BYTES = gcx3_lds_bytes(MODE, WGCO, XR, XP, CCB);
    static_assert(LDS_BYTES == 2 * STAGE * 16 && LDS_BYTES <= kGcX3LdsBudget, "LDS budget");
    static constexpr int XREG = XST / kGcNT;  // window LDS-DMA loads per lane per chunk
};

// four consecutive channels (from channel cg, a multiple of 4) of one pixel of a c8x2 tensor of
// nb channel blocks: each f32 value split once, hi into the block's hi cell, lo into its lo cell
__device__ __forceinline__ void gcx3_store4(__bf16 *y, long long b, int nb, int cg, long long HW, long long pix,
                                            const float (&u)[4], int nvalid) {
    gx3_f4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = r < nvalid ? u[r] : 0.f;  // (pad channels are zero)
    const gx3_bf4 hi = __builtin_convertvector(v, gx3_bf4);
    const gx3_bf4 lo = __builtin_convertvector(v - __builtin_convertvector(hi, gx3_f4), gx3_bf4);
    __bf16 *cell = y + (((b * nb + (cg >> 3)) * 2) * HW + pix) * 8 + (cg & 7);
    *reinterpret_cast<gx3_bf4 *>(cell) = hi;
    *reinterpret_cast<gx3_bf4 *>(cell + HW * 8) = lo;
}

template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CCB, int EPI, int PH>
__device__ __forceinline__ void gconvx3_body(const GconvX3Args &a, gx3_bf8 *lds, int wgi) {
    using Cfg = GcX3Cfg<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI>;
    constexpr int WGCO = Cfg::WGCO, XCS = Cfg::XCS;
    constexpr int NTAP = gc_ntap(MODE, PH);
    constexpr int WCS = NTAP * WGCO;  // cells of one cell block's weights (this phase's taps)
    constexpr int WCELLS = CCB * WCS, WREG = (WCELLS + kGcNT - 1) / kGcNT;
    static_assert(WREG * kGcNT <= Cfg::WST, "the weight loads stay inside the stage");
    constexpr int S = MODE == kGcS2 ? 2 : 1;
    constexpr int XPH = (XP + 1) / 2;  // stride 2: the odd columns' first cell
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv % WGM, wn = wv / WGM;
    const int l16 = lane & 15, lg = lane >> 4;

    // workgroup -> (co tile, image, band, tile), as gconv_body
    const int cot = wgi % a.co_tiles;
    int rest = wgi / a.co_tiles;
    const int tile = rest % a.tpb;
    rest /= a.tpb;
    const int band = rest % a.nbands;
    const int b = rest / a.nbands;
    const int npx = a.npx;
    const GcWindow win = gc_window(MODE, a.gh, a.gw, a.bw, npx, band, tile);
    if (win.empty) return;
    const int bx0 = win.bx0, bwi = win.bwi, f0 = win.f0, ra = win.ra, rb = win.rb;
    const int iy0 = win.iy0, ix0 = win.ix0, nrows = win.nrows, ncols = win.ncols;

    int gyv[WN], gxv[WN], xb[WN];
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int jj = 16 * (wn * WN + n) + l16;
        const int f = f0 + min(jj, npx - 1);
        const int gy = f / bwi, gx = bx0 + (f - gy * bwi);
        gyv[n] = jj < npx ? gy : a.gh;  // (past the tile: not stored)
        gxv[n] = gx;
        const int ry = min(gy, rb) - ra;
        // (stride 2: window column 2 (gx - bx0) + dx sits at cell (gx - bx0) + {0, XPH, 1}[dx])
        xb[n] = lg * XCS + (S * ry) * XP + (gx - bx0);
    }
    // the hi cell block of this lane group's channel block; its lo block is the next one
    const int wb = (lg & 2) * WCS + wm * (16 * WM) + l16;
    const int half = lg & 1;  // the K = 16 fragments: channels 4 half .. 4 half + 3 of a cell

    // the K range in cell blocks: GRU1's qx tile runs over x's blocks only
    int cs = 0;
    if constexpr (EPI == kGcEpiGru1) cs = (cot * WGCO >= 2 * a.hc) ? a.nb0 : 0;
    const int ce = a.nbp;
    const long long HWi = (long long)a.Hi * a.Wi;
    constexpr int TAP0 = MODE == kGcT2 ? (PH == 0 ? 0 : PH == 1 ? 1 : PH == 2 ? 3 : 5) : 0;
    const gx3_bf8 *wsrc = static_cast<const gx3_bf8 *>(a.w) +
                          (long long)a.nbp * WGCO * ((long long)TAP0 * a.co_tiles + (long long)cot * NTAP);

    // Staging by LDS-DMA, one 16-byte cell per lane and load, as gconv16_body: a window cell's
    // source is its byte offset within the chunk's cell blocks (0x80000000 for a cell outside the
    // window or the image, or a pad cell: the load returns 0 = the zero padding; the descriptor
    // ends at the source's last block, so blocks past it read 0 too); the chunk's weights are
    // contiguous (cells past them reload cell 0 into the stage's pad: never read).
    unsigned xoff[Cfg::XREG];
#pragma unroll
    for (int i = 0; i < Cfg::XREG; ++i) {
        const int p = tid + i * kGcNT;
        const int c = p / XCS, rem = p - c * XCS;
        const int row = rem / XP, pos = rem - row * XP;
        const int col = S == 2 ? (pos < XPH ? 2 * pos : 2 * (pos - XPH) + 1) : pos;
        const int iy = iy0 + row, ix = ix0 + col;
        const bool ok = c < CCB && row < nrows && col < ncols && (unsigned)iy < (unsigned)a.Hi &&
                        (unsigned)ix < (unsigned)a.Wi;
        xoff[i] = ok ? (unsigned)(((long long)c * HWi + (long long)iy * a.Wi + ix) * 16) : 0x80000000u;
    }
    typedef __attribute__((address_space(3))) void lds_t;
    auto issue_chunk = [&](int cb0, const int stage) __attribute__((always_inline)) {
        const gx3_bf8 *wc = wsrc + (long long)cb0 * WCS;
        gx3_bf8 *Wd = lds + stage * Cfg::STAGE + 64 * wv, *Xd = lds + stage * Cfg::STAGE + Cfg::WST + 64 * wv;
#pragma unroll
        for (int i = 0; i < WREG; ++i) {
            const int p = tid + i * kGcNT;
            __builtin_amdgcn_global_load_lds(wc + (p < WCELLS ? p : 0), (lds_t *)(Wd + kGcNT * i), 16, 0, 0);
        }
        const bool s0 = cb0 < a.nb0;
        const int nblk = s0 ? a.nb0 - cb0 : a.nb1 - (cb0 - a.nb0);
        const bool any = nblk > 0 && (s0 || a.x1 != nullptr);
        const char *base = !any ? static_cast<const char *>(a.x0)
                           : s0 ? static_cast<const char *>(a.x0) + ((long long)b * a.nb0 + cb0) * HWi * 16
                                : static_cast<const char *>(a.x1) + ((long long)b * a.nb1 + (cb0 - a.nb0)) * HWi * 16;
        const int nrec = any ? (int)(nblk * HWi * 16) : 0;
        const rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), (short)0, nrec, 0x00020000);
#pragma unroll
        for (int i = 0; i < Cfg::XREG; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_t *)(Xd + kGcNT * i), 16, xoff[i], 0, 0, 0);
    };

    f32x4v acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n) acc[m][n] = f32x4v{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](const int stage) __attribute__((always_inline)) {
        const gx3_bf8 *Wc = lds + stage * Cfg::STAGE, *Xc = Wc + Cfg::WST;
        // the chunk's k-steps j = (16-channel group ks, tap t), the operands of step j + 1 read
        // while the MFMAs of step j issue (as gconv_body)
        constexpr int NS = (CCB / 4) * NTAP;
        gx3_bf8 ah[2][WM], bv[2][WN];
        gx3_s4 al[2][WM], bh[2][WN];  // w_lo and x_hi, four channels per lane
        const gx3_s4 *Wc4 = reinterpret_cast<const gx3_s4 *>(Wc), *Xc4 = reinterpret_cast<const gx3_s4 *>(Xc);
        auto fetch = [&](const int j, const int slot) __attribute__((always_inline)) {
            const int ks = j / NTAP, t = j % NTAP;
            int ky, kx, dy, dx;
            gc_tap<MODE, PH>(t, ky, kx, dy, dx);
            (void)ky; (void)kx;
            const int dcell = S == 2 ? (dx == 1 ? XPH : dx / 2) : dx;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                const int o = wb + 4 * ks * WCS + t * WGCO + 16 * m;
                ah[slot][m] = Wc[o];
                al[slot][m] = Wc4[2 * (o + WCS) + half];
            }
#pragma unroll
            for (int n = 0; n < WN; ++n) {
                const int c = xb[n] + 4 * ks * XCS + dy * XP + dcell;
                bv[slot][n] = Xc[c];
                bh[slot][n] = Xc4[2 * (c - half * XCS) + half];  // (the hi cell block of lane group g: g & 2)
            }
        };
        fetch(0, 0);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int cur = j & 1;
            if (j + 1 < NS) fetch(j + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int n = 0; n < WN; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[cur][m], bv[cur][n], acc[m][n], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int n = 0; n < WN; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(al[cur][m], bh[cur][n], acc[m][n], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    issue_chunk(cs, 0);
    __syncthreads();  // (waits for the loads: vmcnt(0), then the barrier)
    // one barrier per chunk, the next chunk landing in the other stage meanwhile (as gconv_body)
    auto step = [&](const int cb0, const int stage) __attribute__((always_inline)) {
        if (cb0 + CCB < ce) issue_chunk(cb0 + CCB, stage ^ 1);
        compute(stage);
        __syncthreads();
    };
    for (int cb0 = cs; cb0 < ce; cb0 += 2 * CCB) {
        step(cb0, 0);
        if (cb0 + CCB < ce) step(cb0 + CCB, 1);
    }

    // epilogue, in f32 on the f32 accumulators: lane l, register r of block (m, n) holds output
    // channel co0 + 16 m + 4 (l >> 4) + r of this lane's pixel of block n; its four channels are
    // eight consecutive bytes of a hi cell and of the lo cell beside it
    const int co0 = cot * WGCO + wm * (16 * WM);
    const long long HWo = (long long)a.Ho * a.Wo;
    float bs[WM][4];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if constexpr (EPI == kGcEpiDact) bs[m][r] = 0.f;  // (a gradient carries no bias)
            else bs[m][r] = a.bias[co0 + 16 * m + 4 * lg + r];  // (padded to the co tiles)
        }
    const int hc = a.hc;
    const int gate = EPI == kGcEpiGru1 ? (cot * WGCO) / hc : 0;  // GRU1: 0 z, 1 r, 2 qx (uniform per tile)
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int gy = gyv[n], gx = gxv[n];
        int oy = gy, ox = gx;
        if constexpr (MODE == kGcT2) {
            oy = 2 * gy + (PH >> 1);
            ox = 2 * gx + (PH & 1);
        }
        const bool ok = gy < a.gh && oy < a.ohs && ox < a.ows;
        const long long pix = ok ? (long long)oy * a.Wo + ox : 0;
        if constexpr (EPI == kGcEpiAct) {
            const long long pixs = ok ? (long long)oy * a.ows + ox : 0;
            const long long HWs = (long long)a.ohs * a.ows;
            const int nbo = (a.cout + 7) >> 3;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                const int cg = co0 + 16 * m + 4 * lg;
                float u[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    u[r] = acc[m][n][r] + bs[m][r];
                    if (a.act == kGcActRelu) u[r] = u[r] < 0.f ? 0.f : u[r];  // (NaN kept, as torch's ReLU)
                    else if (a.act == kGcActTanh) u[r] = tanhf(u[r]);
                    if (a.y32 && ok && cg + r < a.cout) a.y32[((long long)b * a.cout + cg + r) * HWs + pixs] = u[r];
                }
                if (a.ys && ok && cg < 8 * nbo) gcx3_store4(a.ys, b, nbo, cg, HWs, pixs, u, a.cout - cg);
            }
        } else if constexpr (EPI == kGcEpiDact) {
            // the f32 family's arm (nlspn_gconv.h): no bias; the block's saved outputs and addends
            // are loaded first (an addend that is the output itself is this lane's own element)
            const long long pixs = ok ? (long long)oy * a.ows + ox : 0;
            const long long HWs = (long long)a.ohs * a.ows;
            const int nbo = (a.cout + 7) >> 3;
            auto at = [&](const int co) __attribute__((always_inline)) {
                return co < a.ysplit ? ((long long)b * a.ysplit + co) * HWs + pixs
                                     : ((long long)b * (a.cout - a.ysplit) + (co - a.ysplit)) * HWs + pixs;
            };
            float yv[WM][4], av[WM][4];
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = co0 + 16 * m + 4 * lg + r;
                    const bool st = ok && co < a.cout;
                    const float *ad = co < a.ysplit ? a.add : a.add1;
                    yv[m][r] = st && a.act != kGcActNone ? a.ysave[at(co)] : 0.f;
                    av[m][r] = st && ad ? ad[at(co)] : 0.f;
                }
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                const int cg = co0 + 16 * m + 4 * lg;
                float u[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = cg + r;
                    u[r] = acc[m][n][r] * a.scale;
                    if (a.act == kGcActRelu) u[r] = yv[m][r] > 0.f ? u[r] : 0.f;
                    else if (a.act == kGcActTanh) u[r] = u[r] * (1.f - yv[m][r] * yv[m][r]);
                    if (co < a.ysplit ? a.add != nullptr : a.add1 != nullptr) u[r] += av[m][r];
                    if (ok && co < a.cout) (co < a.ysplit ? a.y32 : a.y1)[at(co)] = u[r];
                }
                if (a.ys && ok && cg < 8 * nbo) gcx3_store4(a.ys, b, nbo, cg, HWs, pixs, u, a.cout - cg);
            }
        } else if constexpr (EPI == kGcEpiGru1) {
            float hv[WM][4];
            const int cgate = co0 - gate * hc;  // channel co0 of the gate
            const long long ob = ((long long)b * hc + cgate) * HWo + pix;
            if (gate == 1) {
#pragma unroll
                for (int m = 0; m < WM; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) hv[m][r] = a.h[ob + (long long)(16 * m + 4 * lg + r) * HWo];
            }
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float u = acc[m][n][r] + bs[m][r];
                    if (gate == 0) o[r] = 1.f / (1.f + expf(-u));               // z
                    else if (gate == 1) o[r] = (1.f / (1.f + expf(-u))) * hv[m][r];  // r * h, formed in f32
                    else o[r] = u;                                               // convq's x half + bias
                    if (ok && gate != 1) (gate == 0 ? a.zb : a.qxb)[ob + (long long)(16 * m + 4 * lg + r) * HWo] = o[r];
                }
                if (ok && gate == 1) gcx3_store4(a.rhs, b, hc >> 3, cgate + 16 * m + 4 * lg, HWo, pix, o, 4);
            }
        } else {  // kGcEpiGru2
            float qv[WM][4], zv[WM][4], hv[WM][4];
            const long long ob = ((long long)b * hc + co0) * HWo + pix;
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long o = ob + (long long)(16 * m + 4 * lg + r) * HWo;
                    qv[m][r] = a.qxb[o];
                    zv[m][r] = a.zb[o];
                    hv[m][r] = a.h[o];
                }
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float q = tanhf(acc[m][n][r] + qv[m][r]);
                    const float z = zv[m][r];
                    o[r] = (1.f - z) * hv[m][r] + z * q;  // :402
                    if (ok) a.hout32[ob + (long long)(16 * m + 4 * lg + r) * HWo] = o[r];
                }
                if (ok) gcx3_store4(a.houts, b, hc >> 3, co0 + 16 * m + 4 * lg, HWo, pix, o, 4);
            }
        }
    }
}

template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CCB, int EPI>
__global__ void __launch_bounds__(kGcNT) gconvx3_kernel(GconvX3Args a) {
    extern __shared__ __attribute__((aligned(16))) gx3_bf8 gcx3_lds[];
    if constexpr (EPI == kGcEpiGru1) {
        using Cfg = GcX3Cfg<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI>;
        // (a qx workgroup takes two pixel tiles: gc_gru1_map, nlspn_gconv_plan.h)
        const int nh = gc_gru1_heavy_cots(a.hc, Cfg::WGCO), nr = gc_rest_count(a.B, a.nbands, a.tpb);
        const int wg = xcd_remap((int)blockIdx.x, gc_gru1_wgs(a.hc, Cfg::WGCO, a.co_tiles, nr));
        int cot, r0, r1;
        gc_gru1_map(wg, nh, nr, a.co_tiles, cot, r0, r1);
        gconvx3_body<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI, 0>(a, gcx3_lds, cot + r0 * a.co_tiles);
        if (r1 >= 0) {
            __syncthreads();  // (the first tile's last reads of stage 0 before the second tile's loads)
            gconvx3_body<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI, 0>(a, gcx3_lds, cot + r1 * a.co_tiles);
        }
        return;
    }
    const int per_phase = a.co_tiles * a.B * a.nbands * a.tpb;
    const int nph = MODE == kGcT2 ? 4 : 1;
    const int wg = xcd_remap((int)blockIdx.x, per_phase * nph);
    const int ph = wg / per_phase, wgi = wg - ph * per_phase;
    if constexpr (MODE == kGcT2) {
        switch (ph) {
            case 0: gconvx3_body<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI, 0>(a, gcx3_lds, wgi); break;
            case 1: gconvx3_body<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI, 1>(a, gcx3_lds, wgi); break;
            case 2: gconvx3_body<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI, 2>(a, gcx3_lds, wgi); break;
            default: gconvx3_body<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI, 3>(a, gcx3_lds, wgi); break;
        }
    } else {
        gconvx3_body<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI, 0>(a, gcx3_lds, wgi);
    }
}

// The narrow first layers (1 or 9 -> 16 channels) on the VALU: gsmall_kernel's arithmetic
// unchanged (f32 operands and sums, in_div, bias, activation); only the store differs: the f32
// value split into the c8x2 layout (16 channels = two hi and two lo cells per pixel).
template <int COUT>
__global__ void __launch_bounds__(kGsNT) gsmallx3_kernel(GconvX3Args a, const float *w) {
    static_assert(COUT == 16, "two channel blocks per pixel");
    __shared__ float ws[kGsMaxW];
    const int cin = a.c0;
    for (int i = threadIdx.x; i < COUT * cin * 9; i += kGsNT) ws[i] = w[i];
    __syncthreads();
    const long long HWs = (long long)a.ohs * a.ows;
    const long long npix = (long long)a.B * HWs;
    const long long HWi = (long long)a.Hi * a.Wi;
    const float *x = static_cast<const float *>(a.x0);
    for (long long p = (long long)blockIdx.x * kGsNT + threadIdx.x; p < npix; p += (long long)gridDim.x * kGsNT) {
        const int b = (int)(p / HWs);
        const int rem = (int)(p - (long long)b * HWs);
        const int oy = rem / a.ows, ox = rem - oy * a.ows;
        float acc[COUT];
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] = 0.f;
        const float *xb = x + (long long)b * cin * HWi;
        for (int ci = 0; ci < cin; ++ci) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = 2 * oy - 1 + ky;
                if ((unsigned)iy >= (unsigned)a.Hi) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = 2 * ox - 1 + kx;
                    if ((unsigned)ix >= (unsigned)a.Wi) continue;
                    float v = xb[(long long)ci * HWi + (long long)iy * a.Wi + ix];
                    if (a.in_div != 1.f) v = v / a.in_div;
#pragma unroll
                    for (int co = 0; co < COUT; ++co) acc[co] = fmaf(ws[(co * cin + ci) * 9 + ky * 3 + kx], v, acc[co]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < COUT / 4; ++q) {
            float u[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                u[r] = acc[4 * q + r] + a.bias[4 * q + r];
                if (a.act == kGcActRelu) u[r] = u[r] < 0.f ? 0.f : u[r];
                else if (a.act == kGcActTanh) u[r] = tanhf(u[r]);
            }
            gcx3_store4(a.ys, b, COUT / 8, 4 * q, HWs, rem, u, 4);
        }
    }
}

// f32 NCHW -> c8x2 (nlspn_gconv_x3_split; defined in nlspn_kern_gconv_x3_dg.hip): where a gradient
// enters a chain of split-bf16 data gradients in f32.  A lane per cell: eight channels of one
// pixel, split as gcx3_store4 splits them, a 16-byte hi and a 16-byte lo store.
struct Gx3SplitArgs {
    const float *x;  // (B, C, H, W)
    __bf16 *xs;      // (B, nb, 2, H, W, 8)
    int C, nb;
    long long HW, n;  // n = B nb HW cells
};
__global__ void gcx3_split_kernel(Gx3SplitArgs a);

// (the instantiated configurations: NLSPN_GCX3_CONFIGS, nlspn_kern_gconv_x3.hip; NLSPN_GCX3_DG_CONFIGS,
// nlspn_kern_gconv_x3_dg.hip; both lists in nlspn_gconv_plan.h)

}  // namespace nlspn
