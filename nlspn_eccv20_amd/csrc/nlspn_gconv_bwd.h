// Backward of the GRU-mode convolutions (nlspn_gconv.h): the weight / bias gradient kernels and
// the ConvGRU's gate derivatives.  (The data gradients are forward launches of the adjoint
// layer kind with the kGcEpiDact epilogue, NLSPN_GC_DG_CONFIGS.)
//
// Weight gradient.  Every GRU-mode layer is a 3x3 pad-1 correlation between a SMALL tensor s
// (B, Cs, Hs, Ws) and a LARGE tensor l (B, Cl, Hl, Wl) at stride S in {1, 2}:
//     dW[cs][cl][ky][kx] = sum_{b, sy, sx} s[b, cs, sy, sx] * l[b, cl, S sy - 1 + ky, S sx - 1 + kx]
// (l = 0 outside its stored size).  A stride-S convolution has s = the output gradient and l =
// the input; a stride-2 transposed convolution has s = the input and l = the output gradient
// (stored cropped: the rows / columns past the crop are the zeros above).  In both cases
// (Cs, Cl, 3, 3) is the module's own weight layout.
//
// An implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation): M = small
// channels, N = (large channel, tap), K = pixels.  A workgroup of WGM x WGN waves owns
// 16 WM WGM small channels x 16 WGN large channels x 9 taps; a wave holds WM x 9 16x16 blocks
// (lane l: A[cs = l & 15][pixel = l >> 4], B[pixel = l >> 4][cl = l & 15] at one tap).  K is cut
// into units (image, small row, column band of at most kGwBW pixels); per unit the workgroup
// stages the small row [cs][pixel] and the large window [cl][3 rows][S bw + 2 columns] in LDS
// (zero outside the tensors and past the band), then runs the band's 4-pixel k-steps.
//
// LDS banks: the 16 lanes l & 15 of an operand read sit one channel pitch apart and the lane
// groups l >> 4 one pixel apart, and a ds_read_b32 serves lanes 0-31 (groups 0, 1) and 32-63 in
// turn: a channel pitch = 2 (mod 32) puts the 32 lanes of a half on 32 different banks.  At
// stride 2 the window's even and odd columns are stored apart (kGwHALF = 16 (mod 32) words, so
// the staging stores do not collide either): a tap's pixels are then consecutive words too.
//
// K is split over workgroups (slices of consecutive units) to fill the chip; each slice writes
// its f32 slab [cs][cl][9] into the caller's workspace and gwgrad_reduce_kernel, a second
// launch, sums the slabs in slice order: no float atomics, no waiting between workgroups, and
// the same bits on every run.  The bias gradient (per-channel sum of the output gradient) has
// the same two-launch form (gbias_partial_kernel, then the reduce kernel).
#pragma once

#include "nlspn_gconv.h"
#include "nlspn_gwgrad_plan.h"  // kGwBW (pixels per unit at most) and the plan of a call

namespace nlspn {

constexpr int kGwGP = 66;     // small row pitch per channel (>= kGwBW, = 2 mod 32)
constexpr int kGwHALF = 80;   // stride 2: offset of the odd columns in a window row (>= kGwBW + 1, = 16 mod 32)
// window row pitch: 3 pitches = 2 (mod 32), i.e. the pitch = 22 (mod 32)
__host__ __device__ constexpr int gw_xrp(int S) { return S == 2 ? 150 : 86; }  // >= kGwHALF + kGwBW + 1 / kGwBW + 2
static_assert(kGwGP % 32 == 2 && kGwHALF % 32 == 16 && (3 * gw_xrp(1)) % 32 == 2 && (3 * gw_xrp(2)) % 32 == 2, "bank rule");
static_assert(gw_xrp(2) >= kGwHALF + kGwBW + 1 && gw_xrp(1) >= kGwBW + 2 && kGwGP >= kGwBW, "window fits");

struct GwgradArgs {
    const float *s;         // small (B, Cs, Hs, Ws)
    const float *l0, *l1;   // large: channels [0, c0) of (B, c0, Hl, Wl), then [c0, c0 + c1) of (B, c1, Hl, Wl)
    float *ws;              // slabs [nsl][mtiles MT][ntiles NT][9]
    int Cs, c0, c1, B, Hs, Ws, Hl, Wl;
    int mtiles, ntiles, nsl;
    int bw, nbands, units, ups;  // band width, bands, units = B Hs nbands, units per slice
};

template <int S, int WM, int WGM, int WGN>
struct GwCfg {
    static constexpr int NTHR = 64 * WGM * WGN, MT = 16 * WM * WGM, NT = 16 * WGN;
    static constexpr int XRP = gw_xrp(S), XCP = 3 * XRP;
    static constexpr int LDS_FLOATS = MT * kGwGP + NT * XCP;
};

template <int S, int WM, int WGM, int WGN>
__global__ void __launch_bounds__(64 * WGM * WGN) gwgrad_kernel(GwgradArgs a) {
    using Cfg = GwCfg<S, WM, WGM, WGN>;
    constexpr int NTHR = Cfg::NTHR, MT = Cfg::MT, NT = Cfg::NT, XRP = Cfg::XRP, XCP = Cfg::XCP;
    extern __shared__ __attribute__((aligned(16))) float gw_lds[];
    float *gs = gw_lds, *xs = gw_lds + MT * kGwGP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv % WGM, wn = wv / WGM;
    const int l16 = lane & 15, lg = lane >> 4;
    const int ntile = a.mtiles * a.ntiles;
    const int tile = (int)blockIdx.x % ntile, sl = (int)blockIdx.x / ntile;
    const int mt = tile % a.mtiles, nt = tile / a.mtiles;
    const int cs0 = mt * MT, cl0 = nt * NT;
    const long long HWs = (long long)a.Hs * a.Ws, HWl = (long long)a.Hl * a.Wl;

    f32x4v acc[WM][9];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[m][t] = f32x4v{0.f, 0.f, 0.f, 0.f};

    const int u0 = sl * a.ups, u1 = min(a.units, u0 + a.ups);
    const int ab = (wm * WM * 16 + l16) * kGwGP + lg;  // A: small channel l16 of block m = 0, pixel lg
    const int bb = (wn * 16 + l16) * XCP;              // B: large channel l16
    for (int u = u0; u < u1; ++u) {
        const int band = u % a.nbands;
        const int row = u / a.nbands;  // = b Hs + sy
        const int b = row / a.Hs, sy = row - b * a.Hs;
        const int bx0 = band * a.bw, bwi = min(a.bw, a.Ws - bx0);
        const int k4 = (bwi + 3) & ~3;
        const int ncol = S * (k4 - 1) + 3;  // window columns the k-steps read
        // the small row: [MT][k4], zero past the band / the channels
        for (int i = tid; i < MT * k4; i += NTHR) {
            const int c = i / k4, p = i - c * k4;
            const int cs = cs0 + c;
            float v = 0.f;
            if (cs < a.Cs && p < bwi) v = a.s[((long long)b * a.Cs + cs) * HWs + (long long)sy * a.Ws + bx0 + p];
            gs[c * kGwGP + p] = v;
        }
        // the large window: [NT][3][ncol], zero outside the tensor / past the channels
        const int ly0 = S * sy - 1, lx0 = S * bx0 - 1;
        for (int i = tid; i < NT * 3 * ncol; i += NTHR) {
            const int cr = i / ncol, wc = i - cr * ncol;
            const int c = cr / 3, r = cr - 3 * c;
            const int cl = cl0 + c, ly = ly0 + r, lx = lx0 + wc;
            float v = 0.f;
            if ((unsigned)ly < (unsigned)a.Hl && (unsigned)lx < (unsigned)a.Wl && cl < a.c0 + a.c1) {
                const float *src = cl < a.c0 ? a.l0 + ((long long)b * a.c0 + cl) * HWl
                                             : a.l1 + ((long long)b * a.c1 + (cl - a.c0)) * HWl;
                v = src[(long long)ly * a.Wl + lx];
            }
            xs[c * XCP + r * XRP + (S == 2 ? (wc & 1) * kGwHALF + (wc >> 1) : wc)] = v;
        }
        __syncthreads();
        for (int p0 = 0; p0 < k4; p0 += 4) {
            float av[WM];
#pragma unroll
            for (int m = 0; m < WM; ++m) av[m] = gs[ab + 16 * m * kGwGP + p0];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t % 3;
                // window column S p + kx of pixel p = p0 + lg; stride 2: its parity half and index
                const int wo = S == 2 ? (kx & 1) * kGwHALF + (kx >> 1) : kx;
                const float bv = xs[bb + ky * XRP + wo + p0 + lg];
#pragma unroll
                for (int m = 0; m < WM; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv, acc[m][t], 0, 0, 0);
            }
        }
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

// out[(i * n1 + j) * T + t] = scale * sum_sl ws[sl * slab + (i * n1p + j) * T + t], slices in order

__global__ void gwgrad_reduce_kernel(const float *ws, float *out, int n0, int n1, int n1p, int T, long long slab,
                                     int nsl, float scale);

// Bias gradient partials: ws[sl * C + c] = the sum of channel c of g (B, C, H, W) over slice
// sl's range of the (image, pixel) index space, in a fixed order (a lane's strided elements in
// turn, then a tree over the workgroup).

__global__ void gbias_partial_kernel(const float *g, float *ws, int C, int B, long long HW, int nsl);

// The ConvGRU's gate derivatives (nlspnmodel.py:398-403: z, r = sigmoid(..), q = tanh(..),
// h' = (1 - z) h + z q), pointwise on (B, hc, H, W) planes; duzr is (B, 2 hc, H, W) = [du_z, du_r],
// the pre-activation gradients of convz / convr in torch.cat order.
//   stage 1 (before the q data gradient):  du_q = dh' z (1 - q^2);  du_z = dh' (q - h) z (1 - z)
//   stage 2 (after it returned d(rh)):     du_r = d(rh) h r (1 - r);  dh = dh' (1 - z) + d(rh) r
//   stage 0: a chain's last activation, out = g act'(y) (y in `z`, g in `dhn`, out in `duq`)
struct GgatesArgs {
    const float *dhn, *z, *r, *q, *h, *drh;
    float *duq, *duzr, *dh;
    int hc, act;
    long long HW, n;  // n = B hc HW
};

__global__ void ggates_kernel(GgatesArgs a, int stage);

// The weight-gradient tilings: X(S, WM, WGM, WGN).  64 x 32 channels for the wide layers; 128 x 16
// when the large tensor has at most 16 channels; one wave (16 x 16) for the narrow layers (1 / 9
// -> 16, 16 -> 8), which are bound by their few MB of traffic.  (Which one a shape takes:
// gw_choose, nlspn_gwgrad_plan.h.)
#define NLSPN_GW_CONFIGS(X) \
    X(1, 2, 2, 2)           \
    X(2, 2, 2, 2)           \
    X(2, 2, 4, 1)           \
    X(2, 1, 1, 1)

}  // namespace nlspn
