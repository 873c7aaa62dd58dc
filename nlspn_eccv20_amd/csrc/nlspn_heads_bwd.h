// Backward of the head epilogue (nlspn_heads.h; nlspnmodel.py:296-315): the three last
// convolutions id_dec0 / off_aff_dec0 / cf_dec0 on cat(., fe1) under gradients.  R = nout + 2
// rows in the forward kernel's column order: 0..nout-1 off_aff_dec0, nout id_dec0 (ReLU),
// nout + 1 cf_dec0 (Sigmoid).
//
//   head_pre_kernel           gpre (B, R, H, W): the pre-activation gradient, zero rows for a
//                             missing gradient or head
//   (the two wide data gradients are an nlspn_gconv_dgrad launch of the stride-1 preset)
//   head_dgrad_single_kernel  the one-row adjoints d_fd_id / d_fd_cf on the VALU: 9 fmaf per
//                             element, taps in (ky, kx) order
//   hwgrad_kernel             the weight gradient of every row against [fd_oa | fe1]
//   hwgrad_single_kernel      the id / cf rows against their own decoder halves, VALU sums
//
// hwgrad_kernel is gwgrad_kernel's implicit GEMM (nlspn_gconv_bwd.h: v_mfma_f32_16x16x4_f32,
// exact f32 products, f32 accumulation; M = rows of gpre, N = (channel, tap), K = pixels; the
// same LDS layout and bank rule) retiled for this shape and pipelined:
//   * a tile is kHbMT = 32 rows x kHbNT = 64 channels x 9 taps: the forward's M-blocks (nout =
//     24 is one tile, 26 of 32 rows used, where the 64-row tile of the stride-1 GRU tiling
//     uses 26 of 64), every wave all 32 rows x 16 channels (72 accumulator registers);
//   * the next unit's operands are loaded into registers before the current unit's k-steps
//     and written to LDS after them: the global loads are in flight while the MFMAs run, where
//     gwgrad_kernel stages, waits, computes and waits again.
// Every load is a 4-byte scalar load: operands need 4-byte alignment only.  The id / cf rows
// against the fd_oa channels are padding of the tile (the reduce launches never read them).
// K slices, slabs and the fixed-order reduce are gwgrad_kernel's (gwgrad_reduce_kernel,
// gbias_partial_kernel): no atomics, no waiting between workgroups, the bits a function of the
// shape alone.  Every per-image base is ptr + (long long)b * stride.
#pragma once

#include "nlspn_gconv_bwd.h"
#include "nlspn_heads_bwd_plan.h"

namespace nlspn {

struct HeadPreArgs {
    const float *g_oa, *g_pi, *g_cf;  // incoming gradients (any may be null: zero rows)
    const float *pred_init, *conf;    // saved forward outputs (null with their gradient)
    float *gpre;                      // (B, R, H, W)
    int B, nout;
    long long HW;
};

__global__ void head_pre_kernel(HeadPreArgs a);

struct HeadDgSingleArgs {
    const float *gpre;        // (B, R, H, W)
    const float *w_id, *w_cf;  // the modules' (1, 2C, 3, 3) weights (the decoder half: channels < C)
    float *d_id, *d_cf;       // (B, C, H, W); a null pair skips that head
    int B, C, H, W, nout;
};

__global__ void head_dgrad_single_kernel(HeadDgSingleArgs a);

struct HwgradArgs {
    const float *g;        // gpre (B, R, H, W)
    const float *l0, *l1;  // fd_oa, fe1: (B, C, H, W) each
    const float *fd_id, *fd_cf;  // the one-row kernel's sources (may be null)
    float *ws;             // slabs [nsl][mtiles kHbMT][ntiles kHbNT][9]
    float *vec;            // the one-row partials [nvs][2][C][9]
    int R, C, B, H, W;
    int mtiles, ntiles, nsl, bw, nbands, units, ups, nvs;
};

__global__ void hwgrad_kernel(HwgradArgs a);
__global__ void hwgrad_single_kernel(HwgradArgs a);

#ifdef NLSPN_HEADS_BWD_DEFINE
__global__ void __launch_bounds__(256) head_pre_kernel(HeadPreArgs a) {
    const int R = a.nout + 2;
    const long long n = (long long)a.B * R * a.HW;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long br = e / a.HW, p = e - br * a.HW;
        const long long b = br / R;
        const int r = (int)(br - b * R);
        float v = 0.f;
        if (r < a.nout) {
            if (a.g_oa) v = a.g_oa[(b * a.nout + r) * a.HW + p];
        } else if (r == a.nout) {
            if (a.g_pi) v = a.pred_init[b * a.HW + p] > 0.f ? a.g_pi[b * a.HW + p] : 0.f;
        } else if (a.g_cf) {
            const float c = a.conf[b * a.HW + p];
            v = a.g_cf[b * a.HW + p] * (c * (1.f - c));
        }
        a.gpre[e] = v;
    }
}

__global__ void __launch_bounds__(256) head_dgrad_single_kernel(HeadDgSingleArgs a) {
    const long long HW = (long long)a.H * a.W, n = (long long)a.B * HW;
    const int R = a.nout + 2;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long b = e / HW;
        const int p = (int)(e - b * HW);
        const int y = p / a.W, x = p - y * a.W;
#pragma unroll
        for (int head = 0; head < 2; ++head) {
            float *d = head ? a.d_cf : a.d_id;
            if (!d) continue;
            const float *w = head ? a.w_cf : a.w_id;
            const float *g = a.gpre + (b * R + a.nout + head) * HW;
            // tap (ky, kx) of the forward reads the gradient at (y + 1 - ky, x + 1 - kx)
            float gv[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int gy = y + 1 - t / 3, gx = x + 1 - t % 3;
                gv[t] = (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W ? g[(long long)gy * a.W + gx] : 0.f;
            }
            d += b * a.C * HW + p;
            for (int ci = 0; ci < a.C; ++ci) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < 9; ++t) s = fmaf(w[ci * 9 + t], gv[t], s);
                d[(long long)ci * HW] = s;
            }
        }
    }
}

// One unit's operands in flight, a thread's share.  gpre rows [kHbMT][kHbBW]: pixel tid & 63 of
// rows (tid >> 6) + 4 j.  Window [kHbNT][3][kHbBW + 2]: column tid & 63 of window row j % 3 of
// channels (tid >> 6) + 4 (j / 3), then the two last columns of every (channel, row) spread
// over the threads.  (Offsets within an image are ints: the launcher keeps C H W below 2^29.)
constexpr int kHbGReg = kHbMT * kHbBW / kHbNTHR;
constexpr int kHbXReg = kHbNT * 3 * kHbBW / kHbNTHR, kHbXTail = kHbNT * 3 * 2;
constexpr int kHbXTReg = (kHbXTail + kHbNTHR - 1) / kHbNTHR;
static_assert(kHbBW == 64 && kHbNTHR == 256 && kHbNT % 4 == 0 && kHbMT % 4 == 0, "the staging map");

struct HbUnit {
    float g[kHbGReg], x[kHbXReg], xt[kHbXTReg];
    int k4;
};

__device__ __forceinline__ float hb_win(const HwgradArgs &a, const float *l0, const float *l1, int HW, int cl, int ly, int lx) {
    if (cl >= 2 * a.C || (unsigned)ly >= (unsigned)a.H || (unsigned)lx >= (unsigned)a.W) return 0.f;
    return (cl < a.C ? l0 + cl * HW : l1 + (cl - a.C) * HW)[ly * a.W + lx];
}

__device__ __forceinline__ void hb_load(const HwgradArgs &a, int u, int r0, int cl0, int tid, HbUnit &q) {
    const int band = u % a.nbands, row = u / a.nbands;  // row = b H + y
    const int b = row / a.H, y = row - b * a.H;
    const int bx0 = band * a.bw, bwi = min(a.bw, a.W - bx0);
    const int HW = a.H * a.W;
    const int p = tid & 63, w4 = tid >> 6;
    q.k4 = (bwi + 3) & ~3;
    const float *gb = a.g + (long long)b * a.R * HW + y * a.W + bx0 + p;
#pragma unroll
    for (int j = 0; j < kHbGReg; ++j) {
        const int r = r0 + w4 + 4 * j;
        q.g[j] = r < a.R && p < bwi ? gb[r * HW] : 0.f;
    }
    const float *l0 = a.l0 + (long long)b * a.C * HW, *l1 = a.l1 + (long long)b * a.C * HW;
#pragma unroll
    for (int j = 0; j < kHbXReg; ++j)
        q.x[j] = hb_win(a, l0, l1, HW, cl0 + w4 + 4 * (j / 3), y - 1 + j % 3, bx0 - 1 + p);
#pragma unroll
    for (int j = 0; j < kHbXTReg; ++j) {
        const int k = tid + kHbNTHR * j, cr = k >> 1, c = cr / 3;
        q.xt[j] = k < kHbXTail ? hb_win(a, l0, l1, HW, cl0 + c, y - 1 + cr - 3 * c, bx0 - 1 + kHbBW + (k & 1)) : 0.f;
    }
}

__device__ __forceinline__ void hb_store(const HbUnit &q, float *gs, float *xs, int tid) {
    const int p = tid & 63, w4 = tid >> 6;
#pragma unroll
    for (int j = 0; j < kHbGReg; ++j) gs[(w4 + 4 * j) * kHbGP + p] = q.g[j];
#pragma unroll
    for (int j = 0; j < kHbXReg; ++j) xs[(w4 + 4 * (j / 3)) * kHbXCP + (j % 3) * kHbXRP + p] = q.x[j];
#pragma unroll
    for (int j = 0; j < kHbXTReg; ++j) {
        const int k = tid + kHbNTHR * j, cr = k >> 1, c = cr / 3;
        if (k < kHbXTail) xs[c * kHbXCP + (cr - 3 * c) * kHbXRP + kHbBW + (k & 1)] = q.xt[j];
    }
}

// (two workgroups per CU: 74 KB of LDS each, two waves per SIMD, at most 256 registers a lane)
__global__ void __launch_bounds__(kHbNTHR) __attribute__((amdgpu_waves_per_eu(2, 2))) hwgrad_kernel(HwgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float hb_lds[];
    float *gs = hb_lds, *xs = hb_lds + kHbMT * kHbGP;
    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int l16 = lane & 15, lg = lane >> 4;
    const int ntile = a.mtiles * a.ntiles;
    const int tile = (int)blockIdx.x % ntile, sl = (int)blockIdx.x / ntile;
    const int mt = tile % a.mtiles, nt = tile / a.mtiles;
    const int r0 = mt * kHbMT, cl0 = nt * kHbNT;

    f32x4v acc[2][9];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[m][t] = f32x4v{0.f, 0.f, 0.f, 0.f};

    const int u0 = sl * a.ups, u1 = min(a.units, u0 + a.ups);
    const int ab = l16 * kHbGP + lg;             // A: row l16 of block m = 0, pixel lg
    const int bb = (wn * 16 + l16) * kHbXCP + lg;  // B: channel l16 of this wave's 16, pixel lg
    HbUnit q;
    if (u0 < u1) hb_load(a, u0, r0, cl0, tid, q);
    for (int u = u0; u < u1; ++u) {
        const int k4 = q.k4;
        hb_store(q, gs, xs, tid);
        __syncthreads();
        if (u + 1 < u1) hb_load(a, u + 1, r0, cl0, tid, q);  // in flight during the k-steps below
        for (int p0 = 0; p0 < k4; p0 += 4) {
            const float a0 = gs[ab + p0], a1 = gs[ab + 16 * kHbGP + p0];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float bv = xs[bb + (t / 3) * kHbXRP + t % 3 + p0];
                acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // lane l, register r of block (m, t): row 16 m + 4 (l >> 4) + r, channel l & 15
    const int Clp = a.ntiles * kHbNT;
    float *slab = a.ws + (long long)sl * a.mtiles * kHbMT * Clp * 9;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 16 * m + 4 * lg + r;
            float *d = slab + ((long long)row * Clp + cl0 + wn * 16 + l16) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) d[t] = acc[m][t][r];
        }
}

// vec[((sl 2 + head) C + c) 9 + t] = the sum over slice sl's range of the (image, pixel) index
// space of gpre[nout + head] at the pixel times the head's decoder output c at tap t's
// neighbour, in a fixed order (a thread's strided elements in turn, then a tree)
__global__ void __launch_bounds__(256) hwgrad_single_kernel(HwgradArgs a) {
    __shared__ float red[9][256];
    const int head = (int)blockIdx.x % 2, c = (int)(blockIdx.x / 2) % a.C, sl = (int)blockIdx.x / (2 * a.C);
    const float *src = head ? a.fd_cf : a.fd_id;
    if (!src) return;
    const long long HW = (long long)a.H * a.W, n = (long long)a.B * HW, per = (n + a.nvs - 1) / a.nvs;
    const long long e0 = sl * per, e1 = min(n, e0 + per);
    float sum[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) sum[t] = 0.f;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
        const long long b = e / HW;
        const int p = (int)(e - b * HW);
        const int y = p / a.W, x = p - y * a.W;
        const float v = src[(b * a.C + c) * HW + p];
        const float *g = a.g + (b * a.R + (a.R - 2 + head)) * HW;
        // the source pixel (y, x) is tap (ky, kx)'s neighbour of the gradient at (y + 1 - ky, x + 1 - kx)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int gy = y + 1 - t / 3, gx = x + 1 - t % 3;
            if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) sum[t] = fmaf(g[(long long)gy * a.W + gx], v, sum[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) red[t][threadIdx.x] = sum[t];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int t = 0; t < 9; ++t) red[t][threadIdx.x] += red[t][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 9) a.vec[(((long long)sl * 2 + head) * a.C + c) * 9 + threadIdx.x] = red[threadIdx.x][0];
}
#endif  // NLSPN_HEADS_BWD_DEFINE

}  // namespace nlspn
