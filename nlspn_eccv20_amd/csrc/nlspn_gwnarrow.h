// Streaming weight gradient of the narrow stride-2 layers (1 / 9 -> 16, 16 -> 8: both channel
// counts <= 16), the correlation of nlspn_gconv_bwd.h on v_mfma_f32_16x16x4_f32 (exact f32
// products, f32 sums) for shapes whose cost is traffic and staging, not arithmetic.
//
// M = small channels (one 16-row block), N = (large channel, tap) flattened, 9 Cl entries in NB =
// ceil(9 Cl / 16) blocks (1, 5, 6, 9 for Cl = 1, 8, 9, 16: no N lane is spent on a zero channel),
// K = pixels.  A unit is (image, kGwnR small rows, column band of at most kGwnBW pixels): the
// workgroup's kGwnNW waves stage the R small rows and the 2 R + 1 window rows they share (a
// large row is fetched once; the halo row alone is fetched by the unit above too), then wave w
// runs row w's 4-pixel k-steps.  Staging goes by rows: a half wave takes one (channel, row)
// line and loads it in 16-byte chunks from the 16-byte boundary at or before its first column
// (gwn_chunks: any 4-byte aligned operand and any row pitch); a chunk that is not wholly inside
// the tensor's row is loaded by dwords under predicates.  One division per line, none per
// element.  Everything the k-loop reads is written by the unit's staging (zeros outside the
// tensor and past the band), tests/gwnarrow_plan_check.cpp replays it.
//
// The bias gradient comes from the staged operand: from the small side it is the sum of the A
// operands the k-steps read (a lane's pixels in turn); from the large side the sum of the
// window cells the unit owns (rows 2 sy0 .. 2 sy0 + 2 R - 1, columns 2 bx0 .. 2 (bx0 + bw) - 1:
// window rows 1 .. 2 R, window columns 1 .. 2 bw; zeros stand for what the crop cut off).
//
// A slice of consecutive units ends with the waves' accumulators summed through LDS in wave
// order into one slab; gwnarrow_reduce_kernel sums the slabs in two fixed-order levels (16
// slice lanes, then their 16 partials) and writes dW and db.  No atomics, no waiting between
// workgroups, two launches per call.
#pragma once

#include <cstdint>

#include "nlspn_gconv.h"
#include "nlspn_gwnarrow_plan.h"

namespace nlspn {

struct GwnArgs {
    const float *s;  // small (B, Cs, Hs, Ws)
    const float *l;  // large (B, Cl, Hl, Wl)
    float *ws;       // slabs [nsl][slab]
    int Cs, Cl, B, Hs, Ws, Hl, Wl;
    int nbands, bw, ngroups, units, ups;
    int bias_from_large;
    long long slab;
};

static_assert(gwn_lds_floats(9) * 4 <= kGwnLdsBudget, "LDS budget");

// Columns [xf, xf + cnt) of a tensor row of W floats (row: its column 0; !rowok: a row outside
// the tensor) into LDS at off(k), k = column - xf: the row's values in [lo, hi), zeros elsewhere.
// The 32 lanes of a half wave (l32) take the row's chunks in turn.
template <bool WINDOW>
__device__ inline void gwn_stage_line(float *lds, const float *row, bool rowok, int W, int xf, int cnt, int lo, int hi,
                                      int c, int rj, int l32) {
    const GwnChunks ch = gwn_chunks(rowok ? (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3) : 0, xf, cnt);
    for (int q = l32; q < ch.nch; q += 32) {
        const int x4 = ch.xs + 4 * q;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (rowok) {
            if (x4 >= 0 && x4 + 4 <= W) {
                const float4 t = *reinterpret_cast<const float4 *>(row + x4);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x4 + e >= lo && x4 + e < hi) v[e] = row[x4 + e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = x4 + e, k = x - xf;
            if (k >= 0 && k < cnt) lds[WINDOW ? gwn_b_off(c, rj, k) : gwn_a_off(rj, c, k)] = (x >= lo && x < hi) ? v[e] : 0.f;
        }
    }
}

template <int NB>
__global__ void __launch_bounds__(kGwnNTHR) gwnarrow_kernel(GwnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gwn_lds[];
    float *bl = gwn_lds + (gwn_lds_floats(NB) - 16);  // the large side's bias sums
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l16 = lane & 15, lg = lane >> 4, l32 = lane & 31, hw = 2 * wv + (lane >> 5);
    const int Cs = a.Cs, Cl = a.Cl, nent = 9 * Cl;

    f32x4v acc[NB];
    int boff[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        acc[nb] = f32x4v{0.f, 0.f, 0.f, 0.f};
        const int n = nb * 16 + l16;  // (an entry past the count reads entry 0: its column is never stored)
        boff[nb] = gwn_b_read(n < nent ? n : 0, wv, lg);
    }
    const int aoff = gwn_a_read(l16 < Cs ? l16 : 0, wv, lg);  // (likewise a channel past the count)
    float bsum = 0.f;
    if (tid < 16) bl[tid] = 0.f;

    const int u0 = (int)blockIdx.x * a.ups, u1 = min(a.units, u0 + a.ups);
    for (int u = u0; u < u1; ++u) {
        const GwnUnit n = gwn_unit(u, a.nbands, a.bw, a.ngroups, a.Hs, a.Ws);
        const int nlines = gwn_lines(Cs, Cl, n.nrows);
        for (int li = hw; li < nlines; li += 2 * kGwnNW) {
            const GwnLine q = gwn_line(li, Cs, n.nrows);
            if (!q.window) {
                const float *row = a.s + (((long long)n.b * Cs + q.c) * a.Hs + n.sy0 + q.rj) * a.Ws;
                gwn_stage_line<false>(gwn_lds, row, true, a.Ws, n.bx0, n.k4, n.bx0, n.bx0 + n.bwi, q.c, q.rj, l32);
            } else {
                const int ly = 2 * n.sy0 - 1 + q.rj, xf = 2 * n.bx0 - 1, cnt = 2 * n.k4 + 1;
                const bool ok = ly >= 0 && ly < a.Hl;
                const float *row = ok ? a.l + (((long long)n.b * Cl + q.c) * a.Hl + ly) * a.Wl : a.l;
                gwn_stage_line<true>(gwn_lds, row, ok, a.Wl, xf, cnt, max(0, xf), min(a.Wl, xf + cnt), q.c, q.rj, l32);
            }
        }
        __syncthreads();
        if (wv < n.nrows) {
            for (int p0 = 0; p0 < n.k4; p0 += 4) {
                const float av = gwn_lds[aoff + p0];
                bsum += av;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, gwn_lds[boff[nb] + p0], acc[nb], 0, 0, 0);
            }
        }
        if (a.bias_from_large) {
            for (int cl = wv; cl < Cl; cl += kGwnNW) {
                float v = 0.f;
                for (int j = 1; j <= 2 * n.nrows; ++j)
                    for (int i = lane; i < n.bwi; i += 64) v += gwn_lds[gwn_b_off(cl, j, 2 * i + 1)] + gwn_lds[gwn_b_off(cl, j, 2 * i + 2)];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) bl[cl] += v;
            }
        }
        __syncthreads();
    }
    // the waves' accumulators and bias partials through LDS (over the stage), summed in wave order
    float *red = gwn_lds, *bred = gwn_lds + kGwnNW * NB * 256;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wv * NB + nb) * 256 + r * 64 + lane] = acc[nb][r];
    bred[wv * 64 + lane] = bsum;
    __syncthreads();
    float *slab = a.ws + (long long)blockIdx.x * a.slab;
    for (int e = tid; e < NB * 256; e += kGwnNTHR) {
        float sum = red[e];
#pragma unroll
        for (int w = 1; w < kGwnNW; ++w) sum += red[w * NB * 256 + e];
        slab[e] = sum;
    }
    if (tid < 16) {
        float sum = bl[tid];
        if (!a.bias_from_large) {
            sum = 0.f;
            for (int w = 0; w < kGwnNW; ++w)
                for (int g = 0; g < 4; ++g) sum += bred[w * 64 + g * 16 + tid];
        }
        slab[NB * 256 + tid] = sum;
    }
}

// dw[cs][n] = scale * the sum over the slices of their slabs' element, db[c] = the sum of their
// bias sums.  A workgroup owns 16 outputs (the last one the bias gradient's); slice lane j sums
// slices j, j + 16, .. in turn, then one thread per output sums the 16 lanes' partials in order.
__global__ void gwnarrow_reduce_kernel(const float *ws, float *dw, float *db, int Cs, int Cl, int nbias, int nsl,
                                       long long slab, int nb, float scale);

#define NLSPN_GWN_BLOCKS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9)

}  // namespace nlspn
