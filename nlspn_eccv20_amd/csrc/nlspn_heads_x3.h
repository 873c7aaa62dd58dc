// Head epilogue on the bf16 matrix cores with split operands ("bf16x3",
// v_mfma_f32_32x32x16_bf16), inference only, opt-in (heads.head_epilogue(precision="bf16x3"),
// NLSPNModel.head_precision): heads_kernel's implicit GEMM (nlspn_heads.h) with every f32 MFMA
// operand carried as two bf16 parts.  The f32 kernel, its packing and its unit are untouched.
//
// Numerics contract (include/nlspn_prop.h):
//   - Every MFMA operand value a (f32) travels as hi = rne_bf16(a), lo = rne_bf16(a - hi), the
//     subtraction in f32.  Weights are split once, when they are packed (headsx3_pack_kernel);
//     activations (fe1, off_aff_fd1) while the window is staged into LDS (Hx3Win::store).
//   - Per output element the kernel accumulates sum (w_hi x_hi + w_hi x_lo + w_lo x_hi) in the
//     MFMA's f32 accumulators; lo lo is dropped.  bf16 x bf16 products are exact in f32, and
//     |a - hi - lo| <= 2^-17 |a|, |a - hi| <= 2^-8 |a|, so a term is off by at most 2^-15 |w x|
//     before accumulation rounding.
//   - The one-channel halves (id_fd1 for the id conv, cf_fd1 for the cf conv) stay the f32
//     kernel's VALU fmaf sums on unsplit f32 operands: same window, same order.  Only the MFMA
//     part changes: fe1 for all columns, off_aff_fd1 for the off / aff columns.
//   - Bias, ReLU, sigmoid and the fused prologue run in f32 on the accumulators.  The fused
//     prologue is the f32 kernel's own device function (heads_epilogue_prologue, with its
//     32-lane shuffle and normalize_taps); the plain epilogue is inline in heads_kernel, and
//     moving it into a shared function changed that unit's register allocation, so
//     headsx3_epilogue_plain below repeats its 25 lines word for word.
//   - Nothing is clamped: a NaN input reaches exactly its 3x3 neighbourhood; an inf operand
//     gives NaN there (inf has lo = inf - inf = NaN).
//   - No atomics and no waiting between workgroups: the same bits on every run.
//
// Tile, rounds and accumulator map are the f32 kernel's: 8 x 32 pixels, 256 threads (4 waves x 2
// rows), rounds of 16 channels of one source, lane (px, h) register r of M-block m = output
// channel 32 m + (r&3) + 8(r>>2) + 4h.  One MFMA covers one tap of a whole round: lane
// (l32, h = l >> 5) holds A[co = l32][k = 8h + j] and B[k = 8h + j][px = l32], j = 0..7, each one
// 16-byte LDS read (nlspn_heads_x3_plan.h has the layout and its bank argument).  Three MFMAs
// per (tap, row, M-block): hi hi, hi lo, lo hi.
//
// Staging: a thread loads the 8 channels of one window pixel (8 dwords a channel plane apart,
// consecutive lanes consecutive columns: coalesced, and no alignment rule, so one form serves
// every W), from a clamped in-image address; gw16_split packs channel pairs into dwords and the
// in-image mask is applied at the two 16-byte LDS stores (HdWin's rule).  The window is the 34
// columns the taps read, not the 40 of the aligned float4 form.  The next round's loads are in
// flight in registers while the round computes.  The VALU window is HdWin<VEC> as before.
//
// LDS (hx3_lds_bytes) and registers: 67 / 85 / 103 / 139 KB + 72 C bytes for MB = 1 / 2 / 3 / 5.
// The MB = 1 builds with the float4 VALU window (W % 4 == 0: the NYU and KITTI models, plain and
// fused prologue) hold 252 / 254 registers and run TWO workgroups per CU (waves_per_eu 2), as
// the f32 kernel; every other build runs ONE (waves_per_eu 1, 290-500 registers): the scalar
// VALU window's addresses (MB = 1) or the accumulators and the weights in flight (MB >= 2) do
// not fit in 256, and LDS allows one workgroup from MB = 2 on anyway.  No scratch in any build
// (tests/test_heads_x3_cpu.py).  Measured (tools/head_x3_bench.py): two workgroups
// per CU took the NYU B=8 epilogue from 0.364 to 0.261 ms.
#pragma once

#include "nlspn_gwgrad16.h"  // gw16_split
#include "nlspn_heads.h"
#include "nlspn_heads_x3_plan.h"

namespace nlspn {

static_assert(kHx3TH == kHdTH && kHx3TW == kHdTW && kHx3NT == kHdNT && kHx3CC == kHdCC, "the f32 kernel's tile");

typedef __bf16 hx3_bf8 __attribute__((ext_vector_type(8)));

template <int MB> struct Hx3Cfg {
    static constexpr int WC = hx3_w_cells(MB);               // cells of one round's weights
    static constexpr int WR = (WC + kHx3NT - 1) / kHx3NT;    // per thread
    // A k-loop step is one (tap, M-block) for both tile rows of the wave: 6 MFMAs; with one
    // M-block a step is one row (3 MFMAs), so the fragments of a step stay two b128 pairs
    static constexpr int NH = MB == 1 ? 2 : 1;
    static constexpr int NS = 9 * MB * NH;                   // steps per round
    static constexpr int NV = (kHdCC / 2) * 9;               // the f32 kernel's VALU steps per round (72)
    static constexpr int VG = (NV + NS - 1) / NS;            // VALU steps of an MFMA step at most
};

// The MFMA source window of a round in flight in registers: per staging item the 8 channels of
// one window pixel, and one in-image bit per item.
struct Hx3Win {
    float v[kHx3XR][8];
    unsigned vo[kHx3XR];  // byte offset of the item's first channel within a round's 16 planes (clamped in-image)
    unsigned m;

    __device__ __forceinline__ void init(long long HW, int H, int W, int y0, int x0, int tid) {
        m = 0;
#pragma unroll
        for (int i = 0; i < kHx3XR; ++i) {
            int kh, row, col;
            hx3_x_item(min(tid + i * kHx3NT, kHx3XItems - 1), kh, row, col);
            const int y = y0 - 1 + row, x = x0 - 1 + col;
            m |= ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? (1u << i) : 0u;
            vo[i] = (unsigned)((8 * kh * HW + (long long)min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1)) * 4);
        }
    }
    // rs: the round's 16 channel planes of this image (buffer loads: one 32-bit offset per item,
    // the channel step in a scalar register, so no 64-bit address is held per load)
    __device__ __forceinline__ void load(rsrc_t rs, unsigned plane_bytes) {
#pragma unroll
        for (int i = 0; i < kHx3XR; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                v[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo[i], j * plane_bytes, 0));
    }
    __device__ __forceinline__ void store(u32x4 *XS, int tid) const {
#pragma unroll
        for (int i = 0; i < kHx3XR; ++i) {
            const int it = tid + i * kHx3NT;
            if (it < kHx3XItems) {
                int kh, row, col;
                hx3_x_item(it, kh, row, col);
                const unsigned mk = (m >> i & 1u) ? ~0u : 0u;
                u32x4 hi, lo;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    unsigned a, b;
                    gw16_split(v[i][2 * q], v[i][2 * q + 1], a, b);
                    hi[q] = a & mk;
                    lo[q] = b & mk;
                }
                XS[hx3_x_cell(0, kh, row, col)] = hi;
                XS[hx3_x_cell(1, kh, row, col)] = lo;
            }
        }
    }
};

// heads_kernel's plain epilogue (nlspn_heads.h), word for word: bias + activation on the
// accumulators, the VALU sums by pixel from SV, coalesced row stores.
template <int MB>
__device__ __forceinline__ void headsx3_epilogue_plain(const HeadsArgs &a, const f32x16 (&acc)[MB][2],
                                                       const float (&bv)[MB][16], const float *SV, int b, int y0,
                                                       int x, int wv, int h, int l32) {
    const int H = a.H, W = a.W;
    const long long HW = (long long)H * W;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int yl = 2 * wv + n, y = y0 + yl;
        if (y >= H || x >= W) continue;
        const long long pix = (long long)y * W + x;
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float v = acc[m][n][r] + bv[m][r];
                if (co < a.nout) {
                    a.off_aff[((long long)b * a.nout + co) * HW + pix] = v;
                } else if (co == a.nout) {
                    if (a.pred_init) {
                        const float u = v + SV[yl * kHdTW + l32];
                        a.pred_init[(long long)b * HW + pix] = u < 0.f ? 0.f : u;  // ReLU (NaN kept)
                    }
                } else if (co == a.nout + 1) {
                    if (a.conf) {
                        const float u = v + SV[kHdNT + yl * kHdTW + l32];
                        a.conf[(long long)b * HW + pix] = 1.f / (1.f + expf(-u));  // Sigmoid
                    }
                }
            }
    }
}

template <int MB, bool VEC, bool PRO = false>
__global__ void __launch_bounds__(kHx3NT)
    __attribute__((amdgpu_waves_per_eu((MB == 1 && VEC) ? 2 : 1, (MB == 1 && VEC) ? 2 : 1)))  // workgroups per CU
    headsx3_kernel(HeadsArgs a) {
    using Cfg = Hx3Cfg<MB>;
    constexpr int WC = Cfg::WC, NH = Cfg::NH, NS = Cfg::NS, NV = Cfg::NV, VG = Cfg::VG;
    extern __shared__ __attribute__((aligned(16))) u32x4 hx3_lds[];
    u32x4 *XS = hx3_lds;                                 // the MFMA source window, split
    u32x4 *WS = XS + kHx3XCells;                         // the round's weight fragments
    float *XV = reinterpret_cast<float *>(WS + WC);      // [16][CS]   VALU source window (f32)
    float *SV = XV + kHdCC * kHdCS;                      // [2][256]   the VALU sums per pixel
    float *WVL = SV + 2 * kHdNT;                         // [2][C][9]  the VALU weights (all rounds)

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int ntile = a.tiles_x * a.tiles_y * a.B;
    const int tile = xcd_remap(blockIdx.x, ntile);
    const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * a.tiles_x * a.tiles_y;
    const int ty = tr / a.tiles_x, tx = tr - ty * a.tiles_x;
    const int y0 = ty * kHdTH, x0 = tx * kHdTW;
    const int H = a.H, W = a.W, C = a.C;
    const long long HW = (long long)H * W;
    const int nch = C / kHdCC, nr = 2 * nch;
    const float *vsrc[2] = {a.fd_id ? a.fd_id : a.fe1, a.fd_cf ? a.fd_cf : a.fe1};
    const u32x4 *wpk = reinterpret_cast<const u32x4 *>(a.wm);

    Hx3Win xm;
    HdWin<VEC> xv;
    u32x4 wr[Cfg::WR];
    xm.init(HW, H, W, y0, x0, tid);
    const unsigned plane_bytes = (unsigned)(HW * 4);  // (16 planes stay below 2^31 bytes: the launcher's check)
    auto load_round = [&](int r) __attribute__((always_inline)) {
        const int s = r < nch ? 0 : 1, ck = r - s * nch;
        const long long off = ((long long)b * C + ck * kHdCC) * HW;
        const rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>((s == 0 ? a.fe1 : a.fd_oa) + off), (short)0,
                                                            (int)(kHdCC * plane_bytes), 0x00020000);
        xm.load(rx, plane_bytes);
        xv.load(vsrc[s] + off, HW, H, W, y0, x0, tid);
        const rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4 *>(wpk + hx3_w_round(C, s, ck) * WC), (short)0,
                                                            WC * 16, 0x00020000);
#pragma unroll
        for (int i = 0; i < Cfg::WR; ++i)
            wr[i] = __builtin_amdgcn_raw_buffer_load_b128(rw, (unsigned)min(tid, WC - 1 - i * kHx3NT) * 16u,
                                                          i * kHx3NT * 16, 0);
    };

    f32x16 acc[MB][2];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
    float sv_id = 0.f, sv_cf = 0.f;  // VALU sums of this thread's pixel
    const int vrow = tid >> 5, vcol = tid & 31;

    for (int i = tid; i < 2 * C * 9; i += kHdNT) WVL[i] = a.wv[i];  // read as LDS broadcasts
    load_round(0);
    for (int r = 0; r < nr; ++r) {
        __syncthreads();  // the previous round's LDS reads are done
        xm.store(XS, tid);
        xv.store(XV, tid);
#pragma unroll
        for (int i = 0; i < Cfg::WR; ++i) {
            const int f = tid + i * kHx3NT;
            if (f < WC) WS[f] = wr[i];
        }
        __syncthreads();
        // the next round's loads, in flight while this round computes (the last round reloads
        // round 0, unused: no branch, so no wait at a join)
        load_round(r + 1 < nr ? r + 1 : 0);
        __builtin_amdgcn_sched_barrier(0);  // keep them ahead of the compute
        const int s = r < nch ? 0 : 1;
        const float *wvp = WVL + (s * C + (r - s * nch) * kHdCC) * 9;  // same address in every lane: broadcasts
        const float *xvp = XV + vrow * kHdRS + vcol + 3;
        const hx3_bf8 *XB = reinterpret_cast<const hx3_bf8 *>(XS), *WB = reinterpret_cast<const hx3_bf8 *>(WS);

        // Step st = (tap t, M-block m, row half nh).  The fragments and VALU operands of step
        // st + 1 are read while the MFMAs of step st issue (fragment slots by parity of their own
        // fetch counts); scheduling barriers keep the reads from sinking next to their use.  The
        // VALU sums are the f32 kernel's 72 steps (channel pair, tap) in its order, NV / NS of them
        // per MFMA step, taken at the head of the step from the operands read one step earlier.
        hx3_bf8 af[2][2], bf[2][2][2];  // [slot][part], [slot][row][part]
        float xq[VG][2], wq[VG][2];  // one slot: a step's sums are taken before the next step's operands are read
        auto fetch = [&](const int st) __attribute__((always_inline)) {
            const int t = st / (MB * NH), rem = st % (MB * NH), m = rem / NH, nh = rem % NH;
            const int dy = t / 3, dx = t % 3;
            if (nh == 0) {
#pragma unroll
                for (int p = 0; p < 2; ++p) af[(st / NH) & 1][p] = WB[hx3_a_cell(MB, t, m, p, lane)];
            }
            if (NH == 2) {
#pragma unroll
                for (int p = 0; p < 2; ++p) bf[st & 1][0][p] = XB[hx3_b_cell(p, h, 2 * wv + nh, dy, l32, dx)];
            } else if (m == 0) {
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int p = 0; p < 2; ++p) bf[(st / MB) & 1][n][p] = XB[hx3_b_cell(p, h, 2 * wv + n, dy, l32, dx)];
            }
#pragma unroll
            for (int q = 0; q < VG; ++q) {
                const int j = NV * st / NS + q;
                if (j < NV * (st + 1) / NS) {
                    const int cp = j / 9, tt = j % 9;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        xq[q][e] = xvp[(2 * cp + e) * kHdCS + (tt / 3) * kHdRS + tt % 3];
                        wq[q][e] = wvp[(2 * cp + e) * 9 + tt];
                    }
                }
            }
        };
        float sacc[2] = {0.f, 0.f};
        fetch(0);
#pragma unroll
        for (int st = 0; st < NS; ++st) {
#pragma unroll
            for (int q = 0; q < VG; ++q) {
                if (NV * st / NS + q < NV * (st + 1) / NS) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) sacc[e] = fmaf(xq[q][e], wq[q][e], sacc[e]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (st + 1 < NS) fetch(st + 1);
            __builtin_amdgcn_sched_barrier(0);
            const int rem = st % (MB * NH), m = rem / NH, nh = rem % NH;
            const int sa = (st / NH) & 1;
#pragma unroll
            for (int n = 0; n < 2 / NH; ++n) {
                const int row = NH == 2 ? nh : n;
                const hx3_bf8 bh = NH == 2 ? bf[st & 1][0][0] : bf[(st / MB) & 1][n][0];
                const hx3_bf8 bl = NH == 2 ? bf[st & 1][0][1] : bf[(st / MB) & 1][n][1];
                acc[m][row] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[sa][0], bh, acc[m][row], 0, 0, 0);
                acc[m][row] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[sa][0], bl, acc[m][row], 0, 0, 0);
                acc[m][row] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[sa][1], bh, acc[m][row], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const float svr = sacc[0] + sacc[1];
        sv_id += s == 0 ? svr : 0.f;
        sv_cf += s == 1 ? svr : 0.f;
    }

    // epilogue: the VALU sums by pixel, then the f32 kernel's epilogues on the accumulators
    SV[tid] = sv_id;
    SV[kHdNT + tid] = sv_cf;
    __syncthreads();
    const int x = x0 + l32;
    float bv[MB][16];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) bv[m][r] = a.bias[32 * m + (r & 3) + 8 * (r >> 2) + 4 * h];
    if constexpr (PRO) {
        static_assert(MB == 1, "3x3 / K = 8 only");
        heads_epilogue_prologue(a, acc[0], bv[0], SV, b, y0, x, wv, h, l32);
    } else {
        headsx3_epilogue_plain<MB>(a, acc, bv, SV, b, y0, x, wv, h, l32);
    }
}

// Packs the three convs' weights for headsx3_kernel: wm as bf16 fragments (one thread per
// element: hx3_w_elem names its source channel, tap, column and part; the value is the f32
// pack's, split), then wv and bias exactly as heads_pack_kernel writes them.  HeadsPackArgs::wm
// points at the bf16 array.  Defined in nlspn_kern_heads_x3.hip.
__global__ void headsx3_pack_kernel(HeadsPackArgs a);

#define NLSPN_HDX3_BUILDS(X)                                                                         \
    X(1, true, false) X(1, false, false) X(2, true, false) X(2, false, false) X(3, true, false)      \
    X(3, false, false) X(5, true, false) X(5, false, false) X(1, true, true) X(1, false, true)
#define NLSPN_HDX3_SPEC(LINKAGE, MB, VEC, PRO) LINKAGE template __global__ void headsx3_kernel<MB, VEC, PRO>(HeadsArgs);
#define NLSPN_HDX3_INST(...) NLSPN_HDX3_SPEC(, __VA_ARGS__)
#define NLSPN_HDX3_EXTERN(...) NLSPN_HDX3_SPEC(extern, __VA_ARGS__)

}  // namespace nlspn
