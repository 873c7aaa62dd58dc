// C ABI of the backward (see include/nlspn_prop.h): the section's backward (resident pass 1
// or the step launches, the coefficient pass, the final kernel), the single step's backward
// and the affinity normalisation's.  The backward kernels are instantiated here.
#include "nlspn_host.h"
#include "nlspn_backward.h"
#include "nlspn_bwd_resident.h"

using namespace nlspn;

namespace {

struct BwdLaunch {
    const void *fn = nullptr;
    dim3 grid, block;
};

constexpr int kBwdTH = 8, kBwdTW = 32;  // backward step tile (every geometry)
constexpr int kBwdCoefTH = 16, kBwdCoefTW = 16;  // pass 2's tile: at most 2 x bwd_tiles() of them

long long bwd_tiles(int B, int H, int W) {
    return (long long)B * ((H + kBwdTH - 1) / kBwdTH) * ((W + kBwdTW - 1) / kBwdTW);
}

template <typename S, int KH, int KW, int TH, int TW, int RY, int RX, int SV, bool OFFSET, bool SPLIT = false>
BwdLaunch make_bwd(BwdArgsT<S> &a, bool first) {
    static_assert(TH == kBwdTH && TW == kBwdTW, "bwd_tiles() sizes the dL/dgamma partials");
    BwdLaunch L;
    L.fn = first ? reinterpret_cast<const void *>(&bwd_step_kernel<S, KH, KW, TH, TW, RY, RX, SV, OFFSET, true, 0, SPLIT>)
                 : reinterpret_cast<const void *>(&bwd_step_kernel<S, KH, KW, TH, TW, RY, RX, SV, OFFSET, false, 0, SPLIT>);
    a.tiles_x = (a.W + TW - 1) / TW;
    a.tiles_y = (a.H + TH - 1) / TH;
    L.grid = dim3((unsigned)(a.B * a.tiles_x * a.tiles_y));
    L.block = dim3(TH * TW);
    return L;
}

template <typename S>
int select_bwd(BwdArgsT<S> &a, int kh, int kw, bool offset, bool vec, bool first, BwdLaunch &L, bool split = false) {
    if (split) {  // two-pass form: 3x3 with offsets only (bwd_split_ok)
        // (8 x 32 tiles: 16 x 64 ones, halving the scatter halo's float atomics, measured
        // 41.6 vs 31.6 us per iteration on NYU, profiles/r04/ab_bwd_tile_r4h.txt)
        L = vec ? make_bwd<S, 3, 3, 8, 32, 8, 8, 4, true, true>(a, first) : make_bwd<S, 3, 3, 8, 32, 8, 8, 1, true, true>(a, first);
        return NLSPN_OK;
    }
    if (!offset) {
        if (kh != 3 || kw != 3)
            return fail(NLSPN_EUNSUPPORTED, "no-offset propagation is 3x3 replicate (nlspnmodel.py:209-224)");
        L = make_bwd<S, 3, 3, 8, 32, 1, 1, 1, false>(a, first);
        return NLSPN_OK;
    }
    if (kh == 3 && kw == 3)
        L = vec ? make_bwd<S, 3, 3, 8, 32, 8, 8, 4, true>(a, first) : make_bwd<S, 3, 3, 8, 32, 8, 8, 1, true>(a, first);
    else if (kh == 1 && kw == 17)
        L = vec ? make_bwd<S, 1, 17, 8, 32, 8, 16, 4, true>(a, first) : make_bwd<S, 1, 17, 8, 32, 8, 16, 1, true>(a, first);
    else if (kh == 5 && kw == 5)
        L = vec ? make_bwd<S, 5, 5, 8, 32, 8, 8, 4, true>(a, first) : make_bwd<S, 5, 5, 8, 32, 8, 8, 1, true>(a, first);
    else
        return fail(NLSPN_EUNSUPPORTED, "no backward instantiation for a %dx%d geometry (supported: 3x3, 5x5, 1x17)",
                    kh, kw);
    return NLSPN_OK;
}

// The backward workspace, in floats: the two dL/df planes, then (from a 128-B line) the
// resident pass 1's sync words — contiguous, so one memset clears both — then G = dL/daff -
// dL/daff_ref (K planes), dL/dconf' and the dL/dgamma partials (two per 8x32 tile).  Half
// storage adds `planes` float planes of N behind them: the two-pass form's dL/dout store (T
// planes per item) or the one-pass form's dL/doffset accumulators (2K planes per item).
struct BwdWorkspace {
    size_t gf1, sync, g_aff, g_conf, gpart, extra, total;
    BwdWorkspace(int B, int H, int W, int K, int planes = 0) {
        const size_t N = (size_t)B * H * W;
        gf1 = N;
        sync = (N * 2 + kBrLine - 1) / kBrLine * kBrLine;
        g_aff = sync + kBrSyncWords;
        g_conf = g_aff + (size_t)K * N;
        gpart = g_conf + N;
        extra = gpart + 2 * (size_t)bwd_tiles(B, H, W);
        total = extra + (size_t)planes * N;
    }
};

// The two-pass form's geometry rule (the caller adds: offsets given, NLSPN_BWD_ONEPASS unset).
bool bwd_split_geometry(int kh, int kw, int T) { return kh == 3 && kw == 3 && T <= 3 * (kh * kw - 1); }

// Float planes of N that half storage adds to the workspace: enough for either form the call
// may take (which one depends on the offsets' presence and the environment, not on the sizes).
int bwd_f16_planes(int kh, int kw, int T) {
    const int K = kh * kw - 1;
    return bwd_split_geometry(kh, kw, T) && T > 2 * K ? T : 2 * K;
}

// nlspn_propagate_backward's arguments as its phases see them.
template <typename S>
struct BwdCall {
    BwdCoefArgsT<S> k;  // the call's inputs, strides resolved: every phase reads them, pass 2 launches with them
    const S *grad_pred, *grad_pred_inter;
    S *grad_pred_init, *grad_conf;
    float *grad_gamma;
    float *acc_off;  // the one-pass form's dL/doffset accumulators (float storage: grad_off_raw itself)
    long long grad_aff_bs, grad_off_bs;  // as given (0: contiguous)
    int kh, kw;
    bool vec;    // 16-B loads
    bool split;  // the two-pass form
    float *ws, *gf[2], *g_aff, *g_conf, *gpart;  // the workspace (BwdWorkspace)
    unsigned *sync;
    size_t clear_words;  // both dL/df planes and the sync words
    hipStream_t s;
};

// Resident pass 1 (nlspn_bwd_resident.h): the whole batch in one launch (bp.Bl == B).
template <typename S>
int bwd_resident_pass1(const BwdCall<S> &c, const BrPlan &bp, unsigned dbg) {
    const BwdCoefArgsT<S> &k = c.k;
    const void *fn = reinterpret_cast<const void *>(&bwd_res_kernel<S, kBrPX>);
    const int WH = bp.PR + 2 * kBrR, WW = bp.PC + 2 * kBrR;
    const int lds = ((WH * WW + 1) & ~1) * 8 + bp.PR * bp.PC * 32;  // window + the part's affinities
    NLSPN_TRY(set_lds_attr(fn, lds));
    int occ = 0;
    NLSPN_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, kBrNT, lds));
    if (occ < 1) return fail(NLSPN_EUNSUPPORTED, "resident backward: no room for a %d-thread part", kBrNT);
    DevState *d = dev_state();
    BwdResArgsT<S> r{k.pred_inter, k.conf ? k.conf_eff : nullptr, (k.flags & NLSPN_PRESERVE_INPUT) ? k.dep : nullptr, k.aff,
                 k.off, c.grad_pred, c.grad_pred_inter, c.gf[0], k.conf ? c.g_conf : nullptr, k.go_a, k.go_b, k.go_na,
                 k.go_a_bs, k.go_b_bs, k.off_bs, k.N, c.sync, d ? d->dev_status : nullptr, k.H, k.W, k.T,
                 bp.py, bp.px, bp.PR, bp.PC, WH, WW, k.flags, dbg};
    const unsigned grid = (unsigned)(k.B * bp.py * bp.px);
    if (grid > (unsigned)device_cus() * (unsigned)occ) return fail(NLSPN_EUNSUPPORTED, "resident backward grid too large");
    // both dL/df planes and the sync words in one memset
    NLSPN_HIP_TRY(hipMemsetAsync(c.ws, 0, sizeof(float) * c.clear_words, c.s));
    NLSPN_TRY(res_guard_before(c.s));
    void *args[] = {&r};
    NLSPN_TRY(launch_kernel(fn, dim3(grid), dim3(kBrNT), args, (size_t)lds, c.s, "nlspn_propagate_backward resident pass 1"));
    return res_guard_after(c.s);
}

// Iterations T..1 as step launches.
template <typename S>
int bwd_step_loop(const BwdCall<S> &c) {
    const BwdCoefArgsT<S> &k = c.k;
    const long long N = k.N, HW = (long long)k.H * k.W;
    // the accumulators are initialised by step T; only its scatter target needs clearing
    NLSPN_HIP_TRY(hipMemsetAsync(c.gf[(k.T - 1) & 1], 0, sizeof(float) * N, c.s));
    for (int t = k.T; t >= 1; --t) {
        const bool first = t == 1;
        const S *ce = k.conf ? k.conf_eff : nullptr;  // conf' (step 1 reads the raw conf)
        BwdArgsT<S> a{first ? k.pred_init : k.pred_inter + (size_t)(t - 2) * N, k.pred_inter + (size_t)(t - 1) * N,
                  first ? k.conf : ce, ce, k.dep, k.aff, k.off, c.grad_pred,
                  c.grad_pred_inter ? c.grad_pred_inter + (size_t)(t - 1) * N : nullptr, c.gf[t & 1], c.gf[(t - 1) & 1],
                  c.g_aff, c.acc_off, k.conf ? c.g_conf : nullptr, k.off_bs, k.B, k.H, k.W, 0, 0, t == k.T, 0, k.flags};
        a.goff_bs = sizeof(S) == 4 ? c.grad_off_bs : 0;  // of the accumulators
        a.gaff_bs = c.grad_aff_bs;
        a.grad_off_raw = k.g_off;
        a.groff_bs = c.grad_off_bs;
        if (first) {
            a.aff_raw = k.aff_raw;
            a.aff_raw_bs = k.aff_raw_bs;
            a.gamma = k.gamma;
            a.grad_aff_raw = k.grad_aff_raw;
            a.gamma_part = k.gamma_part;
            a.kind = k.kind;
        }
        if (c.split) {
            const int j = t - 1;  // dL/dout_t -> plane j of the dL/dout store
            a.go_out = j < k.go_na ? k.go_a + (size_t)j * HW : k.go_b + (size_t)(j - k.go_na) * HW;
            a.go_bs = j < k.go_na ? k.go_a_bs : k.go_b_bs;
        }
        BwdLaunch L;
        NLSPN_TRY(select_bwd(a, c.kh, c.kw, k.off != nullptr, c.vec, first, L, c.split));
        void *args[] = {&a};
        NLSPN_TRY(launch_kernel(L.fn, L.grid, L.block, args, 0, c.s, "nlspn_propagate_backward step"));
    }
    return NLSPN_OK;
}

// Pass 2 of the two-pass form: dL/daff and dL/doffset from the dL/dout planes.  *np: the
// dL/dgamma partials it leaves (<= 2 x bwd_tiles(): the partials' room).
template <typename S>
int bwd_coef_pass(const BwdCall<S> &c, int *np) {
    BwdCoefArgsT<S> k = c.k;
    // 16 x 16 tiles: C2 0.4519 vs 0.4631 ms per backward against 8 x 32 (KITTI 0.941 vs 0.946;
    // 16 x 32, 8 x 64, 4 x 64 and 4 x 32 slower or equal, profiles/r06/ab_bwd_coef_tile_*.json)
    constexpr int cth = kBwdCoefTH, ctw = kBwdCoefTW;
    const void *fn = c.vec ? reinterpret_cast<const void *>(&bwd_coef_kernel<S, 3, 3, cth, ctw, 8, 8, 4>)
                           : reinterpret_cast<const void *>(&bwd_coef_kernel<S, 3, 3, cth, ctw, 8, 8, 1>);
    k.tiles_x = (k.W + ctw - 1) / ctw;
    k.tiles_y = (k.H + cth - 1) / cth;
    *np = k.B * k.tiles_x * k.tiles_y;
    void *args[] = {&k};
    return launch_kernel(fn, dim3((unsigned)*np), dim3(cth * ctw), args, 0, c.s, "nlspn_propagate_backward coefficients");
}

// The final kernel: grad_pred_init, grad_conf and the sum of np dL/dgamma partials.
template <typename S>
int bwd_final(const BwdCall<S> &c, int np) {
    const BwdCoefArgsT<S> &k = c.k;
    const float *gf0 = c.gf[0], *cg_conf = c.g_conf, *cgpart = c.gpart;
    float *gg = k.gamma_part ? c.grad_gamma : nullptr;
    if (c.grad_gamma && !gg) NLSPN_HIP_TRY(hipMemsetAsync(c.grad_gamma, 0, sizeof(float), c.s));
    long long n = k.N;
    unsigned fl = k.flags;
    void *args[] = {(void *)&k.pred_init, (void *)&k.dep, (void *)&k.conf, (void *)&k.conf_eff, &gf0, &cg_conf,
                    (void *)&c.grad_pred_init, (void *)&c.grad_conf, &n, &fl, &cgpart, &np, &gg};
    return launch_kernel(reinterpret_cast<const void *>(&bwd_final_kernel<S>), dim3(elementwise_grid(k.N)), dim3(256), args,
                         0, c.s, "nlspn_propagate_backward final");
}

int check_bwd_dtype(int dtype) {
    return dtype == NLSPN_DTYPE_F32 || dtype == NLSPN_DTYPE_F16
               ? NLSPN_OK : fail(NLSPN_EUNSUPPORTED, "the backward: float32 or float16 storage (dtype %d)", dtype);
}

// Half storage: the float planes one batch item spans in the workspace stay below 2 GiB too
// (one buffer descriptor per item, like the storage-typed planes check_item_bytes bounds).
int check_item_float_planes(long long HW, int planes) {
    return HW * planes * 4LL > 0x7fffffffLL
               ? fail(NLSPN_EINVAL, "image too large: one batch item's planes must stay below 2 GiB") : NLSPN_OK;
}

// nlspn_propagate_backward after the argument checks, for storage type S.
template <typename S>
int propagate_backward_run(const void *pred_init, const void *dep, const void *conf, const void *aff_raw,
                           int64_t aff_bstride, const void *off_raw, int64_t off_bstride, const float *gamma,
                           const void *pred_inter, const void *aff_norm, const void *conf_eff, const void *grad_pred,
                           const void *grad_pred_inter, void *grad_pred_init, void *grad_conf, void *grad_aff_raw,
                           int64_t grad_aff_bstride, void *grad_off_raw, int64_t grad_off_bstride, float *grad_gamma,
                           void *workspace, int B, int H, int W, int kh, int kw, int T, int kind, unsigned flags,
                           void *stream) {
    constexpr bool F32 = sizeof(S) == 4;
    const int K = kh * kw - 1;
    const long long HW = (long long)H * W, N = (long long)B * HW;
    NLSPN_TRY(check_item_bytes(HW, K, sizeof(S)));
    if (!F32) NLSPN_TRY(check_item_float_planes(HW, bwd_f16_planes(kh, kw, T)));
    {
        BwdArgsT<S> probe{};
        probe.B = B; probe.H = H; probe.W = W;
        BwdLaunch L;
        NLSPN_TRY(select_bwd(probe, kh, kw, off_raw != nullptr, false, true, L));
    }
    const auto f = [](const void *p) { return static_cast<const S *>(p); };
    const auto g = [](void *p) { return static_cast<S *>(p); };
    const BwdWorkspace lay(B, H, W, K);
    float *ws = static_cast<float *>(workspace);
    BwdCall<S> c{};
    c.ws = c.gf[0] = ws;
    c.gf[1] = ws + lay.gf1;
    c.sync = reinterpret_cast<unsigned *>(ws) + lay.sync;
    c.g_aff = ws + lay.g_aff;
    c.g_conf = ws + lay.g_conf;
    c.gpart = ws + lay.gpart;
    c.clear_words = lay.g_aff;
    const long long goff_bs = grad_off_bstride ? grad_off_bstride : 2LL * K * HW;
    const long long gaff_bs = grad_aff_bstride ? grad_aff_bstride : (long long)K * HW;
    c.k = BwdCoefArgsT<S>{f(pred_init), f(pred_inter), f(conf), f(conf_eff), f(dep), f(aff_norm), f(off_raw), f(aff_raw),
                          gamma, g(grad_off_raw), g(grad_aff_raw),
                          (grad_gamma && kind == NLSPN_AFF_TGASS) ? c.gpart : nullptr, off_bstride, aff_bstride, goff_bs,
                          gaff_bs, N, B, H, W, 0, 0, T, kind, flags, nullptr, nullptr, 0, 0, 0};
    if constexpr (F32) {
        // float storage: the gradient outputs hold dL/dout between the passes and are the
        // one-pass form's accumulators
        c.k.go_a = c.k.g_off; c.k.go_a_bs = goff_bs; c.k.go_na = 2 * K;
        c.k.go_b = c.k.grad_aff_raw; c.k.go_b_bs = gaff_bs;
        c.acc_off = c.k.g_off;
    } else {
        // half storage: T float planes per item (two-pass) or 2K (one-pass) behind the partials
        c.k.go_a = c.k.go_b = ws + lay.extra; c.k.go_a_bs = c.k.go_b_bs = (long long)T * HW; c.k.go_na = T;
        c.acc_off = ws + lay.extra;
    }
    c.grad_pred = f(grad_pred); c.grad_pred_inter = f(grad_pred_inter);
    c.grad_pred_init = g(grad_pred_init); c.grad_conf = g(grad_conf); c.grad_gamma = grad_gamma;
    c.grad_aff_bs = grad_aff_bstride; c.grad_off_bs = grad_off_bstride;
    c.kh = kh; c.kw = kw;
    // 4-element loads: 16 B of floats, 8 B of halves
    constexpr size_t va = 4 * sizeof(S);
    c.vec = (W % 4 == 0) && aligned(pred_init, va) && aligned(pred_inter, va) && aligned(conf, va) &&
            aligned(conf_eff, va) && aligned(dep, va);
    // Two-pass form (3x3 with offsets, T <= 3K): the steps write dL/dout into the dL/dout store
    // and bwd_coef_kernel computes dL/daff, dL/doffset afterwards (see nlspn_backward.h).
    // NLSPN_BWD_ONEPASS=1 keeps the one-pass form (A/B only).  No form depends on the storage type.
    c.split = !env_is("NLSPN_BWD_ONEPASS", '1') && off_raw && bwd_split_geometry(kh, kw, T);
    c.s = as_stream(stream);
    // Resident pass 1 (nlspn_bwd_resident.h): the two-pass form without the clamp's mask,
    // T >= 2, when every part of an image group fits on the device at once.
    // Only when the whole batch fits one launch: with image groups in turn (KITTI B=4: two
    // launches of two images) each group pays the setup and its own T-iteration chain, and the
    // step launches measured faster (0.855 vs 0.938 ms per backward, profiles/r06/
    // ab_bwd_two_parts_per_cu_kitti_rejected.json "steps" vs "nt1024").
    // (NLSPN_BWD_RESIDENT=0, experiments build: the step launches, A/B)
    BrPlan bp;
    const bool resident = c.split && !(flags & NLSPN_ALWAYS_CLIP) && T >= 2 &&
                          !(kExperiments && env_is("NLSPN_BWD_RESIDENT", '0')) &&
                          br_plan(B, H, W, device_cus(), bp) && bp.Bl >= B;
    NLSPN_TRY(resident ? bwd_resident_pass1(c, bp, env_dbg("NLSPN_BWD_RES_DBG", 0)) : bwd_step_loop(c));
    int np = (int)bwd_tiles(B, H, W);
    if (c.split) NLSPN_TRY(bwd_coef_pass(c, &np));
    return bwd_final(c, np);
}

// nlspn_prop_step_backward after the argument checks, for storage type S.  Half storage: the
// step writes its affinity, offset and confidence gradients as float planes of the workspace
// (behind the two dL/df planes: dL/dconf scratch, (K+1) affinity planes, 2K offset planes per
// item) and the finishing kernel rounds them once into the outputs.
template <typename S>
int prop_step_backward_run(const void *feat, const void *conf, const void *dep, const void *aff, const void *off_raw,
                           int64_t off_bstride, const void *grad_out, void *grad_feat, void *grad_conf, void *grad_aff,
                           void *grad_off, void *workspace, int B, int H, int W, int kh, int kw, unsigned flags,
                           void *stream) {
    constexpr bool F32 = sizeof(S) == 4;
    const int K = kh * kw - 1;
    const long long HW = (long long)H * W, N = (long long)B * HW;
    NLSPN_TRY(check_item_bytes(HW, K, sizeof(S)));
    if (!F32) NLSPN_TRY(check_item_float_planes(HW, 2 * K));
    hipStream_t s = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    float *acc_conf = ws + 2 * N, *acc_aff = acc_conf + N, *acc_off = acc_aff + (size_t)(K + 1) * N;  // half storage
    BwdArgsT<S> a{};
    a.p_in = static_cast<const S *>(feat);
    a.p_out = a.p_in;  // read only for terms that vanish at a single step (no incoming dL/df)
    a.conf = static_cast<const S *>(conf);
    a.conf_eff = a.conf;
    a.dep = static_cast<const S *>(dep);
    a.aff = static_cast<const S *>(aff);
    a.off = static_cast<const S *>(off_raw);
    a.g_inter = static_cast<const S *>(grad_out);
    a.gf_write = ws;
    a.gf_read = ws + N;
    a.g_aff_ins = 1;
    if constexpr (F32) {
        a.g_aff = static_cast<float *>(grad_aff);
        a.g_off = static_cast<float *>(grad_off);
        a.g_conf = conf ? static_cast<float *>(grad_conf) : nullptr;
    } else {
        a.g_aff = acc_aff;
        a.g_off = off_raw ? acc_off : nullptr;
        a.g_conf = conf ? acc_conf : nullptr;
    }
    a.off_bs = off_bstride;
    a.B = B; a.H = H; a.W = W;
    a.last = 1;
    a.flags = flags;
    constexpr size_t va = 4 * sizeof(S);
    const bool vec = (W % 4 == 0) && aligned(feat, va) && aligned(conf, va) && aligned(dep, va);
    BwdLaunch L;
    NLSPN_TRY(select_bwd(a, kh, kw, off_raw != nullptr, vec, false, L));
    NLSPN_HIP_TRY(hipMemsetAsync(ws, 0, sizeof(float) * N, s));
    void *args[] = {&a};
    NLSPN_TRY(launch_kernel(L.fn, L.grid, L.block, args, 0, s, "nlspn_prop_step_backward step"));
    const S *pf = a.p_in, *pc = a.conf;
    const float *gf = ws, *ca = F32 ? nullptr : acc_aff, *co = (F32 || !off_raw) ? nullptr : acc_off;
    S *gfe = static_cast<S *>(grad_feat), *gc = static_cast<S *>(grad_conf), *ga = static_cast<S *>(grad_aff),
      *go = static_cast<S *>(grad_off);
    long long hw = HW;
    int b_ = B, k_ = K;
    void *iargs[] = {&pf, &pc, &gf, &gfe, &gc, &ga, &hw, &b_, &k_, &ca, &co, &go};
    return launch_kernel(reinterpret_cast<const void *>(&bwd_step_io_kernel<S>), dim3(elementwise_grid(N)), dim3(256),
                         iargs, 0, s, "nlspn_prop_step_backward io");
}

template <typename S>
int affnorm_backward_run(const void *aff_raw, int64_t aff_bstride, const float *gamma, const void *grad_aff,
                         void *grad_aff_raw, float *grad_gamma, void *workspace, int B, int K, int H, int W, int kind,
                         void *stream) {
    const long long HW = (long long)H * W, N = (long long)B * HW;
    const void *fn = nullptr;
    switch (K) {
        case 8: fn = reinterpret_cast<const void *>(&affnorm_bwd_kernel<S, 8>); break;
        case 16: fn = reinterpret_cast<const void *>(&affnorm_bwd_kernel<S, 16>); break;
        case 24: fn = reinterpret_cast<const void *>(&affnorm_bwd_kernel<S, 24>); break;
        case 48: fn = reinterpret_cast<const void *>(&affnorm_bwd_kernel<S, 48>); break;
        default: return fail(NLSPN_EUNSUPPORTED, "no affinity-normalisation backward for K=%d (8, 16, 24, 48)", K);
    }
    hipStream_t s = as_stream(stream);
    const unsigned grid = elementwise_grid(N);
    float *part = (grad_gamma && kind == NLSPN_AFF_TGASS) ? static_cast<float *>(workspace) : nullptr;
    if (grad_gamma && !part) NLSPN_HIP_TRY(hipMemsetAsync(grad_gamma, 0, sizeof(float), s));
    const S *ar = static_cast<const S *>(aff_raw), *gin = static_cast<const S *>(grad_aff);
    S *gout = static_cast<S *>(grad_aff_raw);
    long long abs_ = aff_bstride, hw = HW;
    int b_ = B, k_ = kind;
    void *args[] = {&ar, &abs_, (void *)&gamma, &gin, &gout, &part, &hw, &b_, &k_};
    NLSPN_TRY(launch_kernel(fn, dim3(grid), dim3(256), args, 0, s, "nlspn_affinity_normalize_backward"));
    if (!part) return NLSPN_OK;
    const float *cp = part;
    int n = (int)grid;
    void *rargs[] = {&cp, &n, &grad_gamma};
    return launch_kernel(reinterpret_cast<const void *>(&sum_partials_kernel), dim3(1), dim3(256), rargs, 0, s,
                         "nlspn_affinity_normalize_backward gamma");
}

}  // namespace

extern "C" {

size_t nlspn_backward_workspace_bytes(int B, int H, int W, int kh, int kw) {
    if (B < 1 || H < 1 || W < 1 || kh < 1 || kw < 1) return 0;
    return sizeof(float) * BwdWorkspace(B, H, W, kh * kw - 1).total;
}

size_t nlspn_backward_workspace_bytes_dtype(int dtype, int B, int H, int W, int kh, int kw, int T) {
    if (B < 1 || H < 1 || W < 1 || kh < 1 || kw < 1 || kh * kw < 2 || T < 1) return 0;
    if (dtype == NLSPN_DTYPE_F32) return nlspn_backward_workspace_bytes(B, H, W, kh, kw);
    if (dtype != NLSPN_DTYPE_F16) return 0;
    return sizeof(float) * BwdWorkspace(B, H, W, kh * kw - 1, bwd_f16_planes(kh, kw, T)).total;
}

int nlspn_propagate_backward(int dtype, const void *pred_init, const void *dep, const void *conf,
                             const void *aff_raw, int64_t aff_bstride, const void *off_raw, int64_t off_bstride,
                             const float *gamma, const void *pred_inter, const void *aff_norm, const void *conf_eff,
                             const void *grad_pred, const void *grad_pred_inter, void *grad_pred_init,
                             void *grad_conf, void *grad_aff_raw, int64_t grad_aff_bstride, void *grad_off_raw,
                             int64_t grad_off_bstride, float *grad_gamma, void *workspace, int B, int H, int W,
                             int kh, int kw, int T, int kind, unsigned flags, void *stream) {
    NLSPN_TRY(check_bwd_dtype(dtype));
    NLSPN_TRY(check_nonempty(B, H, W));
    NLSPN_TRY(check_prop_time(T));
    NLSPN_TRY(check_kind(kind));
    NLSPN_TRY(check_odd_kernel(kh, kw));
    if (!pred_init || !aff_raw || !gamma || !pred_inter || !aff_norm || !grad_pred_init || !grad_aff_raw || !workspace)
        return fail(NLSPN_EINVAL, "null required pointer");
    NLSPN_TRY(check_preserve(flags, dep));
    if (conf && (!conf_eff || !grad_conf)) return fail(NLSPN_EINVAL, "conf given without conf_eff / grad_conf");
    if (off_raw && !grad_off_raw) return fail(NLSPN_EINVAL, "off_raw given without grad_off_raw");
    const int K = kh * kw - 1;
    const long long HW = (long long)H * W;
    NLSPN_TRY(check_batch_stride("aff", aff_bstride, K, HW));
    if (off_raw) NLSPN_TRY(check_batch_stride("offset", off_bstride, 2 * K, HW));
    if (grad_aff_bstride < 0 || grad_off_bstride < 0 || (grad_aff_bstride && grad_aff_bstride < (long long)K * HW) ||
        (grad_off_bstride && grad_off_bstride < 2LL * K * HW))
        return fail(NLSPN_EINVAL, "gradient batch strides below K*H*W / 2K*H*W (0 = contiguous)");
    // (no alignment requirement: every grad_aff_raw / grad_off_raw access is a
    // one-element buffer load/store, nlspn_backward.h)
    if (dtype == NLSPN_DTYPE_F16)
        return propagate_backward_run<__half>(pred_init, dep, conf, aff_raw, aff_bstride, off_raw, off_bstride, gamma,
                                              pred_inter, aff_norm, conf_eff, grad_pred, grad_pred_inter, grad_pred_init,
                                              grad_conf, grad_aff_raw, grad_aff_bstride, grad_off_raw, grad_off_bstride,
                                              grad_gamma, workspace, B, H, W, kh, kw, T, kind, flags, stream);
    return propagate_backward_run<float>(pred_init, dep, conf, aff_raw, aff_bstride, off_raw, off_bstride, gamma,
                                         pred_inter, aff_norm, conf_eff, grad_pred, grad_pred_inter, grad_pred_init,
                                         grad_conf, grad_aff_raw, grad_aff_bstride, grad_off_raw, grad_off_bstride,
                                         grad_gamma, workspace, B, H, W, kh, kw, T, kind, flags, stream);
}

size_t nlspn_prop_step_backward_workspace_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return sizeof(float) * 2 * (size_t)B * H * W;  // dL/df, plus a scratch plane
}

size_t nlspn_prop_step_backward_workspace_bytes_dtype(int dtype, int B, int H, int W, int kh, int kw) {
    if (B < 1 || H < 1 || W < 1 || kh < 1 || kw < 1 || kh * kw < 2) return 0;
    if (dtype == NLSPN_DTYPE_F32) return nlspn_prop_step_backward_workspace_bytes(B, H, W);
    if (dtype != NLSPN_DTYPE_F16) return 0;
    // + the float dL/dconf scratch, (K+1) affinity and 2K offset gradient planes
    return sizeof(float) * (size_t)(3 * (kh * kw - 1) + 4) * B * H * W;
}

int nlspn_prop_step_backward(int dtype, const void *feat, const void *conf, const void *dep, const void *aff,
                             int64_t aff_bstride, const void *off_raw, int64_t off_bstride, const void *grad_out,
                             void *grad_feat, void *grad_conf, void *grad_aff, void *grad_off, void *workspace, int B,
                             int H, int W, int kh, int kw, unsigned flags, void *stream) {
    NLSPN_TRY(check_bwd_dtype(dtype));
    NLSPN_TRY(check_nonempty(B, H, W));
    NLSPN_TRY(check_odd_kernel(kh, kw));
    if (!feat || !aff || !grad_out || !grad_feat || !grad_aff || !workspace)
        return fail(NLSPN_EINVAL, "null required pointer");
    NLSPN_TRY(check_preserve(flags, dep));
    if (conf && !grad_conf) return fail(NLSPN_EINVAL, "conf given without grad_conf");
    if (off_raw && !grad_off) return fail(NLSPN_EINVAL, "off_raw given without grad_off");
    const int K = kh * kw - 1;
    const long long HW = (long long)H * W;
    NLSPN_TRY(check_batch_stride("aff", aff_bstride, K + 1, HW));
    if (off_raw) NLSPN_TRY(check_batch_stride("offset", off_bstride, 2 * K, HW));
    if (dtype == NLSPN_DTYPE_F16)
        return prop_step_backward_run<__half>(feat, conf, dep, aff, off_raw, off_bstride, grad_out, grad_feat, grad_conf,
                                              grad_aff, grad_off, workspace, B, H, W, kh, kw, flags, stream);
    return prop_step_backward_run<float>(feat, conf, dep, aff, off_raw, off_bstride, grad_out, grad_feat, grad_conf,
                                         grad_aff, grad_off, workspace, B, H, W, kh, kw, flags, stream);
}

size_t nlspn_affinity_normalize_backward_workspace_bytes(int B, int K, int H, int W) {
    if (B < 1 || K < 1 || H < 1 || W < 1) return 0;
    return sizeof(float) * elementwise_grid((long long)B * H * W);  // dL/dgamma partials
}

int nlspn_affinity_normalize_backward(int dtype, const void *aff_raw, int64_t aff_bstride, const float *gamma,
                                      const void *grad_aff, void *grad_aff_raw, float *grad_gamma, void *workspace,
                                      int B, int K, int H, int W, int kind, void *stream) {
    NLSPN_TRY(check_bwd_dtype(dtype));
    NLSPN_TRY(check_nonempty(B, H, W));
    NLSPN_TRY(check_kind(kind));
    if (!aff_raw || !gamma || !grad_aff || !grad_aff_raw || !workspace) return fail(NLSPN_EINVAL, "null required pointer");
    NLSPN_TRY(check_batch_stride("aff", aff_bstride, K, (long long)H * W));
    if (dtype == NLSPN_DTYPE_F16)
        return affnorm_backward_run<__half>(aff_raw, aff_bstride, gamma, grad_aff, grad_aff_raw, grad_gamma, workspace, B,
                                            K, H, W, kind, stream);
    return affnorm_backward_run<float>(aff_raw, aff_bstride, gamma, grad_aff, grad_aff_raw, grad_gamma, workspace, B, K,
                                       H, W, kind, stream);
}

}  // extern "C"
