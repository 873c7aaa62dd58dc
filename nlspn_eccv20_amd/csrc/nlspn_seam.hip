// C ABI of the seam-2 and head entry points (see include/nlspn_prop.h): the modulated
// deformable convolution forward and backward, the S2D pyramid, the head epilogue and its
// weight packing, and the affinity normalisation's forward.  The DCN, S2D, packing and
// normalisation kernels are instantiated here; the head kernels in nlspn_kern_heads.hip,
// nlspn_kern_heads_x3.hip and (the backward) nlspn_kern_heads_bwd.hip.
#include "nlspn_host.h"
#include "nlspn_affnorm.h"
#include "nlspn_heads.h"
#include "nlspn_heads_x3.h"
#include "nlspn_heads_bwd.h"
#include "nlspn_mdcn.h"
#include "nlspn_s2d.h"

namespace nlspn {
NLSPN_HD_BUILDS(NLSPN_HD_EXTERN)  // defined in nlspn_kern_heads.hip
NLSPN_HDX3_BUILDS(NLSPN_HDX3_EXTERN)  // defined in nlspn_kern_heads_x3.hip
}  // namespace nlspn

using namespace nlspn;

namespace {

// ------------------------------------------------------- affinity-normalisation dispatch
template <typename T, int K>
const void *affnorm_fn(bool vec) {
    return vec ? reinterpret_cast<const void *>(&affnorm_kernel<T, K, 4>)
               : reinterpret_cast<const void *>(&affnorm_kernel<T, K, 1>);
}
template <typename T>
const void *select_affnorm(int K, bool vec) {
    switch (K) {
        case 8: return affnorm_fn<T, 8>(vec);
        case 16: return affnorm_fn<T, 16>(vec);
        case 24: return affnorm_fn<T, 24>(vec);
        case 48: return affnorm_fn<T, 48>(vec);
        default: return nullptr;
    }
}

// ------------------------------------------------------------------------------ DCN
// The argument check shared by the DCN forward and backward; sets the output size.
int check_mdcn(int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
               int group, int deformable_group, int *Ho, int *Wo) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || Cout < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1 ||
        group < 1 || deformable_group < 1 || ph < 0 || pw < 0)
        return fail(NLSPN_EINVAL, "invalid DCN arguments");
    if ((C % group) != 0 || (Cout % group) != 0)
        return fail(NLSPN_EINVAL, "channels(%d) and channels_out(%d) must divide group(%d)", C, Cout, group);
    if ((C % deformable_group) != 0)
        return fail(NLSPN_EINVAL, "channels(%d) must divide deformable_group(%d)", C, deformable_group);
    *Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
    *Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
    if (*Ho < 1 || *Wo < 1) return fail(NLSPN_EINVAL, "output size %dx%d is empty", *Ho, *Wo);
    return NLSPN_OK;
}

// The two DCN backward launches (nlspn_mdcn.h) in arithmetic type A (float or double).
template <typename A>
int mdcn_backward_impl(const void *input, const void *weight, const void *offset, const void *mask,
                       const void *grad_output, void *grad_input, void *grad_offset, void *grad_mask, void *grad_weight,
                       void *grad_bias, int B, int C, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph,
                       int pw, int dh, int dw, int group, int dg, int Ho, int Wo, long long nd, long long nw,
                       hipStream_t s) {
    MdcnBwdArgs<A> a{static_cast<const A *>(input), static_cast<const A *>(weight), static_cast<const A *>(offset),
                     static_cast<const A *>(mask), static_cast<const A *>(grad_output), static_cast<A *>(grad_input),
                     static_cast<A *>(grad_offset), static_cast<A *>(grad_mask), static_cast<A *>(grad_weight),
                     static_cast<A *>(grad_bias), B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group, dg, Ho, Wo};
    NLSPN_HIP_TRY(hipMemsetAsync(grad_input, 0, sizeof(A) * (size_t)B * C * H * W, s));
    void *args[] = {&a};
    NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&mdcn_bwd_data_kernel<A>), dim3(elementwise_grid(nd)), dim3(256),
                            args, 0, s, "nlspn_mdcn_backward data"));
    return launch_kernel(reinterpret_cast<const void *>(&mdcn_bwd_weight_kernel<A>), dim3((unsigned)nw), dim3(256), args,
                         0, s, "nlspn_mdcn_backward weight");
}

// ---------------------------------------------------------------------- head epilogue
int head_mb(int nout) {
    const int mb = (nout + 2 + 31) / 32;
    return mb <= 3 ? mb : (mb <= 5 ? 5 : -1);
}

// Shared launch of both head-epilogue entry points.
int launch_heads(HeadsArgs &a, void *stream) {
    const int B = a.B, C = a.C, W = a.W, nout = a.nout;
    const long long grid = (long long)B * a.tiles_x * a.tiles_y;
    if (grid > 0x7fffffffLL) return fail(NLSPN_EINVAL, "input too large");
    const bool vec = W % 4 == 0 && aligned(a.fe1, 16) && aligned(a.fd_oa, 16) && aligned(a.fd_id, 16) &&
                     aligned(a.fd_cf, 16);
    const void *fn = nullptr;
    int lds = 0;
    switch (head_mb(nout)) {
#define NLSPN_HD_CASE(MB)                                                                                   \
    case MB:                                                                                                \
        fn = vec ? reinterpret_cast<const void *>(&heads_kernel<MB, true>)                                  \
                 : reinterpret_cast<const void *>(&heads_kernel<MB, false>);                                \
        lds = (int)sizeof(float) * (HdCfg<MB>::LDS_FLOATS + 2 * C * 9);                                     \
        break;
        NLSPN_HD_CASE(1)
        NLSPN_HD_CASE(2)
        NLSPN_HD_CASE(3)
        NLSPN_HD_CASE(5)
#undef NLSPN_HD_CASE
        default: return fail(NLSPN_EUNSUPPORTED, "head epilogue: nout=%d", nout);
    }
    if (a.aff_out)  // the fused propagation prologue (nout = 24: MB = 1)
        fn = vec ? reinterpret_cast<const void *>(&heads_kernel<1, true, 0, true>)
                 : reinterpret_cast<const void *>(&heads_kernel<1, false, 0, true>);
    else if (kExperiments && vec && head_mb(nout) == 1 && (a.dbg & 3u)) {  // ablation kernels (timing only)
        const void *abl[3] = {reinterpret_cast<const void *>(&heads_kernel<1, true, 1>),
                              reinterpret_cast<const void *>(&heads_kernel<1, true, 2>),
                              reinterpret_cast<const void *>(&heads_kernel<1, true, 3>)};
        fn = abl[(a.dbg & 3u) - 1];
    }
    // The attribute is per device (the current device is the caller's, and DataParallel
    // replicas launch from their own threads): set_lds_attr makes the driver call once
    // per device and kernel.
    if (lds > 65536) NLSPN_TRY(set_lds_attr(fn, lds));
    void *args[] = {&a};
    return launch_kernel(fn, dim3((unsigned)grid), dim3(kHdNT), args, (size_t)lds, as_stream(stream), "nlspn_head_epilogue");
}

// The split-bf16 builds (nlspn_heads_x3.h; workgroups per CU: its header).
int launch_heads_x3(HeadsArgs &a, void *stream) {
    const int C = a.C, W = a.W, nout = a.nout;
    const long long grid = (long long)a.B * a.tiles_x * a.tiles_y;
    // (the window's buffer loads address a round's 16 planes with 32-bit byte offsets)
    if (grid > 0x7fffffffLL || 64LL * a.H * W > 0x7fffffffLL) return fail(NLSPN_EINVAL, "input too large");
    const bool vec = W % 4 == 0 && aligned(a.fe1, 16) && aligned(a.fd_oa, 16) && aligned(a.fd_id, 16) &&
                     aligned(a.fd_cf, 16);
    const int mb = hx3_mb(nout);
    const void *fn = nullptr;
    switch (mb) {
#define NLSPN_HDX3_CASE(MB)                                                       \
    case MB:                                                                      \
        fn = vec ? reinterpret_cast<const void *>(&headsx3_kernel<MB, true>)      \
                 : reinterpret_cast<const void *>(&headsx3_kernel<MB, false>);    \
        break;
        NLSPN_HDX3_CASE(1)
        NLSPN_HDX3_CASE(2)
        NLSPN_HDX3_CASE(3)
        NLSPN_HDX3_CASE(5)
#undef NLSPN_HDX3_CASE
        default: return fail(NLSPN_EUNSUPPORTED, "head epilogue: nout=%d", nout);
    }
    if (a.aff_out)  // the fused propagation prologue (nout = 24: MB = 1)
        fn = vec ? reinterpret_cast<const void *>(&headsx3_kernel<1, true, true>)
                 : reinterpret_cast<const void *>(&headsx3_kernel<1, false, true>);
    const int lds = hx3_lds_bytes(mb, C);
    if (lds > kHx3LdsBudget) return fail(NLSPN_EUNSUPPORTED, "head epilogue: C=%d needs %d bytes of LDS", C, lds);
    if (lds > 65536) NLSPN_TRY(set_lds_attr(fn, lds));
    void *args[] = {&a};
    return launch_kernel(fn, dim3((unsigned)grid), dim3(kHdNT), args, (size_t)lds, as_stream(stream),
                         "nlspn_head_epilogue_x3");
}

// ---- the head epilogue's backward (nlspn_heads_bwd.h)
// The shape rules shared by its entries, in the forward's order and wording
int check_head_bwd_shape(int B, int C, int H, int W, int nout) {
    if (C < 16 || C % 16) return fail(NLSPN_EINVAL, "head backward: C=%d (multiple of 16)", C);
    if (nout < 1) return fail(NLSPN_EINVAL, "head backward: nout=%d", nout);
    if (nout > 158) return fail(NLSPN_EUNSUPPORTED, "head backward: nout=%d (at most 158)", nout);
    return check_nonempty(B, H, W);
}
// one image of a source (C planes) and of gpre (nout + 2 planes) below 2 GiB; B H W in int
int check_head_bwd_size(int B, int C, int H, int W, int nout) {
    const long long HW = (long long)H * W, planes = C > nout + 2 ? C : nout + 2;
    if (HW * planes * 4 > 0x7fffffffLL || (long long)B * HW > 0x7fffffffLL) return fail(NLSPN_EINVAL, "head backward: input too large");
    return NLSPN_OK;
}

// out[rows][n1][T] = the sum over nsl slabs of ws[(i n1p + j) T + t], slices in order
int head_reduce(const float *ws, float *out, int n0, int n1, int n1p, int T, long long slab, int nsl, hipStream_t st,
                const char *what) {
    float unit = 1.f;
    void *rargs[] = {&ws, &out, &n0, &n1, &n1p, &T, &slab, &nsl, &unit};
    return launch_kernel(reinterpret_cast<const void *>(&gwgrad_reduce_kernel), dim3(elementwise_grid((long long)n0 * n1 * T)),
                         dim3(256), rargs, 0, st, what);
}

}  // namespace

extern "C" {

int nlspn_head_backward_pre(const float *g_off_aff, const float *g_pred_init, const float *g_conf,
                            const float *pred_init, const float *conf, float *gpre, int B, int H, int W, int nout,
                            void *stream) {
    if (!gpre) return fail(NLSPN_EINVAL, "head backward: null pointer");
    if ((g_pred_init == nullptr) != (pred_init == nullptr) || (g_conf == nullptr) != (conf == nullptr))
        return fail(NLSPN_EINVAL, "head backward: a head's gradient and saved output must both be given or both NULL");
    NLSPN_TRY(check_head_bwd_shape(B, 16, H, W, nout));
    NLSPN_TRY(check_head_bwd_size(B, 16, H, W, nout));
    HeadPreArgs a{g_off_aff, g_pred_init, g_conf, pred_init, conf, gpre, B, nout, (long long)H * W};
    void *args[] = {&a};
    return launch_kernel(reinterpret_cast<const void *>(&head_pre_kernel), dim3(elementwise_grid((long long)B * (nout + 2) * H * W)),
                         dim3(256), args, 0, as_stream(stream), "nlspn_head_backward_pre");
}

int nlspn_head_dgrad_single(const float *gpre, const float *w_id, const float *w_cf, float *d_fd_id, float *d_fd_cf,
                            int B, int C, int H, int W, int nout, void *stream) {
    if (!gpre) return fail(NLSPN_EINVAL, "head backward: null pointer");
    if ((w_id == nullptr) != (d_fd_id == nullptr) || (w_cf == nullptr) != (d_fd_cf == nullptr))
        return fail(NLSPN_EINVAL, "head backward: a head's weight and data gradient must both be given or both NULL");
    NLSPN_TRY(check_head_bwd_shape(B, C, H, W, nout));
    NLSPN_TRY(check_head_bwd_size(B, C, H, W, nout));
    if (!d_fd_id && !d_fd_cf) return NLSPN_OK;
    HeadDgSingleArgs a{gpre, w_id, w_cf, d_fd_id, d_fd_cf, B, C, H, W, nout};
    void *args[] = {&a};
    return launch_kernel(reinterpret_cast<const void *>(&head_dgrad_single_kernel), dim3(elementwise_grid((long long)B * H * W)),
                         dim3(256), args, 0, as_stream(stream), "nlspn_head_dgrad_single");
}

size_t nlspn_head_wgrad_workspace_bytes(int B, int C, int H, int W, int nout) {
    if (check_head_bwd_shape(B, C, H, W, nout) || check_head_bwd_size(B, C, H, W, nout)) return 0;
    const HbPlan pl = hb_plan(B, C, H, W, nout);
    return pl.fits ? (size_t)pl.floats * sizeof(float) : 0;
}

int nlspn_head_wgrad(const float *gpre, const float *fe1, const float *fd_oa, const float *fd_id, const float *fd_cf,
                     float *dw_oa, float *db_oa, float *dw_id, float *db_id, float *dw_cf, float *db_cf, void *workspace,
                     int64_t workspace_bytes, int B, int C, int H, int W, int nout, void *stream) {
    if (!gpre || !fe1 || !fd_oa || !dw_oa || !db_oa || !workspace) return fail(NLSPN_EINVAL, "head backward: null pointer");
    if ((fd_id == nullptr) != (dw_id == nullptr) || (fd_id == nullptr) != (db_id == nullptr) ||
        (fd_cf == nullptr) != (dw_cf == nullptr) || (fd_cf == nullptr) != (db_cf == nullptr))
        return fail(NLSPN_EINVAL, "head backward: a head's source and weight / bias gradients must all be given or all NULL");
    NLSPN_TRY(check_head_bwd_shape(B, C, H, W, nout));
    const HbPlan pl = hb_plan(B, C, H, W, nout);
    if (workspace_bytes < pl.floats * (long long)sizeof(float))
        return fail(NLSPN_EINVAL, "head backward: workspace too small (%lld bytes, needs %lld)", (long long)workspace_bytes,
                    pl.floats * (long long)sizeof(float));
    NLSPN_TRY(check_head_bwd_size(B, C, H, W, nout));
    if (!pl.fits) return fail(NLSPN_EINVAL, "head backward: input too large");
    hipStream_t st = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    HwgradArgs a{gpre, fd_oa, fe1, fd_id, fd_cf, ws, ws + pl.vec_off, pl.R, C, B, H, W,
                 pl.mtiles, pl.ntiles, pl.nsl, pl.bw, pl.nbands, pl.units, pl.ups, pl.nvs};
    void *args[] = {&a};
    const void *fn = reinterpret_cast<const void *>(&hwgrad_kernel);
    NLSPN_TRY(set_lds_attr(fn, kHbLdsBytes));
    NLSPN_TRY(launch_kernel(fn, dim3((unsigned)(pl.mtiles * pl.ntiles * pl.nsl)), dim3(kHbNTHR), args, (size_t)kHbLdsBytes, st,
                            "nlspn_head_wgrad"));
    if (fd_id || fd_cf)
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&hwgrad_single_kernel), dim3((unsigned)(2 * C * pl.nvs)), dim3(256),
                                args, 0, st, "nlspn_head_wgrad single"));
    // one slab feeds three destinations: rows < nout whole, the id / cf rows' fe1 halves (their
    // fd_oa halves are padding); the id / cf decoder halves come from the one-row partials
    const int Clp = pl.ntiles * kHbNT;
    NLSPN_TRY(head_reduce(ws, dw_oa, nout, 2 * C, Clp, 9, pl.slab, pl.nsl, st, "nlspn_head_wgrad reduce"));
    float *const dws[2] = {dw_id, dw_cf};
    for (int k = 0; k < 2; ++k) {
        if (!dws[k]) continue;
        NLSPN_TRY(head_reduce(ws + ((long long)(nout + k) * Clp + C) * 9, dws[k] + (long long)C * 9, 1, C, Clp, 9, pl.slab, pl.nsl,
                              st, "nlspn_head_wgrad reduce"));
        NLSPN_TRY(head_reduce(a.vec + (long long)k * C * 9, dws[k], 1, C, C, 9, 2LL * C * 9, pl.nvs, st, "nlspn_head_wgrad reduce"));
    }
    // db: the per-row sums of gpre
    {
        int R = pl.R, nsb = pl.nsb, Bv = B;
        long long HW = (long long)H * W;
        float *part = ws + pl.bias_off;
        void *pargs[] = {(void *)&gpre, &part, &R, &Bv, &HW, &nsb};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gbias_partial_kernel), dim3((unsigned)(R * nsb)), dim3(256), pargs,
                                0, st, "nlspn_head_wgrad bias"));
        NLSPN_TRY(head_reduce(part, db_oa, nout, 1, 1, 1, R, nsb, st, "nlspn_head_wgrad bias reduce"));
        if (db_id) NLSPN_TRY(head_reduce(part + nout, db_id, 1, 1, 1, 1, R, nsb, st, "nlspn_head_wgrad bias reduce"));
        if (db_cf) NLSPN_TRY(head_reduce(part + nout + 1, db_cf, 1, 1, 1, 1, R, nsb, st, "nlspn_head_wgrad bias reduce"));
    }
    return NLSPN_OK;
}

int nlspn_s2d_pyramid(int dtype, const void *dep, const float *w1, const float *b1, const float *w2,
                      const float *b2, void *out, void *pyr, int B, int H, int W, void *stream) {
    NLSPN_TRY(check_f32(dtype, "S2D pyramid"));
    NLSPN_TRY(check_nonempty(B, H, W));
    if (!dep || !w1 || !b1 || !w2 || !b2 || !out) return fail(NLSPN_EINVAL, "null required pointer");
    S2DArgs a{static_cast<const float *>(dep), w1, b1, w2, b2, static_cast<float *>(out), static_cast<float *>(pyr),
              B, H, W, (W + kS2DTW - 1) / kS2DTW, (H + kS2DTH - 1) / kS2DTH, 0u};
    a.dbg = env_dbg("NLSPN_S2D_DBG");
    const long long grid = (long long)B * a.tiles_x * a.tiles_y;
    if (grid > 0x7fffffffLL) return fail(NLSPN_EINVAL, "input too large");
    void *args[] = {&a};
    return launch_kernel(reinterpret_cast<const void *>(&s2d_pyramid_kernel), dim3((unsigned)grid), dim3(256), args, 0,
                         as_stream(stream), "nlspn_s2d_pyramid");
}

int nlspn_head_packed_size(int C, int nout, int64_t *wm_floats, int64_t *wv_floats, int64_t *bias_floats) {
    if (C < 16 || C % 16 || nout < 1) return fail(NLSPN_EINVAL, "head epilogue: C=%d (multiple of 16) nout=%d", C, nout);
    const int mb = head_mb(nout);
    if (mb < 0) return fail(NLSPN_EUNSUPPORTED, "head epilogue: nout=%d (at most 158)", nout);
    if (wm_floats) *wm_floats = 2LL * C * 9 * 32 * mb;
    if (wv_floats) *wv_floats = 2LL * C * 9;
    if (bias_floats) *bias_floats = 32LL * mb;
    return NLSPN_OK;
}

int nlspn_head_pack_weights(const float *w_oa, const float *b_oa, const float *w_id, const float *b_id,
                            const float *w_cf, const float *b_cf, float *wm, float *wv, float *bias, int C, int nout,
                            void *stream) {
    int64_t nm = 0, nv = 0, nb = 0;
    NLSPN_TRY(nlspn_head_packed_size(C, nout, &nm, &nv, &nb));
    if (!w_oa || !wm || !wv || !bias) return fail(NLSPN_EINVAL, "head epilogue: null pointer");
    HeadsPackArgs a{w_oa, b_oa, w_id, b_id, w_cf, b_cf, wm, wv, bias, C, nout, (int)nb};
    const long long n = nm + nv + nb;
    void *args[] = {&a};
    return launch_kernel(reinterpret_cast<const void *>(&heads_pack_kernel), dim3((unsigned)((n + 255) / 256)), dim3(256),
                         args, 0, as_stream(stream), "nlspn_head_pack_weights");
}

int nlspn_head_epilogue(int dtype, const void *fe1, const void *fd_oa, const void *fd_id, const void *fd_cf,
                        const float *wm, const float *wv, const float *bias, void *off_aff, void *pred_init,
                        void *conf, int B, int C, int H, int W, int nout, void *stream) {
    NLSPN_TRY(check_f32(dtype, "head epilogue"));
    NLSPN_TRY(check_nonempty(B, H, W));
    NLSPN_TRY(nlspn_head_packed_size(C, nout, nullptr, nullptr, nullptr));
    if (!fe1 || !fd_oa || !wm || !wv || !bias || !off_aff) return fail(NLSPN_EINVAL, "head epilogue: null pointer");
    if ((fd_id == nullptr) != (pred_init == nullptr) || (fd_cf == nullptr) != (conf == nullptr))
        return fail(NLSPN_EINVAL, "head epilogue: a head's source and output must both be given or both NULL");
    HeadsArgs a{static_cast<const float *>(fe1), static_cast<const float *>(fd_oa), static_cast<const float *>(fd_id),
                static_cast<const float *>(fd_cf), wm, wv, bias, static_cast<float *>(off_aff),
                static_cast<float *>(pred_init), static_cast<float *>(conf), B, C, H, W, nout,
                (W + kHdTW - 1) / kHdTW, (H + kHdTH - 1) / kHdTH, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                0u, 0u};
    a.dbg = env_dbg("NLSPN_HEADS_DBG");
    return launch_heads(a, stream);
}

int nlspn_head_epilogue_prologue(int dtype, const void *fe1, const void *fd_oa, const void *fd_id, const void *fd_cf,
                                 const float *wm, const float *wv, const float *bias, const void *dep,
                                 const float *gamma, void *pred_init, void *conf_out, void *aff_out, void *off_out,
                                 void *p0, int B, int C, int H, int W, int kh, int kw, int kind, unsigned flags,
                                 void *stream) {
    NLSPN_TRY(check_f32(dtype, "head epilogue"));
    NLSPN_TRY(check_nonempty(B, H, W));
    if (kh != 3 || kw != 3)
        return fail(NLSPN_EUNSUPPORTED, "fused head prologue: 3x3 propagation only (k = %dx%d)", kh, kw);
    NLSPN_TRY(check_kind(kind));
    const int nout = 3 * 8;
    NLSPN_TRY(nlspn_head_packed_size(C, nout, nullptr, nullptr, nullptr));
    if (!fe1 || !fd_oa || !fd_id || !wm || !wv || !bias || !gamma || !pred_init || !aff_out || !off_out || !p0)
        return fail(NLSPN_EINVAL, "fused head prologue: null pointer");
    if ((fd_cf == nullptr) != (conf_out == nullptr))
        return fail(NLSPN_EINVAL, "fused head prologue: cf_fd1 and conf_out must both be given or both NULL");
    NLSPN_TRY(check_preserve(flags, dep));
    HeadsArgs a{static_cast<const float *>(fe1), static_cast<const float *>(fd_oa), static_cast<const float *>(fd_id),
                static_cast<const float *>(fd_cf), wm, wv, bias, nullptr, static_cast<float *>(pred_init),
                static_cast<float *>(conf_out), B, C, H, W, nout, (W + kHdTW - 1) / kHdTW, (H + kHdTH - 1) / kHdTH,
                static_cast<const float *>(dep), gamma, static_cast<float *>(aff_out), static_cast<float *>(off_out),
                static_cast<float *>(p0), kind, flags, 0u};
    return launch_heads(a, stream);
}

// ---- the split-bf16 head epilogue (nlspn_heads_x3.h): the entries above with wm as bf16 fragments
int nlspn_head_x3_packed_size(int C, int nout, int64_t *wm_bf16_elems, int64_t *wv_floats, int64_t *bias_floats) {
    NLSPN_TRY(nlspn_head_packed_size(C, nout, nullptr, nullptr, nullptr));
    const int mb = hx3_mb(nout);
    if (wm_bf16_elems) *wm_bf16_elems = hx3_wm_elems(C, mb);
    if (wv_floats) *wv_floats = hx3_wv_floats(C);
    if (bias_floats) *bias_floats = hx3_bias_floats(mb);
    return NLSPN_OK;
}

int nlspn_head_x3_pack_weights(const float *w_oa, const float *b_oa, const float *w_id, const float *b_id,
                               const float *w_cf, const float *b_cf, void *wm, float *wv, float *bias, int C, int nout,
                               void *stream) {
    int64_t nm = 0, nv = 0, nb = 0;
    NLSPN_TRY(nlspn_head_x3_packed_size(C, nout, &nm, &nv, &nb));
    if (!w_oa || !wm || !wv || !bias) return fail(NLSPN_EINVAL, "head epilogue: null pointer");
    HeadsPackArgs a{w_oa, b_oa, w_id, b_id, w_cf, b_cf, static_cast<float *>(wm), wv, bias, C, nout, (int)nb};
    const long long n = nm + nv + nb;
    void *args[] = {&a};
    return launch_kernel(reinterpret_cast<const void *>(&headsx3_pack_kernel), dim3((unsigned)((n + 255) / 256)), dim3(256),
                         args, 0, as_stream(stream), "nlspn_head_x3_pack_weights");
}

int nlspn_head_epilogue_x3(int dtype, const void *fe1, const void *fd_oa, const void *fd_id, const void *fd_cf,
                           const void *wm, const float *wv, const float *bias, void *off_aff, void *pred_init,
                           void *conf, int B, int C, int H, int W, int nout, void *stream) {
    NLSPN_TRY(check_f32(dtype, "head epilogue"));
    NLSPN_TRY(check_nonempty(B, H, W));
    NLSPN_TRY(nlspn_head_packed_size(C, nout, nullptr, nullptr, nullptr));
    if (!fe1 || !fd_oa || !wm || !wv || !bias || !off_aff) return fail(NLSPN_EINVAL, "head epilogue: null pointer");
    if ((fd_id == nullptr) != (pred_init == nullptr) || (fd_cf == nullptr) != (conf == nullptr))
        return fail(NLSPN_EINVAL, "head epilogue: a head's source and output must both be given or both NULL");
    HeadsArgs a{static_cast<const float *>(fe1), static_cast<const float *>(fd_oa), static_cast<const float *>(fd_id),
                static_cast<const float *>(fd_cf), static_cast<const float *>(wm), wv, bias,
                static_cast<float *>(off_aff), static_cast<float *>(pred_init), static_cast<float *>(conf), B, C, H, W,
                nout, (W + kHdTW - 1) / kHdTW, (H + kHdTH - 1) / kHdTH, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                0u, 0u};
    return launch_heads_x3(a, stream);
}

int nlspn_head_epilogue_prologue_x3(int dtype, const void *fe1, const void *fd_oa, const void *fd_id,
                                    const void *fd_cf, const void *wm, const float *wv, const float *bias,
                                    const void *dep, const float *gamma, void *pred_init, void *conf_out, void *aff_out,
                                    void *off_out, void *p0, int B, int C, int H, int W, int kh, int kw, int kind,
                                    unsigned flags, void *stream) {
    NLSPN_TRY(check_f32(dtype, "head epilogue"));
    NLSPN_TRY(check_nonempty(B, H, W));
    if (kh != 3 || kw != 3)
        return fail(NLSPN_EUNSUPPORTED, "fused head prologue: 3x3 propagation only (k = %dx%d)", kh, kw);
    NLSPN_TRY(check_kind(kind));
    const int nout = 3 * 8;
    NLSPN_TRY(nlspn_head_packed_size(C, nout, nullptr, nullptr, nullptr));
    if (!fe1 || !fd_oa || !fd_id || !wm || !wv || !bias || !gamma || !pred_init || !aff_out || !off_out || !p0)
        return fail(NLSPN_EINVAL, "fused head prologue: null pointer");
    if ((fd_cf == nullptr) != (conf_out == nullptr))
        return fail(NLSPN_EINVAL, "fused head prologue: cf_fd1 and conf_out must both be given or both NULL");
    NLSPN_TRY(check_preserve(flags, dep));
    HeadsArgs a{static_cast<const float *>(fe1), static_cast<const float *>(fd_oa), static_cast<const float *>(fd_id),
                static_cast<const float *>(fd_cf), static_cast<const float *>(wm), wv, bias, nullptr,
                static_cast<float *>(pred_init), static_cast<float *>(conf_out), B, C, H, W, nout,
                (W + kHdTW - 1) / kHdTW, (H + kHdTH - 1) / kHdTH, static_cast<const float *>(dep), gamma,
                static_cast<float *>(aff_out), static_cast<float *>(off_out), static_cast<float *>(p0), kind, flags, 0u};
    return launch_heads_x3(a, stream);
}

int nlspn_affinity_normalize(int dtype, const void *aff_raw, int64_t aff_bstride, const float *gamma,
                             void *aff_out, int B, int K, int H, int W, int kind, void *stream) {
    NLSPN_TRY(check_storage_dtype(dtype));
    NLSPN_TRY(check_nonempty(B, H, W));
    NLSPN_TRY(check_kind(kind));
    if (!aff_raw || !gamma || !aff_out) return fail(NLSPN_EINVAL, "null pointer");
    const long long HW = (long long)H * W;
    NLSPN_TRY(check_batch_stride("aff", aff_bstride, K, HW));
    const size_t vb = 4 * esize(dtype);
    const bool vec = HW % 4 == 0 && aff_bstride % 4 == 0 && aligned(aff_raw, vb) && aligned(aff_out, vb);
    const void *fn = dtype == NLSPN_DTYPE_F32 ? select_affnorm<float>(K, vec) : select_affnorm<__half>(K, vec);
    if (!fn) return fail(NLSPN_EUNSUPPORTED, "no affinity kernel for K=%d (supported 8, 16, 24, 48)", K);
    long long bs = aff_bstride, hw = HW;
    int b = B, k = kind;
    void *args[] = {(void *)&aff_raw, &bs, (void *)&gamma, &aff_out, &hw, &b, &k};
    return launch_kernel(fn, dim3(elementwise_grid((long long)B * HW / (vec ? 4 : 1))), dim3(256), args, 0,
                         as_stream(stream), "nlspn_affinity_normalize");
}

int nlspn_mdcn_forward(int dtype, const void *input, const void *weight, const void *bias, const void *offset,
                       const void *mask, void *output, int B, int C, int H, int W, int Cout, int kh, int kw, int sh,
                       int sw, int ph, int pw, int dh, int dw, int group, int deformable_group, void *stream) {
    if (dtype != NLSPN_DTYPE_F32 && dtype != NLSPN_DTYPE_F16 && dtype != NLSPN_DTYPE_F64)
        return fail(NLSPN_EUNSUPPORTED, "dtype %d", dtype);
    if (!input || !weight || !offset || !mask || !output) return fail(NLSPN_EINVAL, "null required pointer");
    int Ho = 0, Wo = 0;
    NLSPN_TRY(check_mdcn(B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group, deformable_group, &Ho, &Wo));
    MdcnArgs a{input, weight, bias, offset, mask, output, B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw,
               group, deformable_group, Ho, Wo};
    const void *fn = dtype == NLSPN_DTYPE_F32   ? reinterpret_cast<const void *>(&mdcn_forward_kernel<float, float>)
                     : dtype == NLSPN_DTYPE_F64 ? reinterpret_cast<const void *>(&mdcn_forward_kernel<double, double>)
                                                : reinterpret_cast<const void *>(&mdcn_forward_kernel<__half, float>);
    void *args[] = {&a};
    return launch_kernel(fn, dim3(elementwise_grid((long long)B * Cout * Ho * Wo)), dim3(256), args, 0, as_stream(stream),
                         "nlspn_mdcn_forward");
}

int nlspn_mdcn_backward(int dtype, const void *input, const void *weight, const void *offset, const void *mask,
                        const void *grad_output, void *grad_input, void *grad_offset, void *grad_mask,
                        void *grad_weight, void *grad_bias, int B, int C, int H, int W, int Cout, int kh, int kw,
                        int sh, int sw, int ph, int pw, int dh, int dw, int group, int deformable_group,
                        void *stream) {
    if (dtype != NLSPN_DTYPE_F32 && dtype != NLSPN_DTYPE_F64)
        return fail(NLSPN_EUNSUPPORTED, "the DCN backward is implemented for float32 and float64");
    if (!input || !weight || !offset || !mask || !grad_output || !grad_input || !grad_offset || !grad_mask ||
        !grad_weight)
        return fail(NLSPN_EINVAL, "null required pointer");
    int Ho = 0, Wo = 0;
    NLSPN_TRY(check_mdcn(B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group, deformable_group, &Ho, &Wo));
    const long long nw = (long long)Cout * (C / group) * kh * kw + (grad_bias ? Cout : 0);
    if (nw > 0x7fffffffLL) return fail(NLSPN_EINVAL, "too many weight elements");
    const long long nd = (long long)B * deformable_group * kh * kw * Ho * Wo;
    return dtype == NLSPN_DTYPE_F64
               ? mdcn_backward_impl<double>(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask,
                                            grad_weight, grad_bias, B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw,
                                            group, deformable_group, Ho, Wo, nd, nw, as_stream(stream))
               : mdcn_backward_impl<float>(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask,
                                           grad_weight, grad_bias, B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw,
                                           group, deformable_group, Ho, Wo, nd, nw, as_stream(stream));
}

}  // extern "C"
