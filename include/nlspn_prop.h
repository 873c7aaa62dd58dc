/*
 * nlspn_prop.h — C ABI of the MI355X-native NLSPN propagation hot path.
 *
 * Drop-in boundary for XJTUXYC/NLSPN_ECCV20's non-local spatial propagation
 * (src/model/nlspnmodel.py:179-381) and the DCNv2 forward it rides on
 * (src/model/deformconv/src/vision.cpp:9 -> modulated_deform_conv.h:10-44 ->
 *  cuda/modulated_deform_conv_cuda.cu:19-121).  Plain pointers and sizes only:
 * no torch types cross this boundary.  All device pointers are caller-owned
 * (allocated by the caller on the current device); nothing is allocated on the
 * hot path.  `stream` is a hipStream_t passed as void* (NULL = legacy default
 * stream).  Every call only enqueues work; none synchronises the host, so every
 * call may be captured into a hipGraph.
 *
 * Layout: NCHW with one channel per plane; a "plane" is H*W contiguous
 * elements; tensors with several planes per batch item take a batch stride in
 * ELEMENTS (so slices of a (B,3K,H,W) off_aff head output can be passed without
 * a copy, as nlspnmodel.py:304-305 slices it).
 *
 * Errors: functions return 0 on success, a positive NLSPN_E* code otherwise;
 * nlspn_last_error() gives the message (thread-local), worded like the
 * reference's AT_ASSERTM/AT_ERROR messages where one exists.
 */
#ifndef NLSPN_PROP_H
#define NLSPN_PROP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLSPN_ABI_VERSION 3

/* element type of every tensor argument (math is always fp32) */
#define NLSPN_DTYPE_F32 0
#define NLSPN_DTYPE_F16 1
#define NLSPN_DTYPE_F64 2 /* the seam-2 DCN entry points only (nlspn_mdcn_forward/backward) */

/* affinity normalisation kinds, src/config.py:259-263 / nlspnmodel.py:179-201 */
#define NLSPN_AFF_AS 0
#define NLSPN_AFF_ASS 1
#define NLSPN_AFF_TC 2
#define NLSPN_AFF_TGASS 3

/* flags (bit set) — src/config.py:250-257 */
#define NLSPN_PRESERVE_INPUT 0x1u /* args.preserve_input, nlspnmodel.py:328-334,342-344,355-357 */
#define NLSPN_ALWAYS_CLIP 0x2u    /* args.always_clip,    nlspnmodel.py:346-348,359-361,375-377 */

/* offset plane layout for nlspn_prop_step */
#define NLSPN_OFF_INSERTED 0 /* (B, 2(K+1), H, W): tap t uses planes 2t (dh), 2t+1 (dw) — _off_insert output */
#define NLSPN_OFF_RAW 1      /* (B, 2K, H, W): the head's raw slice; the reference tap is implicit zero */

/* error codes */
#define NLSPN_OK 0
#define NLSPN_EINVAL 1       /* bad shape / argument */
#define NLSPN_EUNSUPPORTED 2 /* geometry or dtype without a kernel instantiation */
#define NLSPN_EHIP 3         /* HIP runtime / launch error */
#define NLSPN_EABORTED 4     /* a resident launch aborted (nlspn_resident_status) */
/* nlspn_time_propagate *resident: bit once set when iteration 1 ran inside the resident
 * launches (an A/B form removed in round 4; never set now, kept for ABI stability) */
#define NLSPN_RESIDENT_FIRST 0x100

/* Version of this ABI (NLSPN_ABI_VERSION). */
int nlspn_abi_version(void);

/* Message for the last error on this thread ("" if none). */
const char *nlspn_last_error(void);

/*
 * S2D sparse-depth encoder front, fused.  Replaces the pool
 * pyramid and pool_convs of S2D.forward (src/model/nlspnmodel.py:437-455) and the
 * torch.cat([dep_feat, dep], 1) that feeds S2D.conv (:459):
 *   dep  : B x H x W (sparse depth, 0 = missing)
 *   w1 b1: pool_convs[0] conv weight (8 x 6) and bias (8); w2 b2: pool_convs[1]
 *          weight (16 x 8) and bias (16); device float32
 *   out  : B x 17 x H x W: channels 0..15 = ReLU(w2 . ReLU(w1 . pyramid + b1) + b2),
 *          channel 16 = dep
 *   pyr  : B x 6 x H x W, the min pools 3/5/7/9 (zeros = missing, :441-447) and max
 *          pools 11/13 (:449-452), or NULL (written for the weight gradients)
 * float32 only.
 */
int nlspn_s2d_pyramid(int dtype, const void *dep, const float *w1, const float *b1,
                      const float *w2, const float *b2, void *out, void *pyr,
                      int B, int H, int W, void *stream);

/*
 * Head epilogue: the decoder's last three 3x3 convolutions as one
 * kernel.  Replaces src/model/nlspnmodel.py:296-315 —
 *   pred_init  = ReLU(id_dec0(cat(id_fd1, fe1)))      id_dec0      :68
 *   off_aff    = off_aff_dec0(cat(off_aff_fd1, fe1))  off_aff_dec0 :74 (or :76 without offsets)
 *   confidence = Sigmoid(cf_dec0(cat(cf_fd1, fe1)))   cf_dec0      :83-86
 * with the four C-channel sources read in place (no concatenated copies):
 *   fe1, fd_oa   : B x C x H x W (fe1 and off_aff_fd1), contiguous, device float32
 *   fd_id, fd_cf : B x C x H x W (id_fd1, cf_fd1) or NULL (that head is skipped)
 *   wm, wv, bias : the weights packed by nlspn_head_pack_weights (nlspn_head_packed_size)
 *   off_aff      : B x nout x H x W;  pred_init, conf : B x 1 x H x W (NULL with their source)
 * Arithmetic: f32 operands and products on the matrix cores, f32 accumulation; only the
 * summation order differs from a sequential f32 convolution.  C % 16 == 0; float32 only.
 */
int nlspn_head_packed_size(int C, int nout, int64_t *wm_floats, int64_t *wv_floats,
                           int64_t *bias_floats);
int nlspn_head_pack_weights(const float *w_oa, const float *b_oa, const float *w_id,
                            const float *b_id, const float *w_cf, const float *b_cf,
                            float *wm, float *wv, float *bias, int C, int nout, void *stream);
int nlspn_head_epilogue(int dtype, const void *fe1, const void *fd_oa, const void *fd_id,
                        const void *fd_cf, const float *wm, const float *wv,
                        const float *bias, void *off_aff, void *pred_init, void *conf,
                        int B, int C, int H, int W, int nout, void *stream);

/*
 * The head epilogue with the propagation prologue fused in (3x3, K = 8, offsets on):
 * instead of the raw off_aff planes the epilogue writes what step 1 of the section
 * would — off_out = _off_insert(off) (nlspnmodel.py:324, B x 18 x H x W), aff_out =
 * _affinity_normalization + _aff_insert (:325, B x 9 x H x W), conf_out = the blended
 * confidence (:328-334, NULL with fd_cf), pred_init (:297) and p0 = the blended
 * [clamped] pred_init that iteration 1 propagates (:341-348) — then
 * nlspn_propagate_normalized runs the T iterations from them.  Same IEEE sequence as
 * nlspn_propagate's step 1: bit-identical outputs given the same convolution sums.
 * gamma: device pointer (learnable aff_scale_const); kind: NLSPN_AFF_*.
 */
int nlspn_head_epilogue_prologue(int dtype, const void *fe1, const void *fd_oa, const void *fd_id,
                                 const void *fd_cf, const float *wm, const float *wv,
                                 const float *bias, const void *dep, const float *gamma,
                                 void *pred_init, void *conf_out, void *aff_out, void *off_out,
                                 void *p0, int B, int C, int H, int W, int kh, int kw, int kind,
                                 unsigned flags, void *stream);

/*
 * The head epilogue and its fused-prologue form on the bf16 matrix cores with split
 * operands ("bf16x3", opt-in; csrc/nlspn_heads_x3.h).  Same arguments, validation order
 * and refusals as the entries above; wm is the bf16 array packed by
 * nlspn_head_x3_pack_weights (nlspn_head_x3_packed_size elements), wv and bias are
 * bit-equal to the f32 pack's.  float32 tensors only.  Numerics contract:
 *   - every MFMA operand a (f32) travels as hi = rne_bf16(a), lo = rne_bf16(a - hi), the
 *     subtraction in f32: weights split once when packed, fe1 / off_aff_fd1 while staged;
 *   - per output element sum (w_hi x_hi + w_hi x_lo + w_lo x_hi) in f32 accumulators; lo lo
 *     is dropped; a term is off by at most 2^-15 |w x|;
 *   - the id / cf convolutions' one-channel decoder halves (id_fd1, cf_fd1) stay f32 VALU
 *     fmaf sums of unsplit operands, in the f32 kernel's order;
 *   - bias, ReLU, sigmoid and the fused prologue run in f32, by the f32 kernel's code;
 *   - nothing is clamped (a NaN reaches exactly its 3x3 neighbourhood, an inf gives NaN
 *     there); no atomics: the same bits on every run.
 * H * W below 2^25 (a round's 16 planes are addressed with 32-bit byte offsets).
 */
int nlspn_head_x3_packed_size(int C, int nout, int64_t *wm_bf16_elems, int64_t *wv_floats,
                              int64_t *bias_floats);
int nlspn_head_x3_pack_weights(const float *w_oa, const float *b_oa, const float *w_id,
                               const float *b_id, const float *w_cf, const float *b_cf,
                               void *wm, float *wv, float *bias, int C, int nout, void *stream);
int nlspn_head_epilogue_x3(int dtype, const void *fe1, const void *fd_oa, const void *fd_id,
                           const void *fd_cf, const void *wm, const float *wv,
                           const float *bias, void *off_aff, void *pred_init, void *conf,
                           int B, int C, int H, int W, int nout, void *stream);
int nlspn_head_epilogue_prologue_x3(int dtype, const void *fe1, const void *fd_oa,
                                    const void *fd_id, const void *fd_cf, const void *wm,
                                    const float *wv, const float *bias, const void *dep,
                                    const float *gamma, void *pred_init, void *conf_out,
                                    void *aff_out, void *off_out, void *p0, int B, int C, int H,
                                    int W, int kh, int kw, int kind, unsigned flags, void *stream);

/*
 * Backward of the head epilogue (training through nlspn_head_epilogue; opt-in;
 * csrc/nlspn_heads_bwd.h).  Replaces the autograd of src/model/nlspnmodel.py:296-315 — the
 * three torch.cat copies, their saved copies and MIOpen's convolution backward — by pieces the
 * caller drives (nlspn_eccv20_amd/heads.py _HeadFn).  f32 NCHW, contiguous, no double
 * backward.  R = nout + 2 rows in the forward kernel's column order: 0..nout-1 off_aff_dec0,
 * nout id_dec0, nout + 1 cf_dec0.
 *
 * nlspn_head_backward_pre: gpre (B x R x H x W), the pre-activation gradient, in one launch:
 *   rows < nout = g_off_aff (B x nout x H x W); row nout = g_pred_init where pred_init > 0,
 *   else 0 (a select: -0.0 and NaN outputs give 0); row nout + 1 = g_conf * (conf * (1 - conf)).
 *   pred_init, conf: the saved forward outputs (B x 1 x H x W).  Any of the three gradients may
 *   be NULL (zero rows); pred_init / conf are NULL together with their gradient, else
 *   NLSPN_EINVAL.  Rows < nout and the ReLU row are copies; the sigmoid row is two f32 products.
 *
 * The two wide data gradients are a launch of the existing stride-1 adjoint preset:
 *   nlspn_gconv_dgrad(NLSPN_GC_DG_S1, gpre, R, wadj, NULL, NULL, NULL, d_fd_oa, d_fe1, C, B, H,
 *   W, 2 C, H, W, NLSPN_GC_ACT_NONE, 1, stream), wadj the stacked (R, 2C, 3, 3) weight (the
 *   decoder halves of the id / cf rows zeroed) with taps flipped and channels transposed, packed
 *   for that preset (gru.py pack_adjoint_s1).
 *
 * nlspn_head_dgrad_single: the one-row adjoints on the VALU, d_fd_id[ci] = w_id[0, ci] flipped
 *   (*) gpre[nout], d_fd_cf[ci] = w_cf[0, ci] flipped (*) gpre[nout + 1] (B x C x H x W each):
 *   nine fmaf per element in (ky, kx) order, zero outside the image.  w_id / w_cf: the modules'
 *   own (1, 2C, 3, 3) weights.  A NULL (weight, output) pair skips that head; one of a pair
 *   alone is NLSPN_EINVAL.
 *
 * nlspn_head_wgrad: dW / db of the three convolutions in the modules' own layouts (dw_oa
 *   (nout, 2C, 3, 3), dw_id / dw_cf (1, 2C, 3, 3), the decoder half first, then fe1; db_oa
 *   (nout), db_id / db_cf (1)): dW_r[c][t] = sum over b, y, x of gpre[b, r, y, x] * src[b, c,
 *   y - 1 + ky, x - 1 + kx], zero outside the image, src = fe1 for c >= C and the row's own
 *   decoder output below; db_r = sum gpre[r].  Every row against [fd_oa | fe1] is an implicit
 *   GEMM on the f32 matrix cores (exact f32 products, f32 accumulation; rows in tiles of 32, K =
 *   pixels); the id / cf rows against fd_id / fd_cf are VALU fmaf sums.  K is cut into slices by
 *   the shape alone; each slice writes f32 partials into the workspace
 *   (nlspn_head_wgrad_workspace_bytes; 0 for a shape the entry refuses) and further launches sum
 *   them in slice order: no atomics, no waiting between workgroups, the same bits on every run
 *   and device.  fd_id / fd_cf are NULL together with their dw / db pair.  Operands need 4-byte
 *   alignment only.
 *
 * Refusals, before any device call and in this order: NULL required pointers or a half-given
 * pair (NLSPN_EINVAL); C not a positive multiple of 16 (NLSPN_EINVAL); nout < 1 (NLSPN_EINVAL)
 * or > 158 (NLSPN_EUNSUPPORTED); empty sizes (NLSPN_EINVAL); workspace too small
 * (NLSPN_EINVAL); "input too large" (NLSPN_EINVAL): one image's C (or R) planes reach 2 GiB,
 * B * H * W or a unit / workgroup count does not fit an int.
 */
int nlspn_head_backward_pre(const float *g_off_aff, const float *g_pred_init, const float *g_conf,
                            const float *pred_init, const float *conf, float *gpre, int B, int H,
                            int W, int nout, void *stream);
int nlspn_head_dgrad_single(const float *gpre, const float *w_id, const float *w_cf,
                            float *d_fd_id, float *d_fd_cf, int B, int C, int H, int W, int nout,
                            void *stream);
size_t nlspn_head_wgrad_workspace_bytes(int B, int C, int H, int W, int nout);
int nlspn_head_wgrad(const float *gpre, const float *fe1, const float *fd_oa, const float *fd_id,
                     const float *fd_cf, float *dw_oa, float *db_oa, float *dw_id, float *db_id,
                     float *dw_cf, float *db_cf, void *workspace, int64_t workspace_bytes, int B,
                     int C, int H, int W, int nout, void *stream);

/*
 * Affinity normalisation + reference-tap insertion.
 * Replaces NLSPNModel._affinity_normalization (src/model/nlspnmodel.py:179-201)
 * followed by _aff_insert (:261-269).
 *   aff_raw : B x K planes, batch stride aff_bstride
 *   gamma   : device pointer to ONE float32 (aff_scale_const, :93-104); read on
 *             the device so a graph replay sees the current value (learnable γ)
 *   aff_out : B x (K+1) planes, contiguous, reference tap at index K/2
 */
int nlspn_affinity_normalize(int dtype, const void *aff_raw, int64_t aff_bstride,
                             const float *gamma, void *aff_out,
                             int B, int K, int H, int W, int kind, void *stream);

/*
 * One fused propagation iteration: f = p_in * conf (conf may be NULL,
 * nlspnmodel.py:350-353), out = _propagate_once(f, offset, aff) (:203-226),
 * then the preserve-input blend (:355-357) and clamp (:359-361) per flags.
 * Replaces, per iteration, DCN.modulated_deform_conv_forward
 * (modulated_deform_conv_func.py:26; vision.cpp:9; .cu:19-121) with NLSPN's
 * all-ones 1x1xkhxkw weight and zero bias, plus ~5 elementwise torch ops.
 *   p_in, conf, dep : B planes (contiguous); dep may be NULL without PRESERVE
 *   aff     : normalised affinity, B x (K+1) planes, batch stride aff_bstride
 *             (the tap at K/2 is NOT read: it is recomputed as 1 - sum of the
 *             others, bit-identical to what nlspn_affinity_normalize wrote)
 *   off     : offsets, batch stride off_bstride, layout NLSPN_OFF_* (NULL ->
 *             the no-offset branch :209-224: 3x3 replicate padding, K must be 8)
 *   p_out   : B planes; pred_out (optional): max(out, 0) — the epilogue :375-377
 *   kh, kw  : DCN kernel geometry (odd; K = kh*kw - 1). 3x3 = prop_kernel 3.
 */
int nlspn_prop_step(int dtype, const void *p_in, const void *conf, const void *dep,
                    const void *aff, int64_t aff_bstride,
                    const void *off, int64_t off_bstride, int off_layout,
                    void *p_out, void *pred_out,
                    int B, int H, int W, int kh, int kw, unsigned flags, void *stream);

/* Bytes of device workspace nlspn_propagate uses: the resident kernel's abort word
 * (index 0) and one 128-byte line per workgroup (its placement word).  With a NULL
 * workspace nlspn_propagate runs iterations 2..T as T-1 launches instead.  The resident
 * kernel also uses pred_inter itself for its hand-offs: planes 1..T-2 hold a poison
 * value (a signalling NaN) until written, so they must not alias any input. */
size_t nlspn_workspace_bytes(int dtype, int B, int H, int W);

/*
 * The whole propagation section, src/model/nlspnmodel.py:323-381, as T launches:
 *   step 1   : the prologue fused into the first iteration — _off_insert (:324)
 *              if off_out, _affinity_normalization (:325), mask_fix / confidence
 *              blend (:328-334), first blend+clamp (:341-348), then iteration 1
 *   steps 2..T: resident launches — the invariant planes held on chip for all
 *              iterations, one launch per image group (C2: all 8 NYU images in one;
 *              C3: the 4 KITTI images as two launches of 2), per-workgroup progress
 *              words in `workspace` — when the geometry allows it (3x3 learned
 *              offsets, W % 4 == 0, 16-B aligned planes, every rectangular part fits
 *              a workgroup: nlspn_resident_config), else T-1 nlspn_prop_step
 *              launches; pred_inter[t] each, the last also pred.
 *   Every form is bit-identical.
 * Inputs : pred_init, dep (B planes), conf (B planes, or NULL = conf_prop off),
 *          aff_raw (B x K planes, stride aff_bstride), off_raw (B x 2K planes,
 *          stride off_bstride, or NULL = no-offset branch), gamma (device f32).
 * Outputs: pred_inter (T x B planes, contiguous: list_pred), pred (B planes),
 *          aff_out (B x (K+1) planes), off_out (B x 2(K+1) planes, optional),
 *          conf_out (B planes, required iff conf != NULL).
 * workspace: nlspn_workspace_bytes() bytes of device memory (may be NULL when 0).
 */
int nlspn_propagate(int dtype, const void *pred_init, const void *dep, const void *conf,
                    const void *aff_raw, int64_t aff_bstride,
                    const void *off_raw, int64_t off_bstride, const float *gamma,
                    void *pred_inter, void *pred, void *aff_out, void *off_out,
                    void *conf_out, void *workspace,
                    int B, int H, int W, int kh, int kw, int T, int kind,
                    unsigned flags, void *stream);

/*
 * Plans: nlspn_propagate captured once into a hipGraph (T kernel nodes) and
 * replayed with one hipGraphLaunch.  Pointers are baked in at creation; γ stays
 * live because it is read from device memory.  A resident plan (step 1 + the
 * resident launches) re-issues its recorded launches directly instead, which
 * costs less than a graph launch; NLSPN_PLAN_GRAPH=1 forces the graph.
 */
typedef struct nlspn_plan *nlspn_plan_t;
int nlspn_plan_create(nlspn_plan_t *plan, int dtype, const void *pred_init, const void *dep,
                      const void *conf, const void *aff_raw, int64_t aff_bstride,
                      const void *off_raw, int64_t off_bstride, const float *gamma,
                      void *pred_inter, void *pred, void *aff_out, void *off_out,
                      void *conf_out, void *workspace,
                      int B, int H, int W, int kh, int kw, int T, int kind, unsigned flags);
int nlspn_plan_launch(nlspn_plan_t plan, void *stream);
int nlspn_plan_destroy(nlspn_plan_t plan);

/*
 * Backward of nlspn_propagate (float32 or float16 storage): what autograd computes through
 * src/model/nlspnmodel.py:323-381 with the DCNv2 backward for each of the T DCN
 * calls (modulated_deform_conv_cuda.cu:124-280; vision.cpp:10 ->
 * modulated_deform_conv.h:46-86).  Takes the forward's inputs and its saved
 * outputs (pred_inter, aff_out as aff_norm, conf_out as conf_eff) and the
 * incoming gradients (grad_pred and/or grad_pred_inter, T x B planes; either may
 * be NULL).  Writes grad_pred_init (B planes), grad_conf (B planes, iff conf),
 * grad_aff_raw (B x K planes, contiguous), grad_off_raw (B x 2K planes,
 * contiguous, iff off_raw), grad_gamma (1 float, TGASS only; may be NULL).
 * grad_aff_bstride / grad_off_bstride: batch strides of grad_aff_raw / grad_off_raw
 * in elements (0 = contiguous), so both can land in ONE packed (B, 3K, H, W)
 * gradient of the head output the two slices came from (nlspnmodel.py:304-305).
 * dep receives no gradient (the reference's sparse input).  workspace:
 * nlspn_backward_workspace_bytes() bytes.  dL/df is scattered with float
 * atomics (as the reference's col2im), so its last bits depend on arrival order.
 * Scratch use: the two-pass form (3x3 with offsets, T <= 3K: the default there)
 * first stores each iteration's dL/d(output) plane in grad_aff_raw / grad_off_raw
 * (the 3K planes per item they span together) and overwrites them with the gradients
 * in its second pass.  So neither may overlap any input, pred_inter, aff_norm,
 * conf_eff, the incoming gradients or each other (beyond the packed (B, 3K, H, W)
 * layout above), and after a failed call their contents are undefined.
 *
 * dtype NLSPN_DTYPE_F16: every const void * operand (pred_init, dep, conf, aff_raw,
 * off_raw, pred_inter, aff_norm, conf_eff, grad_pred, grad_pred_inter) points to
 * halves and grad_pred_init, grad_conf, grad_aff_raw, grad_off_raw are written as
 * halves; gamma and grad_gamma stay float.  All arithmetic and every accumulator are
 * float32 (or the float path's fixed point) in the workspace; each half gradient
 * element is the float32 value rounded once (to nearest even, overflow to inf).
 * The gradient outputs are not used as scratch: the two-pass form keeps dL/d(output)
 * in T float planes per item of the workspace, the one-pass form accumulates the
 * offsets' gradient in 2K.  The workspace is then
 * nlspn_backward_workspace_bytes_dtype() bytes: the float32 size plus
 * 4 * B*H*W * (T if 3x3 and 2K < T <= 3K, else 2K) bytes.  The launch form (resident
 * pass 1, step launches, one-pass) is chosen as for float32.
 * nlspn_backward_workspace_bytes_dtype(NLSPN_DTYPE_F32, ...) equals
 * nlspn_backward_workspace_bytes(); a bad argument or dtype gives 0.
 */
size_t nlspn_backward_workspace_bytes(int B, int H, int W, int kh, int kw);
size_t nlspn_backward_workspace_bytes_dtype(int dtype, int B, int H, int W, int kh, int kw, int T);
int nlspn_propagate_backward(int dtype, const void *pred_init, const void *dep, const void *conf,
                             const void *aff_raw, int64_t aff_bstride,
                             const void *off_raw, int64_t off_bstride, const float *gamma,
                             const void *pred_inter, const void *aff_norm, const void *conf_eff,
                             const void *grad_pred, const void *grad_pred_inter,
                             void *grad_pred_init, void *grad_conf, void *grad_aff_raw,
                             int64_t grad_aff_bstride, void *grad_off_raw,
                             int64_t grad_off_bstride, float *grad_gamma, void *workspace,
                             int B, int H, int W, int kh, int kw, int T, int kind,
                             unsigned flags, void *stream);

/*
 * Backward of nlspn_prop_step (float32 or float16 storage, raw offsets or the no-offset
 * branch): what
 * autograd computes through one loop iteration, src/model/nlspnmodel.py:350-361, with
 * the DCNv2 backward of its _propagate_once (modulated_deform_conv_cuda.cu:124-280).
 * Used by the ConvGRU mode, where every iteration has its own affinity (:365-373).
 * Inputs are the step's inputs (feat, conf, dep, aff with (K+1) planes, raw offsets)
 * and grad_out = dL/d(step output).  Writes grad_feat and grad_conf (iff conf),
 * grad_aff ((K+1) planes per item, contiguous; plane K/2 is 0 because the step
 * recomputes that tap as 1 - sum of the others, so chaining it into
 * nlspn_affinity_normalize_backward gives the reference's _aff_insert gradient) and
 * grad_off (2K planes per item, contiguous).  workspace:
 * nlspn_prop_step_backward_workspace_bytes() bytes.  NLSPN_DTYPE_F16: operands and
 * gradients are halves, each gradient element the float32 value rounded once; the
 * workspace is nlspn_prop_step_backward_workspace_bytes_dtype() bytes
 * (4 * B*H*W * (3K + 4): the float gradient planes before the rounding), which for
 * NLSPN_DTYPE_F32 equals the function above; a bad argument or dtype gives 0.
 */
size_t nlspn_prop_step_backward_workspace_bytes(int B, int H, int W);
size_t nlspn_prop_step_backward_workspace_bytes_dtype(int dtype, int B, int H, int W, int kh, int kw);
int nlspn_prop_step_backward(int dtype, const void *feat, const void *conf, const void *dep,
                             const void *aff, int64_t aff_bstride, const void *off_raw,
                             int64_t off_bstride, const void *grad_out, void *grad_feat,
                             void *grad_conf, void *grad_aff, void *grad_off, void *workspace,
                             int B, int H, int W, int kh, int kw, unsigned flags, void *stream);

/*
 * Backward of nlspn_affinity_normalize (_affinity_normalization + _aff_insert,
 * src/model/nlspnmodel.py:179-201, :261-269): grad_aff is dL/d(output), (K+1) planes
 * per item, contiguous; writes grad_aff_raw (K planes per item, contiguous) and, for
 * TGASS, grad_gamma (1 float, summed in a fixed order; 0 for other kinds; may be
 * NULL).  workspace: nlspn_affinity_normalize_backward_workspace_bytes() bytes.
 * NLSPN_DTYPE_F16: aff_raw, grad_aff and grad_aff_raw are halves (float32 arithmetic,
 * one rounding per element); gamma, grad_gamma and the workspace are as for float32.
 */
size_t nlspn_affinity_normalize_backward_workspace_bytes(int B, int K, int H, int W);
int nlspn_affinity_normalize_backward(int dtype, const void *aff_raw, int64_t aff_bstride,
                                      const float *gamma, const void *grad_aff, void *grad_aff_raw,
                                      float *grad_gamma, void *workspace, int B, int K, int H,
                                      int W, int kind, void *stream);

/*
 * Modulated DCNv2 forward, seam 2 of the drop-in (the `DCN` pybind module,
 * src/model/deformconv/src/vision.cpp:9, modulated_deform_conv.h:10-44,
 * cuda/modulated_deform_conv_cuda.cu:19-121), as one direct (GEMM-free) gather
 * kernel.  dtype: float32, float16 (float arithmetic) or float64 (double
 * arithmetic, .cu:93's AT_DISPATCH_FLOATING_TYPES).  All tensors contiguous NCHW.
 *   input (B,C,H,W), weight (Cout, C/group, kh, kw), bias (Cout) or NULL,
 *   offset (B, 2*dg*kh*kw, Ho, Wo), mask (B, dg*kh*kw, Ho, Wo),
 *   output (B, Cout, Ho, Wo) with Ho = (H + 2ph - (dh(kh-1)+1))/sh + 1 (.cu:75-76).
 * Unlike the reference there is no im2col_step batch-divisibility restriction
 * (.cu:58-60); im2col_step is accepted and ignored.
 */
int nlspn_mdcn_forward(int dtype, const void *input, const void *weight, const void *bias,
                       const void *offset, const void *mask, void *output,
                       int B, int C, int H, int W, int Cout, int kh, int kw,
                       int sh, int sw, int ph, int pw, int dh, int dw,
                       int group, int deformable_group, void *stream);

/*
 * Modulated DCNv2 backward, seam 2 (DCN.modulated_deform_conv_backward,
 * src/model/deformconv/src/vision.cpp:10, modulated_deform_conv.h:46-86,
 * cuda/modulated_deform_conv_cuda.cu:124-280), float32 or float64 (dtype
 * NLSPN_DTYPE_F64: double arithmetic throughout, as the reference's
 * AT_DISPATCH_FLOATING_TYPES at .cu:221 — what gradcheck runs in).  Same layouts as
 * nlspn_mdcn_forward; grad_output (B, Cout, Ho, Wo).  Writes grad_input (zeroed
 * here, then scattered with atomics as the reference's col2im, so its last
 * bits depend on arrival order), grad_offset, grad_mask, grad_weight and — if
 * non-NULL — grad_bias.  Reproduces the reference's col2im call passing pad_h for
 * pad_w (.cuh:371): identical results for square padding, the reference's own
 * (shifted) grad_input otherwise.  No im2col_step batch-divisibility restriction.
 */
int nlspn_mdcn_backward(int dtype, const void *input, const void *weight, const void *offset,
                        const void *mask, const void *grad_output, void *grad_input,
                        void *grad_offset, void *grad_mask, void *grad_weight, void *grad_bias,
                        int B, int C, int H, int W, int Cout, int kh, int kw,
                        int sh, int sw, int ph, int pw, int dh, int dw,
                        int group, int deformable_group, void *stream);

/*
 * Diagnostics (not part of the reference surface): enqueue `reps` back-to-back
 * nlspn_prop_step launches on `stream`, each bracketed by its own HIP event
 * pair recorded by the dispatch itself (hipExtLaunchKernelGGL start/stop
 * events), then synchronise and return the mean and min per-launch kernel
 * duration in ms.  Used by bench.py for the roofline's kernel time.
 */
int nlspn_time_prop_step(int dtype, const void *p_in, const void *conf, const void *dep,
                         const void *aff, int64_t aff_bstride,
                         const void *off, int64_t off_bstride, int off_layout,
                         void *p_out, int B, int H, int W, int kh, int kw, unsigned flags,
                         int reps, void *stream, float *mean_ms, float *min_ms);

/*
 * Diagnostics: run nlspn_propagate `reps` times with dispatch-recorded HIP events
 * around every launch, synchronise, and return the mean duration of step 1
 * (first_ms) and of iterations 2..T (rest_ms: from the start of the first
 * resident launch to the end of the last, or the sum of the T-1 step kernels);
 * *resident = the number of resident launches (image groups), 0 for step launches,
 */
int nlspn_time_propagate(int dtype, const void *pred_init, const void *dep, const void *conf,
                         const void *aff_raw, int64_t aff_bstride, const void *off_raw,
                         int64_t off_bstride, const float *gamma, void *pred_inter, void *pred,
                         void *aff_out, void *off_out, void *conf_out, void *workspace,
                         int B, int H, int W, int kh, int kw, int T, int kind, unsigned flags,
                         int reps, void *stream, float *first_ms, float *rest_ms, int *resident);

/*
 * The propagation loop (nlspnmodel.py:340-381) from already-prologued inputs: p0
 * (iteration 1's input), conf_eff (the blended confidence, or NULL), aff_norm
 * (B x (K+1) planes, normalised, reference tap inserted), off_ins (B x 2(K+1)
 * planes, _off_insert layout) — the outputs of nlspn_head_epilogue_prologue or of
 * nlspn_propagate's step 1.  Writes pred_inter (T x B planes) and pred as
 * nlspn_propagate does (same kernels: iteration 1 a plain step, 2..T resident where it
 * applies); workspace as nlspn_propagate's.
 */
int nlspn_propagate_normalized(int dtype, const void *p0, const void *dep, const void *conf_eff,
                               const void *aff_norm, const void *off_ins, void *pred_inter,
                               void *pred, void *workspace, int B, int H, int W, int kh,
                               int kw, int T, unsigned flags, void *stream);

/*
 * Diagnostics: 1 if nlspn_propagate would run iterations 2..T as the resident
 * kernel for this shape (given 16-B aligned planes and a workspace), with the
 * launch shape of its first image group; 0 otherwise.  Queries the current
 * device's CU count.
 */
int nlspn_resident_config(int dtype, int B, int H, int W, int kh, int kw, int T, int has_conf,
                          int *grid, int *block, int *lds_bytes);

/*
 * Diagnostics: 1 if the resident launches of an nlspn_propagate call of this shape
 * (16-B aligned planes, raw offsets, a workspace; off_out given iff has_off_out) carry
 * the helper wave that copies the output dict's inserted offsets (one wave behind the
 * quad-owning threads nlspn_resident_config reports; NLSPN_RES_HELPER=0 in the
 * environment keeps the main waves' copy), 0 otherwise.  *block (optional): the
 * threads per workgroup the first resident launch is given, 0 without a resident plan.
 */
int nlspn_resident_helper(int dtype, int B, int H, int W, int kh, int kw, int T, int has_conf,
                          int has_off_out, int *block);

/*
 * Sticky abort status of the resident path on the current device: 1 if a resident
 * launch aborted since the last clear (a part polled past its spin limit, i.e. the
 * grid was not co-resident — e.g. a concurrent resident launch from another
 * process; launches from this process are serialised per device across streams).
 * Such a launch fills the outputs it had not written with NaN.  Reads a
 * host-mapped word the kernel writes: never synchronises, so the host sees an
 * abort once the launch has finished.  Sets nlspn_last_error (NLSPN_EABORTED).
 * clear != 0 resets the word after reading it.  Replaces nothing in the
 * reference, whose kernels only printf launch errors (.cuh:348-352); the torch
 * layer raises RuntimeError on it, as c10::Error surfaces in the reference.
 */
int nlspn_resident_status(int clear);

/*
 * GRU-mode convolutions (the reference's forced default mode, src/config.py:225-228): one
 * convolution of a GRU-mode iteration, f32 NCHW, inference (nlspnmodel.py:365-373), on the
 * f32-input matrix cores with bias and activation in the epilogue (csrc/nlspn_gconv.h).
 * Replaces the torch/MIOpen module calls of
 *   encode_dep / encode_aff   (:127-138)  NLSPN_GC_S2 / NLSPN_GC_S2_C16: 3x3 stride 2 pad 1
 *   ConvGRU                   (:386-403)  NLSPN_GC_GRU1 then NLSPN_GC_GRU2
 *   decode_aff + _clip_as     (:140-143, :228-250)  NLSPN_GC_T2 / NLSPN_GC_T2_C16: 3x3
 *                                          transposed stride 2 pad 1 output pad 1
 * x0 (c0 channels) then x1 (c1 channels, may be null with c1 = 0) are the input channels
 * (torch.cat order, read in place; with c1 > 0, c0 must be a multiple of 16: a chunk of
 * input channels is staged from one source, else NLSPN_EINVAL); Hi x Wi the input size.  wpk: the weights packed by
 * nlspn_gconv_pack_layout's layout (nlspn_eccv20_amd/gru.py packs them), bias padded to
 * the co tiles.  NLSPN_GC_S2* / NLSPN_GC_T2*: y = act(conv + bias) stored as (B, cout, ohs,
 * ows) (ohs / ows <= the full output size: the crop), act NLSPN_GC_ACT_*, inputs divided by
 * in_div while read (encode_dep's new_pred / max_depth; 1: none; != 1 only with
 * NLSPN_GC_S2_SMALL, else NLSPN_EINVAL).  NLSPN_GC_GRU1 (x0 = h, x1
 * = x, cout = 3 hc): z, r*h and qx (convq's x half + bias) into zb / rhb / qxb;
 * NLSPN_GC_GRU2 (x0 = rhb, c1 = 0, cout = hc): h' = (1 - z) h + z tanh(convq's r*h half +
 * qx) into hout.  Returns NLSPN_EUNSUPPORTED when a shape's window does not fit the kernel.
 */
#define NLSPN_GC_S2 0
#define NLSPN_GC_S2_C16 1
#define NLSPN_GC_GRU1 2
#define NLSPN_GC_GRU2 3
#define NLSPN_GC_T2 4
#define NLSPN_GC_T2_C16 5
/* the narrow first encoder convs on the VALU: wpk is then the module's own (16, cin, 3, 3)
 * weight tensor (cin <= 16) and bias its own (16) */
#define NLSPN_GC_S2_SMALL 6
/* NLSPN_GC_S2 / NLSPN_GC_GRU2 on 32-pixel tiles (their co tile, hence their packed weights):
 * nlspn_gconv switches to them by itself when 64-pixel tiles would give fewer than two
 * workgroups per CU (the 1/8-scale layers at NYU B=8) */
#define NLSPN_GC_S2_N32 23
#define NLSPN_GC_GRU2_N32 24
/* NLSPN_GC_T2_C16 (its packed weights) with the affinity normalisation in its epilogue: the
 * preset of nlspn_gconv_affnorm only (nlspn_gconv refuses it) */
#define NLSPN_GC_T2_AFF 25
#define NLSPN_GC_ACT_NONE 0
#define NLSPN_GC_ACT_RELU 1
#define NLSPN_GC_ACT_TANH 2
/* the packed weight layout of a preset: *co_tile output channels per tile, *cin_chunk input
 * channels per chunk (the packed input channel count is a multiple), *transposed */
int nlspn_gconv_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed);
int nlspn_gconv(int layer, const float *x0, int c0, const float *x1, int c1, const float *wpk,
                const float *bias, float *y, const float *h, float *zb, float *rhb, float *qxb,
                float *hout, int B, int Hi, int Wi, int cout, int ohs, int ows, int act,
                float in_div, int hc, void *stream);
/*
 * decode_aff's last layer fused with the affinity normalisation that follows it
 * (nlspnmodel.py:373 _aff_head, then :179-201 _affinity_normalization and :261-269
 * _aff_insert at the next iteration's start; replaces nlspn_gconv(NLSPN_GC_T2_C16, ...)
 * + nlspn_affinity_normalize): the K = 8 raw taps of the transposed conv (x0: (B, c0, Hi,
 * Wi), weights packed as NLSPN_GC_T2_C16, act NLSPN_GC_ACT_*) are normalised per pixel as
 * they leave the accumulators and stored as aff_out (B, K + 1, ohs, ows) with the reference
 * tap at K / 2, kind NLSPN_AFF_*, *gamma the device scalar.  Bit-equal to the two launches.
 */
int nlspn_gconv_affnorm(const float *x0, int c0, const float *wpk, const float *bias, float *aff_out,
                        const float *gamma, int kind, int B, int Hi, int Wi, int K, int ohs, int ows, int act,
                        void *stream);

/*
 * Backward of the GRU-mode convolutions (training through encode_dep -> ConvGRU ->
 * decode_aff, nlspnmodel.py:365-373; replaces the autograd of the torch/MIOpen modules).
 * f32 NCHW, no double backward.  csrc/nlspn_gconv_bwd.h; nlspn_eccv20_amd/gru.py drives them.
 *
 * Data gradient: a forward launch of the adjoint layer kind on adjoint-packed weights, with
 * the epilogue  dx = act'(ysave) * scale * sum (+ add).  Presets:
 *   NLSPN_GC_DG_T2 / _T2_C16   adjoint of a stride-2 conv (weights packed as the transposed
 *       conv of the same (Cout, Cin, 3, 3) tensor; Ho x Wo = the conv's input size, at most one
 *       row / column less than 2 Hg x 2 Wg)
 *   NLSPN_GC_DG_S2 / _S2_C16   adjoint of a stride-2 transposed conv (its (Cin, Cout, 3, 3)
 *       tensor packed as a conv's; the gradient g may be stored cropped, Hg x Wg <= 2 Ho x 2 Wo:
 *       the rows / columns past the crop read as zeros)
 *   NLSPN_GC_DG_S1             adjoint of a stride-1 conv (taps flipped, channels transposed)
 * g: (B, cg, Hg, Wg).  Output channels [0, split) go to dx0 (B, split, Ho, Wo), [split, cout) to
 * dx1 (null when split = cout); add0 / add1 (optional, laid out as dx0 / dx1, may alias them)
 * are added.  act / ysave: the activation of the layer whose OUTPUT dx is the gradient of, and
 * that saved output (B, cout, Ho, Wo): ReLU y > 0, Tanh 1 - y^2 (split = cout then).  One
 * source only: a two-source chunk that straddles its sources would read zeros.
 *
 * Weight and bias gradient: dW[cs][cl][ky][kx] = scale * sum s[b, cs, sy, sx] * l[b, cl, stride
 * sy - 1 + ky, stride sx - 1 + kx] with s the SMALL tensor (B, Cs, Hs, Ws) and l the LARGE one
 * (B, c0 + c1, Hl, Wl) = l0 then l1 (c1 may be 0; c0 % 16 == 0 otherwise), zero outside its
 * stored size.  A conv: s = output gradient, l = input; a transposed conv: s = input, l =
 * output gradient; either way dw is the module's own weight layout (Cs, c0 + c1, 3, 3).  db
 * (optional): the per-channel sum of s, or of l0 with bias_from_large.  K (pixels) is split
 * over workgroups that write f32 slabs into the workspace
 * (nlspn_gconv_wgrad_workspace_bytes); a second launch sums them in a fixed order: no
 * atomics, bit-reproducible.
 *
 * nlspn_gconv_wgrad_bf16x3 (opt-in; csrc/nlspn_gwgrad16.h): the same call, arguments and
 * validation with the products on the bf16 matrix cores.  Each f32 operand a is split while
 * staging into hi = bf16(a), lo = bf16(a - hi) (round to nearest even) and the kernel sums
 * s_hi l_hi + s_hi l_lo + s_lo l_hi in f32: a term is off by at most 2^-15 |s l|.  Slabs,
 * slab reduce, scale and db are the f32 entry's (db is bit-equal); its workspace query is
 * nlspn_gconv_wgrad_bf16x3_workspace_bytes.  Nothing is clamped (an inf operand gives NaN).
 * Shapes with both channel counts <= 16 are forwarded to nlspn_gconv_wgrad, bit for bit.
 *
 * nlspn_gconv_wgrad_narrow (opt-in; csrc/nlspn_gwnarrow.h): the same call, arguments and
 * validation for the stride-2 layers whose channel counts are both <= 16 and whose large tensor
 * is one source (nlspn_gconv_wgrad_narrow_covers(stride, Cs, c0, c1) = 1): exact f32 products
 * and f32 sums by a kernel that streams each large row once, with db from the operand it has
 * staged, and one two-level fixed-order reduce: two launches, no atomics, bit-reproducible, the
 * bits a function of the shape alone.  Operands need 4-byte alignment only.  Any other shape
 * is forwarded to nlspn_gconv_wgrad, bit for bit; nlspn_gconv_wgrad_narrow_workspace_bytes is
 * then that entry's size.
 *
 * ConvGRU: nlspn_gconv_gru_train is the NLSPN_GC_GRU1 (stage 1: x0 = h, x1 = x, also stores r
 * into rb) / NLSPN_GC_GRU2 (stage 2: x0 = r*h, also stores q into qb) launch of nlspn_gconv,
 * bit-identical in its other outputs.  nlspn_gconv_gru_gates_backward: stage 1 du_q = dh' z
 * (1 - q^2), du_z = dh' (q - h) z (1 - z) (duzr: (B, 2 hc, H, W) = [du_z, du_r]); stage 2 du_r =
 * d(rh) h r (1 - r), dh = dh' (1 - z) + d(rh) r; stage 0 a plain activation derivative, duq =
 * dhn * act'(z) on B * hc * H * W elements.
 */
#define NLSPN_GC_DG_T2 32
#define NLSPN_GC_DG_T2_C16 33
#define NLSPN_GC_DG_S2 34
#define NLSPN_GC_DG_S2_C16 35
#define NLSPN_GC_DG_S1 36
int nlspn_gconv_dgrad(int layer, const float *g, int cg, const float *wpk, const float *ysave, const float *add0,
                      const float *add1, float *dx0, float *dx1, int split, int B, int Hg, int Wg, int cout, int Ho,
                      int Wo, int act, float scale, void *stream);
size_t nlspn_gconv_wgrad_workspace_bytes(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl);
int nlspn_gconv_wgrad(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1, float *dw,
                      float *db, int bias_from_large, float scale, void *workspace, int64_t workspace_bytes, int B,
                      int Hs, int Ws, int Hl, int Wl, void *stream);
size_t nlspn_gconv_wgrad_bf16x3_workspace_bytes(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl);
int nlspn_gconv_wgrad_bf16x3(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1,
                             float *dw, float *db, int bias_from_large, float scale, void *workspace,
                             int64_t workspace_bytes, int B, int Hs, int Ws, int Hl, int Wl, void *stream);
int nlspn_gconv_wgrad_narrow_covers(int stride, int Cs, int c0, int c1);
size_t nlspn_gconv_wgrad_narrow_workspace_bytes(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl);
int nlspn_gconv_wgrad_narrow(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1,
                             float *dw, float *db, int bias_from_large, float scale, void *workspace,
                             int64_t workspace_bytes, int B, int Hs, int Ws, int Hl, int Wl, void *stream);
int nlspn_gconv_gru_train(int stage, const float *x0, const float *x1, int c1, const float *wpk, const float *bias,
                          const float *h, float *zb, float *rhb, float *qxb, float *hout, float *rb, float *qb, int B,
                          int H, int W, int hc, void *stream);
int nlspn_gconv_gru_gates_backward(int stage, const float *dhn, const float *z, const float *r, const float *q,
                                   const float *h, const float *drh, float *duq, float *duzr, float *dh, int act, int B,
                                   int hc, int H, int W, void *stream);

/*
 * GRU-mode convolutions on the f16 matrix cores, inference only, opt-in (csrc/nlspn_gconv16.h;
 * NLSPNModel.gru_precision = "fp16").  The same layers as nlspn_gconv on
 * v_mfma_f32_16x16x32_f16.  Numerics contract:
 *   - MFMA operands are IEEE half: weights rounded to nearest-even once, when packed;
 *     activations rounded once, in the epilogue of the layer that produces them (a plain
 *     conversion: overflow gives inf, NaN is kept); no clamping anywhere;
 *   - products are exact in f32 (11 + 11 significand bits), accumulation is f32 inside the MFMA;
 *   - every epilogue (bias, ReLU, tanhf, sigmoid, the GRU blend) runs in f32 on the f32
 *     accumulators, exactly as nlspn_gconv's;
 *   - the ConvGRU state h is carried in f32 (every step also writes the f16 copy the next
 *     convolutions read); z and qx stay f32; r*h is formed in f32 and stored as f16.
 * Activation layout "c8": a (B, C, H, W) tensor as [B][ceil(C/8)][H][W][8] halves, pad channels
 * zero (one window cell of eight channels = 16 bytes = one B fragment of the MFMA).  Weights:
 * per co tile [ci/8][tap][co][8] halves (transposed: per output phase, the phases one after
 * another), input channels padded to *cin_chunk (nlspn_gconv16_pack_layout; gru.py pack_conv16
 * / pack_convt16); bias f32, padded to the co tiles.
 *
 * nlspn_gconv16(layer, ...): x0 (c0 channels) then x1 (c1 channels, null with c1 = 0) in c8
 * (NLSPN_GC16_S2_SMALL: x0 f32 NCHW, wpk the module's own f32 (16, cin, 3, 3) tensor); with
 * c1 > 0, c0 must be a multiple of the chunk (a chunk is staged from one source), else
 * NLSPN_EINVAL.  Kinds:
 *   NLSPN_GC16_S2_SMALL  1 / 9 -> 16 stride 2 on the VALU, nlspn_gconv's arithmetic (f32
 *                        operands and sums, in_div); y16 only
 *   NLSPN_GC16_S2        3x3 stride 2 pad 1; y16 (c8) and / or y32 (f32 NCHW), act
 *   NLSPN_GC16_GRU1      x0 = h as c8, x1 = x, cout = 3 hc; reads h (f32); writes zb (f32),
 *                        rh16 (c8), qxb (f32)
 *   NLSPN_GC16_GRU2      x0 = rh16, cout = hc; reads h, zb, qxb (f32); writes hout32 (f32) and
 *                        hout16 (c8), both required
 *   NLSPN_GC16_T2 / NLSPN_GC16_T2_C16   transposed 3x3 stride 2 (64- / 16-channel co tile);
 *                        y16 and / or y32, cropped to ohs x ows
 * y16: (B, ceil(cout/8), ohs, ows, 8) halves; y32: (B, cout, ohs, ows) floats; either may be
 * null, not both.  NLSPN_EINVAL before any device call for null required pointers, a preset
 * that is not NLSPN_GC16_*, both outputs null, an output the kind does not write, in_div != 1
 * outside NLSPN_GC16_S2_SMALL and a chunk that would straddle the two sources;
 * NLSPN_EUNSUPPORTED for a grid no tile fits.
 */
#define NLSPN_GC16_S2 48
#define NLSPN_GC16_GRU1 49
#define NLSPN_GC16_GRU2 50
#define NLSPN_GC16_T2 51
#define NLSPN_GC16_T2_C16 52
#define NLSPN_GC16_S2_SMALL 53
int nlspn_gconv16_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed);
int nlspn_gconv16(int layer, const void *x0, int c0, const void *x1, int c1, const void *wpk, const float *bias,
                  void *y16, float *y32, const float *h, float *zb, void *rh16, float *qxb, float *hout32,
                  void *hout16, int B, int Hi, int Wi, int cout, int ohs, int ows, int act, float in_div, int hc,
                  void *stream);

/*
 * GRU-mode convolutions on the bf16 matrix cores with split operands, inference only, opt-in
 * (csrc/nlspn_gconv_x3.h; NLSPNModel.gru_precision = "bf16x3").  The same layers as nlspn_gconv
 * on v_mfma_f32_16x16x32_bf16.  Numerics contract:
 *   - every MFMA operand value a (f32) is the pair hi = rne_bf16(a), lo = rne_bf16(a - hi), the
 *     subtraction in f32; weights are split once, when packed; activations once, from the f32
 *     value the producing layer's epilogue holds;
 *   - per output element the kernel accumulates sum (w_hi x_hi + w_hi x_lo + w_lo x_hi) in the
 *     MFMAs' f32 accumulators (the third product on v_mfma_f32_16x16x16_bf16); lo lo is dropped;
 *     bf16 x bf16 products are exact in f32;
 *   - |a - hi| <= 2^-8 |a| and |a - hi - lo| <= 2^-17 |a|: a term is off by at most
 *     (2^-17 + 2^-17 + 2^-16) |w x| = 2^-15 |w x| before accumulation rounding;
 *   - every epilogue (bias, ReLU, tanhf, sigmoid, the GRU blend) runs in f32 on the accumulators
 *     with nlspn_gconv's device functions; the ConvGRU state h is carried in f32 beside its
 *     split copy; z and qx stay f32; r*h is formed in f32 and stored split;
 *   - the 1 / 9 -> 16 first encoder layers keep the VALU kernel's f32 arithmetic (their output
 *     is the f32 kernel's value, split); the last decoder layer stays nlspn_gconv_affnorm on the
 *     f32 NCHW output of the layer before it;
 *   - nothing is clamped: non-finite inputs give non-finite outputs, not necessarily of the f32
 *     kernel's kind (inf has lo = NaN); no atomics and no waiting between workgroups: the same
 *     bits on every run.
 * Activation layout "c8x2": a (B, C, H, W) tensor as [B][ceil(C/8)][2][H][W][8] bf16, pad
 * channels zero: per 8-channel block the hi cells' plane, then the lo cells'.  Weights: per co
 * tile [cell block][tap][co][8] bf16 with cell block 2 (ci/8) + part (transposed: per output
 * phase, the phases one after another), input channels padded to *cin_chunk (16)
 * (nlspn_gconv_x3_pack_layout; gru.py pack_conv_x3 / pack_convt_x3); bias f32, padded to the
 * co tiles.
 *
 * nlspn_gconv_x3(layer, ...): nlspn_gconv16's arguments, the half pointers (x0, x1, ys, rhs,
 * houts) pointing to c8x2 tensors (NLSPN_GCX3_S2_SMALL: x0 f32 NCHW, wpk the module's own f32
 * (16, cin, 3, 3) tensor).  The kinds NLSPN_GCX3_* read and write what their NLSPN_GC16_*
 * namesakes do, and the same calls are refused with NLSPN_EINVAL before any device call: null
 * required pointers, a preset that is not NLSPN_GCX3_*, both outputs null, an output the kind
 * does not write, in_div != 1 outside NLSPN_GCX3_S2_SMALL, c0 not a multiple of the 16-channel
 * chunk with two sources (the straddle case), hc not a multiple of the co tile;
 * NLSPN_EUNSUPPORTED for a grid no tile fits.
 */
#define NLSPN_GCX3_S2 64
#define NLSPN_GCX3_GRU1 65
#define NLSPN_GCX3_GRU2 66
#define NLSPN_GCX3_T2 67
#define NLSPN_GCX3_T2_C16 68
#define NLSPN_GCX3_S2_SMALL 69
int nlspn_gconv_x3_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed);
int nlspn_gconv_x3(int layer, const void *x0, int c0, const void *x1, int c1, const void *wpk, const float *bias,
                   void *ys, float *y32, const float *h, float *zb, void *rhs, float *qxb, float *hout32,
                   void *houts, int B, int Hi, int Wi, int cout, int ohs, int ows, int act, float in_div, int hc,
                   void *stream);

/*
 * Data gradients of the GRU-mode convolutions on the split-bf16 family, training, opt-in
 * (csrc/nlspn_gconv_x3.h, the kGcEpiDact epilogue; NLSPNModel.gru_dgrad_precision = "bf16x3").
 * nlspn_gconv_dgrad's launches (a forward launch of the adjoint layer kind with the derivative
 * epilogue) with the gradient read as c8x2 and the adjoint weights packed split.  Numerics
 * contract, beside the one above: per output element
 *     dx = act'(ysave) * scale * sum (w_hi g_hi + w_hi g_lo + w_lo g_hi) (+ add),
 * the sum in the MFMAs' f32 accumulators, the epilogue in f32 with nlspn_gconv_dgrad's
 * arithmetic; a term is off by at most 2^-15 |w g| before accumulation rounding; nothing is
 * clamped; no atomics and no waiting between workgroups: the same bits on every run.
 * Presets (weights: nlspn_gconv_x3_dgrad_pack_layout; gru.py pack_adjoint_x3 / pack_adjoint_s1_x3):
 *   NLSPN_GCX3_DG_T2       adjoint of a stride-2 conv, 64-channel co tile (NLSPN_GCX3_T2's tiling)
 *   NLSPN_GCX3_DG_T2_C16   the same, 16-channel co tile (NLSPN_GCX3_T2_C16's tiling)
 *   NLSPN_GCX3_DG_S2       adjoint of a stride-2 transposed conv (NLSPN_GCX3_S2's tiling)
 *   NLSPN_GCX3_DG_S1       adjoint of a stride-1 conv (NLSPN_GCX3_GRU2's tile, plain epilogue)
 * nlspn_gconv_x3_dgrad: nlspn_gconv_dgrad's arguments with gs the gradient (B, cg, Hg, Wg) as
 * c8x2 and wpk bf16; ysave, add0, add1, dx0, dx1 stay f32 NCHW (add0 / add1 may alias dx0 / dx1).
 * dxs (optional; needs split = cout): dx0's values split into a c8x2 tensor (B, ceil(cout/8), 2,
 * Ho, Wo, 8), what the next data gradient of a chain reads.  Validation is nlspn_gconv_dgrad's
 * (NLSPN_EINVAL: null pointers, a preset that is not NLSPN_GCX3_DG_*, split / second output
 * mismatch, dxs with two outputs, an activation without ysave or with two outputs, an output
 * size that does not belong to the gradient, a problem too large for 32-bit offsets);
 * NLSPN_EUNSUPPORTED for what the family does not serve and nlspn_gconv_dgrad does: a
 * stride-2-mode gradient stored cropped (Hg != 2 Ho or Wg != 2 Wo), a gradient of at most 16
 * channels (cg <= 16, whatever cout: the problems with both channel counts <= 16 and, by
 * measurement, the 2hc -> 16 decoder layer's adjoint), a grid no tile fits.  nlspn_gconv_x3_dgrad_covers answers 1 exactly for the
 * shapes the entry serves (no device call, no error text).
 * nlspn_gconv_x3_split: f32 (B, C, H, W) -> c8x2 (B, ceil(C/8), 2, H, W, 8), pad channels zero,
 * every value split as the kernels' epilogues split it (bit-equal to gru.py to_c8x2): where a
 * gradient enters a chain in f32.  x needs 4-byte alignment only, xs 16-byte.
 */
#define NLSPN_GCX3_DG_T2 80
#define NLSPN_GCX3_DG_T2_C16 81
#define NLSPN_GCX3_DG_S2 82
#define NLSPN_GCX3_DG_S1 83
int nlspn_gconv_x3_split(const float *x, void *xs, int B, int C, int H, int W, void *stream);
int nlspn_gconv_x3_dgrad_covers(int layer, int cg, int cout, int Hg, int Wg, int Ho, int Wo);
int nlspn_gconv_x3_dgrad(int layer, const void *gs, int cg, const void *wpk, const float *ysave, const float *add0,
                         const float *add1, float *dx0, float *dx1, int split, void *dxs, int B, int Hg, int Wg,
                         int cout, int Ho, int Wo, int act, float scale, void *stream);
int nlspn_gconv_x3_dgrad_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed);

#ifdef __cplusplus
}
#endif

#endif /* NLSPN_PROP_H */
