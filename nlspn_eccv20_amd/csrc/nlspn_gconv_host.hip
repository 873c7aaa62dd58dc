// C ABI of the GRU-mode convolutions (see include/nlspn_prop.h): preset lookup, tiling and
// launch of the implicit-GEMM kernels, which are instantiated in nlspn_kern_gconv.hip.
#include <algorithm>

#include "nlspn_host.h"
#include "nlspn_gconv_bwd.h"
#include "nlspn_gconv16.h"
#include "nlspn_gwgrad16.h"

namespace nlspn {
// defined in nlspn_kern_gconv.hip
#define NLSPN_GC_EXTERN(id, ...) extern template __global__ void gconv_kernel<__VA_ARGS__>(GconvArgs);
NLSPN_GC_CONFIGS(NLSPN_GC_EXTERN)
extern template __global__ void gsmall_kernel<16>(GconvArgs, const float *);
// defined in nlspn_kern_gconv_bwd.hip
NLSPN_GC_DG_CONFIGS(NLSPN_GC_EXTERN)
#define NLSPN_GW_EXTERN(...) extern template __global__ void gwgrad_kernel<__VA_ARGS__>(GwgradArgs);
NLSPN_GW_CONFIGS(NLSPN_GW_EXTERN)
// defined in nlspn_kern_gconv16.hip
#define NLSPN_GC16_EXTERN(id, ...) extern template __global__ void gconv16_kernel<__VA_ARGS__>(Gconv16Args);
NLSPN_GC16_CONFIGS(NLSPN_GC16_EXTERN)
extern template __global__ void gsmall16_kernel<16>(Gconv16Args, const float *);
// defined in nlspn_kern_gwgrad16.hip
#define NLSPN_GW16_EXTERN(...) extern template __global__ void gwgrad16_kernel<__VA_ARGS__>(GwgradArgs);
NLSPN_GW16_CONFIGS(NLSPN_GW16_EXTERN)
}  // namespace nlspn

using namespace nlspn;

namespace {
struct GcPreset {
    const void *fn;
    int mode, wgco, npx, xr, xp, lds, epi;
};
template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CC, int EPI>
GcPreset gc_preset() {
    using Cfg = GcCfg<MODE, WM, WN, WGM, WGN, XR, XP, CC, EPI>;
    return GcPreset{reinterpret_cast<const void *>(&gconv_kernel<MODE, WM, WN, WGM, WGN, XR, XP, CC, EPI>), MODE,
                    Cfg::WGCO, Cfg::NPX, XR, XP, (int)(Cfg::LDS_FLOATS * sizeof(float)), EPI};
}
bool gc_get(int layer, GcPreset &p) {
    switch (layer) {
#define NLSPN_GC_CASE(id, ...) \
    case id: p = gc_preset<__VA_ARGS__>(); return true;
        NLSPN_GC_CONFIGS(NLSPN_GC_CASE)
        NLSPN_GC_DG_CONFIGS(NLSPN_GC_CASE)
        default: return false;
    }
}
}  // namespace
extern "C" {

int nlspn_gconv_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed) {
    if (layer == NLSPN_GC_S2_SMALL) {  // the module's own weight layout
        if (co_tile) *co_tile = 0;
        if (cin_chunk) *cin_chunk = 1;
        if (transposed) *transposed = 0;
        return NLSPN_OK;
    }
    GcPreset p;
    if (!gc_get(layer, p)) return fail(NLSPN_EINVAL, "unknown GRU-mode conv preset %d", layer);
    if (co_tile) *co_tile = p.wgco;
    if (cin_chunk) *cin_chunk = kGcCP;
    if (transposed) *transposed = p.mode == kGcT2;
    return NLSPN_OK;
}

}  // extern "C"
namespace {
// the pixel tiling of a launch (a.Hi / a.Wi / a.Ho / a.Wo set): column bands and tiles per band
// (gc_tile, nlspn_gconv_plan.h)
int gc_tile(const GcPreset &p, GconvArgs &a) {
    GcTiling t;
    const bool ok = nlspn::gc_tile(GcGeo{p.mode, p.wgco, p.npx, p.xr, p.xp}, p.mode == kGcT2 ? a.Hi : a.Ho,
                                   p.mode == kGcT2 ? a.Wi : a.Wo, t);
    a.gh = t.gh; a.gw = t.gw; a.bw = t.bw; a.nbands = t.nbands; a.tpb = t.tpb; a.npx = t.npx;
    if (!ok)
        return fail(NLSPN_EUNSUPPORTED, "gconv: a tile of a %d-wide band spans more than %d window rows", a.bw, p.xr);
    return NLSPN_OK;
}

// nlspn_gconv, and with gamma / aff_kind nlspn_gconv_affnorm (preset NLSPN_GC_T2_AFF)
int gconv_impl(int layer, const float *x0, int c0, const float *x1, int c1, const float *wpk, const float *bias,
               float *y, const float *h, float *zb, float *rhb, float *qxb, float *hout, int B, int Hi, int Wi,
               int cout, int ohs, int ows, int act, float in_div, int hc, const float *gamma, int aff_kind,
               void *stream, float *rb = nullptr, float *qb = nullptr) {
    if (layer == NLSPN_GC_S2_SMALL) {
        // (the kernel reads the module's own (16, cin, 3, 3) tensor)
        if (B < 1 || Hi < 1 || Wi < 1 || c0 < 1 || c1 != 0 || cout != 16 || c0 * 16 * 9 > kGsMaxW)
            return fail(NLSPN_EINVAL, "gconv small: cin %d (c1 %d), cout %d outside the VALU kernel's range (cout 16, "
                        "cin <= 16)", c0, c1, cout);
        if (!x0 || !wpk || !bias || !y) return fail(NLSPN_EINVAL, "gconv small: null pointer");
        GconvArgs a{};
        a.x0 = x0; a.bias = bias; a.y = y; a.c0 = c0; a.B = B; a.Hi = Hi; a.Wi = Wi;
        a.Ho = (Hi - 1) / 2 + 1;
        a.Wo = (Wi - 1) / 2 + 1;
        a.ohs = ohs; a.ows = ows; a.cout = cout; a.act = act; a.in_div = in_div;
        if (ohs < 1 || ows < 1 || ohs > a.Ho || ows > a.Wo)
            return fail(NLSPN_EINVAL, "gconv small: stored size %dx%d outside the output %dx%d", ohs, ows, a.Ho, a.Wo);
        const long long npix = (long long)B * ohs * ows;
        const unsigned grid = (unsigned)std::min<long long>((npix + kGsNT - 1) / kGsNT, 1 << 20);
        void *args[] = {&a, const_cast<float **>(&wpk)};
        return launch_kernel(reinterpret_cast<const void *>(&gsmall_kernel<16>), dim3(grid), dim3(kGsNT), args, 0,
                             as_stream(stream), "nlspn_gconv small");
    }
    GcPreset p;
    if (!gc_get(layer, p)) return fail(NLSPN_EINVAL, "unknown GRU-mode conv preset %d", layer);
    if (p.epi == kGcEpiDact) return fail(NLSPN_EINVAL, "gconv: preset %d is nlspn_gconv_dgrad's", layer);
    if (B < 1 || Hi < 1 || Wi < 1 || cout < 1 || c0 < 1 || c1 < 0 || (c1 > 0 && !x1))
        return fail(NLSPN_EINVAL, "gconv: bad shape B=%d Hi=%d Wi=%d c0=%d c1=%d cout=%d", B, Hi, Wi, c0, c1, cout);
    if (!x0 || !wpk || !bias) return fail(NLSPN_EINVAL, "gconv: null input, weights or bias");
    // (a chunk of input channels is staged from one source: a chunk over x0's last channels
    // would read zeros past them and the next one start past x1's first channels)
    if (c1 > 0 && c0 % kGcCP != 0)
        return fail(NLSPN_EINVAL, "gconv: a channel chunk would straddle the two sources (c0 = %d, not a multiple of %d)",
                    c0, kGcCP);
    // (the MFMA kernels stage their inputs by LDS-DMA, untouched: a divided input is the VALU
    // kernel's, NLSPN_GC_S2_SMALL)
    if (in_div != 1.f) return fail(NLSPN_EINVAL, "gconv: in_div %g needs the NLSPN_GC_S2_SMALL preset", (double)in_div);
    const bool gru = p.epi == kGcEpiGru1 || p.epi == kGcEpiGru2, gru1 = p.epi == kGcEpiGru1;
    if ((p.epi == kGcEpiAff) != (gamma != nullptr))
        return fail(NLSPN_EINVAL, "gconv: preset %d %s", layer,
                    gamma ? "has no affinity epilogue" : "is nlspn_gconv_affnorm's (needs gamma)");
    if (p.epi == kGcEpiAff && (cout != 8 || aff_kind < NLSPN_AFF_AS || aff_kind > NLSPN_AFF_TGASS))
        return fail(NLSPN_EINVAL, "gconv affnorm: K = %d raw taps (supported 8), kind %d", cout, aff_kind);
    GconvArgs a{};
    a.x0 = x0; a.x1 = x1; a.w = wpk; a.bias = bias; a.y = y;
    a.h = h; a.zb = zb; a.rhb = rhb; a.qxb = qxb; a.hout = hout;
    a.rb = rb; a.qb = qb;
    a.c0 = c0; a.c1 = c1; a.cin_pad = (c0 + c1 + kGcCP - 1) / kGcCP * kGcCP;
    a.B = B; a.Hi = Hi; a.Wi = Wi;
    if (p.mode == kGcS1) { a.Ho = Hi; a.Wo = Wi; }
    else if (p.mode == kGcS2) { a.Ho = (Hi - 1) / 2 + 1; a.Wo = (Wi - 1) / 2 + 1; }
    else { a.Ho = 2 * Hi; a.Wo = 2 * Wi; }
    a.ohs = gru ? a.Ho : ohs;
    a.ows = gru ? a.Wo : ows;
    if (a.ohs < 1 || a.ows < 1 || a.ohs > a.Ho || a.ows > a.Wo)
        return fail(NLSPN_EINVAL, "gconv: stored size %dx%d outside the output %dx%d", a.ohs, a.ows, a.Ho, a.Wo);
    a.cout = cout;
    a.co_tiles = (cout + p.wgco - 1) / p.wgco;
    a.act = act;
    a.in_div = in_div;
    a.hc = hc;
    a.gamma = gamma;
    a.aff_kind = aff_kind;
    if (gru) {
        if (hc < 1 || hc % p.wgco != 0 || !h || (gru1 ? (!zb || !rhb || !qxb || cout != 3 * hc || c0 != hc)
                                                                          : (!zb || !qxb || !hout || cout != hc || c1 != 0 || c0 != hc)))
            return fail(NLSPN_EINVAL, "gconv: GRU launch needs hc %% %d == 0, h, z / r*h / qx buffers and cout 3hc (GRU1) "
                        "or hc (GRU2)", p.wgco);
    } else if (!y) {
        return fail(NLSPN_EINVAL, "gconv: null output");
    }
    NLSPN_TRY(gc_tile(p, a));
    long long nwg = (long long)(p.mode == kGcT2 ? 4 : 1) * a.co_tiles * B * a.nbands * a.tpb;
    if (gru1) nwg = gc_gru1_wgs(a.hc, p.wgco, a.co_tiles, gc_rest_count(a.B, a.nbands, a.tpb));  // (the qx workgroups take two pixel tiles each)
    // Small grids: the same layer kind on 32-pixel tiles (the same co tile, hence the same packed
    // weights) when 64-pixel tiles would leave most CUs one workgroup (NYU B=8: the 1/8-scale last
    // encoder conv 104.1 -> 85.2 us, GRU2 52.6 -> 50.6 us; profiles/r06/gc_bench_layers_v4_n32.json)
    if ((layer == NLSPN_GC_S2 || layer == NLSPN_GC_GRU2) && nwg < 2LL * device_cus())
        return gconv_impl(layer == NLSPN_GC_S2 ? NLSPN_GC_S2_N32 : NLSPN_GC_GRU2_N32, x0, c0, x1, c1, wpk, bias, y, h,
                          zb, rhb, qxb, hout, B, Hi, Wi, cout, ohs, ows, act, in_div, hc, nullptr, 0, stream, rb, qb);
    // (one image's channels of a source within a 32-bit buffer descriptor)
    if (nwg > 0x7fffffffLL || (long long)std::max(c0, c1) * Hi * Wi * 4 > 0x7fffffffLL)
        return fail(NLSPN_EINVAL, "gconv: problem too large");
    NLSPN_TRY(set_lds_attr(p.fn, p.lds));
    void *args[] = {&a};
    return launch_kernel(p.fn, dim3((unsigned)nwg), dim3(kGcNT), args, (size_t)p.lds, as_stream(stream), "nlspn_gconv");
}
}  // namespace
extern "C" {

int nlspn_gconv(int layer, const float *x0, int c0, const float *x1, int c1, const float *wpk, const float *bias,
                float *y, const float *h, float *zb, float *rhb, float *qxb, float *hout, int B, int Hi, int Wi,
                int cout, int ohs, int ows, int act, float in_div, int hc, void *stream) {
    return gconv_impl(layer, x0, c0, x1, c1, wpk, bias, y, h, zb, rhb, qxb, hout, B, Hi, Wi, cout, ohs, ows, act,
                      in_div, hc, nullptr, 0, stream);
}

int nlspn_gconv_affnorm(const float *x0, int c0, const float *wpk, const float *bias, float *aff_out,
                        const float *gamma, int kind, int B, int Hi, int Wi, int K, int ohs, int ows, int act,
                        void *stream) {
    if (!gamma || !aff_out) return fail(NLSPN_EINVAL, "gconv affnorm: null gamma or output");
    return gconv_impl(NLSPN_GC_T2_AFF, x0, c0, nullptr, 0, wpk, bias, aff_out, nullptr, nullptr, nullptr, nullptr,
                      nullptr, B, Hi, Wi, K, ohs, ows, act, 1.f, 0, gamma, kind, stream);
}

// ---------------------------------------------------------------- backward (nlspn_gconv_bwd.h)
}  // extern "C"
namespace {
struct GwPreset {
    const void *fn;
    int mt, nt, nthr, lds;
};
template <int S, int WM, int WGM, int WGN>
GwPreset gw_preset() {
    using Cfg = GwCfg<S, WM, WGM, WGN>;
    return GwPreset{reinterpret_cast<const void *>(&gwgrad_kernel<S, WM, WGM, WGN>), Cfg::MT, Cfg::NT, Cfg::NTHR,
                    (int)(Cfg::LDS_FLOATS * sizeof(float))};
}
// The plan of one weight-gradient call, a pure function of the shape: the tiling by channel
// counts, the K slices so that about kGwTargetWgs workgroups run (a constant, not the device's
// CU count: the summation order, hence the bits, is the same on every device).
constexpr int kGwTargetWgs = 512, kGwMaxBiasSlices = 64;
struct GwPlan {
    GwPreset p;
    int mtiles, ntiles, nsl, bw, nbands, units, ups, nsb;
    long long slab, bias_off, floats;  // slab floats; the bias partials' offset; the workspace's floats
};
int gw_plan(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl, GwPlan &pl) {
    if (stride != 1 && stride != 2) return fail(NLSPN_EINVAL, "gconv wgrad: stride %d (supported 1, 2)", stride);
    if (B < 1 || Cs < 1 || Cl < 1 || Hs < 1 || Ws < 1 || Hl < 1 || Wl < 1)
        return fail(NLSPN_EINVAL, "gconv wgrad: bad shape B=%d Cs=%d Cl=%d small %dx%d large %dx%d", B, Cs, Cl, Hs, Ws, Hl, Wl);
    if (stride == 1 ? (Hl != Hs || Wl != Ws) : (Hl > 2 * Hs || Wl > 2 * Ws))
        return fail(NLSPN_EINVAL, "gconv wgrad: large size %dx%d does not belong to small size %dx%d at stride %d", Hl, Wl,
                    Hs, Ws, stride);
    if ((long long)B * Hs > 0x3fffffffLL / ((Ws + kGwBW - 1) / kGwBW)) return fail(NLSPN_EINVAL, "gconv wgrad: problem too large");
    pl.p = stride == 1 ? gw_preset<1, 2, 2, 2>()
           : Cl > 16   ? gw_preset<2, 2, 2, 2>()
           : Cs > 16   ? gw_preset<2, 2, 4, 1>()
                       : gw_preset<2, 1, 1, 1>();
    pl.mtiles = (Cs + pl.p.mt - 1) / pl.p.mt;
    pl.ntiles = (Cl + pl.p.nt - 1) / pl.p.nt;
    pl.nbands = (Ws + kGwBW - 1) / kGwBW;
    pl.bw = (Ws + pl.nbands - 1) / pl.nbands;
    pl.units = B * Hs * pl.nbands;
    const int tiles = pl.mtiles * pl.ntiles;
    int nsl = std::max(1, std::min(pl.units, (kGwTargetWgs + tiles - 1) / tiles));
    pl.ups = (pl.units + nsl - 1) / nsl;
    pl.nsl = (pl.units + pl.ups - 1) / pl.ups;
    pl.slab = (long long)pl.mtiles * pl.p.mt * pl.ntiles * pl.p.nt * 9;
    pl.nsb = (int)std::max(1LL, std::min<long long>(kGwMaxBiasSlices, ((long long)B * Hl * Wl + 16383) / 16384));
    pl.bias_off = pl.slab * pl.nsl;
    pl.floats = pl.bias_off + (long long)pl.nsb * std::max(Cs, Cl);
    return NLSPN_OK;
}
}  // namespace
extern "C" {

size_t nlspn_gconv_wgrad_workspace_bytes(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    GwPlan pl;
    return gw_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl, pl) ? 0 : (size_t)pl.floats * sizeof(float);
}

int nlspn_gconv_wgrad(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1, float *dw,
                      float *db, int bias_from_large, float scale, void *workspace, int64_t workspace_bytes, int B,
                      int Hs, int Ws, int Hl, int Wl, void *stream) {
    if (!s || !l0 || !dw || !workspace) return fail(NLSPN_EINVAL, "gconv wgrad: null tensor, gradient or workspace");
    if (c0 < 1 || c1 < 0 || (c1 > 0 && !l1)) return fail(NLSPN_EINVAL, "gconv wgrad: bad channels c0=%d c1=%d", c0, c1);
    // (a 16-channel block of the large tensor reads one source)
    if (c1 > 0 && c0 % 16 != 0)
        return fail(NLSPN_EINVAL, "gconv wgrad: a channel block would straddle the two sources (c0 = %d, not a multiple of 16)", c0);
    if (db && bias_from_large && c1 > 0) return fail(NLSPN_EINVAL, "gconv wgrad: the bias gradient reads one source");
    GwPlan pl;
    NLSPN_TRY(gw_plan(stride, Cs, c0 + c1, B, Hs, Ws, Hl, Wl, pl));
    if (workspace_bytes < pl.floats * (long long)sizeof(float))
        return fail(NLSPN_EINVAL, "gconv wgrad: workspace too small (%lld bytes, needs %lld)", (long long)workspace_bytes,
                    pl.floats * (long long)sizeof(float));
    GwgradArgs a{};
    a.s = s; a.l0 = l0; a.l1 = l1; a.ws = static_cast<float *>(workspace);
    a.Cs = Cs; a.c0 = c0; a.c1 = c1; a.B = B; a.Hs = Hs; a.Ws = Ws; a.Hl = Hl; a.Wl = Wl;
    a.mtiles = pl.mtiles; a.ntiles = pl.ntiles; a.nsl = pl.nsl;
    a.bw = pl.bw; a.nbands = pl.nbands; a.units = pl.units; a.ups = pl.ups;
    const int Cl = c0 + c1;
    hipStream_t st = as_stream(stream);
    NLSPN_TRY(set_lds_attr(pl.p.fn, pl.p.lds));
    void *args[] = {&a};
    NLSPN_TRY(launch_kernel(pl.p.fn, dim3((unsigned)(pl.mtiles * pl.ntiles * pl.nsl)), dim3(pl.p.nthr), args,
                            (size_t)pl.p.lds, st, "nlspn_gconv_wgrad"));
    {
        const float *wsp = a.ws;
        int n0 = Cs, n1 = Cl, n1p = pl.ntiles * pl.p.nt, T = 9, nsl = pl.nsl;
        long long slab = pl.slab;
        void *rargs[] = {&wsp, &dw, &n0, &n1, &n1p, &T, &slab, &nsl, &scale};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gwgrad_reduce_kernel),
                                dim3(elementwise_grid((long long)Cs * Cl * 9)), dim3(256), rargs, 0, st,
                                "nlspn_gconv_wgrad reduce"));
    }
    if (db) {
        const float *g = bias_from_large ? l0 : s;
        int C = bias_from_large ? Cl : Cs, nsb = pl.nsb, one = 1;
        long long HW = bias_from_large ? (long long)Hl * Wl : (long long)Hs * Ws;
        float *part = a.ws + pl.bias_off;
        void *pargs[] = {&g, &part, &C, &B, &HW, &nsb};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gbias_partial_kernel), dim3((unsigned)(C * nsb)), dim3(256),
                                pargs, 0, st, "nlspn_gconv_wgrad bias"));
        const float *cpart = part;
        long long bslab = C;
        float unit = 1.f;
        void *rargs[] = {&cpart, &db, &C, &one, &one, &one, &bslab, &nsb, &unit};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gwgrad_reduce_kernel), dim3(elementwise_grid(C)), dim3(256),
                                rargs, 0, st, "nlspn_gconv_wgrad bias reduce"));
    }
    return NLSPN_OK;
}

// ---- the split-bf16 weight gradient (nlspn_gwgrad16.h): the same call on the bf16 matrix cores
}  // extern "C"
namespace {
template <int S, int WM, int WGM, int WGN>
const void *gw16_fn(const Gw16Geo &g) {
    return g.S == S && g.wm == WM && g.wgm == WGM && g.wgn == WGN
               ? reinterpret_cast<const void *>(&gwgrad16_kernel<S, WM, WGM, WGN>) : nullptr;
}
const void *gw16_kernel_of(const Gw16Geo &g) {
    const void *fn = nullptr;
#define NLSPN_GW16_PICK(...) if (!fn) fn = gw16_fn<__VA_ARGS__>(g);
    NLSPN_GW16_CONFIGS(NLSPN_GW16_PICK)
    return fn;
}
}  // namespace
extern "C" {

size_t nlspn_gconv_wgrad_bf16x3_workspace_bytes(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    GwPlan f32;
    if (gw_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl, f32)) return 0;  // (the shape rules are the f32 entry's)
    if (gw16_choose(stride, Cs, Cl) == kGw16F32) return (size_t)f32.floats * sizeof(float);
    return (size_t)gw16_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl).floats * sizeof(float);
}

int nlspn_gconv_wgrad_bf16x3(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1,
                             float *dw, float *db, int bias_from_large, float scale, void *workspace,
                             int64_t workspace_bytes, int B, int Hs, int Ws, int Hl, int Wl, void *stream) {
    if (!s || !l0 || !dw || !workspace) return fail(NLSPN_EINVAL, "gconv wgrad: null tensor, gradient or workspace");
    if (c0 < 1 || c1 < 0 || (c1 > 0 && !l1)) return fail(NLSPN_EINVAL, "gconv wgrad: bad channels c0=%d c1=%d", c0, c1);
    if (c1 > 0 && c0 % 16 != 0)
        return fail(NLSPN_EINVAL, "gconv wgrad: a channel block would straddle the two sources (c0 = %d, not a multiple of 16)", c0);
    if (db && bias_from_large && c1 > 0) return fail(NLSPN_EINVAL, "gconv wgrad: the bias gradient reads one source");
    const int Cl = c0 + c1;
    GwPlan f32;
    NLSPN_TRY(gw_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl, f32));
    // both channel counts <= 16: the one-wave f32 kernel, bit for bit (its cost is staging, not MFMA)
    if (gw16_choose(stride, Cs, Cl) == kGw16F32)
        return nlspn_gconv_wgrad(stride, s, Cs, l0, c0, l1, c1, dw, db, bias_from_large, scale, workspace, workspace_bytes,
                                 B, Hs, Ws, Hl, Wl, stream);
    const Gw16Plan pl = gw16_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl);
    if (workspace_bytes < pl.floats * (long long)sizeof(float))
        return fail(NLSPN_EINVAL, "gconv wgrad: workspace too small (%lld bytes, needs %lld)", (long long)workspace_bytes,
                    pl.floats * (long long)sizeof(float));
    // (the kernel's per-thread staging offsets are 32 bits: a pass's 8 channel planes and one window row)
    if ((long long)pl.mtiles * pl.ntiles * pl.nsl > 0x7fffffffLL || (long long)Hs * Ws > (1LL << 27) || (long long)Hl * Wl > (1LL << 27))
        return fail(NLSPN_EINVAL, "gconv wgrad: problem too large");
    const void *fn = gw16_kernel_of(pl.g);
    if (!fn) return fail(NLSPN_EUNSUPPORTED, "gconv wgrad bf16x3: no kernel for tiling %d", pl.tiling);
    GwgradArgs a{};
    a.s = s; a.l0 = l0; a.l1 = l1; a.ws = static_cast<float *>(workspace);
    a.Cs = Cs; a.c0 = c0; a.c1 = c1; a.B = B; a.Hs = Hs; a.Ws = Ws; a.Hl = Hl; a.Wl = Wl;
    a.mtiles = pl.mtiles; a.ntiles = pl.ntiles; a.nsl = pl.nsl;
    a.bw = pl.bw; a.nbands = pl.nbands; a.units = pl.units; a.ups = pl.ups;
    hipStream_t st = as_stream(stream);
    NLSPN_TRY(set_lds_attr(fn, pl.g.lds_bytes()));
    void *args[] = {&a};
    NLSPN_TRY(launch_kernel(fn, dim3((unsigned)(pl.mtiles * pl.ntiles * pl.nsl)), dim3(pl.g.nthr()), args,
                            (size_t)pl.g.lds_bytes(), st, "nlspn_gconv_wgrad_bf16x3"));
    {   // the slab reduce: the f32 entry's kernel and order
        const float *wsp = a.ws;
        int n0 = Cs, n1 = Cl, n1p = pl.ntiles * pl.g.nt(), T = 9, nsl = pl.nsl;
        long long slab = pl.slab;
        void *rargs[] = {&wsp, &dw, &n0, &n1, &n1p, &T, &slab, &nsl, &scale};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gwgrad_reduce_kernel),
                                dim3(elementwise_grid((long long)Cs * Cl * 9)), dim3(256), rargs, 0, st,
                                "nlspn_gconv_wgrad_bf16x3 reduce"));
    }
    if (db) {  // the bias gradient: the f32 entry's launches with its slice count (bit-equal)
        const float *g = bias_from_large ? l0 : s;
        int C = bias_from_large ? Cl : Cs, nsb = f32.nsb, one = 1;
        long long HW = bias_from_large ? (long long)Hl * Wl : (long long)Hs * Ws;
        float *part = a.ws + pl.bias_off;
        void *pargs[] = {&g, &part, &C, &B, &HW, &nsb};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gbias_partial_kernel), dim3((unsigned)(C * nsb)), dim3(256),
                                pargs, 0, st, "nlspn_gconv_wgrad_bf16x3 bias"));
        const float *cpart = part;
        long long bslab = C;
        float unit = 1.f;
        void *rargs[] = {&cpart, &db, &C, &one, &one, &one, &bslab, &nsb, &unit};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gwgrad_reduce_kernel), dim3(elementwise_grid(C)), dim3(256),
                                rargs, 0, st, "nlspn_gconv_wgrad_bf16x3 bias reduce"));
    }
    return NLSPN_OK;
}

int nlspn_gconv_dgrad(int layer, const float *g, int cg, const float *wpk, const float *ysave, const float *add0,
                      const float *add1, float *dx0, float *dx1, int split, int B, int Hg, int Wg, int cout, int Ho,
                      int Wo, int act, float scale, void *stream) {
    GcPreset p;
    if (!gc_get(layer, p) || p.epi != kGcEpiDact)
        return fail(NLSPN_EINVAL, "gconv dgrad: preset %d is not a data-gradient preset (NLSPN_GC_DG_*)", layer);
    if (!g || !wpk || !dx0) return fail(NLSPN_EINVAL, "gconv dgrad: null gradient, weights or output");
    if (B < 1 || Hg < 1 || Wg < 1 || cg < 1 || cout < 1 || Ho < 1 || Wo < 1)
        return fail(NLSPN_EINVAL, "gconv dgrad: bad shape B=%d %dx%d cg=%d cout=%d out %dx%d", B, Hg, Wg, cg, cout, Ho, Wo);
    if (split < 1 || split > cout || (split < cout) != (dx1 != nullptr) || (add1 && !dx1))
        return fail(NLSPN_EINVAL, "gconv dgrad: cout mismatch: split %d of cout %d %s a second output", split, cout,
                    dx1 ? "with" : "without");
    if (act < NLSPN_GC_ACT_NONE || act > NLSPN_GC_ACT_TANH || (act != NLSPN_GC_ACT_NONE && (!ysave || split != cout)))
        return fail(NLSPN_EINVAL, "gconv dgrad: activation %d needs the saved output and one output tensor", act);
    // the output size of the adjoint: the transposed conv's crop is at most one row / column (the
    // forward conv's input was Ho x Wo); the stride-2 conv's input gradient may be stored cropped
    // (Hg x Wg of the 2 Ho x 2 Wo the forward transposed conv produced: the rest reads as zeros)
    const bool oksize = p.mode == kGcS1 ? (Ho == Hg && Wo == Wg)
                        : p.mode == kGcT2 ? (Ho <= 2 * Hg && Ho >= 2 * Hg - 1 && Wo <= 2 * Wg && Wo >= 2 * Wg - 1)
                                          : (Hg <= 2 * Ho && Wg <= 2 * Wo);
    if (!oksize) return fail(NLSPN_EINVAL, "gconv dgrad: output %dx%d does not belong to gradient %dx%d", Ho, Wo, Hg, Wg);
    GconvArgs a{};
    a.x0 = g; a.w = wpk; a.y = dx0; a.y1 = dx1; a.ysplit = split; a.ysave = ysave; a.add = add0; a.add1 = add1;
    a.scale = scale; a.act = act; a.in_div = 1.f;
    a.c0 = cg; a.cin_pad = (cg + kGcCP - 1) / kGcCP * kGcCP;
    a.B = B; a.Hi = Hg; a.Wi = Wg;
    if (p.mode == kGcT2) { a.Ho = 2 * Hg; a.Wo = 2 * Wg; }
    else { a.Ho = Ho; a.Wo = Wo; }
    a.ohs = Ho; a.ows = Wo;
    a.cout = cout;
    a.co_tiles = (cout + p.wgco - 1) / p.wgco;
    NLSPN_TRY(gc_tile(p, a));
    const long long nwg = (long long)(p.mode == kGcT2 ? 4 : 1) * a.co_tiles * B * a.nbands * a.tpb;
    if (nwg > 0x7fffffffLL || (long long)cg * Hg * Wg * 4 > 0x7fffffffLL) return fail(NLSPN_EINVAL, "gconv dgrad: problem too large");
    NLSPN_TRY(set_lds_attr(p.fn, p.lds));
    void *args[] = {&a};
    return launch_kernel(p.fn, dim3((unsigned)nwg), dim3(kGcNT), args, (size_t)p.lds, as_stream(stream), "nlspn_gconv_dgrad");
}

int nlspn_gconv_gru_train(int stage, const float *x0, const float *x1, int c1, const float *wpk, const float *bias,
                          const float *h, float *zb, float *rhb, float *qxb, float *hout, float *rb, float *qb, int B,
                          int H, int W, int hc, void *stream) {
    if (stage != 1 && stage != 2) return fail(NLSPN_EINVAL, "gconv gru train: stage %d (1: GRU1, 2: GRU2)", stage);
    if (stage == 1 ? !rb : !qb) return fail(NLSPN_EINVAL, "gconv gru train: null %s buffer", stage == 1 ? "r" : "q");
    if (hc < 1 || hc % 128 != 0)
        return fail(NLSPN_EINVAL, "gconv gru train: hidden width %d is not a multiple of the tile (128)", hc);
    if (stage == 1)
        return gconv_impl(NLSPN_GC_GRU1, x0, hc, x1, c1, wpk, bias, nullptr, h, zb, rhb, qxb, nullptr, B, H, W, 3 * hc, 0, 0,
                          NLSPN_GC_ACT_NONE, 1.f, hc, nullptr, 0, stream, rb, nullptr);
    return gconv_impl(NLSPN_GC_GRU2, x0, hc, nullptr, 0, wpk, bias, nullptr, h, zb, nullptr, qxb, hout, B, H, W, hc, 0, 0,
                      NLSPN_GC_ACT_NONE, 1.f, hc, nullptr, 0, stream, nullptr, qb);
}

int nlspn_gconv_gru_gates_backward(int stage, const float *dhn, const float *z, const float *r, const float *q,
                                   const float *h, const float *drh, float *duq, float *duzr, float *dh, int act, int B,
                                   int hc, int H, int W, void *stream) {
    if (stage < 0 || stage > 2) return fail(NLSPN_EINVAL, "gconv gates backward: stage %d (0, 1, 2)", stage);
    if (B < 1 || hc < 1 || H < 1 || W < 1) return fail(NLSPN_EINVAL, "gconv gates backward: bad shape B=%d hc=%d %dx%d", B, hc, H, W);
    const bool ok = stage == 0 ? (dhn && z && duq && act >= NLSPN_GC_ACT_NONE && act <= NLSPN_GC_ACT_TANH)
                    : stage == 1 ? (dhn && z && q && h && duq && duzr)
                                 : (dhn && z && r && h && drh && duzr && dh);
    if (!ok) return fail(NLSPN_EINVAL, "gconv gates backward: null pointer (stage %d)", stage);
    GgatesArgs a{};
    a.dhn = dhn; a.z = z; a.r = r; a.q = q; a.h = h; a.drh = drh; a.duq = duq; a.duzr = duzr; a.dh = dh;
    a.hc = hc; a.act = act; a.HW = (long long)H * W; a.n = (long long)B * hc * a.HW;
    void *args[] = {&a, &stage};
    return launch_kernel(reinterpret_cast<const void *>(&ggates_kernel), dim3(elementwise_grid(a.n)), dim3(256), args, 0,
                         as_stream(stream), "nlspn_gconv_gru_gates_backward");
}

}  // extern "C"

// ---------------------------------------------------------------- f16 operands (nlspn_gconv16.h)
namespace {
struct Gc16Preset {
    const void *fn;
    int mode, wgco, npx, xr, xp, ccb, lds, epi;
};
template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CCB, int EPI>
Gc16Preset gc16_preset() {
    using Cfg = Gc16Cfg<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI>;
    return Gc16Preset{reinterpret_cast<const void *>(&gconv16_kernel<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI>), MODE,
                      Cfg::WGCO, Cfg::NPX, XR, XP, CCB, Cfg::LDS_BYTES, EPI};
}
bool gc16_get(int layer, Gc16Preset &p) {
    switch (layer) {
#define NLSPN_GC16_CASE(id, ...) \
    case id: p = gc16_preset<__VA_ARGS__>(); return true;
        NLSPN_GC16_CONFIGS(NLSPN_GC16_CASE)
        default: return false;
    }
}
}  // namespace
extern "C" {

int nlspn_gconv16_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed) {
    if (layer == NLSPN_GC16_S2_SMALL) {  // the module's own f32 weight layout
        if (co_tile) *co_tile = 0;
        if (cin_chunk) *cin_chunk = 1;
        if (transposed) *transposed = 0;
        return NLSPN_OK;
    }
    Gc16Preset p;
    if (!gc16_get(layer, p)) return fail(NLSPN_EINVAL, "gconv16: preset %d is not an f16 preset (NLSPN_GC16_*)", layer);
    if (co_tile) *co_tile = p.wgco;
    if (cin_chunk) *cin_chunk = 8 * p.ccb;
    if (transposed) *transposed = p.mode == kGcT2;
    return NLSPN_OK;
}

int nlspn_gconv16(int layer, const void *x0, int c0, const void *x1, int c1, const void *wpk, const float *bias,
                  void *y16, float *y32, const float *h, float *zb, void *rh16, float *qxb, float *hout32,
                  void *hout16, int B, int Hi, int Wi, int cout, int ohs, int ows, int act, float in_div, int hc,
                  void *stream) {
    Gc16Preset p{};
    const bool small = layer == NLSPN_GC16_S2_SMALL;
    if (!small && !gc16_get(layer, p))
        return fail(NLSPN_EINVAL, "gconv16: preset %d is not an f16 preset (NLSPN_GC16_*)", layer);
    if (B < 1 || Hi < 1 || Wi < 1 || cout < 1 || c0 < 1 || c1 < 0 || (c1 > 0 && !x1))
        return fail(NLSPN_EINVAL, "gconv16: bad shape B=%d Hi=%d Wi=%d c0=%d c1=%d cout=%d", B, Hi, Wi, c0, c1, cout);
    if (!x0 || !wpk || !bias) return fail(NLSPN_EINVAL, "gconv16: null input, weights or bias");
    if (act < NLSPN_GC_ACT_NONE || act > NLSPN_GC_ACT_TANH) return fail(NLSPN_EINVAL, "gconv16: activation %d", act);
    // (a chunk of channel blocks is staged from one source, through one descriptor)
    if (!small && c1 > 0 && c0 % (8 * p.ccb) != 0)
        return fail(NLSPN_EINVAL, "gconv16: a channel chunk would straddle the two sources (c0 = %d, not a multiple of %d)",
                    c0, 8 * p.ccb);
    if (!small && in_div != 1.f)
        return fail(NLSPN_EINVAL, "gconv16: in_div %g needs the NLSPN_GC16_S2_SMALL preset", (double)in_div);
    const bool gru = !small && (p.epi == kGcEpiGru1 || p.epi == kGcEpiGru2), gru1 = !small && p.epi == kGcEpiGru1;
    Gconv16Args a{};
    a.x0 = x0; a.x1 = x1; a.w = wpk; a.bias = bias;
    a.y16 = static_cast<_Float16 *>(y16); a.y32 = y32;
    a.h = h; a.zb = zb; a.rh16 = static_cast<_Float16 *>(rh16); a.qxb = qxb;
    a.hout32 = hout32; a.hout16 = static_cast<_Float16 *>(hout16);
    a.c0 = c0; a.c1 = c1; a.B = B; a.Hi = Hi; a.Wi = Wi; a.cout = cout; a.act = act; a.in_div = in_div; a.hc = hc;
    if (small || p.mode == kGcS2) { a.Ho = (Hi - 1) / 2 + 1; a.Wo = (Wi - 1) / 2 + 1; }
    else if (p.mode == kGcS1) { a.Ho = Hi; a.Wo = Wi; }
    else { a.Ho = 2 * Hi; a.Wo = 2 * Wi; }
    a.ohs = gru ? a.Ho : ohs;
    a.ows = gru ? a.Wo : ows;
    if (gru) {
        if (y16 || y32) return fail(NLSPN_EINVAL, "gconv16: a GRU launch writes no y16 / y32 (output format not supported)");
        if (hc < 1 || hc % p.wgco != 0 || !h || !zb || !qxb || c0 != hc ||
            (gru1 ? (!rh16 || cout != 3 * hc) : (!hout32 || !hout16 || cout != hc || c1 != 0)))
            return fail(NLSPN_EINVAL, "gconv16: GRU launch needs hc %% %d == 0, c0 = hc, h, z / qx, r*h (GRU1, cout 3hc) or "
                        "both h' outputs (GRU2, cout hc)", p.wgco);
    } else {
        if (!y16 && !y32) return fail(NLSPN_EINVAL, "gconv16: both outputs null");
        if (small && y32) return fail(NLSPN_EINVAL, "gconv16 small: the VALU kernel writes y16 only (output format not supported)");
    }
    if (a.ohs < 1 || a.ows < 1 || a.ohs > a.Ho || a.ows > a.Wo)
        return fail(NLSPN_EINVAL, "gconv16: stored size %dx%d outside the output %dx%d", a.ohs, a.ows, a.Ho, a.Wo);
    if (small) {
        if (c1 != 0 || cout != 16 || c0 * 16 * 9 > kGsMaxW)
            return fail(NLSPN_EINVAL, "gconv16 small: cin %d (c1 %d), cout %d outside the VALU kernel's range (cout 16, "
                        "cin <= 16)", c0, c1, cout);
        const long long npix = (long long)B * a.ohs * a.ows;
        const unsigned grid = (unsigned)std::min<long long>((npix + kGsNT - 1) / kGsNT, 1 << 20);
        const float *wf = static_cast<const float *>(wpk);
        void *args[] = {&a, &wf};
        return launch_kernel(reinterpret_cast<const void *>(&gsmall16_kernel<16>), dim3(grid), dim3(kGsNT), args, 0,
                             as_stream(stream), "nlspn_gconv16 small");
    }
    a.nb0 = (c0 + 7) / 8;
    a.nb1 = (c1 + 7) / 8;
    a.nbp = (a.nb0 + a.nb1 + p.ccb - 1) / p.ccb * p.ccb;
    a.co_tiles = (cout + p.wgco - 1) / p.wgco;
    {
        GcTiling t;
        const bool ok = nlspn::gc_tile(GcGeo{p.mode, p.wgco, p.npx, p.xr, p.xp}, p.mode == kGcT2 ? Hi : a.Ho,
                                       p.mode == kGcT2 ? Wi : a.Wo, t);
        a.gh = t.gh; a.gw = t.gw; a.bw = t.bw; a.nbands = t.nbands; a.tpb = t.tpb; a.npx = t.npx;
        if (!ok)
            return fail(NLSPN_EUNSUPPORTED, "gconv16: a tile of a %d-wide band spans more than %d window rows", a.bw, p.xr);
    }
    long long nwg = (long long)(p.mode == kGcT2 ? 4 : 1) * a.co_tiles * B * a.nbands * a.tpb;
    if (gru1) nwg = gc_gru1_wgs(a.hc, p.wgco, a.co_tiles, gc_rest_count(a.B, a.nbands, a.tpb));
    // (one image's channel blocks of a source within a 32-bit buffer descriptor)
    if (nwg > 0x7fffffffLL || (long long)std::max(a.nb0, a.nb1) * Hi * Wi * 16 > 0x7fffffffLL)
        return fail(NLSPN_EINVAL, "gconv16: problem too large");
    NLSPN_TRY(set_lds_attr(p.fn, p.lds));
    void *args[] = {&a};
    return launch_kernel(p.fn, dim3((unsigned)nwg), dim3(kGcNT), args, (size_t)p.lds, as_stream(stream), "nlspn_gconv16");
}

}  // extern "C"
