// C ABI of the GRU-mode convolutions (see include/nlspn_prop.h): preset lookup, tiling and
// launch of the implicit-GEMM kernels, which are instantiated in nlspn_kern_gconv.hip.
#include <algorithm>

#include "nlspn_host.h"
#include "nlspn_gconv_bwd.h"
#include "nlspn_gconv16.h"
#include "nlspn_gconv_x3.h"
#include "nlspn_gwgrad16.h"
#include "nlspn_gwnarrow.h"

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
// defined in nlspn_kern_gconv_x3.hip
#define NLSPN_GCX3_EXTERN(id, ...) extern template __global__ void gconvx3_kernel<__VA_ARGS__>(GconvX3Args);
NLSPN_GCX3_CONFIGS(NLSPN_GCX3_EXTERN)
NLSPN_GCX3_DG_CONFIGS(NLSPN_GCX3_EXTERN)
extern template __global__ void gsmallx3_kernel<16>(GconvX3Args, const float *);
// defined in nlspn_kern_gwgrad16.hip
#define NLSPN_GW16_EXTERN(...) extern template __global__ void gwgrad16_kernel<__VA_ARGS__>(GwgradArgs);
NLSPN_GW16_CONFIGS(NLSPN_GW16_EXTERN)
// defined in nlspn_kern_gwnarrow.hip
#define NLSPN_GWN_EXTERN(NB) extern template __global__ void gwnarrow_kernel<NB>(GwnArgs);
NLSPN_GWN_BLOCKS(NLSPN_GWN_EXTERN)
}  // namespace nlspn

using namespace nlspn;

namespace {
// A preset of any family.  cc: the input channels of a chunk as packed (f32: kGcCP, which
// every chunk size divides; f16: the chunk's CCB blocks of 8; split bf16: its CCB / 2 blocks of 8,
// each a hi and a lo cell block).
struct GcPreset {
    const void *fn;
    int mode, wgco, npx, xr, xp, cc, lds, epi;
};
template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CC, int EPI>
GcPreset gc_preset() {
    using Cfg = GcCfg<MODE, WM, WN, WGM, WGN, XR, XP, CC, EPI>;
    return GcPreset{reinterpret_cast<const void *>(&gconv_kernel<MODE, WM, WN, WGM, WGN, XR, XP, CC, EPI>), MODE,
                    Cfg::WGCO, Cfg::NPX, XR, XP, kGcCP, (int)(Cfg::LDS_FLOATS * sizeof(float)), EPI};
}
template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CCB, int EPI>
GcPreset gc16_preset() {
    using Cfg = Gc16Cfg<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI>;
    return GcPreset{reinterpret_cast<const void *>(&gconv16_kernel<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI>), MODE,
                    Cfg::WGCO, Cfg::NPX, XR, XP, 8 * CCB, Cfg::LDS_BYTES, EPI};
}
template <int MODE, int WM, int WN, int WGM, int WGN, int XR, int XP, int CCB, int EPI>
GcPreset gcx3_preset() {
    using Cfg = GcX3Cfg<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI>;
    return GcPreset{reinterpret_cast<const void *>(&gconvx3_kernel<MODE, WM, WN, WGM, WGN, XR, XP, CCB, EPI>), MODE,
                    Cfg::WGCO, Cfg::NPX, XR, XP, gcx3_chunk_channels(CCB), Cfg::LDS_BYTES, EPI};
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
bool gc16_get(int layer, GcPreset &p) {
    switch (layer) {
#define NLSPN_GC16_CASE(id, ...) \
    case id: p = gc16_preset<__VA_ARGS__>(); return true;
        NLSPN_GC16_CONFIGS(NLSPN_GC16_CASE)
        default: return false;
    }
}
bool gcx3_get(int layer, GcPreset &p) {
    switch (layer) {
#define NLSPN_GCX3_CASE(id, ...) \
    case id: p = gcx3_preset<__VA_ARGS__>(); return true;
        NLSPN_GCX3_CONFIGS(NLSPN_GCX3_CASE)
        default: return false;
    }
}
bool gcx3_dg_get(int layer, GcPreset &p) {
    switch (layer) {
        NLSPN_GCX3_DG_CONFIGS(NLSPN_GCX3_CASE)
        default: return false;
    }
}

// ---- the steps the f32 forward, the data gradient and the f16 / split-bf16 forwards share
// the packing of a preset's weights (p null: the VALU kernel reads the module's own layout)
int gc_pack_layout(const GcPreset *p, int *co_tile, int *cin_chunk, int *transposed) {
    if (co_tile) *co_tile = p ? p->wgco : 0;
    if (cin_chunk) *cin_chunk = p ? p->cc : 1;
    if (transposed) *transposed = p && p->mode == kGcT2;
    return NLSPN_OK;
}
// the output size of a mode, before any crop
void gc_out_size(int mode, int Hi, int Wi, int &Ho, int &Wo) {
    if (mode == kGcS1) { Ho = Hi; Wo = Wi; }
    else if (mode == kGcS2) { Ho = (Hi - 1) / 2 + 1; Wo = (Wi - 1) / 2 + 1; }
    else { Ho = 2 * Hi; Wo = 2 * Wi; }
}
// the pixel tiling of a launch (a.Hi / a.Wi / a.Ho / a.Wo set): column bands and tiles per band
// (gc_tile, nlspn_gconv_plan.h); who: the family in the error text
template <class Args>
int gc_tile(const GcPreset &p, Args &a, const char *who) {
    GcTiling t;
    const bool ok = nlspn::gc_tile(GcGeo{p.mode, p.wgco, p.npx, p.xr, p.xp}, p.mode == kGcT2 ? a.Hi : a.Ho,
                                   p.mode == kGcT2 ? a.Wi : a.Wo, t);
    a.gh = t.gh; a.gw = t.gw; a.bw = t.bw; a.nbands = t.nbands; a.tpb = t.tpb; a.npx = t.npx;
    if (!ok)
        return fail(NLSPN_EUNSUPPORTED, "%s: a tile of a %d-wide band spans more than %d window rows", who, a.bw, p.xr);
    return NLSPN_OK;
}
// the workgroups of a tiled launch (a.co_tiles set; GRU1: the qx workgroups take two pixel tiles each)
template <class Args>
long long gc_wgs(const GcPreset &p, const Args &a) {
    if (p.epi == kGcEpiGru1) return gc_gru1_wgs(a.hc, p.wgco, a.co_tiles, gc_rest_count(a.B, a.nbands, a.tpb));
    return (long long)(p.mode == kGcT2 ? 4 : 1) * a.co_tiles * a.B * a.nbands * a.tpb;
}
// the VALU kernels' grid: a thread per stored pixel, grid-stride past 2^20 workgroups
unsigned gs_grid(long long npix) { return (unsigned)std::min<long long>((npix + kGsNT - 1) / kGsNT, 1 << 20); }
template <class Args>
int gc_launch(const GcPreset &p, Args &a, long long nwg, void *stream, const char *what) {
    NLSPN_TRY(set_lds_attr(p.fn, p.lds));
    void *args[] = {&a};
    return launch_kernel(p.fn, dim3((unsigned)nwg), dim3(kGcNT), args, (size_t)p.lds, as_stream(stream), what);
}
}  // namespace
extern "C" {

int nlspn_gconv_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed) {
    GcPreset p;
    const bool small = layer == NLSPN_GC_S2_SMALL;
    if (!small && !gc_get(layer, p)) return fail(NLSPN_EINVAL, "unknown GRU-mode conv preset %d", layer);
    return gc_pack_layout(small ? nullptr : &p, co_tile, cin_chunk, transposed);
}

}  // extern "C"
namespace {
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
        gc_out_size(kGcS2, Hi, Wi, a.Ho, a.Wo);
        a.ohs = ohs; a.ows = ows; a.cout = cout; a.act = act; a.in_div = in_div;
        if (ohs < 1 || ows < 1 || ohs > a.Ho || ows > a.Wo)
            return fail(NLSPN_EINVAL, "gconv small: stored size %dx%d outside the output %dx%d", ohs, ows, a.Ho, a.Wo);
        void *args[] = {&a, const_cast<float **>(&wpk)};
        return launch_kernel(reinterpret_cast<const void *>(&gsmall_kernel<16>), dim3(gs_grid((long long)B * ohs * ows)),
                             dim3(kGsNT), args, 0, as_stream(stream), "nlspn_gconv small");
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
    gc_out_size(p.mode, Hi, Wi, a.Ho, a.Wo);
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
    NLSPN_TRY(gc_tile(p, a, "gconv"));
    const long long nwg = gc_wgs(p, a);
    // Small grids: the same layer kind on 32-pixel tiles (the same co tile, hence the same packed
    // weights) when 64-pixel tiles would leave most CUs one workgroup (NYU B=8: the 1/8-scale last
    // encoder conv 104.1 -> 85.2 us, GRU2 52.6 -> 50.6 us; profiles/r06/gc_bench_layers_v4_n32.json)
    if ((layer == NLSPN_GC_S2 || layer == NLSPN_GC_GRU2) && nwg < 2LL * device_cus())
        return gconv_impl(layer == NLSPN_GC_S2 ? NLSPN_GC_S2_N32 : NLSPN_GC_GRU2_N32, x0, c0, x1, c1, wpk, bias, y, h,
                          zb, rhb, qxb, hout, B, Hi, Wi, cout, ohs, ows, act, in_div, hc, nullptr, 0, stream, rb, qb);
    // (one image's channels of a source within a 32-bit buffer descriptor)
    if (nwg > 0x7fffffffLL || (long long)std::max(c0, c1) * Hi * Wi * 4 > 0x7fffffffLL)
        return fail(NLSPN_EINVAL, "gconv: problem too large");
    return gc_launch(p, a, nwg, stream, "nlspn_gconv");
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
// The kernel of a tiling (nullptr: none instantiated); the f32 kernels' LDS bytes come with it
template <int S, int WM, int WGM, int WGN>
const void *gw_fn(const GwGeo &g, int &lds) {
    if (g.S != S || g.wm != WM || g.wgm != WGM || g.wgn != WGN) return nullptr;
    lds = (int)(GwCfg<S, WM, WGM, WGN>::LDS_FLOATS * sizeof(float));
    return reinterpret_cast<const void *>(&gwgrad_kernel<S, WM, WGM, WGN>);
}
const void *gw_kernel_of(const GwGeo &g, int &lds) {
    const void *fn = nullptr;
#define NLSPN_GW_PICK(...) if (!fn) fn = gw_fn<__VA_ARGS__>(g, lds);
    NLSPN_GW_CONFIGS(NLSPN_GW_PICK)
    return fn;
}
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

// The shape rules of a weight-gradient call, for both entries and both workspace queries (the
// plans themselves are pure arithmetic on a shape that passed: nlspn_gwgrad_plan.h,
// nlspn_gwgrad16_plan.h; kGw16BW = kGwBW, so one unit-count bound serves both)
static_assert(kGw16BW == kGwBW, "one unit-count bound for both plans");
int gw_check_shape(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    if (stride != 1 && stride != 2) return fail(NLSPN_EINVAL, "gconv wgrad: stride %d (supported 1, 2)", stride);
    if (B < 1 || Cs < 1 || Cl < 1 || Hs < 1 || Ws < 1 || Hl < 1 || Wl < 1)
        return fail(NLSPN_EINVAL, "gconv wgrad: bad shape B=%d Cs=%d Cl=%d small %dx%d large %dx%d", B, Cs, Cl, Hs, Ws, Hl, Wl);
    if (stride == 1 ? (Hl != Hs || Wl != Ws) : (Hl > 2 * Hs || Wl > 2 * Ws))
        return fail(NLSPN_EINVAL, "gconv wgrad: large size %dx%d does not belong to small size %dx%d at stride %d", Hl, Wl,
                    Hs, Ws, stride);
    if ((long long)B * Hs > 0x3fffffffLL / ((Ws + kGwBW - 1) / kGwBW)) return fail(NLSPN_EINVAL, "gconv wgrad: problem too large");
    return NLSPN_OK;
}
// ... preceded, in an entry, by the rules of its tensors
int gw_check_call(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1, const float *dw,
                  const float *db, int bias_from_large, const void *workspace, int B, int Hs, int Ws, int Hl, int Wl) {
    if (!s || !l0 || !dw || !workspace) return fail(NLSPN_EINVAL, "gconv wgrad: null tensor, gradient or workspace");
    if (c0 < 1 || c1 < 0 || (c1 > 0 && !l1)) return fail(NLSPN_EINVAL, "gconv wgrad: bad channels c0=%d c1=%d", c0, c1);
    // (a 16-channel block of the large tensor reads one source)
    if (c1 > 0 && c0 % 16 != 0)
        return fail(NLSPN_EINVAL, "gconv wgrad: a channel block would straddle the two sources (c0 = %d, not a multiple of 16)", c0);
    if (db && bias_from_large && c1 > 0) return fail(NLSPN_EINVAL, "gconv wgrad: the bias gradient reads one source");
    return gw_check_shape(stride, Cs, c0 + c1, B, Hs, Ws, Hl, Wl);
}
int gw_check_workspace(int64_t workspace_bytes, long long floats) {
    if (workspace_bytes < floats * (long long)sizeof(float))
        return fail(NLSPN_EINVAL, "gconv wgrad: workspace too small (%lld bytes, needs %lld)", (long long)workspace_bytes,
                    floats * (long long)sizeof(float));
    return NLSPN_OK;
}

// the kernels' arguments of a planned call
GwgradArgs gw_args(const float *s, int Cs, const float *l0, int c0, const float *l1, int c1, void *workspace, int B,
                   int Hs, int Ws, int Hl, int Wl, const GwSplit &pl) {
    GwgradArgs a{};
    a.s = s; a.l0 = l0; a.l1 = l1; a.ws = static_cast<float *>(workspace);
    a.Cs = Cs; a.c0 = c0; a.c1 = c1; a.B = B; a.Hs = Hs; a.Ws = Ws; a.Hl = Hl; a.Wl = Wl;
    a.mtiles = pl.mtiles; a.ntiles = pl.ntiles; a.nsl = pl.nsl;
    a.bw = pl.bw; a.nbands = pl.nbands; a.units = pl.units; a.ups = pl.ups;
    return a;
}
// The launches of a planned call: the slabs by the tiling's kernel fn (nthr threads, lds bytes,
// nt large channels per tile), their sum into dw in slice order, and the bias gradient's
// partials and their sum.  All but the first are the same kernels on the same slices for every
// precision (pl.nsb is gw_split's, a function of B Hl Wl alone): the bias gradient is bit-equal
// between the entries.  what: the labels of the four launches, naming the entry that was called.
struct GwLabels {
    const char *slabs, *reduce, *bias, *bias_reduce;
};
#define NLSPN_GW_LABELS(entry) GwLabels{entry, entry " reduce", entry " bias", entry " bias reduce"}
int gw_launch(const void *fn, int nthr, int lds, int nt, GwgradArgs &a, const GwSplit &pl, float *dw, float *db,
              int bias_from_large, float scale, void *stream, const GwLabels &what) {
    const int Cs = a.Cs, Cl = a.c0 + a.c1;
    hipStream_t st = as_stream(stream);
    NLSPN_TRY(set_lds_attr(fn, lds));
    void *args[] = {&a};
    NLSPN_TRY(launch_kernel(fn, dim3((unsigned)(pl.mtiles * pl.ntiles * pl.nsl)), dim3(nthr), args, (size_t)lds, st,
                            what.slabs));
    {
        const float *wsp = a.ws;
        int n0 = Cs, n1 = Cl, n1p = pl.ntiles * nt, T = 9, nsl = pl.nsl;
        long long slab = pl.slab;
        void *rargs[] = {&wsp, &dw, &n0, &n1, &n1p, &T, &slab, &nsl, &scale};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gwgrad_reduce_kernel),
                                dim3(elementwise_grid((long long)Cs * Cl * 9)), dim3(256), rargs, 0, st, what.reduce));
    }
    if (db) {
        const float *g = bias_from_large ? a.l0 : a.s;
        int C = bias_from_large ? Cl : Cs, B = a.B, nsb = pl.nsb, one = 1;
        long long HW = bias_from_large ? (long long)a.Hl * a.Wl : (long long)a.Hs * a.Ws;
        float *part = a.ws + pl.bias_off;
        void *pargs[] = {&g, &part, &C, &B, &HW, &nsb};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gbias_partial_kernel), dim3((unsigned)(C * nsb)), dim3(256),
                                pargs, 0, st, what.bias));
        const float *cpart = part;
        long long bslab = C;
        float unit = 1.f;
        void *rargs[] = {&cpart, &db, &C, &one, &one, &one, &bslab, &nsb, &unit};
        NLSPN_TRY(launch_kernel(reinterpret_cast<const void *>(&gwgrad_reduce_kernel), dim3(elementwise_grid(C)), dim3(256),
                                rargs, 0, st, what.bias_reduce));
    }
    return NLSPN_OK;
}
}  // namespace
extern "C" {

size_t nlspn_gconv_wgrad_workspace_bytes(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    if (gw_check_shape(stride, Cs, Cl, B, Hs, Ws, Hl, Wl)) return 0;
    return (size_t)gw_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl).floats * sizeof(float);
}

int nlspn_gconv_wgrad(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1, float *dw,
                      float *db, int bias_from_large, float scale, void *workspace, int64_t workspace_bytes, int B,
                      int Hs, int Ws, int Hl, int Wl, void *stream) {
    NLSPN_TRY(gw_check_call(stride, s, Cs, l0, c0, l1, c1, dw, db, bias_from_large, workspace, B, Hs, Ws, Hl, Wl));
    const GwPlan pl = gw_plan(stride, Cs, c0 + c1, B, Hs, Ws, Hl, Wl);
    NLSPN_TRY(gw_check_workspace(workspace_bytes, pl.floats));
    int lds = 0;
    const void *fn = gw_kernel_of(pl.g, lds);
    if (!fn) return fail(NLSPN_EUNSUPPORTED, "gconv wgrad: no kernel for the tiling of stride %d, Cs %d, Cl %d", stride, Cs, c0 + c1);
    GwgradArgs a = gw_args(s, Cs, l0, c0, l1, c1, workspace, B, Hs, Ws, Hl, Wl, pl);
    return gw_launch(fn, pl.g.nthr(), lds, pl.g.nt(), a, pl, dw, db, bias_from_large, scale, stream,
                     NLSPN_GW_LABELS("nlspn_gconv_wgrad"));
}

// ---- the split-bf16 weight gradient (nlspn_gwgrad16.h): the same call on the bf16 matrix cores
size_t nlspn_gconv_wgrad_bf16x3_workspace_bytes(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    if (gw_check_shape(stride, Cs, Cl, B, Hs, Ws, Hl, Wl)) return 0;
    const long long floats = gw16_choose(stride, Cs, Cl) == kGw16F32 ? gw_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl).floats
                                                                     : gw16_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl).floats;
    return (size_t)floats * sizeof(float);
}

int nlspn_gconv_wgrad_bf16x3(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1,
                             float *dw, float *db, int bias_from_large, float scale, void *workspace,
                             int64_t workspace_bytes, int B, int Hs, int Ws, int Hl, int Wl, void *stream) {
    NLSPN_TRY(gw_check_call(stride, s, Cs, l0, c0, l1, c1, dw, db, bias_from_large, workspace, B, Hs, Ws, Hl, Wl));
    const int Cl = c0 + c1;
    // both channel counts <= 16: the one-wave f32 kernel, bit for bit (its cost is staging, not MFMA)
    if (gw16_choose(stride, Cs, Cl) == kGw16F32)
        return nlspn_gconv_wgrad(stride, s, Cs, l0, c0, l1, c1, dw, db, bias_from_large, scale, workspace, workspace_bytes,
                                 B, Hs, Ws, Hl, Wl, stream);
    const Gw16Plan pl = gw16_plan(stride, Cs, Cl, B, Hs, Ws, Hl, Wl);
    NLSPN_TRY(gw_check_workspace(workspace_bytes, pl.floats));
    // (the kernel's per-thread staging offsets are 32 bits: a pass's 8 channel planes and one window row)
    if ((long long)pl.mtiles * pl.ntiles * pl.nsl > 0x7fffffffLL || (long long)Hs * Ws > (1LL << 27) || (long long)Hl * Wl > (1LL << 27))
        return fail(NLSPN_EINVAL, "gconv wgrad: problem too large");
    const void *fn = gw16_kernel_of(pl.g);
    if (!fn) return fail(NLSPN_EUNSUPPORTED, "gconv wgrad bf16x3: no kernel for tiling %d", pl.tiling);
    GwgradArgs a = gw_args(s, Cs, l0, c0, l1, c1, workspace, B, Hs, Ws, Hl, Wl, pl);
    return gw_launch(fn, pl.g.nthr(), pl.g.lds_bytes(), pl.g.nt(), a, pl, dw, db, bias_from_large, scale, stream,
                     NLSPN_GW_LABELS("nlspn_gconv_wgrad_bf16x3"));
}

// ---- the streaming weight gradient of the narrow layers (nlspn_gwnarrow.h)
int nlspn_gconv_wgrad_narrow_covers(int stride, int Cs, int c0, int c1) { return gwn_covers(stride, Cs, c0, c1) ? 1 : 0; }

size_t nlspn_gconv_wgrad_narrow_workspace_bytes(int stride, int Cs, int Cl, int B, int Hs, int Ws, int Hl, int Wl) {
    if (gw_check_shape(stride, Cs, Cl, B, Hs, Ws, Hl, Wl)) return 0;
    if (!gwn_covers(stride, Cs, Cl, 0)) return nlspn_gconv_wgrad_workspace_bytes(stride, Cs, Cl, B, Hs, Ws, Hl, Wl);
    return (size_t)gwn_plan(Cs, Cl, B, Hs, Ws, Hl, Wl).floats * sizeof(float);
}

int nlspn_gconv_wgrad_narrow(int stride, const float *s, int Cs, const float *l0, int c0, const float *l1, int c1,
                             float *dw, float *db, int bias_from_large, float scale, void *workspace,
                             int64_t workspace_bytes, int B, int Hs, int Ws, int Hl, int Wl, void *stream) {
    NLSPN_TRY(gw_check_call(stride, s, Cs, l0, c0, l1, c1, dw, db, bias_from_large, workspace, B, Hs, Ws, Hl, Wl));
    // a shape the streaming kernel does not cover: the f32 entry, bit for bit
    if (!gwn_covers(stride, Cs, c0, c1))
        return nlspn_gconv_wgrad(stride, s, Cs, l0, c0, l1, c1, dw, db, bias_from_large, scale, workspace, workspace_bytes,
                                 B, Hs, Ws, Hl, Wl, stream);
    const GwnPlan pl = gwn_plan(Cs, c0, B, Hs, Ws, Hl, Wl);
    NLSPN_TRY(gw_check_workspace(workspace_bytes, pl.floats));
    const void *fn = nullptr;
#define NLSPN_GWN_PICK(NB) if (pl.nb == NB) fn = reinterpret_cast<const void *>(&gwnarrow_kernel<NB>);
    NLSPN_GWN_BLOCKS(NLSPN_GWN_PICK)
    if (!fn) return fail(NLSPN_EUNSUPPORTED, "gconv wgrad narrow: no kernel for %d blocks", pl.nb);
    GwnArgs a{};
    a.s = s; a.l = l0; a.ws = static_cast<float *>(workspace);
    a.Cs = Cs; a.Cl = c0; a.B = B; a.Hs = Hs; a.Ws = Ws; a.Hl = Hl; a.Wl = Wl;
    a.nbands = pl.nbands; a.bw = pl.bw; a.ngroups = pl.ngroups; a.units = pl.units; a.ups = pl.ups;
    a.bias_from_large = bias_from_large ? 1 : 0;
    a.slab = pl.slab;
    hipStream_t st = as_stream(stream);
    NLSPN_TRY(set_lds_attr(fn, pl.lds_bytes));
    void *args[] = {&a};
    NLSPN_TRY(launch_kernel(fn, dim3((unsigned)pl.nsl), dim3(kGwnNTHR), args, (size_t)pl.lds_bytes, st, "nlspn_gconv_wgrad_narrow"));
    const float *wsp = a.ws;
    int Cl = c0, nbias = !db ? 0 : bias_from_large ? Cl : Cs, nsl = pl.nsl, nb = pl.nb;
    long long slab = pl.slab;
    void *rargs[] = {&wsp, &dw, &db, &Cs, &Cl, &nbias, &nsl, &slab, &nb, &scale};
    return launch_kernel(reinterpret_cast<const void *>(&gwnarrow_reduce_kernel), dim3((unsigned)((Cs * 9 * Cl + 15) / 16 + (db ? 1 : 0))),
                         dim3(256), rargs, 0, st, "nlspn_gconv_wgrad_narrow reduce");
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
    if (p.mode == kGcT2) gc_out_size(kGcT2, Hg, Wg, a.Ho, a.Wo);
    else { a.Ho = Ho; a.Wo = Wo; }
    a.ohs = Ho; a.ows = Wo;
    a.cout = cout;
    a.co_tiles = (cout + p.wgco - 1) / p.wgco;
    NLSPN_TRY(gc_tile(p, a, "gconv"));
    const long long nwg = gc_wgs(p, a);
    if (nwg > 0x7fffffffLL || (long long)cg * Hg * Wg * 4 > 0x7fffffffLL) return fail(NLSPN_EINVAL, "gconv dgrad: problem too large");
    return gc_launch(p, a, nwg, stream, "nlspn_gconv_dgrad");
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

// ---------------------------------------------------------------- f16 operands (nlspn_gconv16.h)
int nlspn_gconv16_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed) {
    GcPreset p;
    const bool small = layer == NLSPN_GC16_S2_SMALL;  // (the module's own f32 weight layout)
    if (!small && !gc16_get(layer, p)) return fail(NLSPN_EINVAL, "gconv16: preset %d is not an f16 preset (NLSPN_GC16_*)", layer);
    return gc_pack_layout(small ? nullptr : &p, co_tile, cin_chunk, transposed);
}

int nlspn_gconv16(int layer, const void *x0, int c0, const void *x1, int c1, const void *wpk, const float *bias,
                  void *y16, float *y32, const float *h, float *zb, void *rh16, float *qxb, float *hout32,
                  void *hout16, int B, int Hi, int Wi, int cout, int ohs, int ows, int act, float in_div, int hc,
                  void *stream) {
    GcPreset p{};
    const bool small = layer == NLSPN_GC16_S2_SMALL;
    if (!small && !gc16_get(layer, p))
        return fail(NLSPN_EINVAL, "gconv16: preset %d is not an f16 preset (NLSPN_GC16_*)", layer);
    if (B < 1 || Hi < 1 || Wi < 1 || cout < 1 || c0 < 1 || c1 < 0 || (c1 > 0 && !x1))
        return fail(NLSPN_EINVAL, "gconv16: bad shape B=%d Hi=%d Wi=%d c0=%d c1=%d cout=%d", B, Hi, Wi, c0, c1, cout);
    if (!x0 || !wpk || !bias) return fail(NLSPN_EINVAL, "gconv16: null input, weights or bias");
    if (act < NLSPN_GC_ACT_NONE || act > NLSPN_GC_ACT_TANH) return fail(NLSPN_EINVAL, "gconv16: activation %d", act);
    // (a chunk of channel blocks is staged from one source, through one descriptor)
    if (!small && c1 > 0 && c0 % p.cc != 0)
        return fail(NLSPN_EINVAL, "gconv16: a channel chunk would straddle the two sources (c0 = %d, not a multiple of %d)",
                    c0, p.cc);
    if (!small && in_div != 1.f)
        return fail(NLSPN_EINVAL, "gconv16: in_div %g needs the NLSPN_GC16_S2_SMALL preset", (double)in_div);
    const bool gru = !small && (p.epi == kGcEpiGru1 || p.epi == kGcEpiGru2), gru1 = !small && p.epi == kGcEpiGru1;
    Gconv16Args a{};
    a.x0 = x0; a.x1 = x1; a.w = wpk; a.bias = bias;
    a.y16 = static_cast<_Float16 *>(y16); a.y32 = y32;
    a.h = h; a.zb = zb; a.rh16 = static_cast<_Float16 *>(rh16); a.qxb = qxb;
    a.hout32 = hout32; a.hout16 = static_cast<_Float16 *>(hout16);
    a.c0 = c0; a.c1 = c1; a.B = B; a.Hi = Hi; a.Wi = Wi; a.cout = cout; a.act = act; a.in_div = in_div; a.hc = hc;
    gc_out_size(small ? kGcS2 : p.mode, Hi, Wi, a.Ho, a.Wo);
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
        const float *wf = static_cast<const float *>(wpk);
        void *args[] = {&a, &wf};
        return launch_kernel(reinterpret_cast<const void *>(&gsmall16_kernel<16>), dim3(gs_grid((long long)B * a.ohs * a.ows)),
                             dim3(kGsNT), args, 0, as_stream(stream), "nlspn_gconv16 small");
    }
    const int ccb = p.cc / 8;  // the 8-channel blocks of a chunk
    a.nb0 = (c0 + 7) / 8;
    a.nb1 = (c1 + 7) / 8;
    a.nbp = (a.nb0 + a.nb1 + ccb - 1) / ccb * ccb;
    a.co_tiles = (cout + p.wgco - 1) / p.wgco;
    NLSPN_TRY(gc_tile(p, a, "gconv16"));
    const long long nwg = gc_wgs(p, a);
    // (one image's channel blocks of a source within a 32-bit buffer descriptor)
    if (nwg > 0x7fffffffLL || (long long)std::max(a.nb0, a.nb1) * Hi * Wi * 16 > 0x7fffffffLL)
        return fail(NLSPN_EINVAL, "gconv16: problem too large");
    return gc_launch(p, a, nwg, stream, "nlspn_gconv16");
}

// ---------------------------------------------------------------- split bf16 operands (nlspn_gconv_x3.h)
int nlspn_gconv_x3_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed) {
    GcPreset p;
    const bool small = layer == NLSPN_GCX3_S2_SMALL;  // (the module's own f32 weight layout)
    if (!small && !gcx3_get(layer, p))
        return fail(NLSPN_EINVAL, "gconv_x3: preset %d is not a split-bf16 preset (NLSPN_GCX3_*)", layer);
    return gc_pack_layout(small ? nullptr : &p, co_tile, cin_chunk, transposed);
}

int nlspn_gconv_x3(int layer, const void *x0, int c0, const void *x1, int c1, const void *wpk, const float *bias,
                   void *ys, float *y32, const float *h, float *zb, void *rhs, float *qxb, float *hout32,
                   void *houts, int B, int Hi, int Wi, int cout, int ohs, int ows, int act, float in_div, int hc,
                   void *stream) {
    GcPreset p{};
    const bool small = layer == NLSPN_GCX3_S2_SMALL;
    if (!small && !gcx3_get(layer, p))
        return fail(NLSPN_EINVAL, "gconv_x3: preset %d is not a split-bf16 preset (NLSPN_GCX3_*)", layer);
    if (B < 1 || Hi < 1 || Wi < 1 || cout < 1 || c0 < 1 || c1 < 0 || (c1 > 0 && !x1))
        return fail(NLSPN_EINVAL, "gconv_x3: bad shape B=%d Hi=%d Wi=%d c0=%d c1=%d cout=%d", B, Hi, Wi, c0, c1, cout);
    if (!x0 || !wpk || !bias) return fail(NLSPN_EINVAL, "gconv_x3: null input, weights or bias");
    if (act < NLSPN_GC_ACT_NONE || act > NLSPN_GC_ACT_TANH) return fail(NLSPN_EINVAL, "gconv_x3: activation %d", act);
    // (a chunk of cell blocks is staged from one source, through one descriptor)
    if (!small && c1 > 0 && c0 % p.cc != 0)
        return fail(NLSPN_EINVAL, "gconv_x3: a channel chunk would straddle the two sources (c0 = %d, not a multiple of %d)",
                    c0, p.cc);
    if (!small && in_div != 1.f)
        return fail(NLSPN_EINVAL, "gconv_x3: in_div %g needs the NLSPN_GCX3_S2_SMALL preset", (double)in_div);
    const bool gru = !small && (p.epi == kGcEpiGru1 || p.epi == kGcEpiGru2), gru1 = !small && p.epi == kGcEpiGru1;
    GconvX3Args a{};
    a.x0 = x0; a.x1 = x1; a.w = wpk; a.bias = bias;
    a.ys = static_cast<__bf16 *>(ys); a.y32 = y32;
    a.h = h; a.zb = zb; a.rhs = static_cast<__bf16 *>(rhs); a.qxb = qxb;
    a.hout32 = hout32; a.houts = static_cast<__bf16 *>(houts);
    a.c0 = c0; a.c1 = c1; a.B = B; a.Hi = Hi; a.Wi = Wi; a.cout = cout; a.act = act; a.in_div = in_div; a.hc = hc;
    gc_out_size(small ? kGcS2 : p.mode, Hi, Wi, a.Ho, a.Wo);
    a.ohs = gru ? a.Ho : ohs;
    a.ows = gru ? a.Wo : ows;
    if (gru) {
        if (ys || y32) return fail(NLSPN_EINVAL, "gconv_x3: a GRU launch writes no ys / y32 (output format not supported)");
        if (hc < 1 || hc % p.wgco != 0 || !h || !zb || !qxb || c0 != hc ||
            (gru1 ? (!rhs || cout != 3 * hc) : (!hout32 || !houts || cout != hc || c1 != 0)))
            return fail(NLSPN_EINVAL, "gconv_x3: GRU launch needs hc %% %d == 0, c0 = hc, h, z / qx, r*h (GRU1, cout 3hc) or "
                        "both h' outputs (GRU2, cout hc)", p.wgco);
    } else {
        if (!ys && !y32) return fail(NLSPN_EINVAL, "gconv_x3: both outputs null");
        if (small && y32) return fail(NLSPN_EINVAL, "gconv_x3 small: the VALU kernel writes ys only (output format not supported)");
    }
    if (a.ohs < 1 || a.ows < 1 || a.ohs > a.Ho || a.ows > a.Wo)
        return fail(NLSPN_EINVAL, "gconv_x3: stored size %dx%d outside the output %dx%d", a.ohs, a.ows, a.Ho, a.Wo);
    if (small) {
        if (c1 != 0 || cout != 16 || c0 * 16 * 9 > kGsMaxW)
            return fail(NLSPN_EINVAL, "gconv_x3 small: cin %d (c1 %d), cout %d outside the VALU kernel's range (cout 16, "
                        "cin <= 16)", c0, c1, cout);
        const float *wf = static_cast<const float *>(wpk);
        void *args[] = {&a, &wf};
        return launch_kernel(reinterpret_cast<const void *>(&gsmallx3_kernel<16>), dim3(gs_grid((long long)B * a.ohs * a.ows)),
                             dim3(kGsNT), args, 0, as_stream(stream), "nlspn_gconv_x3 small");
    }
    const int ccb = p.cc / 4;  // the cell blocks of a chunk: a hi and a lo one per 8 channels
    a.nb0 = 2 * ((c0 + 7) / 8);
    a.nb1 = 2 * ((c1 + 7) / 8);
    a.nbp = (a.nb0 + a.nb1 + ccb - 1) / ccb * ccb;
    a.co_tiles = (cout + p.wgco - 1) / p.wgco;
    NLSPN_TRY(gc_tile(p, a, "gconv_x3"));
    const long long nwg = gc_wgs(p, a);
    // (one image's cell blocks of a source within a 32-bit buffer descriptor)
    if (nwg > 0x7fffffffLL || (long long)std::max(a.nb0, a.nb1) * Hi * Wi * 16 > 0x7fffffffLL)
        return fail(NLSPN_EINVAL, "gconv_x3: problem too large");
    return gc_launch(p, a, nwg, stream, "nlspn_gconv_x3");
}

// ---------------------------------------------------------------- split-bf16 data gradients
int nlspn_gconv_x3_split(const float *x, void *xs, int B, int C, int H, int W, void *stream) {
    if (!x || !xs) return fail(NLSPN_EINVAL, "gconv_x3 split: null input or output");
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(NLSPN_EINVAL, "gconv_x3 split: bad shape B=%d C=%d %dx%d", B, C, H, W);
    Gx3SplitArgs a{};
    a.x = x; a.xs = static_cast<__bf16 *>(xs); a.C = C; a.nb = (C + 7) / 8;
    a.HW = (long long)H * W; a.n = (long long)B * a.nb * a.HW;
    void *args[] = {&a};
    return launch_kernel(reinterpret_cast<const void *>(&gcx3_split_kernel), dim3(elementwise_grid(a.n)), dim3(256), args, 0,
                         as_stream(stream), "nlspn_gconv_x3_split");
}

int nlspn_gconv_x3_dgrad_pack_layout(int layer, int *co_tile, int *cin_chunk, int *transposed) {
    GcPreset p;
    if (!gcx3_dg_get(layer, p))
        return fail(NLSPN_EINVAL, "gconv_x3 dgrad: preset %d is not a split-bf16 data-gradient preset (NLSPN_GCX3_DG_*)", layer);
    return gc_pack_layout(&p, co_tile, cin_chunk, transposed);
}

}  // extern "C"
namespace {
// a data gradient's sizes against its preset's mode, as nlspn_gconv_dgrad accepts them
bool gcx3_dg_oksize(int mode, int Hg, int Wg, int Ho, int Wo) {
    return mode == kGcS1   ? (Ho == Hg && Wo == Wg)
           : mode == kGcT2 ? (Ho <= 2 * Hg && Ho >= 2 * Hg - 1 && Wo <= 2 * Wg && Wo >= 2 * Wg - 1)
                           : (Hg <= 2 * Ho && Wg <= 2 * Wo);
}
// what the family serves of those: null, or why not.  A stride-2-mode gradient stored cropped is
// the f32 last decoder layer's alone.  A gradient of at most 16 channels is one 16-channel chunk:
// nine k-steps under an epilogue that stores as much as the f32 kernel's, and it measured slower
// than the f32 entry (the 2hc -> 16 decoder layer's adjoint at NYU B=8: 97.6 us with its split
// launch against 52.3 us); with at most 16 output channels too it is mostly padding.
// Both stay on nlspn_gconv_dgrad.
const char *gcx3_dg_unserved(const GcPreset &p, int cg, int cout, int Hg, int Wg, int Ho, int Wo) {
    if (p.mode == kGcS2 && (Hg != 2 * Ho || Wg != 2 * Wo)) return "a stride-2-mode gradient stored cropped";
    if (cg <= 16) return "a gradient of at most 16 channels";
    GcTiling t;
    const bool tr = p.mode == kGcT2;
    if (!nlspn::gc_tile(GcGeo{p.mode, p.wgco, p.npx, p.xr, p.xp}, tr ? Hg : Ho, tr ? Wg : Wo, t))
        return "a grid no tile fits";
    return nullptr;
}
}  // namespace
extern "C" {

int nlspn_gconv_x3_dgrad_covers(int layer, int cg, int cout, int Hg, int Wg, int Ho, int Wo) {
    GcPreset p;
    if (!gcx3_dg_get(layer, p) || cg < 1 || cout < 1 || Hg < 1 || Wg < 1 || Ho < 1 || Wo < 1) return 0;
    return gcx3_dg_oksize(p.mode, Hg, Wg, Ho, Wo) && !gcx3_dg_unserved(p, cg, cout, Hg, Wg, Ho, Wo) ? 1 : 0;
}

int nlspn_gconv_x3_dgrad(int layer, const void *gs, int cg, const void *wpk, const float *ysave, const float *add0,
                         const float *add1, float *dx0, float *dx1, int split, void *dxs, int B, int Hg, int Wg,
                         int cout, int Ho, int Wo, int act, float scale, void *stream) {
    GcPreset p;
    if (!gcx3_dg_get(layer, p))
        return fail(NLSPN_EINVAL, "gconv_x3 dgrad: preset %d is not a split-bf16 data-gradient preset (NLSPN_GCX3_DG_*)", layer);
    if (!gs || !wpk || !dx0) return fail(NLSPN_EINVAL, "gconv_x3 dgrad: null gradient, weights or output");
    if (B < 1 || Hg < 1 || Wg < 1 || cg < 1 || cout < 1 || Ho < 1 || Wo < 1)
        return fail(NLSPN_EINVAL, "gconv_x3 dgrad: bad shape B=%d %dx%d cg=%d cout=%d out %dx%d", B, Hg, Wg, cg, cout, Ho, Wo);
    if (split < 1 || split > cout || (split < cout) != (dx1 != nullptr) || (add1 && !dx1))
        return fail(NLSPN_EINVAL, "gconv_x3 dgrad: cout mismatch: split %d of cout %d %s a second output", split, cout,
                    dx1 ? "with" : "without");
    if (dxs && split != cout) return fail(NLSPN_EINVAL, "gconv_x3 dgrad: the split copy needs one output tensor (split = cout)");
    if (act < NLSPN_GC_ACT_NONE || act > NLSPN_GC_ACT_TANH || (act != NLSPN_GC_ACT_NONE && (!ysave || split != cout)))
        return fail(NLSPN_EINVAL, "gconv_x3 dgrad: activation %d needs the saved output and one output tensor", act);
    if (!gcx3_dg_oksize(p.mode, Hg, Wg, Ho, Wo))
        return fail(NLSPN_EINVAL, "gconv_x3 dgrad: output %dx%d does not belong to gradient %dx%d", Ho, Wo, Hg, Wg);
    if (const char *why = gcx3_dg_unserved(p, cg, cout, Hg, Wg, Ho, Wo))
        return fail(NLSPN_EUNSUPPORTED, "gconv_x3 dgrad: %s is nlspn_gconv_dgrad's (nlspn_gconv_x3_dgrad_covers)", why);
    GconvX3Args a{};
    a.x0 = gs; a.w = wpk; a.y32 = dx0; a.y1 = dx1; a.ysplit = split; a.ys = static_cast<__bf16 *>(dxs);
    a.ysave = ysave; a.add = add0; a.add1 = add1; a.scale = scale; a.act = act; a.in_div = 1.f;
    a.c0 = cg; a.B = B; a.Hi = Hg; a.Wi = Wg;
    if (p.mode == kGcT2) gc_out_size(kGcT2, Hg, Wg, a.Ho, a.Wo);
    else { a.Ho = Ho; a.Wo = Wo; }
    a.ohs = Ho; a.ows = Wo;
    a.cout = cout;
    const int ccb = p.cc / 4;  // the cell blocks of a chunk: a hi and a lo one per 8 channels
    a.nb0 = 2 * ((cg + 7) / 8);
    a.nbp = (a.nb0 + ccb - 1) / ccb * ccb;
    a.co_tiles = (cout + p.wgco - 1) / p.wgco;
    NLSPN_TRY(gc_tile(p, a, "gconv_x3 dgrad"));
    const long long nwg = gc_wgs(p, a);
    // (one image's cell blocks of the gradient within a 32-bit buffer descriptor)
    if (nwg > 0x7fffffffLL || (long long)a.nb0 * Hg * Wg * 16 > 0x7fffffffLL)
        return fail(NLSPN_EINVAL, "gconv_x3 dgrad: problem too large");
    return gc_launch(p, a, nwg, stream, "nlspn_gconv_x3_dgrad");
}

}  // extern "C"
