// C ABI of the GRU-mode convolutions (see include/nlspn_prop.h): preset lookup, tiling and
// launch of the implicit-GEMM kernels, which are instantiated in nlspn_kern_gconv.hip.
#include <algorithm>

#include "nlspn_host.h"
#include "nlspn_gconv.h"

namespace nlspn {
// defined in nlspn_kern_gconv.hip
#define NLSPN_GC_EXTERN(id, ...) extern template __global__ void gconv_kernel<__VA_ARGS__>(GconvArgs);
NLSPN_GC_CONFIGS(NLSPN_GC_EXTERN)
extern template __global__ void gsmall_kernel<16>(GconvArgs, const float *);
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
// nlspn_gconv, and with gamma / aff_kind nlspn_gconv_affnorm (preset NLSPN_GC_T2_AFF)
int gconv_impl(int layer, const float *x0, int c0, const float *x1, int c1, const float *wpk, const float *bias,
               float *y, const float *h, float *zb, float *rhb, float *qxb, float *hout, int B, int Hi, int Wi,
               int cout, int ohs, int ows, int act, float in_div, int hc, const float *gamma, int aff_kind,
               void *stream) {
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
    if (B < 1 || Hi < 1 || Wi < 1 || cout < 1 || c0 < 1 || c1 < 0 || (c1 > 0 && !x1))
        return fail(NLSPN_EINVAL, "gconv: bad shape B=%d Hi=%d Wi=%d c0=%d c1=%d cout=%d", B, Hi, Wi, c0, c1, cout);
    if (!x0 || !wpk || !bias) return fail(NLSPN_EINVAL, "gconv: null input, weights or bias");
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
    a.gh = p.mode == kGcT2 ? Hi : a.Ho;
    a.gw = p.mode == kGcT2 ? Wi : a.Wo;
    // column bands: the window's columns within the LDS pitch
    const int bwmax = p.mode == kGcS1 ? p.xp - 2 : p.mode == kGcS2 ? (p.xp - 3) / 2 + 1 : p.xp - 1;
    a.nbands = (a.gw + bwmax - 1) / bwmax;
    a.bw = (a.gw + a.nbands - 1) / a.nbands;
    // the rows a tile of npx pixels spans (at most (npx + bw - 2) / bw row steps), within the
    // window's XR rows: narrow bands take fewer pixels per tile
    const auto rows_of = [&](int npx) {
        const int dr = (npx + a.bw - 2) / a.bw;
        return p.mode == kGcS1 ? dr + 3 : p.mode == kGcS2 ? 2 * dr + 3 : dr + 2;
    };
    a.npx = p.npx;
    while (a.npx > 1 && rows_of(a.npx) > p.xr) --a.npx;
    if (rows_of(a.npx) > p.xr)
        return fail(NLSPN_EUNSUPPORTED, "gconv: a tile of a %d-wide band spans more than %d window rows", a.bw, p.xr);
    a.tpb = (a.gh * a.bw + a.npx - 1) / a.npx;
    long long nwg = (long long)(p.mode == kGcT2 ? 4 : 1) * a.co_tiles * B * a.nbands * a.tpb;
    if (gru1) nwg = gc_gru1_wgs(a, p.wgco);  // (the qx workgroups take two pixel tiles each)
    // Small grids: the same layer kind on 32-pixel tiles (the same co tile, hence the same packed
    // weights) when 64-pixel tiles would leave most CUs one workgroup (NYU B=8: the 1/8-scale last
    // encoder conv 104.1 -> 85.2 us, GRU2 52.6 -> 50.6 us; profiles/r06/gc_bench_layers_v4_n32.json)
    if ((layer == NLSPN_GC_S2 || layer == NLSPN_GC_GRU2) && nwg < 2LL * device_cus())
        return gconv_impl(layer == NLSPN_GC_S2 ? NLSPN_GC_S2_N32 : NLSPN_GC_GRU2_N32, x0, c0, x1, c1, wpk, bias, y, h,
                          zb, rhb, qxb, hout, B, Hi, Wi, cout, ohs, ows, act, in_div, hc, nullptr, 0, stream);
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

}  // extern "C"
