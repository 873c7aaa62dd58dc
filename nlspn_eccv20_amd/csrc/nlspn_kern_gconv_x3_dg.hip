// Device code of the split-bf16 data gradients of the GRU-mode convolutions (nlspn_gconv_x3.h,
// the kGcEpiDact epilogue), their own translation unit.  Launched from nlspn_gconv_host.hip
// (nlspn_gconv_x3_dgrad, nlspn_gconv_x3_split); the configurations are NLSPN_GCX3_DG_CONFIGS.
#include "nlspn_gconv_x3.h"

namespace nlspn {
#define NLSPN_GCX3_INST(id, ...) template __global__ void gconvx3_kernel<__VA_ARGS__>(GconvX3Args);
NLSPN_GCX3_DG_CONFIGS(NLSPN_GCX3_INST)

typedef float gx3_f8 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(256) gcx3_split_kernel(Gx3SplitArgs a) {
    gx3_bf8 *out = reinterpret_cast<gx3_bf8 *>(a.xs);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long long)gridDim.x * 256) {
        const long long bc = i / a.HW, pix = i - bc * a.HW;  // (image, channel block), pixel
        const long long b = bc / a.nb;
        const int c0 = 8 * (int)(bc - b * a.nb);
        const float *src = a.x + (b * a.C + c0) * a.HW + pix;
        gx3_f8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = c0 + j < a.C ? src[j * a.HW] : 0.f;  // (pad channels are zero)
        const gx3_bf8 hi = __builtin_convertvector(v, gx3_bf8);
        const gx3_bf8 lo = __builtin_convertvector(v - __builtin_convertvector(hi, gx3_f8), gx3_bf8);
        out[2 * bc * a.HW + pix] = hi;
        out[(2 * bc + 1) * a.HW + pix] = lo;
    }
}
}  // namespace nlspn
