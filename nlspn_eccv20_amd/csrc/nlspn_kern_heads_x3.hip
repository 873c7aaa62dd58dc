// Device code of the split-bf16 head epilogue (nlspn_heads_x3.h) and its weight packer, their
// own translation unit: the f32 head unit (nlspn_kern_heads.hip) keeps its kernels and resource
// remarks.  Launched from nlspn_seam.hip.
#include "nlspn_heads_x3.h"

namespace nlspn {
NLSPN_HDX3_BUILDS(NLSPN_HDX3_INST)

__global__ void headsx3_pack_kernel(HeadsPackArgs a) {
    const int mb = a.nco / 32;
    const long long nm = hx3_wm_elems(a.C, mb), nv = hx3_wv_floats(a.C);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int C2 = 2 * a.C;
    if (i < nm) {
        const Hx3WElem e = hx3_w_elem(i, a.C, mb);
        // input channel of the conv: source 0 = fe1 = channels C..2C-1, source 1 = fd = 0..C-1
        const int ci = e.s == 0 ? a.C + e.c : e.c;
        float v = 0.f;
        if (e.co < a.nout) v = a.w_oa[((long long)e.co * C2 + ci) * 9 + e.t];
        else if (e.s == 0 && e.co == a.nout && a.w_id) v = a.w_id[(long long)ci * 9 + e.t];
        else if (e.s == 0 && e.co == a.nout + 1 && a.w_cf) v = a.w_cf[(long long)ci * 9 + e.t];
        const __bf16 hi = (__bf16)v;
        reinterpret_cast<__bf16 *>(a.wm)[i] = e.part == 0 ? hi : (__bf16)(v - (float)hi);
    } else if (i < nm + nv) {
        const long long j = i - nm;
        const int t = (int)(j % 9), c = (int)((j / 9) % a.C), s = (int)(j / (9LL * a.C));
        const float *w = s == 0 ? a.w_id : a.w_cf;
        a.wv[j] = w ? w[(long long)c * 9 + t] : 0.f;  // the decoder half: input channels 0..C-1
    } else if (i < nm + nv + a.nco) {
        const int co = (int)(i - nm - nv);
        float v = 0.f;
        if (co < a.nout) v = a.b_oa ? a.b_oa[co] : 0.f;
        else if (co == a.nout && a.b_id) v = a.b_id[0];
        else if (co == a.nout + 1 && a.b_cf) v = a.b_cf[0];
        a.bias[co] = v;
    }
}
}  // namespace nlspn
