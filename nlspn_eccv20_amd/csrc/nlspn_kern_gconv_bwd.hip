// Device code of the GRU-mode convolutions' backward (nlspn_gconv_bwd.h), its own translation
// unit: the data-gradient presets of the forward kernel (NLSPN_GC_DG_CONFIGS), the weight /
// bias gradient kernels and the gate derivatives.  Launched from nlspn_gconv_host.hip.
#include "nlspn_gconv_bwd.h"

namespace nlspn {
#define NLSPN_GC_INST(id, ...) template __global__ void gconv_kernel<__VA_ARGS__>(GconvArgs);
NLSPN_GC_DG_CONFIGS(NLSPN_GC_INST)
#define NLSPN_GW_INST(...) template __global__ void gwgrad_kernel<__VA_ARGS__>(GwgradArgs);
NLSPN_GW_CONFIGS(NLSPN_GW_INST)

__global__ void __launch_bounds__(256) gwgrad_reduce_kernel(const float *ws, float *out, int n0, int n1, int n1p, int T,
                                                            long long slab, int nsl, float scale) {
    const long long n = (long long)n0 * n1 * T;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int t = (int)(e % T);
        const long long ij = e / T;
        const int j = (int)(ij % n1);
        const long long i = ij / n1;
        const float *p = ws + (i * n1p + j) * T + t;
        float sum = 0.f;
        for (int s = 0; s < nsl; ++s) sum += p[(long long)s * slab];
        out[e] = sum * scale;
    }
}

__global__ void __launch_bounds__(256) gbias_partial_kernel(const float *g, float *ws, int C, int B, long long HW, int nsl) {
    __shared__ float red[256];
    const int c = (int)blockIdx.x % C, sl = (int)blockIdx.x / C;
    const long long n = (long long)B * HW, per = (n + nsl - 1) / nsl;
    const long long e0 = sl * per, e1 = min(n, e0 + per);
    float sum = 0.f;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
        const long long b = e / HW;
        sum += g[(b * C + c) * HW + (e - b * HW)];
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) ws[(long long)sl * C + c] = red[0];
}

__global__ void __launch_bounds__(256) ggates_kernel(GgatesArgs a, int stage) {
    const long long chw = (long long)a.hc * a.HW;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < a.n; e += (long long)gridDim.x * 256) {
        if (stage == 0) {
            const float y = a.z[e], g = a.dhn[e];
            a.duq[e] = a.act == kGcActRelu ? (y > 0.f ? g : 0.f) : a.act == kGcActTanh ? g * (1.f - y * y) : g;
            continue;
        }
        const long long b = e / chw;
        const long long e2 = e + b * chw;  // the element in the first half of a (B, 2 hc, H, W) tensor
        if (stage == 1) {
            const float g = a.dhn[e], z = a.z[e], q = a.q[e], h = a.h[e];
            a.duq[e] = g * z * (1.f - q * q);
            a.duzr[e2] = g * (q - h) * (z * (1.f - z));
        } else {
            const float d = a.drh[e], r = a.r[e];
            a.duzr[e2 + chw] = d * a.h[e] * (r * (1.f - r));
            a.dh[e] = a.dhn[e] * (1.f - a.z[e]) + d * r;
        }
    }
}
}  // namespace nlspn
