// Device code of the streaming weight gradient of the narrow layers (nlspn_gwnarrow.h), its own
// translation unit.  Launched from nlspn_gconv_host.hip (nlspn_gconv_wgrad_narrow).
#include "nlspn_gwnarrow.h"

namespace nlspn {
#define NLSPN_GWN_INST(NB) template __global__ void gwnarrow_kernel<NB>(GwnArgs);
NLSPN_GWN_BLOCKS(NLSPN_GWN_INST)

__global__ void __launch_bounds__(256) gwnarrow_reduce_kernel(const float *ws, float *dw, float *db, int Cs, int Cl, int nbias,
                                                              int nsl, long long slab, int nb, float scale) {
    __shared__ float part[kGwnRedLanes][17];
    const int i = threadIdx.x & 15, j = threadIdx.x >> 4;
    const int nent = 9 * Cl, nout = Cs * nent, ngw = (nout + 15) / 16;
    const bool bias = (int)blockIdx.x >= ngw;
    const int o = bias ? i : (int)blockIdx.x * 16 + i;
    const bool live = bias ? i < nbias : o < nout;
    float sum = 0.f;
    if (live) {
        const float *p = ws + (bias ? nb * 256 + i : gwn_slab_off(o / nent, o % nent));
        for (int sl = j; sl < nsl; sl += kGwnRedLanes) sum += p[(long long)sl * slab];
    }
    part[j][i] = sum;
    __syncthreads();
    if (j == 0 && live) {
        float t = part[0][i];
        for (int k = 1; k < kGwnRedLanes; ++k) t += part[k][i];
        if (bias) db[i] = t;
        else dw[o] = t * scale;
    }
}
}  // namespace nlspn
