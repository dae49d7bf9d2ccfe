// pn_probes.h — what the kernels that read HDR light probes share (pn_lighting.hip, pn_ibl.hip, pn_objects.hip,
// pn_emitters.hip; pn_volume.hip takes the SH basis): the strided view of a batch of probes, the real SH basis in the
// order and with the constants of include/panonerf_hip.h, and the clamped cell of an interpolation axis.  One definition
// each, so every user computes the same bits.
#pragma once
#include "pn_common.h"

// radiance of P probes read in place: [P, 3, H, W] tensors and [P, H, W, 3] buffers alike
struct Probes {
    const float* x;
    int64_t probe_stride, cs, ps;  // element (p, c, pix) at x[p * probe_stride + c * cs + pix * ps]
};

// real SH basis up to l = kDeg <= 2 at direction (x, y, z), order (0,0) (1,-1) (1,0) (1,1) (2,-2) (2,-1) (2,0) (2,1) (2,2)
template <int kDeg>
__device__ __forceinline__ void sh_basis(double x, double y, double z, double (&Y)[(kDeg + 1) * (kDeg + 1)]) {
    static_assert(kDeg >= 0 && kDeg <= 2, "SH degree");
    Y[0] = PN_SH_C0;
    if constexpr (kDeg >= 1) {
        Y[1] = PN_SH_C1 * y;
        Y[2] = PN_SH_C1 * z;
        Y[3] = PN_SH_C1 * x;
    }
    if constexpr (kDeg >= 2) {
        Y[4] = PN_SH_C2 * (x * y);
        Y[5] = PN_SH_C2 * (y * z);
        Y[6] = PN_SH_C3 * (3.0 * (z * z) - 1.0);
        Y[7] = PN_SH_C2 * (x * z);
        Y[8] = PN_SH_C4 * (x * x - y * y);
    }
}

// continuous coordinate u clamped to [0, top], top >= 1 (NaN passes through): cell index in [0, top - 1] and weight
__device__ __forceinline__ void clamped_cell(double u, int top, int& i, double& t) {
    if (u < 0.0) u = 0.0;
    if (u > (double)top) u = (double)top;
    if (isnan(u)) {
        i = 0, t = u;
        return;
    }
    i = (int)floor(u);
    if (i > top - 1) i = top - 1;
    t = u - (double)i;
}
