// pn_pano_ray.h — one ray of an equirectangular camera: the arithmetic every panorama ray of the library comes from
// (pn_render.hip: the pool generator and the batch sampler; pn_cameras.hip: the stereo-panorama camera), so that all
// of them give the same bits.
#pragma once
#include "pn_common.h"

// One pixel of an equirectangular camera (datasets/pano_datasets.py:157-213): shared by the pool generator and by the
// batch sampler that regenerates rays from (camera, pixel), so that both give the same bits.
struct PanoCam {
    float r00, r01, r02, r10, r11, r12, r20, r21, r22, tx, ty, tz;
};
struct PanoRay {
    float d[3], nrm, radius, noise_var;
};
__device__ __forceinline__ PanoRay pano_ray(int H, int W, const PanoCam& c, int i, int j) {
    const float PI_F = 3.14159265358979323846f;
    auto cam_dir = [&](int ii, int jj, float out[3]) {
        float theta = -((float)jj + 0.5f) / (float)W * 2.f * PI_F;
        float phi = ((float)ii + 0.5f) / (float)H * PI_F;
        float sp = sinf(phi);
        float x = sp * sinf(theta), y = cosf(phi), z = sp * cosf(theta);
        out[0] = x * c.r00 + y * c.r01 + z * c.r02;  // camera_dirs @ c2w[:3,:3].T
        out[1] = x * c.r10 + y * c.r11 + z * c.r12;
        out[2] = x * c.r20 + y * c.r21 + z * c.r22;
    };
    PanoRay r;
    cam_dir(i, j, r.d);
    r.nrm = sqrtf(r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2]);
    // constant pixel radius: |dir(H/2, jj) - dir(H/2, jj+1)| * 2 / sqrt(12); column W-1 repeats column W-3
    int jj = (j < W - 1) ? j : W - 3;
    if (jj < 0) jj = 0;
    float a[3], b[3];
    cam_dir(H / 2, jj, a);
    cam_dir(H / 2, jj + 1 < W ? jj + 1 : jj, b);
    float dx = sqrtf((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
    float phi = ((float)i + 0.5f) / (float)H * PI_F;
    r.radius = (float)((double)dx * 2.0 / sqrt(12.0));
    r.noise_var = sinf(phi) * PI_F / (float)W;
    return r;
}
__device__ __forceinline__ void store_pano_ray(int64_t o, const PanoRay& r, const PanoCam& c, float near_, float far_,
                                               float* origins, float* directions, float* viewdirs, float* radii,
                                               float* lossmult, float* near_out, float* far_out, float* noise_var) {
    origins[o * 3 + 0] = c.tx;
    origins[o * 3 + 1] = c.ty;
    origins[o * 3 + 2] = c.tz;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        directions[o * 3 + k] = r.d[k];
        viewdirs[o * 3 + k] = r.d[k] / r.nrm;
    }
    radii[o] = r.radius;
    lossmult[o] = 1.f;
    near_out[o] = near_;
    far_out[o] = far_;
    noise_var[o] = r.noise_var;
}
