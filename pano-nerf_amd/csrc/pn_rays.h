// pn_rays.h — one ray of any camera: what every ray generator of the library (pn_cameras.hip: the panorama pool
// generator and the batch samplers of all camera kinds) is built from, so that all of them give the same bits.
// A pool row (camera * H W + pixel) is decoded once (decode_row), the camera builds the pixel's RayRow, store_ray writes
// the eight Rays fields.  Further down, the way back: image_pos (direction -> image position of any central camera) and
// bilinear_taps, templated over fp32 / fp64 for pn_cameras.hip and pn_ibl.hip; pn_fusion.hip and pn_relight.hip restate them.
// Every expression keeps its parenthesisation: the library builds with -ffp-contract=off.
#pragma once
#include "pn_common.h"

// the eight Rays fields of a batch plus the gathered target colours (rgb_out may be null)
struct RayOut {
    float *origins, *directions, *viewdirs, *radii, *lossmult, *near_out, *far_out, *noise_var, *rgb_out;
};
struct RayRow {
    float o[3], d[3], v[3], radius, lossmult, noise_var;
};
__device__ __forceinline__ void store_ray(int64_t b, const RayRow& r, float near_, float far_, const RayOut& out) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out.origins[b * 3 + k] = r.o[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out.directions[b * 3 + k] = r.d[k];
        out.viewdirs[b * 3 + k] = r.v[k];
    }
    out.radii[b] = r.radius;
    out.lossmult[b] = r.lossmult;
    out.near_out[b] = near_;
    out.far_out[b] = far_;
    out.noise_var[b] = r.noise_var;
}

// pool row r -> (row, camera, pixel); an index outside the pool reads ray 0
struct RowId {
    int64_t row;
    int cam, pix;
};
__device__ __forceinline__ RowId decode_row(int64_t r, int64_t hw, int n_cam) {
    r = (r >= 0 && r < hw * n_cam) ? r : 0;
    return RowId{r, (int)(r / hw), (int)(r % hw)};
}

// out = m[:3, :3] @ c for a row-major matrix of leading dimension ld: 3-term fp32 dot products in index order
__device__ __forceinline__ void rotate3(const float* m, int ld, const float c[3], float out[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (m[ld * k] * c[0] + m[ld * k + 1] * c[1]) + m[ld * k + 2] * c[2];
}

// mip-NeRF cone radius of pixel (i, j) from the next row's direction: |dir(y, j) - dir(y + 1, j)| * 2 / sqrt(12), rows
// counted within [top, top + rows); the last row reuses the one before
template <class Dir>
__device__ __forceinline__ float row_step_radius(int rows, int top, int i, int j, Dir dir) {
    const int y = i - top;
    const int yy = y < rows - 1 ? y : rows - 2;
    float a[3], n[3];
    dir(top + yy, j, a);
    dir(top + yy + 1, j, n);
    const float dx = sqrtf((a[0] - n[0]) * (a[0] - n[0]) + (a[1] - n[1]) * (a[1] - n[1]) + (a[2] - n[2]) * (a[2] - n[2]));
    return (float)((double)dx * 2.0 / sqrt(12.0));
}

// One pixel of an equirectangular camera (datasets/pano_datasets.py:157-213)
struct PanoCam {
    float r00, r01, r02, r10, r11, r12, r20, r21, r22, tx, ty, tz;
};
__host__ __device__ inline PanoCam pano_cam(const float* m) {  // of a row-major c2w [4, 4]
    return PanoCam{m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10], m[3], m[7], m[11]};
}
// the panorama's ray of pixel (i, j): every field but near and far
__device__ __forceinline__ RayRow pano_ray(int H, int W, const PanoCam& c, int i, int j) {
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
    RayRow r;
    r.o[0] = c.tx, r.o[1] = c.ty, r.o[2] = c.tz;
    cam_dir(i, j, r.d);
    const float nrm = sqrtf(r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2]);
    // constant pixel radius: |dir(H/2, jj) - dir(H/2, jj+1)| * 2 / sqrt(12); column W-1 repeats column W-3
    int jj = (j < W - 1) ? j : W - 3;
    if (jj < 0) jj = 0;
    float a[3], b[3];
    cam_dir(H / 2, jj, a);
    cam_dir(H / 2, jj + 1 < W ? jj + 1 : jj, b);
    float dx = sqrtf((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
    float phi = ((float)i + 0.5f) / (float)H * PI_F;
    r.radius = (float)((double)dx * 2.0 / sqrt(12.0));
    r.lossmult = 1.f;
    r.noise_var = sinf(phi) * PI_F / (float)W;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.v[k] = r.d[k] / nrm;  // last: nrm, not three quotients, stays live over the radius
    return r;
}

// ------------------------------------------------------------------------------------------------- pixel -> direction
// camera-space direction of the continuous cube-strip position (px, py); face = the strip's face of py
__device__ __forceinline__ void cube_dir(int S, float px, float py, float d[3]) {
    int face = (int)floorf(py / (float)S);
    face = face < 0 ? 0 : (face > 5 ? 5 : face);
    const float s = 2.f * px / (float)S - 1.f;
    const float t = 2.f * (py - (float)(face * S)) / (float)S - 1.f;
    switch (face) {
        case 0: d[0] = 1.f, d[1] = -t, d[2] = -s; break;
        case 1: d[0] = -1.f, d[1] = -t, d[2] = s; break;
        case 2: d[0] = s, d[1] = 1.f, d[2] = t; break;
        case 3: d[0] = s, d[1] = -1.f, d[2] = -t; break;
        case 4: d[0] = s, d[1] = -t, d[2] = 1.f; break;
        default: d[0] = -s, d[1] = -t, d[2] = -1.f; break;
    }
}

// math functions and pi by the type of the operands: what lets one template serve fp32 and fp64
__device__ __forceinline__ float atan2_t(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double atan2_t(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ float hypot_t(float x, float y) { return hypotf(x, y); }
__device__ __forceinline__ double hypot_t(double x, double y) { return hypot(x, y); }
__device__ __forceinline__ float floor_t(float x) { return floorf(x); }
__device__ __forceinline__ double floor_t(double x) { return floor(x); }
__device__ __forceinline__ float abs_t(float x) { return fabsf(x); }
__device__ __forceinline__ double abs_t(double x) { return fabs(x); }
template <class T>
struct PiOf;  // pi as T: the fp32 constant is its own literal, not a rounded kPiD
template <>
struct PiOf<float> {
    static constexpr float value = 3.14159265358979323846f;
};
template <>
struct PiOf<double> {
    static constexpr double value = kPiD;
};

// the inverse: direction d -> the strip's face and the continuous position (px, py) within that face of a cube of size
// S.  The major axis picks the face, ties to the earlier face of +x -x +y -y +z -z; false for a zero or NaN direction.
// pn_reproject looks up in fp32, the IBL evaluation (pn_ibl.hip) in fp64: one definition, the same faces.
template <class T>
__device__ __forceinline__ bool cube_pos(int S, const T d[3], T& px, T& py, int& face) {
    const T ax = abs_t(d[0]), ay = abs_t(d[1]), az = abs_t(d[2]);
    T s, t, mj;
    if (ax >= ay && ax >= az) {
        mj = ax;
        if (d[0] > (T)0) face = 0, s = -d[2] / mj, t = -d[1] / mj;
        else face = 1, s = d[2] / mj, t = -d[1] / mj;
    } else if (ay >= az) {
        mj = ay;
        if (d[1] > (T)0) face = 2, s = d[0] / mj, t = d[2] / mj;
        else face = 3, s = d[0] / mj, t = -d[2] / mj;
    } else {
        mj = az;
        if (d[2] > (T)0) face = 4, s = d[0] / mj, t = -d[1] / mj;
        else face = 5, s = -d[0] / mj, t = -d[1] / mj;
    }
    if (!(mj > (T)0)) return false;
    px = (s + (T)1) * ((T)0.5 * (T)S);
    py = (t + (T)1) * ((T)0.5 * (T)S);
    return true;
}

// equidistant fisheye: unit camera-space direction of (px, py) and its angle from the axis
__device__ __forceinline__ float fisheye_dir(int H, int W, float f, float px, float py, float d[3]) {
    const float u = px - 0.5f * (float)W, v = -(py - 0.5f * (float)H);
    const float r = hypotf(u, v);
    const float theta = r / f;
    if (r > 0.f) {
        float sn, cs;
        sincosf(theta, &sn, &cs);
        d[0] = sn * u / r;
        d[1] = sn * v / r;
        d[2] = -cs;
    } else {
        d[0] = 0.f, d[1] = 0.f, d[2] = -1.f;
    }
    return theta;
}

__device__ __forceinline__ void normalize3(float d[3]) {
    const float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = d[k] / n;
}

// ------------------------------------------------------------------------------------------------- direction -> pixel
// The inverse projections and the bilinear tap rule of include/panonerf_hip.h, once, over T = float (pn_reproject, the
// warps) and T = double (the cube maps of pn_ibl; TSDF fusion and pn_relight keep a written-out copy): the same trees
// in either precision, the math functions picked by overload.
// camera-space direction d -> the continuous image position (px, py) of a camera of `kind` (centres at k + 1/2) and, for
// a cube, the face, with py counted within it; false where the camera does not see d.  Of the camera's params PINHOLE
// reads cam2pix at [9, 18), FISHEYE f and theta_max at [0] and [1], the others nothing (params may be null).
// A caller whose kind is a compile-time constant keeps that kind's projection only.
template <class T>
__device__ __forceinline__ bool image_pos(int kind, int H, int W, const float* params, const T d[3], T& px, T& py, int& face) {
    constexpr T pi = PiOf<T>::value;
    face = 0;
    if (kind == PN_CAM_PANO) {
        const T phi = atan2_t(hypot_t(d[0], d[2]), d[1]), theta = atan2_t(d[0], d[2]);
        T t = -theta / ((T)2 * pi);
        t = t - floor_t(t);
        px = t * (T)W;
        py = phi / pi * (T)H;
        return true;
    }
    if (kind == PN_CAM_PINHOLE) {
        T q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = ((T)params[9 + 3 * k] * d[0] + (T)params[10 + 3 * k] * d[1]) + (T)params[11 + 3 * k] * d[2];
        if (!(q[2] > (T)0)) return false;
        px = q[0] / q[2];
        py = q[1] / q[2];
        return px >= (T)0 && px <= (T)W && py >= (T)0 && py <= (T)H;
    }
    if (kind == PN_CAM_FISHEYE) {
        const T rho = hypot_t(d[0], d[1]);
        const T theta = atan2_t(rho, -d[2]);
        if (!(theta <= (T)params[1])) return false;
        const T r = (T)params[0] * theta;
        px = (T)0.5 * (T)W, py = (T)0.5 * (T)H;
        if (rho > (T)0) {  // the axis itself lands on the centre
            px = px + r * d[0] / rho;
            py = py - r * d[1] / rho;
        }
        return px >= (T)0 && px <= (T)W && py >= (T)0 && py <= (T)H;
    }
    return cube_pos<T>(W, d, px, py, face);
}

// the four bilinear taps of a continuous position: pixel index (row * W + column, of index type I) and weight of
// (y0, x0) (y0, x1) (y1, x0) (y1, x1); every caller adds the products as ((w0 c0 + w1 c1) + w2 c2) + w3 c3
template <class T, class I>
struct Taps {
    I o[4];
    T w[4];
};

// taps of image_pos' (px, py, face): columns wrap for a panorama and clamp otherwise, rows clamp; a cube's taps clamp
// within its face.  The indices are computed in I throughout.
template <class T, class I>
__device__ __forceinline__ Taps<T, I> bilinear_taps(int kind, int H, int W, T px, T py, int face) {
    const T gx = px - (T)0.5, gy = py - (T)0.5;
    const T fx = floor_t(gx), fy = floor_t(gy);
    const T wx = gx - fx, wy = gy - fy;
    I x0 = (I)fx, y0 = (I)fy, x1 = x0 + 1, y1 = y0 + 1;
    const int rows = kind == PN_CAM_CUBE ? W : H;
    if (kind == PN_CAM_PANO) {
        x0 = ((x0 % W) + W) % W;
        x1 = ((x1 % W) + W) % W;
    } else {
        x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);
        x1 = x1 < 0 ? 0 : (x1 > W - 1 ? W - 1 : x1);
    }
    y0 = y0 < 0 ? 0 : (y0 > rows - 1 ? rows - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 > rows - 1 ? rows - 1 : y1);
    const I top = kind == PN_CAM_CUBE ? (I)face * W : 0;
    Taps<T, I> t;
    t.o[0] = (top + y0) * W + x0;
    t.o[1] = (top + y0) * W + x1;
    t.o[2] = (top + y1) * W + x0;
    t.o[3] = (top + y1) * W + x1;
    t.w[0] = ((T)1 - wy) * ((T)1 - wx);
    t.w[1] = ((T)1 - wy) * wx;
    t.w[2] = wy * ((T)1 - wx);
    t.w[3] = wy * wx;
    return t;
}

// ------------------------------------------------------------------------------------------------------------ cameras
// A camera kind is a struct with RayRow ray(cam, i, j): the ray of pixel (i, j) of camera `cam` of n_cam sharing one
// model, each with its own c2w (c2ws [n_cam, 16]).  k_sample_rays (pn_cameras.hip) is instantiated once per kind.
struct PanoCams {
    int H, W;
    const float* c2ws;
    __device__ __forceinline__ RayRow ray(int cam, int i, int j) const { return pano_ray(H, W, pano_cam(c2ws + 16 * (int64_t)cam), i, j); }
};

// omnidirectional stereo: the panorama's ray from an origin on the viewing circle; half = +ipd / 2 for the right eye,
// -ipd / 2 for the left, and 0 keeps the panorama's origin bits
struct StereoPanoCams {
    int H, W;
    const float* c2ws;
    float half;
    __device__ __forceinline__ RayRow ray(int cam, int i, int j) const {
        const float* m = c2ws + 16 * (int64_t)cam;
        float o[3] = {m[3], m[7], m[11]};
        if (half != 0.f) {  // before pano_ray: three values stay live over it, not the whole row over this
            const float theta = -((float)j + 0.5f) / (float)W * 2.f * 3.14159265358979323846f;  // pano_ray's heading angle
            const float off[3] = {half * -cosf(theta), 0.f, half * sinf(theta)};
            float w[3];
            rotate3(m, 4, off, w);
            o[0] = w[0] + m[3];
            o[1] = w[1] + m[7];
            o[2] = w[2] + m[11];
        }
        RayRow r = pano_ray(H, W, pano_cam(m), i, j);
#pragma unroll
        for (int k = 0; k < 3; ++k) r.o[k] = o[k];
        return r;
    }
};

// a central camera's ray from its world direction d: origin c2w[:3, 3], no noise
__device__ __forceinline__ RayRow central_ray(const float* m, const float d[3], const float v[3], float radius, float lossmult) {
    RayRow r;
    r.o[0] = m[3], r.o[1] = m[7], r.o[2] = m[11];
#pragma unroll
    for (int k = 0; k < 3; ++k) r.d[k] = d[k], r.v[k] = v[k];
    r.radius = radius;
    r.lossmult = lossmult;
    r.noise_var = 0.f;
    return r;
}

// pinhole: d = c2w[:3,:3] @ (pix2cam @ (px, py, 1)), not normalised; per-camera pix2cams [n_cam, 9]
struct PinholeCams {
    int H, W;
    const float *pix2cams, *c2ws;
    __device__ __forceinline__ RayRow ray(int cam, int i, int j) const {
        const float* p2c = pix2cams + 9 * (int64_t)cam;
        const float* m = c2ws + 16 * (int64_t)cam;
        auto dir = [&](int ii, int jj, float out[3]) {
            const float px = (float)jj + 0.5f, py = (float)ii + 0.5f;
            float c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = (p2c[3 * k] * px + p2c[3 * k + 1] * py) + p2c[3 * k + 2];
            rotate3(m, 4, c, out);
        };
        float d[3], v[3];
        dir(i, j, d);
        const float radius = row_step_radius(H, 0, i, j, dir);
        const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = d[k] / nrm;
        return central_ray(m, d, v, radius, 1.f);
    }
};

// cube-map strip (H = 6 W): unit directions; rows count within the face
struct CubeCams {
    int H, W;
    const float* c2ws;
    __device__ __forceinline__ RayRow ray(int cam, int i, int j) const {
        const float* m = c2ws + 16 * (int64_t)cam;
        auto dir = [&](int ii, int jj, float out[3]) {
            float c[3];
            cube_dir(W, (float)jj + 0.5f, (float)ii + 0.5f, c);
            normalize3(c);
            rotate3(m, 4, c, out);
        };
        float d[3];
        dir(i, j, d);
        return central_ray(m, d, d, row_step_radius(W, (i / W) * W, i, j, dir), 1.f);
    }
};

// equidistant fisheye: unit directions; outside the image circle (theta > theta_max) the forward direction, no loss
struct FisheyeCams {
    int H, W;
    const float* c2ws;
    float f, theta_max;
    __device__ __forceinline__ RayRow ray(int cam, int i, int j) const {
        const float* m = c2ws + 16 * (int64_t)cam;
        auto dir = [&](int ii, int jj, float out[3]) {
            float c[3];
            const float theta = fisheye_dir(H, W, f, (float)jj + 0.5f, (float)ii + 0.5f, c);
            rotate3(m, 4, c, out);
            return theta;
        };
        float d[3];
        const bool inside = dir(i, j, d) <= theta_max;
        const float radius = row_step_radius(H, 0, i, j, dir);
        if (!inside) {
            const float fwd[3] = {0.f, 0.f, -1.f};
            rotate3(m, 4, fwd, d);
        }
        return central_ray(m, d, d, radius, inside ? 1.f : 0.f);
    }
};
