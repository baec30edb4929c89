// R3D_INPUT_UV_DIST: the per-keypoint arithmetic of the undistortion pre-pass (r3d_k_undistort.hip), __host__ __device__ so
// that the hooks build runs the very same routine on the CPU (r3d_debug_undistort_host).  float64 throughout, in the
// reference's order (lib/camera/camera.py:412-441): cv2.undistortPoints(uv, K, dist, P=K) - five fixed-point iterations of
// OpenCV's documented algorithm for the 5-coefficient Brown-Conrady model, then re-projection with K - followed by the
// ray encoding of get_cam_ray_given_uv (:460-471).  PARITY UNPINNED against cv2 itself (OpenCV is not a dependency of this
// project); pinned against the restatements in ray3d_amd/camera.py, oracle.undistort_points and tests/golden/undistort.npz.
#pragma once

#include <hip/hip_runtime.h>

namespace r3d {

// A camera row of R3D_INPUT_UV_DIST: {fx, fy, cx, cy, cos(pitch), sin(pitch), 0, 0, k1, k2, p1, p2, k3, 0, 0, 0}
constexpr int UNDIST_ROW_DOUBLES = 16;

struct UndistRow { double fx, fy, cx, cy, c, s, k1, k2, p1, p2, k3; };

__host__ __device__ inline UndistRow undist_row(const double *r) {
    return UndistRow{r[0], r[1], r[2], r[3], r[4], r[5], r[8], r[9], r[10], r[11], r[12]};
}

// All five coefficients zero: the reference's undistort=False - no iteration, no re-projection (bit-identical to UV mode)
__host__ __device__ inline bool undist_identity(const UndistRow &k) {
    return k.k1 == 0.0 && k.k2 == 0.0 && k.p1 == 0.0 && k.p2 == 0.0 && k.k3 == 0.0;
}

// Pixel (u, v) with the lens distortion removed, in pixels (Camera.undistort_points of ray3d_amd/camera.py, term for term).
// Divisions are IEEE (correctly rounded) in both compilations: no reciprocal approximations.
__host__ __device__ inline void undistort_pixel(const UndistRow &k, double u, double v, double &uo, double &vo) {
    if (undist_identity(k)) { uo = u; vo = v; return; }
    const double x0 = (u - k.cx) / k.fx, y0 = (v - k.cy) / k.fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icd = 1.0 / (1 + ((k.k3 * r2 + k.k2) * r2 + k.k1) * r2);
        const double dx = 2 * k.p1 * x * y + k.p2 * (r2 + 2 * x * x);
        const double dy = k.p1 * (r2 + 2 * y * y) + 2 * k.p2 * x * y;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    uo = x * k.fx + k.cx;                   // re-projection with P = K
    vo = y * k.fy + k.cy;
}

// The ray of an (undistorted) pixel: ((u-cx)/fx, c*y+s, -s*y+c) with y = (v-cy)/fy - the expressions of uv_to_ray
// (r3d_tiles.hpp), so that zero coefficients give UV mode's values bit for bit.
__host__ __device__ inline void pixel_to_ray(const UndistRow &k, double u, double v, double r[3]) {
    const double tx = (u - k.cx) / k.fx;
    const double t = (v - k.cy) / k.fy;
    r[0] = tx;
    r[1] = k.c * t + k.s;
    r[2] = -k.s * t + k.c;
}

}  // namespace r3d
