// r3d_clips_project: a virtual camera's view of a world pose - the per-point arithmetic in front of the encoding, __host__
// __device__ so that the hooks build runs the very same routines on the CPU (r3d_debug_clips_project_host).  The pixel is
// CameraInfoPacket.project (lib/camera/camera.py:485-496) on catesian2homogenous of the float32 world point: h = P [x y z 1]^T with
// P = K [R|t] (camera.py:231), u = h0 / h2, v = h1 / h2, float64 throughout, no distortion.  Every product and every sum is rounded
// once, in the order ((P0 x + P1 y) + P2 z) + P3: floating-point contraction is OFF, as in pose_world of r3d_poses.hpp - an FMA would
// round a product and a sum together, the compiler forms them on the device and not on the host, and the two are held to the same
// bits.  The divisions are IEEE (correctly rounded) in both compilations.  The ground truth is pose_world itself with the
// descriptor's world -> ground-truth-frame transform, cast once through encoded_f32 (r3d_undistort.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_poses.hpp"
#include "r3d_undistort.hpp"

namespace r3d {

// The pixel of world point p through the row-major 3x4 projection matrix P.  A point in the camera's plane (h2 == 0) or behind it
// divides as IEEE does: +-Inf, NaN (0 / 0) or a mirrored pixel - not an error, the caller's in-frame verdict sees it.
__host__ __device__ inline void project_pixel(const double *P, const float p[3], double &u, double &v) {
#pragma clang fp contract(off)
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    double h[3];
    for (int k = 0; k < 3; ++k) {
        const double a = P[4 * k] * x, b = P[4 * k + 1] * y, c = P[4 * k + 2] * z;
        const double ab = a + b;
        const double abc = ab + c;
        h[k] = abc + P[4 * k + 3];
    }
    u = h[0] / h[2];
    v = h[1] / h[2];
}

// check_in_frame (data/camera_augmentation.py) with the comparisons turned round so that a NaN pixel is OUTSIDE: the reference's
// `u < 0 or u > w or ...` is false for a NaN and would call it inside.
__host__ __device__ inline bool pixel_outside(double u, double v, double res_w, double res_h) {
    return !(u >= 0.0 && u <= res_w && v >= 0.0 && v <= res_h);
}

// A descriptor the call follows (include/ray3d_hip.h: "invalid descriptors", written so that no sum can overflow): the rule of
// r3d_clips_encode on the source frames and the output rows and - when the call writes gt_dev or px_dev (`has_gt`) - the clip's n
// ground-truth rows inside [0, gt_rows).
__host__ __device__ inline bool clip_project_valid(long long first, long long n, long long out_first, int pad_front, int pad_back,
                                                   long long gt_first, long long total_frames, long long out_rows, long long max_rows,
                                                   long long gt_rows, bool has_gt) {
    if (!clip_input_valid(first, n, out_first, pad_front, pad_back, total_frames, out_rows, max_rows)) return false;
    return !has_gt || (gt_first >= 0 && n <= gt_rows && gt_first <= gt_rows - n);
}

}  // namespace r3d
