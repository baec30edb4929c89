// r3d_streams_poses: the output side of a live tick - for every stream that finished a frame this tick (what r3d_streams_step left in
// emit / status) the flip average and the world transform of r3d_poses.hpp, and the one quality signal a stream without ground truth
// has: the distance, in undistorted pixels, between the projection of the predicted absolute pose (normalized2camera,
// lib/camera/camera.py:379-388, then the pinhole division) and the keypoints that were fed in (get_uv_given_cam_ray,
// camera.py:473-483; the overlay of lib/train_val/trainer.py:535-537).  The routines the kernel (r3d_k_elementwise.hip) and the
// host hook (r3d_debug_streams_poses_host) share, __host__ __device__ so that the hooks build runs the very same ones on the CPU. 
// Floating-point contraction is OFF (r3d_poses.hpp says why); the divisions and the square root are the
// correctly rounded float64 ones on both sides, so the two are held to the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_poses.hpp"
#include "r3d_undistort.hpp"

namespace r3d {

// r3d_streams_poses: the arguments of r3d_k_streams_poses.  blockIdx.x names a stream,
// thread j < J one joint of it.
struct StreamsPosesArgs {
    const float *raw, *raw_mirror;      // (S, J, 3): what the forwards wrote; raw_mirror nullptr: no flip pass
    const long long *emit;              // S words of r3d_streams_step
    const int32_t *status;              // S words of r3d_streams_step
    const r3d_stream_pose_desc *desc;   // S descriptors; nullptr: neither world nor reproj
    const double *cam;                  // (S, 16) camera rows; nullptr: no reproj
    const float *x;                     // (S, RF, J, 3) windows; nullptr: no reproj
    float *pred;                        // (S, J, 3) or nullptr
    double *world;                      // (S, J, 3) or nullptr
    double *reproj;                     // (S, J) or nullptr
    double *quality;                    // (S, 2) or nullptr (only with reproj)
    unsigned long long mirror_perm[2];  // pose_pack_perm (r3d_poses.hpp)
    int S, J, RF, lag;
};

constexpr int STREAMS_POSES_THREADS = 64;     // one wavefront per stream: J <= 17 threads of it work

// A stream the call follows: r3d_streams_step followed it and wrote a window for it this tick
__host__ __device__ inline bool stream_finished(int status, long long emit) { return status == 0 && emit >= 0; }

// The canonical quiet NaN for a NaN, decided on the BITS: written as `v != v ? qnan : v` the compiler drops the selection behind a
// square root (any NaN is as good as another to it), on the host and on the device alike, and the two then differ in the payload
constexpr unsigned long long STREAM_QNAN64 = 0x7ff8000000000000ull;
__host__ __device__ __forceinline__ double stream_canon_f64(const double v, const bool force = false) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return __builtin_bit_cast(double, (force || (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) ? STREAM_QNAN64 : b);
}

// The residual of one joint: `cam` the stream's camera row (fx, fy, cx, cy, cos, sin ...: r3d_undistort.hpp), `h` the camera height,
// `p` the finished point (pos + trj, normalised frame), `r` the ray that was fed in for the joint (the window's current-frame row).
// Predicted: normalized2camera is Rn2c (p - Tc2n), Tc2n = (0, -h, 0), Rn2c = [1 0 0; 0 c -s; 0 s c]; then x / z, y / z.  Observed:
// rows 0 and 1 of Rn2c r - the reference does not divide by the third component.  The principal point cancels and is not read.
__host__ __device__ inline double stream_reproj(const double *cam, double h, const float p[3], const float r[3]) {
#pragma clang fp contract(off)
    const double fx = cam[0], fy = cam[1], c = cam[4], sn = cam[5];
    const double yy = (double)p[1] + h, z = (double)p[2];
    const double Xc = (double)p[0];
    const double cy = c * yy, sz = sn * z, sy = sn * yy, cz = c * z;
    const double Yc = cy - sz;
    const double Zc = sy + cz;
    const double a = Xc / Zc, b = Yc / Zc;
    const double xo = (double)r[0];
    const double c1 = c * (double)r[1], s2 = sn * (double)r[2];
    const double yo = c1 - s2;
    const double ex = a - xo, ey = b - yo;
    const double du = fx * ex, dv = fy * ey;
    const double uu = du * du, vv = dv * dv;
    return stream_canon_f64(sqrt(uu + vv));
}

// The two quality words of a stream from its J residuals: the mean (summed in joint order from zero, one division) and the maximum;
// both the canonical quiet NaN when any residual is one
__host__ __device__ inline void stream_quality(const double *res, int J, double out[2]) {
#pragma clang fp contract(off)
    double sum = 0.0, mx = res[0];
    bool nan = false;
    for (int j = 0; j < J; ++j) {
        const double v = res[j];
        nan = nan || v != v;
        sum = sum + v;
        if (v > mx) mx = v;
    }
    out[0] = stream_canon_f64(sum / (double)J, nan);
    out[1] = stream_canon_f64(mx, nan);
}

// Joint j of finished stream s: the point, its stores, and the residual (0 when reproj is not asked for)
__host__ __device__ inline double stream_pose_point(const StreamsPosesArgs &u, int s, int j) {
    const long long at = (long long)s * u.J + j;
    const float *mir = u.raw_mirror ? u.raw_mirror + 3 * ((long long)s * u.J + pose_mirror_source(u.mirror_perm[0], u.mirror_perm[1], j)) : nullptr;
    float p[3];
    pose_finish(u.raw + 3 * at, mir, p);
    if (u.pred) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(u.pred) + 3 * at;      // (32-bit patterns: a copied NaN keeps its payload)
        dst[0] = __builtin_bit_cast(uint32_t, p[0]);
        dst[1] = __builtin_bit_cast(uint32_t, p[1]);
        dst[2] = __builtin_bit_cast(uint32_t, p[2]);
    }
    if (u.world) {
        double w[3];
        pose_world(u.desc[s].rn2w, u.desc[s].tn2w, p, w);
        u.world[3 * at] = w[0];
        u.world[3 * at + 1] = w[1];
        u.world[3 * at + 2] = w[2];
    }
    if (!u.reproj) return 0.0;
    // (S * RF * J fits in 31 bits - checked on the host; row RF - 1 - lag lies in [0, RF))
    const float *r = u.x + 3 * (((long long)s * u.RF + (u.RF - 1 - u.lag)) * u.J + j);
    const float ray[3] = {r[0], r[1], r[2]};
    const double e = stream_reproj(u.cam + (long long)s * UNDIST_ROW_DOUBLES, u.desc[s].height, p, ray);
    u.reproj[at] = e;
    return e;
}

}  // namespace r3d
