// r3d_clips_poses: what lies between a shard's forwards and its measurement - the flip average of lib/train_val/trainer.py:340-346
// and the world transform of lib/camera/camera.py:401-410 - per output point, __host__ __device__ so that the hooks build runs
// the very same routines on the CPU (r3d_debug_clips_poses_host).  The rounding contract of include/ray3d_hip.h: without a mirrored
// pass the raw bits are copied; with one the point is fl32(fl32(raw + m) * 0.5f), m the mirrored pass's point with component 0
// negated; the world point is computed from that float32 value promoted to float64, every product and every sum rounded once.
// Floating-point contraction is OFF in both routines: an FMA would round a product and a sum together, and the compiler forms
// them on the device and not on the host - the two are held to the same bits.  A NaN RESULT of the arithmetic leaves as the
// canonical quiet NaN (which operand's sign and payload a NaN result carries differs between the GPU and a host CPU); a raw
// value that is only copied keeps its bits, NaN payloads included.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ray3d_hip.h"
#include "r3d_valid.hpp"

namespace r3d {

// mirror_perm (J entries of 0..J-1: the caller checked), five bits each, twelve to a word: kernel arguments, read with shifts
__host__ __device__ inline int pose_mirror_source(unsigned long long w0, unsigned long long w1, int j) {
    return (int)((j < 12 ? w0 >> (5 * j) : w1 >> (5 * (j - 12))) & 31ull);
}
inline void pose_pack_perm(const int32_t *perm, int J, unsigned long long w[2]) {
    w[0] = w[1] = 0ull;
    for (int j = 0; j < J; ++j) w[j < 12 ? 0 : 1] |= (unsigned long long)perm[j] << (5 * (j < 12 ? j : j - 12));
}

// A descriptor the call follows (include/ray3d_hip.h: "invalid descriptors", written so that no sum can overflow): the rule of
// r3d_clips_metrics on the output rows, and the clip's n raw rows inside [0, raw_rows).
__host__ __device__ inline bool clip_pose_valid(long long first, long long n, long long raw_first, long long total_frames,
                                                long long max_frames, long long raw_rows) {
    return clip_range_valid(first, n, total_frames, max_frames) && raw_first >= 0 && n <= raw_rows && raw_first <= raw_rows - n;
}

__host__ __device__ __forceinline__ float pose_f32(const float v) {
    return v != v ? __builtin_bit_cast(float, 0x7fc00000u) : v;
}
__host__ __device__ __forceinline__ double pose_f64(const double v) {
    return v != v ? __builtin_bit_cast(double, 0x7ff8000000000000ull) : v;
}

// The finished point: `raw` the straight pass's three floats; `mir` the mirrored pass's three floats of joint mirror_perm[j] in
// the same row, or null (no flip pass: the bits of `raw`).  torch.add(dst, mirror_output(pred_m)); dst.mul_(0.5) in float32.
__host__ __device__ inline void pose_finish(const float *raw, const float *mir, float p[3]) {
#pragma clang fp contract(off)
    if (!mir) {
        memcpy(p, raw, 3 * sizeof(float));
        return;
    }
    const float m0 = -mir[0], m1 = mir[1], m2 = mir[2];
    const float s0 = raw[0] + m0, s1 = raw[1] + m1, s2 = raw[2] + m2;
    p[0] = pose_f32(s0 * 0.5f);
    p[1] = pose_f32(s1 * 0.5f);
    p[2] = pose_f32(s2 * 0.5f);
}

// p @ R^T + T^T in float64 (camera.py:401-410), R row-major: component r = ((R[3r] x + R[3r+1] y) + R[3r+2] z) + T[r]
__host__ __device__ inline void pose_world(const double *R, const double *T, const float p[3], double w[3]) {
#pragma clang fp contract(off)
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    for (int r = 0; r < 3; ++r) {
        const double a = R[3 * r] * x, b = R[3 * r + 1] * y, c = R[3 * r + 2] * z;
        const double ab = a + b;
        const double abc = ab + c;
        w[r] = pose_f64(abc + T[r]);
    }
}

}  // namespace r3d
