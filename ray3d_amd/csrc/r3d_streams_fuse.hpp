// r3d_streams_fuse: one world skeleton per person from several cameras - per group of streams and joint the gated, weighted mean of
// the world poses r3d_streams_poses wrote this tick, weighted by the re-projection residuals it wrote beside them.  The routines the
// kernel (r3d_k_elementwise.hip) and the host hook (r3d_debug_streams_fuse_host) share, __host__ __device__
// so that the hooks build runs the very same ones on the CPU.  Integers decide first (which slots are candidates); after that the
// arithmetic is float64 with floating-point contraction OFF: every operation rounds once, slots are visited in ascending order and
// sums start from zero, the divisions and the square roots are the correctly rounded ones on both sides - the two are held to the
// same bits.  The reference is monocular and has no counterpart: include/ray3d_hip.h is the definition.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_streams_poses.hpp"

namespace r3d {

// r3d_streams_fuse: the arguments of r3d_k_streams_fuse.  blockIdx.x names a group,
// thread j < J one joint of it.
struct StreamsFuseArgs {
    const double *world;                // (S, J, 3): what r3d_streams_poses wrote
    const double *reproj;               // (S, J) or nullptr: every weight is 1
    const long long *emit;              // S words of r3d_streams_step
    const int32_t *status;              // S words of r3d_streams_step
    const uint32_t *synthetic;          // S words of r3d_streams_repair, or nullptr
    const int32_t *member;              // (G, M) stream index per slot, < 0: empty
    double *fused;                      // (G, J, 3)
    double *spread;                     // (G, J) or nullptr
    int32_t *count;                     // (G, J) or nullptr
    uint32_t *used;                     // (G, M) or nullptr
    double soft_px, max_px, max_dist;   // > 0; <= 0: off; <= 0: off
    int S, J, G, M;
};

constexpr int STREAMS_FUSE_THREADS = 64;      // one wavefront per group: J <= 17 threads of it own a joint
constexpr int STREAMS_FUSE_JOINTS = 17;       // the stride of the kernel's staging area
// doubles of one joint's staging area at stride 1: x, y, z and the weight of up to R3D_FUSE_MAX_MEMBERS candidates (the kernel keeps
// J <= 17 of them side by side in LDS - component c of slot m of joint j at (c * R3D_FUSE_MAX_MEMBERS + m) * 17 + j, so that the
// wavefront's threads read consecutive doubles -: 4 * 16 * 17 * 8 = 8704 bytes)
constexpr int STREAMS_FUSE_STAGE = 4 * R3D_FUSE_MAX_MEMBERS;

// Finite, on the exponent bits (a comparison the compiler may fold under fast-math assumptions is not used)
__host__ __device__ inline bool stream_finite_bits64(double v) {
    return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// d(a, b) squared: ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded once
__host__ __device__ inline double stream_fuse_q(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double s = xx + yy;
    return s + zz;
}

// Joint j of group g.  `st` is the joint's staging area: component c (x, y, z, weight) of slot m at st[(c * R3D_FUSE_MAX_MEMBERS + m) *
// stride] - written for the candidates only and read back for them only, by this thread alone.  Writes fused, spread and count of
// (g, j) -> the inliers' slots as a bit mask (bit m: slot m contributed to joint j).
__host__ __device__ inline uint32_t stream_fuse_joint(const StreamsFuseArgs &a, int g, int j, double *st, int stride) {
#pragma clang fp contract(off)
    constexpr int MM = R3D_FUSE_MAX_MEMBERS;
    double *X = st, *Y = st + (long long)MM * stride, *Z = st + 2ll * MM * stride, *W = st + 3ll * MM * stride;
    // 1. candidates: integers decide.  The one index taken from device memory, a member word, is range-checked before use.
    uint32_t cand = 0, syn = 0;
    const double ss = a.soft_px * a.soft_px;
    for (int m = 0; m < a.M; ++m) {
        const int s = a.member[(long long)g * a.M + m];      // (one address for the workgroup; g < G, m < M)
        if (s < 0 || s >= a.S) continue;                       // not followed: nothing of it is read
        if (!stream_finished(a.status[s], a.emit[s])) continue;
        const long long at = (long long)s * a.J + j;
        const double x = a.world[3 * at], y = a.world[3 * at + 1], z = a.world[3 * at + 2];
        if (!(stream_finite_bits64(x) && stream_finite_bits64(y) && stream_finite_bits64(z))) continue;
        double w = 1.0;
        if (a.reproj) {
            const double r = a.reproj[at];
            if (!stream_finite_bits64(r)) continue;
            if (a.max_px > 0.0 && !(r <= a.max_px)) continue;
            const double rr = r * r;
            const double sum = ss + rr;
            w = 1.0 / sum;
        }
        X[m * stride] = x;
        Y[m * stride] = y;
        Z[m * stride] = z;
        W[m * stride] = w;
        cand |= 1u << m;
        if (a.synthetic && ((a.synthetic[s] >> j) & 1u)) syn |= 1u << m;
    }
    if (cand & ~syn) cand &= ~syn;       // the tier rule: a made-up keypoint does not vote against an observed one
    // 3. the gate: the weighted medoid and what lies within max_dist of it
    uint32_t inl = cand;
    if (a.max_dist > 0.0 && (cand & (cand - 1u))) {
        int best = -1;
        double c_best = 0.0;
        for (int m = 0; m < a.M; ++m) {
            if (!((cand >> m) & 1u)) continue;
            double c = 0.0;
            for (int t = 0; t < a.M; ++t) {
                if (t == m || !((cand >> t) & 1u)) continue;
                const double d = sqrt(stream_fuse_q(X[m * stride], Y[m * stride], Z[m * stride], X[t * stride], Y[t * stride], Z[t * stride]));
                const double wd = W[t * stride] * d;
                c = c + wd;
            }
            if (best < 0 || c < c_best) {        // ties and NaN costs keep the earlier slot
                best = m;
                c_best = c;
            }
        }
        inl = 0;
        for (int m = 0; m < a.M; ++m) {
            if (!((cand >> m) & 1u)) continue;
            const double d = sqrt(stream_fuse_q(X[best * stride], Y[best * stride], Z[best * stride], X[m * stride], Y[m * stride], Z[m * stride]));
            if (d <= a.max_dist) inl |= 1u << m;
        }
    }
    // 4. the outputs
    double den = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    int n = 0;
    for (int m = 0; m < a.M; ++m) {
        if (!((inl >> m) & 1u)) continue;
        const double w = W[m * stride];
        const double wx = w * X[m * stride], wy = w * Y[m * stride], wz = w * Z[m * stride];
        den = den + w;
        nx = nx + wx;
        ny = ny + wy;
        nz = nz + wz;
        ++n;
    }
    const double fx = nx / den, fy = ny / den, fz = nz / den;
    const long long out = (long long)g * a.J + j;
    a.fused[3 * out] = stream_canon_f64(fx, n == 0);
    a.fused[3 * out + 1] = stream_canon_f64(fy, n == 0);
    a.fused[3 * out + 2] = stream_canon_f64(fz, n == 0);
    if (a.spread) {
        double acc = 0.0;
        for (int m = 0; m < a.M; ++m) {
            if (!((inl >> m) & 1u)) continue;
            const double wq = W[m * stride] * stream_fuse_q(fx, fy, fz, X[m * stride], Y[m * stride], Z[m * stride]);
            acc = acc + wq;
        }
        const double v = acc / den;
        a.spread[out] = stream_canon_f64(sqrt(v), n == 0);
    }
    if (a.count) a.count[out] = n;
    return inl;
}

}  // namespace r3d
