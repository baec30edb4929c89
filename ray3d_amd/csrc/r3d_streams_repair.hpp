// r3d_streams_repair: live streams that survive dropped keypoints - the routines the kernel (r3d_k_elementwise.hip) and the host
// hook (r3d_debug_streams_repair_host) share, __host__ __device__ so that the hooks build runs the very same ones on the CPU: the
// observed test, the track's layout, the per-joint step with its two ring rewrites, the interpolation arithmetic and
// the mask words.  The call runs BEFORE r3d_streams_step of the same tick and judges the head and the action word with that call's
// own stream_step (r3d_streams.hpp), on the head as it stands: it never writes a head.  Floating-point contraction is OFF in the
// interpolation: every operation rounds once, on the host and on the device alike.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_streams.hpp"
#include "r3d_undistort.hpp"

namespace r3d {

// r3d_streams_repair: the arguments of r3d_k_streams_repair.  blockIdx.x names a stream,
// thread j < J one joint of it.
struct StreamsRepairArgs {
    const r3d_stream_head *heads;       // S heads: the front of the state, READ only
    uint32_t *ring;                     // S rings of (RF, J, F) 32-bit patterns, behind the heads
    int32_t *age;                       // the track: (S, J) ages ...
    uint32_t *last;                     // ... (S, J, width) last observed inputs ...
    uint32_t *missing;                  // ... (S, RF) masks of the joints not observed, per ring slot
    const uint32_t *frame;              // (S, J, width) what the caller would have given the step
    const float *conf;                  // (S, J) or nullptr
    const double *cam;                  // (S, 16) camera rows, or nullptr (R3D_ENCODE_NONE)
    const int32_t *action;              // S words
    uint32_t *frame_out;                // (S, J, width) what the step is given
    uint32_t *synthetic;                // S words
    float min_conf;
    int S, RF, lag, J, F, width, encoding, max_gap;
};

constexpr int STREAMS_REPAIR_THREADS = 64;    // one wavefront per stream: J <= 17 threads of it own a joint
constexpr uint32_t STREAM_QNAN32 = 0x7fc00000u;

// bytes of the track: (S, J) int32 ages, (S, J, width) float32 last inputs, (S, RF) uint32 masks, in that order, rounded up to 8
// (the arguments passed the shape rules of r3d_streams_step: no overflow)
inline size_t streams_track_bytes(long long S, long long RF, long long J, long long width) {
    const long long words = S * (J + J * width + RF);
    return (size_t)((words * 4 + 7) / 8 * 8);
}

// Finite, on the exponent bits (a comparison the compiler may fold under fast-math assumptions is not used)
__host__ __device__ inline bool stream_finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

// Joint j of stream s was observed: every input component finite, and - with confidences - conf >= min_conf (a NaN confidence
// compares false)
__host__ __device__ inline bool stream_observed(const StreamsRepairArgs &a, int s, int j) {
    const uint32_t *in = a.frame + a.width * ((long long)s * a.J + j);
    bool ok = stream_finite_bits(in[0]) && stream_finite_bits(in[1]);
    if (a.width == 3) ok = ok && stream_finite_bits(in[2]);
    if (a.conf) ok = ok && a.conf[(long long)s * a.J + j] >= a.min_conf;
    return ok;
}

// Step m of g + 1 from a (the held copy of the last observation) to e (the new one), one component:
// fl32((double)a + ((double)e - (double)a) * ((double)m / (double)(g + 1))), every operation rounded once; a NaN leaves as the
// canonical quiet NaN (decided on the bits: which payload a NaN result carries differs between the GPU and a host CPU)
__host__ __device__ inline uint32_t stream_interp_bits(uint32_t a_bits, uint32_t e_bits, int m, int g) {
#pragma clang fp contract(off)
    const double a = (double)__builtin_bit_cast(float, a_bits), e = (double)__builtin_bit_cast(float, e_bits);
    const double t = (double)m / (double)(g + 1);
    const double d = e - a;
    const double p = d * t;
    const double r = a + p;
    const uint32_t b = __builtin_bit_cast(uint32_t, (float)r);
    return (b & 0x7fffffffu) > 0x7f800000u ? STREAM_QNAN32 : b;
}

// What a stream's workgroup decides uniformly before anything is written: `st` is stream_step on the head as it stands, `c` the
// count before the push (0 after a RESTART)
struct StreamRepairStep {
    StreamStep st;
    bool restart;
    long long c;
};
__host__ __device__ inline StreamRepairStep stream_repair_step(const StreamsRepairArgs &a, int s) {
    StreamRepairStep r;
    const int action = a.action[s];
    r.st = stream_step(a.heads[s].count, a.heads[s].drained, action, a.lag, a.RF);
    r.restart = r.st.push && action == R3D_STREAM_RESTART;
    r.c = r.st.count - 1;               // (meaningful with st.push only: stream_step counted the push)
    return r;
}

// A stream that takes no push: its word of synthetic - the mask of the frame a DRAIN emits, or 0.  (emit is a frame in [0, c - 1] of a
// head that passed stream_head_valid: the slot lies in [0, RF).)
__host__ __device__ inline uint32_t stream_repair_idle_word(const StreamsRepairArgs &a, int s, const StreamStep &st) {
    if (st.refused || st.emit < 0) return 0u;
    return a.missing[(long long)s * a.RF + stream_slot(st.emit, a.RF)];
}

// RESTART: element i of the stream's track zeroed (i < J + J * width + RF, in the track's order)
__host__ __device__ inline void stream_repair_zero(const StreamsRepairArgs &a, int s, int i) {
    if (i < a.J) a.age[(long long)s * a.J + i] = 0;
    else if (i < a.J + a.J * a.width) a.last[(long long)s * a.J * a.width + (i - a.J)] = 0u;
    else a.missing[(long long)s * a.RF + (i - a.J - a.J * a.width)] = 0u;
}
__host__ __device__ inline int stream_repair_track_words(const StreamsRepairArgs &a) { return a.J + a.J * a.width + a.RF; }

// PUSH, joint j of stream s, c frames in the ring before the push -> true: the joint was NOT observed.  Writes the joint's row of
// frame_out, its age and last, and - when a gap closes - the joint's entries of ring frames in [max(0, c - (RF - 1)), c - 1].
// An age below 0 (a track nobody zeroed) reads as 0.
__host__ __device__ inline bool stream_repair_joint(const StreamsRepairArgs &a, int s, int j, long long c, bool restart) {
    const long long at = (long long)s * a.J + j;
    const uint32_t *in = a.frame + a.width * at;
    uint32_t *out = a.frame_out + a.width * at, *last = a.last + a.width * at;
    int k = restart ? 0 : a.age[at];
    if (k < 0) k = 0;
    if (!stream_observed(a, s, j)) {
        if (k == 0) {                    // never seen: the canonical quiet NaN
            out[0] = STREAM_QNAN32;
            out[1] = STREAM_QNAN32;
            if (a.width == 3) out[2] = STREAM_QNAN32;
            a.age[at] = 0;
        } else {                         // zero-order hold in input space: the step encodes it to the bits it encoded before
            out[0] = last[0];
            out[1] = last[1];
            if (a.width == 3) out[2] = last[2];
            a.age[at] = k == INT32_MAX ? k : k + 1;
        }
        return true;
    }
    uint32_t e[3] = {in[0], in[1], a.width == 3 ? in[2] : 0u};
    out[0] = last[0] = in[0];
    out[1] = last[1] = in[1];
    if (a.width == 3) out[2] = last[2] = in[2];
    a.age[at] = 1;
    if (a.encoding != R3D_ENCODE_NONE) {     // the routine and the bits the step will push
        const float *px = reinterpret_cast<const float *>(in);
        const EncodedPoint p = encode_point_f32(a.cam + (long long)s * UNDIST_ROW_DOUBLES, a.encoding, (double)px[0], (double)px[1]);
        e[0] = stream_f32_bits(p.x);
        e[1] = stream_f32_bits(p.y);
        e[2] = stream_f32_bits(p.z);
    }
    uint32_t *ring = a.ring + (long long)s * a.RF * a.J * a.F;       // entry (slot, j): ring + F * (slot * J + j), slot < RF
    if (k == 0 && c >= 1) {              // back-fill: the per-joint analogue of the reference's front edge padding
        for (long long f = c > a.RF - 1 ? c - (a.RF - 1) : 0; f <= c - 1; ++f) {
            uint32_t *dst = ring + a.F * ((long long)stream_slot(f, a.RF) * a.J + j);
            dst[0] = e[0];
            dst[1] = e[1];
            if (a.F == 3) dst[2] = e[2];
        }
    } else if (k >= 2) {                 // a gap of g = k - 1 frames closes
        const int g = k - 1;
        if (g <= a.max_gap && (long long)g + 1 <= c) {               // (max_gap <= RF - 1: the frames c - g .. c - 1 are in the ring)
            const uint32_t *held = ring + a.F * ((long long)stream_slot(c - 1, a.RF) * a.J + j);
            const uint32_t h[3] = {held[0], held[1], a.F == 3 ? held[2] : 0u};
            for (int m = 1; m <= g; ++m) {
                uint32_t *dst = ring + a.F * ((long long)stream_slot(c - 1 - g + m, a.RF) * a.J + j);
                dst[0] = stream_interp_bits(h[0], e[0], m, g);
                dst[1] = stream_interp_bits(h[1], e[1], m, g);
                if (a.F == 3) dst[2] = stream_interp_bits(h[2], e[2], m, g);
            }
        }
    }
    return false;
}

// After the joints of a PUSH: the new frame's mask into the track, and the stream's word of synthetic - the mask of the frame the
// step will emit (n = c - lag, a frame in [c - (RF - 1), c]), or 0
__host__ __device__ inline void stream_repair_finish(const StreamsRepairArgs &a, int s, long long c, uint32_t mask) {
    uint32_t *missing = a.missing + (long long)s * a.RF;
    missing[stream_slot(c, a.RF)] = mask;
    const long long n = c - a.lag;
    a.synthetic[s] = n < 0 ? 0u : missing[stream_slot(n, a.RF)];
}

}  // namespace r3d
