// r3d_streams_step: live streams lifted a frame at a time - the routines the kernels (r3d_k_elementwise.hip)
// and the host hook (r3d_debug_streams_step_host) share, __host__ __device__ so that the hooks build runs the very same ones on the
// CPU: the head's validity test, the action step, the frame-to-slot index and the point copy.  The head arithmetic is integers
// only; values are 32-bit copies, or - for the pixel encodings - encode_point_f32 of r3d_undistort.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_undistort.hpp"
#include "r3d_windows.hpp"

namespace r3d {

constexpr long long STREAM_COUNT_MAX = 1ll << 62;    // a head's count lies in [0, 2^62]: c - 1 - lag + k and c % RF cannot overflow

// r3d_streams_step: the arguments of its two kernels.  r3d_k_streams_advance advances the heads (blockIdx.x names a stream, one new
// point per thread), r3d_k_streams_gather gathers the windows (blockIdx.y names a stream, one output point (row, joint) per thread)
// from the heads, emit and status words the advance launch wrote.
struct StreamsArgs {
    r3d_stream_head *heads;             // S heads: the front of the state
    uint32_t *ring;                     // S rings of (RF, J, F) 32-bit patterns, behind the heads
    const uint32_t *frame;              // (S, J, 2) pixels or (S, J, F) model-input rows
    const double *cam;                  // (S, 16) camera rows, or nullptr (R3D_ENCODE_NONE)
    const int32_t *action;              // S words
    uint32_t *x, *x_mirror;             // (S, RF, J, F); x_mirror nullptr: no mirrored copy
    long long *emit;                    // S words: the frame index of the window written this tick, or -1
    int32_t *status;                    // S words: 0 followed, 1 refused
    unsigned long long mirror_perm[2];  // window_pack_perm (r3d_windows.hpp)
    int S, RF, lag, J, F;
    int encoding;                       // R3D_ENCODE_RAY / INTRINSIC / SCREEN (= ENC_* of r3d_undistort.hpp) or R3D_ENCODE_NONE
};

// bytes of the state: S heads, then S rings (the arguments passed the checks of streams_check_args: no overflow)
inline size_t streams_state_bytes(long long S, long long RF, long long J, long long F) {
    return (size_t)(S * (long long)sizeof(r3d_stream_head) + S * RF * J * F * (long long)sizeof(float));
}

// A head the call follows (include/ray3d_hip.h: "refused streams")
__host__ __device__ inline bool stream_head_valid(long long count, long long drained, int lag) {
    return count >= 0 && count <= STREAM_COUNT_MAX && drained >= 0 && drained <= lag;
}

// What one action does to one head.  `refused`: nothing but status = 1, emit = -1 may be written.  `push`: the new frame goes to
// ring slot `slot` (the count before the push, modulo RF).  `write_head`: the head becomes (count, drained).  `emit`: the frame
// index of the window to gather, or -1.
struct StreamStep {
    bool refused, push, write_head;
    int slot;
    long long count, drained, emit;
};
__host__ __device__ inline StreamStep stream_step(long long count, long long drained, int action, int lag, int RF) {
    StreamStep r = {false, false, false, 0, count, drained, -1};
    if (action == R3D_STREAM_IDLE) return r;                     // the head is not looked at
    if (action == R3D_STREAM_RESTART) {                          // ... nor here: it is zeroed, then the action is a PUSH
        count = 0;
        drained = 0;
    } else if (action != R3D_STREAM_PUSH && action != R3D_STREAM_DRAIN) {
        r.refused = true;
        return r;
    }
    if (!stream_head_valid(count, drained, lag)) { r.refused = true; return r; }
    long long k;
    if (action == R3D_STREAM_DRAIN) {
        if (count == 0 || drained == lag) return r;              // nothing (left) to drain: a valid no-op
        drained += 1;
        k = drained;
    } else {
        if (drained > 0 || count == STREAM_COUNT_MAX) { r.refused = true; return r; }      // PUSH after a drain began; a full counter
        r.push = true;
        r.slot = (int)(count % RF);
        count += 1;
        k = 0;
    }
    r.write_head = true;
    r.count = count;
    r.drained = drained;
    const long long n = count - 1 - lag + k;                     // (count <= 2^62, lag and k below 2^31)
    r.emit = n < 0 ? -1 : n;
    return r;
}

// Row i of the window of frame n repeats stream frame clamp(n - (RF - 1 - lag) + i, 0, c - 1): the clamp at 0 is the reference's
// front edge padding, the clamp at c - 1 (during a drain) its back edge padding.  c >= 1.
__host__ __device__ inline long long stream_window_frame(long long n, int RF, int lag, int i, long long c) {
    const long long t = n - (RF - 1 - lag) + i;
    return t < 0 ? 0 : (t > c - 1 ? c - 1 : t);
}
// ... and is found at ring slot frame % RF (frame >= 0: the slot lies in [0, RF))
__host__ __device__ inline int stream_slot(long long frame, int RF) { return (int)(frame % RF); }

__host__ __device__ inline uint32_t stream_f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// Point j of stream s's new frame into ring slot `slot`: encoded from the pixel pair through the stream's camera row (the routine
// r3d_clips_encode writes with), or copied as F 32-bit patterns (R3D_ENCODE_NONE)
__host__ __device__ inline void stream_store_point(const StreamsArgs &a, int s, int slot, int j) {
    uint32_t *dst = a.ring + a.F * (((long long)s * a.RF + slot) * a.J + j);
    if (a.encoding == R3D_ENCODE_NONE) {
        const uint32_t *src = a.frame + a.F * ((long long)s * a.J + j);
        dst[0] = src[0];
        dst[1] = src[1];
        if (a.F == 3) dst[2] = src[2];
        return;
    }
    const float *px = reinterpret_cast<const float *>(a.frame) + 2 * ((long long)s * a.J + j);
    const EncodedPoint e = encode_point_f32(a.cam + (long long)s * UNDIST_ROW_DOUBLES, a.encoding, (double)px[0], (double)px[1]);
    dst[0] = stream_f32_bits(e.x);
    dst[1] = stream_f32_bits(e.y);
    if (a.F == 3) dst[2] = stream_f32_bits(e.z);
}

// Output point (row i, joint j) of stream s's window of frame n, c frames pushed so far: x[s, i, j] is the ring's copy of the
// clamped frame, x_mirror[s, i, j] = x[s, i, mirror_perm[j]] with the sign bit of component 0 turned (window_point's rule)
__host__ __device__ inline void stream_gather_point(const StreamsArgs &a, int s, long long n, long long c, int i, int j) {
    const int slot = stream_slot(stream_window_frame(n, a.RF, a.lag, i, c), a.RF);
    const uint32_t *row = a.ring + (long long)a.F * (((long long)s * a.RF + slot) * a.J);
    const long long at = a.F * (((long long)s * a.RF + i) * a.J + j);
    const uint32_t *p = row + a.F * j;
    a.x[at] = p[0];
    a.x[at + 1] = p[1];
    if (a.F == 3) a.x[at + 2] = p[2];
    if (a.x_mirror) {
        const uint32_t *m = row + a.F * window_mirror_source(a.mirror_perm[0], a.mirror_perm[1], j);
        a.x_mirror[at] = m[0] ^ 0x80000000u;
        a.x_mirror[at + 1] = m[1];
        if (a.F == 3) a.x_mirror[at + 2] = m[2];
    }
}

// What the gather launch decides per stream, uniformly, from what the advance launch left: a window is written only for a stream
// that was followed, emits a frame, and whose head holds it (c >= 1 and n <= c - 1: what stream_step wrote always does; a head that
// does not is not followed)
__host__ __device__ inline bool stream_emits(long long count, long long drained, long long n, int status, int lag) {
    return status == 0 && n >= 0 && stream_head_valid(count, drained, lag) && count >= 1 && n <= count - 1;
}

}  // namespace r3d
