// r3d_streams_peek: early poses for live streams of centred models - the routines the kernel (r3d_k_elementwise.hip) and the host
// hook (r3d_debug_streams_peek_host) share, __host__ __device__ so that the hooks build runs the very same ones on the CPU: the
// verdict on a stream and a look, and the point copy.  Integers only; values are 32-bit copies.  The head rule, the
// frame clamp and the slot index are those of r3d_streams.hpp: the window of preview frame p = c - 1 - look is the one a drain
// started now would emit at its (lag - look)-th tick.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_streams.hpp"
#include "r3d_windows.hpp"

namespace r3d {

// r3d_streams_peek: the arguments of r3d_k_streams_peek.  One launch: blockIdx.y
// names a stream, blockIdx.z a look, one output point (row, joint) per thread.  Nothing of the state is written: it is const here.
struct StreamsPeekArgs {
    const r3d_stream_head *heads;       // S heads: the front of the state
    const uint32_t *ring;               // S rings of (RF, J, F) 32-bit patterns, behind the heads
    const int32_t *action;              // S words of this tick's step, or nullptr: every stream counts as pushed
    const int32_t *status;              // S words the step wrote
    uint32_t *x, *x_mirror;             // (K, S, RF, J, F); x_mirror nullptr: no mirrored copy
    long long *emit;                    // (K, S) words: the preview frame, or -1
    int32_t *peek_status;               // (K, S) words: 0, or 1 (the step refused the stream, or its head is invalid)
    unsigned long long mirror_perm[2];  // window_pack_perm (r3d_windows.hpp)
    int32_t looks[R3D_STREAMS_PEEK_MAX];    // strictly increasing, each in [0, lag)
    int S, RF, lag, J, F, K;
};

// What the call decides per (look, stream), uniformly, before anything is written.  `bad`: peek_status 1.  `previews`: emit = p and
// the row block is written; otherwise emit = -1 and nothing of the row block is read or written.  A head that passed
// stream_head_valid has count in [0, 2^62], so p = count - 1 - look cannot overflow, and with previews 0 <= p <= count - 1.
struct StreamPeek {
    bool bad, previews;
    long long p;
};
__host__ __device__ inline StreamPeek stream_peek(long long count, long long drained, bool has_action, int action, int status, int look,
                                                  int lag) {
    StreamPeek r = {false, false, -1};
    r.bad = status != 0 || !stream_head_valid(count, drained, lag);
    if (r.bad) return r;
    const bool pushed = !has_action || action == R3D_STREAM_PUSH || action == R3D_STREAM_RESTART;
    const long long p = count - 1 - look;
    if (!pushed || drained != 0 || count < 1 || p < 0) return r;
    r.previews = true;
    r.p = p;
    return r;
}

// the look of blockIdx.z / of the hook's loop, without indexing the by-value arguments with a runtime index (k < K <= 8)
__host__ __device__ inline int stream_peek_look(const StreamsPeekArgs &a, int k) {
    int look = a.looks[0];
#pragma unroll
    for (int i = 1; i < R3D_STREAMS_PEEK_MAX; ++i) look = k == i ? a.looks[i] : look;
    return look;
}

// Output point (row i, joint j) of look k, stream s: stream_gather_point's arithmetic with the preview frame p in place of n - the
// ring's copy of frame clamp(p - (RF - 1 - lag) + i, 0, c - 1) at slot frame % RF (the oldest frame named is c - RF + lag - look >
// c - RF: the ring holds it), the mirrored copy x[.., mirror_perm[j]] with the sign bit of component 0 turned.
__host__ __device__ inline void stream_peek_point(const StreamsPeekArgs &a, int k, int s, long long p, long long c, int i, int j) {
    const int slot = stream_slot(stream_window_frame(p, a.RF, a.lag, i, c), a.RF);
    const uint32_t *row = a.ring + (long long)a.F * (((long long)s * a.RF + slot) * a.J);
    const long long at = a.F * ((((long long)k * a.S + s) * a.RF + i) * a.J + j);
    const uint32_t *q = row + a.F * j;
    a.x[at] = q[0];
    a.x[at + 1] = q[1];
    if (a.F == 3) a.x[at + 2] = q[2];
    if (a.x_mirror) {
        const uint32_t *m = row + a.F * window_mirror_source(a.mirror_perm[0], a.mirror_perm[1], j);
        a.x_mirror[at] = m[0] ^ 0x80000000u;
        a.x_mirror[at + 1] = m[1];
        if (a.F == 3) a.x_mirror[at + 2] = m[2];
    }
}

}  // namespace r3d
