// r3d_clips_repair: shard evaluation that survives dropped keypoints - the routines the kernel (r3d_k_elementwise.hip) and the host
// hook (r3d_debug_clips_repair_host) share, __host__ __device__ so that the hooks build runs the very same ones on the CPU: the
// descriptor rule, the observed test, the searches in a clip-joint's bitmap of observed rows and the per-point
// routine that applies the rule of include/ray3d_hip.h.  The call runs BEHIND r3d_clips_encode, in place on its output: observed
// points are never written and a missing point's value depends on observed points only, so the result does not depend on the order
// in which the points are visited.  The interpolation is r3d_streams_repair's own routine (stream_interp_bits): the same bits.
// No index comes from a float: p and q are bit positions of a bitmap indexed by r < R <= R3D_REPAIR_MAX_ROWS, a source frame is a
// clamped index of a descriptor that passed the rule.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_streams_repair.hpp"
#include "r3d_undistort.hpp"

namespace r3d {

// r3d_clips_repair: the arguments of r3d_k_clips_repair.  blockIdx.y names a clip of
// the device-side table, blockIdx.x a joint: one workgroup of 256 threads per (clip, joint).
struct ClipsRepairArgs {
    const r3d_clip_input_desc *table;   // num_clips (= gridDim.y) descriptors in device memory: the table r3d_clips_encode read
    uint32_t *x;                        // (out_rows, J, F) 32-bit patterns, repaired IN PLACE
    uint32_t *x_mirror;                 // the flip pass's inputs, or nullptr
    const float *conf;                  // (total_frames, J) over SOURCE frames, or nullptr
    uint8_t *state;                     // (out_rows, J) or nullptr
    int32_t *stats;                     // (num_clips, J, 4) or nullptr
    int32_t *status;                    // num_clips words: 0 followed, 1 invalid descriptor
    long long out_rows, max_rows, total_frames;
    unsigned long long mirror_inv[2];   // mirror_pack_inverse (r3d_undistort.hpp)
    float min_conf;
    int J, F, max_gap;
};

constexpr int CLIPS_REPAIR_THREADS = 256;                       // four wavefronts: a step of the two passes is 256 rows, four bitmap words
constexpr int CLIPS_REPAIR_WAVES = CLIPS_REPAIR_THREADS / 64;
constexpr int CLIPS_REPAIR_WORDS = R3D_REPAIR_MAX_ROWS / 64;    // 1 024 words of 64 bits: a clip-joint's observed bitmap
// the mode's LDS, inside the kernel's shared block: the bitmap, then per wavefront the first row it saw observed (min O is the
// smallest of the four) and its four counters
constexpr int CLIPS_REPAIR_LDS_BITS = 0;
constexpr int CLIPS_REPAIR_LDS_FIRST = CLIPS_REPAIR_WORDS * 8;                             // [wave]
constexpr int CLIPS_REPAIR_LDS_COUNT = CLIPS_REPAIR_LDS_FIRST + CLIPS_REPAIR_WAVES * 4;    // [wave][4]
constexpr int CLIPS_REPAIR_LDS_BYTES = CLIPS_REPAIR_LDS_COUNT + CLIPS_REPAIR_WAVES * 4 * 4;
static_assert(R3D_REPAIR_MAX_ROWS % CLIPS_REPAIR_THREADS == 0, "a step's four words never pass the bitmap's end");

// states of a point (include/ray3d_hip.h)
constexpr int CLIP_REPAIR_OBSERVED = 0, CLIP_REPAIR_INTERP = 1, CLIP_REPAIR_HELD = 2, CLIP_REPAIR_BACKFILLED = 3, CLIP_REPAIR_NEVER = 4;

// What a workgroup reads of its descriptor, and the verdict on it
struct ClipRepairClip {
    long long first, n, out_first;
    int pad_front, R;                   // R = pad_front + n + pad_back <= R3D_REPAIR_MAX_ROWS once ok
    bool ok;
};
// clip_input_valid's rule with the call's out_rows / max_rows; the source range is judged when confidences are read from it - it is
// the only thing the call reads by source frame -; and R <= R3D_REPAIR_MAX_ROWS (max_rows is: checked on the host; kept here so that
// the bitmap's bound does not lean on an argument check)
__host__ __device__ inline ClipRepairClip clip_repair_clip(const ClipsRepairArgs &a, const r3d_clip_input_desc *d) {
    ClipRepairClip c;
    c.first = d->first_frame;
    c.n = d->n_frames;
    c.out_first = d->out_first;
    c.pad_front = d->pad_front;
    const int pad_back = d->pad_back;
    c.ok = a.conf ? clip_input_valid(c.first, c.n, c.out_first, c.pad_front, pad_back, a.total_frames, a.out_rows, a.max_rows)
                  : clip_input_valid(0, c.n, c.out_first, c.pad_front, pad_back, c.n, a.out_rows, a.max_rows);
    const long long rows = c.ok ? c.pad_front + c.n + pad_back : 0;
    c.ok = c.ok && rows <= R3D_REPAIR_MAX_ROWS;
    c.R = c.ok ? (int)rows : 0;
    return c;
}

// OBSERVED(r, j): every component of x[out_first + r, j] finite and - with confidences - conf[source frame, j] >= min_conf (a NaN
// confidence compares false).  r < R of a clip that passed the rule.
__host__ __device__ inline bool clip_repair_observed(const ClipsRepairArgs &a, const ClipRepairClip &c, int r, int j) {
    const uint32_t *in = a.x + a.F * ((c.out_first + r) * a.J + j);
    bool ok = stream_finite_bits(in[0]) && stream_finite_bits(in[1]);
    if (a.F == 3) ok = ok && stream_finite_bits(in[2]);
    if (a.conf) ok = ok && a.conf[(c.first + clip_input_source(r, c.pad_front, c.n)) * a.J + j] >= a.min_conf;
    return ok;
}

// The largest observed row below r inside r's step of 256 rows (words [r / 256 * 4, r / 64] of the bitmap), else `carry`: the largest
// observed row in front of the step, or -1
__host__ __device__ inline int clip_repair_prev(const unsigned long long *bits, int r, int carry) {
    int w = r >> 6;
    const int w0 = w & ~(CLIPS_REPAIR_WAVES - 1);
    unsigned long long m = bits[w] & ((1ull << (r & 63)) - 1ull);
    for (;;) {
        if (m) return w * 64 + 63 - __builtin_clzll(m);
        if (--w < w0) return carry;
        m = bits[w];
    }
}
// The carry behind the step whose first word is w0 (a multiple of 4): its largest observed row, else the carry in front of it
__host__ __device__ inline int clip_repair_carry(const unsigned long long *bits, int w0, int carry) {
    for (int w = w0 + CLIPS_REPAIR_WAVES - 1; w >= w0; --w)
        if (bits[w]) return w * 64 + 63 - __builtin_clzll(bits[w]);
    return carry;
}
// The smallest observed row in (r, min(r + max_gap, R - 1)], or -1: a q further away closes no gap of at most max_gap rows (g = q - p
// - 1 >= q - r).  It looks at words r / 64 .. (r + max_gap) / 64: no more than max_gap / 64 + 2 of them.
__host__ __device__ inline int clip_repair_next(const unsigned long long *bits, int r, int R, int max_gap) {
    const long long far = (long long)r + max_gap;
    const int hi = far > R - 1 ? R - 1 : (int)far;
    if (hi <= r) return -1;
    int w = r >> 6;
    const int wl = hi >> 6;
    unsigned long long m = (r & 63) == 63 ? 0ull : bits[w] & (~0ull << ((r & 63) + 1));
    for (;;) {
        if (m) {
            const int q = w * 64 + __builtin_ctzll(m);
            return q <= hi ? q : -1;
        }
        if (++w > wl) return -1;
        m = bits[w];
    }
}

// The MISSING point (r, j) of a clip: `bits` the clip-joint's bitmap (rows >= R read as not observed), `first` = min O or -1, p the
// largest observed row below r or -1 (clip_repair_prev).  Writes the point of x, x_mirror and - by the caller - nothing else;
// returns its state.  Reads rows of O only: they are never written.
__host__ __device__ inline int clip_repair_point(const ClipsRepairArgs &a, const ClipRepairClip &c, const unsigned long long *bits, int first,
                                                 int p, int r, int j) {
    uint32_t v[3] = {STREAM_QNAN32, STREAM_QNAN32, STREAM_QNAN32};
    int state = CLIP_REPAIR_NEVER;
    const long long row0 = c.out_first * a.J + j;        // point (row, j) of x: F * (row0 + row * J)
    if (first >= 0) {
        if (p < 0) {                         // r < min O: the back-fill
            const uint32_t *s = a.x + a.F * (row0 + (long long)first * a.J);
            v[0] = s[0];
            v[1] = s[1];
            if (a.F == 3) v[2] = s[2];
            state = CLIP_REPAIR_BACKFILLED;
        } else {
            const uint32_t *s = a.x + a.F * (row0 + (long long)p * a.J);
            const int q = clip_repair_next(bits, r, c.R, a.max_gap);
            const int g = q - p - 1;
            if (q >= 0 && g <= a.max_gap) {
                const uint32_t *e = a.x + a.F * (row0 + (long long)q * a.J);
                v[0] = stream_interp_bits(s[0], e[0], r - p, g);
                v[1] = stream_interp_bits(s[1], e[1], r - p, g);
                if (a.F == 3) v[2] = stream_interp_bits(s[2], e[2], r - p, g);
                state = CLIP_REPAIR_INTERP;
            } else {                         // the hold
                v[0] = s[0];
                v[1] = s[1];
                if (a.F == 3) v[2] = s[2];
                state = CLIP_REPAIR_HELD;
            }
        }
    }
    const long long row = (c.out_first + r) * a.J;
    uint32_t *o = a.x + a.F * (row + j);
    o[0] = v[0];
    o[1] = v[1];
    if (a.F == 3) o[2] = v[2];
    if (a.x_mirror) {                        // r3d_clips_encode's rule: the sign bit of component 0 turned, left <-> right
        uint32_t *m = a.x_mirror + a.F * (row + mirror_dest(a.mirror_inv[0], a.mirror_inv[1], j));
        m[0] = v[0] ^ 0x80000000u;
        m[1] = v[1];
        if (a.F == 3) m[2] = v[2];
    }
    return state;
}

}  // namespace r3d
