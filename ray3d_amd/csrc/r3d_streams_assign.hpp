// r3d_streams_assign: detections to live streams - per camera the association of a tick's unordered 2D detections with that
// camera's stream slots, the births and the ends of tracks, and the action words, frame rows and confidence rows that
// r3d_streams_repair / r3d_streams_step of the same tick read.  The routines the kernel (r3d_k_elementwise.hip) and the host hook
// (r3d_debug_streams_assign_host) share, __host__ __device__ so that the hooks build runs the very same ones on the CPU: the
// observed test, the per-detection summary, the per-pair cost, the order of the greedy matching's keys, the per-slot
// step (state and outputs) and the per-camera finish.  Integers decide first; the arithmetic is float64 with floating-point
// contraction OFF: every operation rounds once, joints are visited in ascending order and sums start from zero, the divisions and
// the square roots are the correctly rounded ones on both sides.  The reference works on pre-associated archives and has no
// counterpart: include/ray3d_hip.h is the definition.  NOTHING of the state is ever used as an index.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ray3d_hip.h"
#include "r3d_streams_repair.hpp"      // stream_finite_bits, STREAM_QNAN32

namespace r3d {

// r3d_streams_assign: the arguments of r3d_k_streams_assign.  blockIdx.x names a
// camera; the workgroup is one wavefront.
struct StreamsAssignArgs {
    void *state;                        // next_id[C], id[S], phase[S], missed[S], left[S], seen[S], ref[S][J][width] (assign_state)
    const uint32_t *det;                // (C, D, J, width) 32-bit patterns
    const float *det_conf;              // (C, D, J) or nullptr
    const int32_t *det_count;           // (C)
    int32_t *action;                    // (S)
    uint32_t *frame_out;                // (S, J, width)
    uint32_t *conf_out;                 // (S, J) float32 patterns, or nullptr
    int32_t *match;                     // (S)
    long long *id_out;                  // (S)
    int32_t *stats;                     // (C, 4) or nullptr
    double max_cost;
    float min_conf;
    int C, P, D, J, width, lag, min_joints, min_common, max_missed, fill;
};

constexpr int STREAMS_ASSIGN_THREADS = 64;    // one wavefront per camera: its lanes own detections, pairs, then slots
// The kernel's LDS: the P x D cost keys (at most 32 x 32 of 8 bytes), then the detections' sizes and observed masks
constexpr int STREAMS_ASSIGN_LDS_KEYS = 0;
constexpr int STREAMS_ASSIGN_LDS_SIZE = 8 * R3D_ASSIGN_MAX_SLOTS * R3D_ASSIGN_MAX_DETECTIONS;
constexpr int STREAMS_ASSIGN_LDS_OBS = STREAMS_ASSIGN_LDS_SIZE + 8 * R3D_ASSIGN_MAX_DETECTIONS;
constexpr int STREAMS_ASSIGN_LDS_BYTES = STREAMS_ASSIGN_LDS_OBS + 4 * R3D_ASSIGN_MAX_DETECTIONS;
static_assert(R3D_ASSIGN_MAX_SLOTS <= 32 && R3D_ASSIGN_MAX_DETECTIONS <= 32, "slots and detections are bits of 32-bit masks");
static_assert(R3D_ASSIGN_MAX_SLOTS <= STREAMS_ASSIGN_THREADS && R3D_ASSIGN_MAX_DETECTIONS <= STREAMS_ASSIGN_THREADS,
              "one lane per detection, one lane per slot");

// The cost key of a pair that is not admissible: the bits of +inf.  An admissible cost is a finite double >= +0, so the keys
// order as unsigned integers exactly as the costs order as doubles.
constexpr unsigned long long STREAM_ASSIGN_NONE = 0x7ff0000000000000ull;

// bytes of the state (the arguments passed the shape rules: no overflow), rounded up to 8
inline size_t streams_assign_bytes(long long C, long long P, long long J, long long width) {
    const long long S = C * P;
    const long long bytes = 8 * C + S * (8 + 4 * 4 + 4 * J * width);
    return (size_t)((bytes + 7) / 8 * 8);
}

// The state's arrays, in the header's order
struct StreamAssignState {
    long long *next_id;                 // [C]
    long long *id;                      // [S]
    int32_t *phase, *missed, *left;     // [S] each
    uint32_t *seen;                     // [S]
    uint32_t *ref;                      // [S][J][width]
};
__host__ __device__ inline StreamAssignState stream_assign_state(const StreamsAssignArgs &a) {
    const long long S = (long long)a.C * a.P;
    StreamAssignState st;
    st.next_id = static_cast<long long *>(a.state);
    st.id = st.next_id + a.C;
    st.phase = reinterpret_cast<int32_t *>(st.id + S);
    st.missed = st.phase + S;
    st.left = st.missed + S;
    st.seen = reinterpret_cast<uint32_t *>(st.left + S);
    st.ref = st.seen + S;
    return st;
}

// A phase word as the rule reads it: 1 live, 2 draining (only with lag > 0: a stream without lag has no drain), anything else 0
__host__ __device__ inline int stream_assign_phase(int32_t word, int lag) {
    if (word == 1) return 1;
    if (word == 2 && lag > 0) return 2;
    return 0;
}

// det_count[c] as the rule reads it
__host__ __device__ inline int stream_assign_count(int32_t word, int D) { return word < 0 ? 0 : word > D ? D : word; }

// Joint j of detection d of camera c was observed: every component finite, and - with confidences - conf >= min_conf (a NaN
// confidence compares false)
__host__ __device__ inline bool stream_assign_observed(const StreamsAssignArgs &a, int c, int d, int j) {
    const long long at = ((long long)c * a.D + d) * a.J + j;
    const uint32_t *in = a.det + a.width * at;
    bool ok = stream_finite_bits(in[0]) && stream_finite_bits(in[1]);
    if (a.width == 3) ok = ok && stream_finite_bits(in[2]);
    if (a.det_conf) ok = ok && a.det_conf[at] >= a.min_conf;
    return ok;
}

// What step 1 knows of a detection: the mask of its observed joints, its size and whether it is valid
struct StreamAssignDet {
    uint32_t obs;
    double size;
    bool valid;
};
__host__ __device__ inline StreamAssignDet stream_assign_detection(const StreamsAssignArgs &a, int c, int d) {
#pragma clang fp contract(off)
    StreamAssignDet r;
    r.obs = 0;
    int n = 0;
    double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
    for (int j = 0; j < a.J; ++j) {
        if (!stream_assign_observed(a, c, d, j)) continue;
        const uint32_t *in = a.det + a.width * (((long long)c * a.D + d) * a.J + j);
        const double x = (double)__builtin_bit_cast(float, in[0]), y = (double)__builtin_bit_cast(float, in[1]);
        if (n == 0) {
            x0 = x1 = x;
            y0 = y1 = y;
        } else {
            if (x < x0) x0 = x;
            if (x > x1) x1 = x;
            if (y < y0) y0 = y;
            if (y > y1) y1 = y;
        }
        ++n;
        r.obs |= 1u << j;
    }
    const double dx = x1 - x0, dy = y1 - y0;
    r.size = dy > dx ? dy : dx;
    r.valid = n >= a.min_joints && r.size > 0.0;
    return r;
}

// Step 2: the cost key of slot p and detection d of camera c - the bits of the cost, or STREAM_ASSIGN_NONE when the slot is not
// live, the detection not valid, the common joints too few or the cost not <= max_cost (a NaN fails).  `seen` and `ref` are only
// ever compared and subtracted: whatever the state holds, nothing is indexed with it.
__host__ __device__ inline unsigned long long stream_assign_pair(const StreamsAssignArgs &a, const StreamAssignState &st, int c, int p, int d,
                                                                 const StreamAssignDet &det) {
#pragma clang fp contract(off)
    const long long s = (long long)c * a.P + p;
    if (stream_assign_phase(st.phase[s], a.lag) != 1 || !det.valid) return STREAM_ASSIGN_NONE;
    const uint32_t common = det.obs & st.seen[s];          // (det.obs holds bits below J only)
    const int n = __builtin_popcount(common);
    if (n < a.min_common) return STREAM_ASSIGN_NONE;
    const uint32_t *in = a.det + (long long)a.width * (((long long)c * a.D + d) * a.J);
    const uint32_t *ref = st.ref + (long long)a.width * (s * a.J);
    // Every joint's distance is formed - j < J lies inside both rows, whatever the words hold - and only the common ones are summed:
    // without a branch around the loads those of several joints are in flight together (on the device they are most of the call's time)
    double sum = 0.0;
#pragma unroll 4
    for (int j = 0; j < a.J; ++j) {
        const double dx = (double)__builtin_bit_cast(float, in[a.width * j]) - (double)__builtin_bit_cast(float, ref[a.width * j]);
        const double dy = (double)__builtin_bit_cast(float, in[a.width * j + 1]) - (double)__builtin_bit_cast(float, ref[a.width * j + 1]);
        const double xx = dx * dx, yy = dy * dy;
        const double q = xx + yy;
        const double r = sqrt(q);
        const double with = sum + r;
        sum = ((common >> j) & 1u) ? with : sum;
    }
    const double mean = sum / (double)n;
    const double cost = mean / det.size;
    if (!(cost <= a.max_cost)) return STREAM_ASSIGN_NONE;
    return __builtin_bit_cast(unsigned long long, cost);
}

// Step 3's order: (key, pair index p * D + d) is better than the best so far - the smaller cost, then the smaller p, then the smaller d
__host__ __device__ inline bool stream_assign_better(unsigned long long key, int index, unsigned long long best_key, int best_index) {
    return key < best_key || (key == best_key && index < best_index);
}

// Step 3 on the device, for one wavefront of STREAMS_ASSIGN_THREADS lanes: the greedy matching over the R x C keys key[r * C + c] in
// LDS (R, C <= 32).  Lane (c, half) = (lane % 32, lane / 32) scans the untaken pairs of its column c with the rows of its parity,
// a six-step xor butterfly over (key, pair index) leaves every lane with the same winner, `won(row, column)` hears of it, and its
// row and column are taken: at most min(R, C) rounds, ended by the first without an admissible pair.  R, C, `rows` and `cols` are
// the same in every lane, so every loop bound and the break are uniform; no lane may have left.
template <class Won>
__device__ __forceinline__ void stream_assign_greedy(const unsigned long long *key, int R, int C, uint32_t &rows, uint32_t &cols, Won won) {
    const int c = threadIdx.x & 31, half = threadIdx.x >> 5;
    const int rounds = R < C ? R : C;
    for (int round = 0; round < rounds; ++round) {
        unsigned long long best = STREAM_ASSIGN_NONE;
        int at = R * C;
        if (c < C && !((cols >> c) & 1u))                           // (a lane whose column is taken has nothing left to offer)
            for (int r = half; r < R; r += 2) {
                if ((rows >> r) & 1u) continue;
                const int i = r * C + c;
                const unsigned long long k = key[i];
                if (stream_assign_better(k, i, best, at)) {
                    best = k;
                    at = i;
                }
            }
        for (int off = STREAMS_ASSIGN_THREADS / 2; off > 0; off >>= 1) {
            const unsigned long long k = __shfl_xor(best, off);
            const int i = __shfl_xor(at, off);
            if (stream_assign_better(k, i, best, at)) {
                best = k;
                at = i;
            }
        }
        if (best == STREAM_ASSIGN_NONE) break;                      // uniform: no admissible pair is left
        const int wr = at / C, wc = at - wr * C;                    // (at < R * C: an admissible key came from a real pair)
        rows |= 1u << wr;
        cols |= 1u << wc;
        won(wr, wc);
    }
}

// The position of the r-th (from 0) set bit of `mask`; r < popcount(mask)
__host__ __device__ inline int stream_assign_nth_bit(uint32_t mask, int r) {
    for (int i = 0; i < r; ++i) mask &= mask - 1u;
    return __builtin_ctz(mask);
}

// Steps 4 to 7 for slot p of camera c: its state words and its row of every output.  `matched`: the detection step 3 gave the slot,
// or -1; `free_mask`: the camera's slots that were free at entry; `unmatched`: its valid detections that step 3 left over; `next`:
// next_id[c] at entry.  Reads the slot's own state as it was at entry - nobody else writes it.
__host__ __device__ inline void stream_assign_slot(const StreamsAssignArgs &a, const StreamAssignState &st, int c, int p, int matched,
                                                   uint32_t free_mask, uint32_t unmatched, long long next) {
    const long long s = (long long)c * a.P + p;
    const int phase = stream_assign_phase(st.phase[s], a.lag);
    int action = R3D_STREAM_IDLE, src = -1;             // src: the detection whose bits the slot pushes
    bool synthetic = false;                             // an unmatched live slot that pushes a made-up frame
    long long id = -1;
    uint32_t seen = 0;
    if (phase == 1) {
        id = st.id[s];
        seen = st.seen[s];                              // (only bits j < J are ever looked at)
        int missed = st.missed[s];
        if (missed < 0) missed = 0;
        if (matched >= 0) {
            action = R3D_STREAM_PUSH;
            src = matched;
            st.missed[s] = 0;
        } else if (missed < a.max_missed) {             // (missed + 1 <= max_missed, without the overflow)
            action = R3D_STREAM_PUSH;
            synthetic = true;
            st.missed[s] = missed + 1;
        } else if (a.lag > 0) {                         // the track ends: lag DRAIN ticks, this one included
            action = R3D_STREAM_DRAIN;
            st.left[s] = a.lag - 1;
            st.phase[s] = a.lag - 1 == 0 ? 0 : 2;
        } else {
            st.phase[s] = 0;
        }
    } else if (phase == 2) {
        id = st.id[s];
        action = R3D_STREAM_DRAIN;
        int left = st.left[s];
        left = left < 1 ? 1 : left > a.lag ? a.lag : left;
        left -= 1;
        st.left[s] = left;
        st.phase[s] = left == 0 ? 0 : 2;
    } else {
        const int rank = __builtin_popcount(free_mask & ((1u << p) - 1u));     // (p < 32)
        if (rank < __builtin_popcount(unmatched)) {     // a birth: the rank-th leftover detection takes the rank-th free slot
            action = R3D_STREAM_RESTART;
            src = stream_assign_nth_bit(unmatched, rank);
            id = (long long)((unsigned long long)next + (unsigned long long)rank);
            st.id[s] = id;
            st.phase[s] = 1;
            st.missed[s] = 0;
        }
    }
    uint32_t *out = a.frame_out + (long long)a.width * (s * a.J);
    uint32_t *ref = st.ref + (long long)a.width * (s * a.J);
    uint32_t *conf = a.conf_out ? a.conf_out + s * a.J : nullptr;
    if (src >= 0) {                                     // (src < n <= D: a detection step 1 looked at)
        const long long at = ((long long)c * a.D + src) * a.J;
        const uint32_t *in = a.det + (long long)a.width * at;
        for (int j = 0; j < a.J; ++j) {
            const bool obs = stream_assign_observed(a, c, src, j);
            for (int k = 0; k < a.width; ++k) {
                const uint32_t b = in[a.width * j + k];
                out[a.width * j + k] = b;
                if (obs) ref[a.width * j + k] = b;
            }
            if (obs) seen |= 1u << j;
            if (conf) conf[j] = a.det_conf ? reinterpret_cast<const uint32_t *>(a.det_conf)[at + j] : 0x3f800000u;     // (the bits; 1.0f)
        }
        st.seen[s] = seen;
    } else {
        const bool hold = synthetic && a.fill == R3D_ASSIGN_FILL_HOLD;
        for (int j = 0; j < a.J; ++j) {
            const bool have = hold && ((seen >> j) & 1u);
            for (int k = 0; k < a.width; ++k) out[a.width * j + k] = have ? ref[a.width * j + k] : STREAM_QNAN32;
            if (conf) conf[j] = 0u;
        }
    }
    a.action[s] = action;
    a.match[s] = src;
    a.id_out[s] = id;
}

// After a camera's slots: its identity counter and its row of stats (valid, matched, born, dropped)
__host__ __device__ inline void stream_assign_finish(const StreamsAssignArgs &a, const StreamAssignState &st, int c, uint32_t valid,
                                                     uint32_t cols, uint32_t free_mask, uint32_t unmatched, long long next) {
    const int want = __builtin_popcount(unmatched), room = __builtin_popcount(free_mask);
    const int born = want < room ? want : room;
    st.next_id[c] = (long long)((unsigned long long)next + (unsigned long long)born);
    if (a.stats) {
        a.stats[4 * c] = __builtin_popcount(valid);
        a.stats[4 * c + 1] = __builtin_popcount(cols);
        a.stats[4 * c + 2] = born;
        a.stats[4 * c + 3] = want - born;
    }
}

}  // namespace r3d
