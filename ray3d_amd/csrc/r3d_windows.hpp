// r3d_clips_windows: a batch of (RF, J, F) windows gathered from a pool of windows drawn from many clips - the routines the kernel
// (r3d_k_elementwise.hip) and the host hook (r3d_debug_clips_windows_host) share, __host__ __device__ so
// that the hooks build runs the very same ones on the CPU.  Integer arithmetic and 32-bit copies only: nothing here rounds.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ray3d_hip.h"

namespace r3d {

// r3d_clips_windows: the arguments of r3d_k_clips_windows.  blockIdx.y names a window
// of the batch; one output point (row, joint) per thread.
struct WindowsArgs {
    const r3d_window_run_desc *runs;    // num_runs descriptors in device memory
    const uint32_t *src;                // (total_frames, J, F) model-input rows, as 32-bit patterns
    const uint32_t *run_param;          // (num_runs, E) or nullptr
    uint32_t *x;                        // (batch, RF, J, F)
    uint32_t *param;                    // (batch, E) or nullptr
    int32_t *status;                    // num_runs words: 0 followed, 1 invalid descriptor
    long long total_frames, window0;
    unsigned long long mirror_perm[2];  // window_pack_perm: 5 bits per joint, 12 joints per word
    int num_runs, RF, J, F, E;
    int has_perm;                       // a mirror_perm was given: a flip run is valid
};

// x[.., j, :] of a flip run reads joint perm[j]
__host__ __device__ inline int window_mirror_source(unsigned long long w0, unsigned long long w1, int j) {
    return (int)((j < 12 ? w0 >> (5 * j) : w1 >> (5 * (j - 12))) & 31ull);
}
inline void window_pack_perm(const int32_t *perm, int J, unsigned long long w[2]) {
    w[0] = w[1] = 0ull;
    for (int j = 0; j < J; ++j) w[j < 12 ? 0 : 1] |= (unsigned long long)perm[j] << (5 * (j < 12 ? j : j - 12));
}

// The run a pooled window is looked up in: the last one of the table whose win_first is <= g (a sorted table: the run that holds g,
// if any does), run 0 when none is.  Whatever the table holds the result is an index in [0, num_runs).
__host__ __device__ inline int window_find_run(const r3d_window_run_desc *runs, int num_runs, long long g) {
    int lo = 0, hi = num_runs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (runs[mid].win_first <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A run the call follows (include/ray3d_hip.h: "invalid descriptors", written so that no sum can overflow).  With the limits below
// (n_windows - 1) * step < 2^62 and every frame index start + k * step + i of a valid run lies within +-(2^31 + 2^31 + 2^31).
__host__ __device__ inline bool window_run_valid(long long first, long long n, long long win_first, long long n_windows, long long start,
                                                 int step, int flip, long long total_frames, bool has_perm) {
    const long long lim = R3D_ENCODE_MAX_POINTS;
    if (n < 1 || n_windows < 1 || step < 1) return false;
    if (flip != 0 && flip != 1) return false;
    if (flip && !has_perm) return false;
    if (first < 0 || n > total_frames || first > total_frames - n) return false;
    if (win_first < 0 || n_windows > lim) return false;
    if (start < -lim || start > lim) return false;
    return (n_windows - 1) * (long long)step <= lim - start;      // start + (n_windows - 1) * step <= lim
}

// Row i of window k of a run repeats clip frame clamp(start + k * step + i, 0, n - 1): np.pad(..., 'edge') (generators.py:213-216)
// and the sliding windows of eval_data_prepare (trainer.py:47-58) in one index; no padded copy exists.
__host__ __device__ inline long long window_source_frame(long long start, long long k, int step, int i, long long n) {
    const long long t = start + k * step + i;
    return t < 0 ? 0 : (t > n - 1 ? n - 1 : t);
}

// One output point: F 32-bit patterns copied from (source row, joint j or its mirror partner); a flip run's component 0 has its
// sign bit turned - the exact negation, NaN payloads kept.
__host__ __device__ inline void window_point(const WindowsArgs &a, long long src_row, int flip, int j, uint32_t *o) {
    const int sj = flip ? window_mirror_source(a.mirror_perm[0], a.mirror_perm[1], j) : j;
    const uint32_t *s = a.src + a.F * (src_row * a.J + sj);
    o[0] = flip ? s[0] ^ 0x80000000u : s[0];
    o[1] = s[1];
    if (a.F == 3) o[2] = s[2];
}

// Window w of the batch (pooled window g = window0 + w): the run it is looked up in, that run's verdict and the window's place in it -
// what the workgroup decides, uniformly, before any thread follows the descriptor.
struct WindowRun {
    int r;              // the run the window was looked up in
    bool ok, member;    // its descriptor is valid; it holds the window
    long long first, n, k, start;
    int step, flip;
};
__host__ __device__ inline WindowRun window_lookup(const WindowsArgs &a, long long w) {
    const long long g = a.window0 + w;
    WindowRun q;
    q.r = window_find_run(a.runs, a.num_runs, g);
    const r3d_window_run_desc *d = a.runs + q.r;
    q.first = d->first_frame;
    q.n = d->n_frames;
    q.start = d->start;
    q.step = d->step;
    q.flip = d->flip;
    const long long win_first = d->win_first, n_windows = d->n_windows;
    q.ok = window_run_valid(q.first, q.n, win_first, n_windows, q.start, q.step, q.flip, a.total_frames, a.has_perm != 0);
    q.k = q.ok ? g - win_first : 0;      // (win_first >= 0 and g >= 0: no overflow)
    q.member = q.ok && q.k >= 0 && q.k < n_windows;
    return q;
}

}  // namespace r3d
