// Per-clip validation losses of Trainer.test (lib/train_val/trainer.py:187-223) on the device: the workgroup body and the
// row-adding step, run as a MODE of the clip-metrics kernels (r3d_metrics.hip: their ValidArgs argument set) - the library's two
// float64 metrics kernels serve both calls, as they serve r3d_clip_metrics_detail.  The normalised frame, float32
// differences as the reference takes them, float64 from the norms on (r3d_valid.hpp holds the per-frame arithmetic and the
// rounding contract).  The scheme of the clip metrics: a thread owns a frame, a wavefront walks the clip 64 frames at a
// time, at most R3D_METRIC_MAX_BLOCKS workgroups with a fixed frame-to-thread assignment beyond that.  A result row has
// R3D_VALID_DOUBLES (71) columns - seven sums and four per-bone rows - so no thread keeps them: every column is added over
// the wavefront's 64 frames by a fixed shuffle tree, the first lane keeps the wavefront's running sums in LDS, the workgroup
// adds its four wavefronts in index order and the second, one-wavefront launch the workgroups' rows in index order.  No
// floating-point atomics: the same bits on every run.
#pragma once

#include <hip/hip_runtime.h>
#include "r3d_valid.hpp"

namespace r3d {

constexpr int VALID_THREADS = 256;
constexpr int VALID_WAVES = VALID_THREADS / 64;

// r3d_clips_valid_losses (the kernels' ClipsArgs table set as well): in.pos / in.trj / in.gt and `frame` are the SHARD's buffers,
// `out` the strided result rows (only its being set is read); a workgroup moves the buffers to its clip's first frame and takes
// n from the descriptor
struct ValidArgs {
    ValidIn in;
    double *out;       // R3D_VALID_DOUBLES results, then as many per workgroup; null: the launch is not a validation-loss one
    double *frame;     // optional (n, R3D_VALID_COUNT) per-frame terms
    long long n;
};

// the sum of v over the wavefront's 64 lanes, in lane 0: a fixed tree, the same bits on every run (all lanes active)
__device__ inline double valid_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// One workgroup of VALID_THREADS threads - workgroup `wg` of the `nwg` that share the clip `a` describes: it adds up frames
// wg * 256 + k * nwg * 256 ... and leaves its R3D_VALID_DOUBLES sums in `row`.  `cols`: VALID_WAVES * R3D_VALID_DOUBLES doubles
// of LDS.  `wg`, `nwg`, `row` and every field of `a` are the same for the whole workgroup.  The per-clip launch enters with
// (blockIdx.x, gridDim.x) and a row behind its results, r3d_clips_valid_losses with blockIdx.x, the clip's OWN workgroup count
// and the clip's slice of the scratch: the same instructions, the same bits.
__device__ inline void valid_block(const ValidArgs &a, const int wg, const int nwg, double *row, double *cols) {
    for (int i = threadIdx.x; i < VALID_WAVES * R3D_VALID_DOUBLES; i += VALID_THREADS) cols[i] = 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63, J = a.in.J, nb = a.in.bones ? J - 1 : 0;
    const bool first = lane == 0;
    double *mine = cols + (threadIdx.x >> 6) * R3D_VALID_DOUBLES;
    // the wavefront's lanes stay together (the columns are added across them); a lane past the clip's end adds zeros
    for (long long f0 = (long long)wg * VALID_THREADS + (threadIdx.x - lane); f0 < a.n; f0 += (long long)nwg * VALID_THREADS) {
        const long long f = f0 + lane;
        const bool live = f < a.n;
        double term[R3D_VALID_COUNT] = {0, 0, 0, 0, 0, 0, 0};
        if (live) valid_frame_terms(a.in, f, term);
        double bl = 0, bd = 0;
        for (int b = 0; b < nb; ++b) {
            double v[R3D_VALID_BONE_ROWS] = {0, 0, 0, 0}, dir = 0;
            if (live) valid_frame_bone(a.in, f, b, v, dir);
            bl += v[0];
            bd += dir;
            for (int r = 0; r < R3D_VALID_BONE_ROWS; ++r) {
                const double s = valid_wave_sum(v[r]);
                if (first) mine[R3D_VALID_COUNT + r * R3D_VALID_MAX_BONES + b] += s;
            }
        }
        if (live && a.in.bones) {
            // mean over the J - 1 bones (trainer.py:205, :209); a one-joint tree has none: 0 / 0, the empty mean's NaN
            term[R3D_VALID_BONE_LEN] = bl / (double)nb;
            term[R3D_VALID_BONE_DIR] = bd / (double)nb;
        }
        if (live && a.frame)
            for (int k = 0; k < R3D_VALID_COUNT; ++k) a.frame[f * R3D_VALID_COUNT + k] = term[k];
        for (int k = 0; k < R3D_VALID_COUNT; ++k) {
            const double s = valid_wave_sum(term[k]);
            if (first) mine[k] += s;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < R3D_VALID_DOUBLES; c += VALID_THREADS) {
        double v = 0;
        for (int w = 0; w < VALID_WAVES; ++w) v += cols[w * R3D_VALID_DOUBLES + c];
        row[c] = v;
    }
}

// The second launch (one wavefront per clip): the clip's `blocks` partial rows at `part` added in index order into `out`
__device__ inline void valid_sum_rows(const double *part, int blocks, double *out) {
    for (int c = threadIdx.x; c < R3D_VALID_DOUBLES; c += 64) {
        double s = 0;
        for (int b = 0; b < blocks; ++b) s += part[R3D_VALID_DOUBLES * b + c];
        out[c] = s;
    }
}

}  // namespace r3d
