// Per-clip pose-error sums of the evaluation loop, on the device in float64.
//
// Replaces, for one clip of N frames, the host side of Trainer.evaluate_core after the forward
// (lib/train_val/trainer.py:355-397): D2H copy, cam.normalized2world in NumPy (lib/camera/camera.py:401-410),
// mpjpe / n_mpjpe (lib/loss/loss.py:12-18, :72-82, torch), p_mpjpe (:30-69, NumPy SVD) and mean_velocity_error
// (:95-104).  Everything is per frame and independent, so a thread owns a frame: it moves prediction and ground
// truth to world coordinates in float64 (fp32 inputs promoted, as NumPy does), evaluates the four per-frame
// errors and the first-difference error against the next frame; a fixed-order tree adds a workgroup's frames up
// and a second, one-wavefront launch adds the workgroups' partial sums in index order - no atomics, the same bits
// on every run.
//
// r3d_clip_metrics_detail runs the same two kernels with MetricArgs::detail set: the frame's five terms go to a per-frame
// table, and the per-joint distances (raw, after the frame's Procrustes fit, root-relative) and the PCK histogram of the
// root-relative distances are added up next to the five sums - a wavefront adds a column over its 64 frames by a fixed
// shuffle tree, its first lane keeps the running sums in LDS, the workgroup adds its four wavefronts in index order and the
// second launch the workgroups.  The counts are integers (LDS integer atomics, exact in any order).  The code of the five
// sums is the same in both modes: the detail is computed again from the poses and the fit, behind a uniform branch.
//
// r3d_clip_valid_losses (Trainer.test's validation losses; r3d_valid_dev.hpp, r3d_valid.hpp) runs on the same two kernels with
// their ValidArgs argument set: a uniform branch at the top of each hands the launch to that mode's own workgroup body, which
// borrows the LDS of the five sums' tree; nothing of the error sums' code runs then, and nothing of that mode otherwise.
//
// r3d_clips_metrics (a whole shard of clips in one launch pair) runs on the same two kernels as well, with their ClipsArgs
// argument set: blockIdx.y names a clip, the workgroup builds its MetricArgs from the clip's descriptor in device memory and
// runs metrics_block - the one workgroup body of the five-sum / detail mode, which the per-clip launch enters with
// (blockIdx.x, gridDim.x) and this one with blockIdx.x and the clip's OWN workgroup count - on the clip's slice of the scratch.
// The frame loop, the wave-of-64 detail sums and both reduction trees are therefore the same instructions for both calls: a
// clip's results have the bits of the per-clip call by construction.  (A mode of the two kernels, as the detail and the
// validation losses are: the modes share the reduction trees.)
//
// r3d_clips_valid_losses (a shard's validation losses in one launch pair) is the two modes combined: ValidArgs AND ClipsArgs set.
// The validation-loss branch then takes its clip from the table by the rule of r3d_clips_metrics - descriptor read once, decided
// on first - moves the shard's buffers to the clip's first frame and runs valid_block, the one workgroup body of that mode, with
// blockIdx.x and the clip's OWN workgroup count on the clip's slice of the scratch; the second launch adds a clip's partial rows
// with valid_sum_rows, one wavefront per clip.  The per-clip call enters the same two bodies with (blockIdx.x, gridDim.x) and the
// rows behind its results: the same instructions, the same bits.
#include <hip/hip_runtime.h>
#include "r3d_internal.hpp"
#include "r3d_valid_dev.hpp"

namespace r3d {

namespace {

constexpr int METRIC_THREADS = 256;
constexpr int MAX_J = 17;
constexpr int METRIC_WAVES = METRIC_THREADS / 64;
constexpr int JOINT_COLS = R3D_DETAIL_JOINT_ROWS * MAX_J;     // per-joint columns of a detail row; the counts follow
static_assert(R3D_DETAIL_DOUBLES == JOINT_COLS + R3D_DETAIL_THRESHOLDS, "layout of a detail row");
constexpr double PCK_STEP = 0.005;                             // threshold k is PCK_STEP * k metres

struct MetricArgs {
    const float *pred, *gt;      // (N, J, 3) each, normalised frame
    double *out;                 // R3D_METRIC_COUNT sums, then R3D_METRIC_COUNT partial sums per workgroup
    long long n;
    int J;
    double R[9], T[3];           // world = R @ p + T  (Rn2w, Tn2w: camera.py:258-259, :401-410)
    double *detail;              // r3d_clip_metrics_detail only (null otherwise): R3D_DETAIL_DOUBLES results, then as many per workgroup
    double *frame;               // ... and, optional, the (N, R3D_METRIC_COUNT) per-frame terms
};
static_assert(METRIC_THREADS == VALID_THREADS && R3D_METRIC_COUNT * METRIC_THREADS >= VALID_WAVES * R3D_VALID_DOUBLES,
              "the validation-loss mode runs in this kernel's workgroups and in the LDS of its five-sum tree");

// r3d_clips_metrics: the table of clips and the shard's buffers (`table` null: not that mode)
struct ClipsArgs {
    const r3d_clip_desc *table;  // num_clips descriptors, device memory
    const float *pred, *gt;      // (total, J, 3) each
    long long total, max_frames;
    int J, blocks;               // blocks = metric_blocks(max_frames): workgroups (and partial rows) per clip
    double *rows, *detail;       // clip c: its five sums at rows + c * row_stride, its detail row (optional) at detail + c * detail_stride
    long long row_stride, detail_stride;
    double *frame;               // optional (total, R3D_METRIC_COUNT)
    double *part, *dpart;        // scratch: (num_clips, blocks, R3D_METRIC_COUNT) partial sums, (num_clips, blocks, R3D_DETAIL_DOUBLES) partial detail rows
    // r3d_clips_valid_losses (ValidArgs::out set as well) reads table, total, max_frames, blocks, rows, row_stride and part - there
    // (num_clips, blocks, R3D_VALID_DOUBLES) partial rows; the buffers and the frame table are ValidArgs's
};
static_assert(sizeof(r3d_clip_desc) == 112 && alignof(r3d_clip_desc) == 8, "layout of r3d_clip_desc (include/ray3d_hip.h)");

// the workgroups that share a clip of n frames
__host__ __device__ inline long long metric_blocks(long long n) {
    const long long b = (n + METRIC_THREADS - 1) / METRIC_THREADS;
    return b < 1 ? 1 : (b > R3D_METRIC_MAX_BLOCKS ? R3D_METRIC_MAX_BLOCKS : b);
}

// a descriptor is followed only when its frames lie inside the buffers and within the caller's bound (uniform per workgroup)
__device__ inline bool clip_desc_valid(long long first, long long n, const ClipsArgs &c) {
    return clip_range_valid(first, n, c.total, c.max_frames);
}

// a double every lane holds the same value of, moved to scalar registers
__device__ inline double uniform(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ inline long long uniform(long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// the similarity fit of one frame: aligned = a * (p Rm) + t
struct Fit {
    double a, Rm[3][3], t[3];
};

// the sum of v over the wavefront's 64 lanes, in lane 0: a fixed tree, the same bits on every run (all lanes active)
__device__ inline double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ inline void to_world(const MetricArgs &a, const float *src, double (*dst)[3]) {
    for (int j = 0; j < a.J; ++j) {
        const double x = (double)src[3 * j], y = (double)src[3 * j + 1], z = (double)src[3 * j + 2];
        for (int r = 0; r < 3; ++r) dst[j][r] = a.R[3 * r] * x + a.R[3 * r + 1] * y + a.R[3 * r + 2] * z + a.T[r];
    }
}

// Singular value decomposition of a 3x3 matrix by one-sided Jacobi rotations (Hestenes): columns of A are rotated
// until mutually orthogonal, A = U diag(s) V^T with U's columns the normalised columns of the result.  Returns the
// columns ordered by decreasing singular value, as LAPACK (np.linalg.svd in loss.py:50) does.
__device__ inline void svd3(double A[3][3], double U[3][3], double s[3], double V[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; ++i) {
                    al += A[i][p] * A[i][p];
                    be += A[i][q] * A[i][q];
                    ga += A[i][p] * A[i][q];
                }
                if (fabs(ga) <= 1e-17 * sqrt(al * be) || ga == 0.0) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double ap = A[i][p], aq = A[i][q];
                    A[i][p] = c * ap - sn * aq;
                    A[i][q] = sn * ap + c * aq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - sn * vq;
                    V[i][q] = sn * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    int order[3] = {0, 1, 2};
    double nrm[3];
    for (int j = 0; j < 3; ++j) nrm[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (nrm[order[j]] < nrm[order[j + 1]]) { const int t = order[j]; order[j] = order[j + 1]; order[j + 1] = t; }
    double Vs[3][3];
    for (int k = 0; k < 3; ++k) {
        const int j = order[k];
        s[k] = nrm[j];
        for (int i = 0; i < 3; ++i) {
            U[i][k] = nrm[j] > 0 ? A[i][j] / nrm[j] : 0.0;
            Vs[i][k] = V[i][j];
        }
    }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) V[i][k] = Vs[i][k];
    // a (nearly) vanishing singular value - planar poses - leaves its left vector to rounding noise: complete the
    // orthonormal basis instead, keeping the column's side (for an exactly zero column either side gives the same
    // aligned pose once the reflection test below has fixed the sign)
    if (s[2] <= 1e-7 * s[0]) {
        const double c0 = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        const double c1 = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        const double c2 = U[0][0] * U[1][1] - U[1][0] * U[0][1];
        const double side = c0 * U[0][2] + c1 * U[1][2] + c2 * U[2][2] < 0 ? -1.0 : 1.0;
        U[0][2] = side * c0;
        U[1][2] = side * c1;
        U[2][2] = side * c2;
    }
}

// mean_j || a * (p_j R) + t - g_j || after the similarity alignment of loss.py:35-66 (target = g, predicted = p)
__device__ inline double procrustes_error(const double (*p)[3], const double (*g)[3], int J, Fit &fit) {
    double mu_g[3] = {0, 0, 0}, mu_p[3] = {0, 0, 0};
    for (int j = 0; j < J; ++j)
        for (int r = 0; r < 3; ++r) { mu_g[r] += g[j][r]; mu_p[r] += p[j][r]; }
    for (int r = 0; r < 3; ++r) { mu_g[r] /= J; mu_p[r] /= J; }
    double ng = 0, np_ = 0;
    for (int j = 0; j < J; ++j)
        for (int r = 0; r < 3; ++r) {
            const double a = g[j][r] - mu_g[r], b = p[j][r] - mu_p[r];
            ng += a * a;
            np_ += b * b;
        }
    ng = sqrt(ng);
    np_ = sqrt(np_);
    // H = X0^T Y0 with X0 = (g - mu_g)/|.|, Y0 = (p - mu_p)/|.|   (:47)
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int j = 0; j < J; ++j)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) H[r][c] += ((g[j][r] - mu_g[r]) / ng) * ((p[j][c] - mu_p[c]) / np_);
    double U[3][3], s[3], V[3][3];
    svd3(H, U, s, V);
    // R = V U^T; reflections are undone by negating V's last column and the last singular value (:51-57)
    double Rm[3][3];
    auto vut = [&]() {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Rm[r][c] = V[r][0] * U[c][0] + V[r][1] * U[c][1] + V[r][2] * U[c][2];
    };
    vut();
    const double det = Rm[0][0] * (Rm[1][1] * Rm[2][2] - Rm[1][2] * Rm[2][1]) - Rm[0][1] * (Rm[1][0] * Rm[2][2] - Rm[1][2] * Rm[2][0]) +
                       Rm[0][2] * (Rm[1][0] * Rm[2][1] - Rm[1][1] * Rm[2][0]);
    const double sg = det > 0 ? 1.0 : (det < 0 ? -1.0 : 0.0);
    for (int r = 0; r < 3; ++r) V[r][2] *= sg;
    s[2] *= sg;
    vut();
    const double a = (s[0] + s[1] + s[2]) * ng / np_;                       // :61
    double t[3];                                                            // t = mu_g - a * (mu_p R)   (:62)
    for (int c = 0; c < 3; ++c) t[c] = mu_g[c] - a * (mu_p[0] * Rm[0][c] + mu_p[1] * Rm[1][c] + mu_p[2] * Rm[2][c]);
    double e = 0;
    for (int j = 0; j < J; ++j) {
        double d2 = 0;
        for (int c = 0; c < 3; ++c) {
            const double v = a * (p[j][0] * Rm[0][c] + p[j][1] * Rm[1][c] + p[j][2] * Rm[2][c]) + t[c] - g[j][c];
            d2 += v * v;
        }
        e += sqrt(d2);
    }
    fit.a = a;
    for (int r = 0; r < 3; ++r) {
        fit.t[r] = t[r];
        for (int c = 0; c < 3; ++c) fit.Rm[r][c] = Rm[r][c];
    }
    return e / J;
}

// The detail of one frame (a lane whose frame lies past the clip's end comes with live = false and adds zeros): every
// per-joint distance is added over the wavefront and kept by lane 0 in `cols` (this wavefront's JOINT_COLS running sums);
// the root-relative distances of joints >= 1 below 150 mm are counted in hist[k], k the first threshold above them.
__device__ __noinline__ void frame_detail(const double (*p)[3], const double (*g)[3], int J, const Fit &fit, bool live,
                                          double *cols, unsigned int *hist) {
    const bool first = (threadIdx.x & 63) == 0;
    for (int j = 0; j < J; ++j) {
        double raw = 0, fitted = 0, rel = 0;
        for (int c = 0; c < 3; ++c) {
            const double d = p[j][c] - g[j][c];
            raw += d * d;
            const double v = fit.a * (p[j][0] * fit.Rm[0][c] + p[j][1] * fit.Rm[1][c] + p[j][2] * fit.Rm[2][c]) + fit.t[c] - g[j][c];
            fitted += v * v;
            const double w = (p[j][c] - p[0][c]) - (g[j][c] - g[0][c]);
            rel += w * w;
        }
        raw = live ? sqrt(raw) : 0.0;
        fitted = live ? sqrt(fitted) : 0.0;
        rel = live ? sqrt(rel) : 0.0;
        if (live && j >= 1 && rel < PCK_STEP * (R3D_DETAIL_THRESHOLDS - 1)) {
            // the first k with rel < PCK_STEP * k, compared against the very products the thresholds are defined by
            int k = (int)(rel / PCK_STEP);
            k = k < 1 ? 1 : (k > R3D_DETAIL_THRESHOLDS - 1 ? R3D_DETAIL_THRESHOLDS - 1 : k);
            while (k < R3D_DETAIL_THRESHOLDS - 1 && !(rel < PCK_STEP * k)) ++k;
            while (k > 1 && rel < PCK_STEP * (k - 1)) --k;
            atomicAdd(&hist[k], 1u);
        }
        raw = wave_sum(raw);
        fitted = wave_sum(fitted);
        rel = wave_sum(rel);
        if (first) {
            cols[j] += raw;
            cols[MAX_J + j] += fitted;
            cols[2 * MAX_J + j] += rel;
        }
    }
}

// The workgroup body of the five-sum / detail mode: workgroup `wg` of the `nwg` that share the clip `a` describes adds up its
// frames - wg * 256 + k * nwg * 256 ... - and leaves its five partial sums in part[0..4] and, with a.detail, its detail row in
// dpart[0..R3D_DETAIL_DOUBLES).  `wg`, `nwg` and every field of `a` are the same for the whole workgroup.
__device__ __forceinline__ void metrics_block(const MetricArgs &a, const int wg, const int nwg, double *part, double *dpart,
                                              double (*red)[METRIC_THREADS], double (*cols)[JOINT_COLS], unsigned int *hist) {
    double acc[R3D_METRIC_COUNT] = {0, 0, 0, 0, 0};
    const int J = a.J;
    const bool detail = a.detail != nullptr;
    if (detail) {
        for (int i = threadIdx.x; i < METRIC_WAVES * JOINT_COLS; i += METRIC_THREADS) (&cols[0][0])[i] = 0.0;
        if (threadIdx.x <= R3D_DETAIL_THRESHOLDS) hist[threadIdx.x] = 0u;
        __syncthreads();
    }
    // a wavefront walks the clip 64 frames at a time: its lanes stay together (the detail adds across them), a lane past
    // the clip's end idles
    const int lane = threadIdx.x & 63;
    for (long long f0 = (long long)wg * METRIC_THREADS + (threadIdx.x - lane); f0 < a.n; f0 += (long long)nwg * METRIC_THREADS) {
        const long long f = f0 + lane;
        const bool live = f < a.n;
        double p[MAX_J][3], g[MAX_J][3];
        Fit fit;
        if (live) {
            double term[R3D_METRIC_COUNT];
            to_world(a, a.pred + f * J * 3, p);
            to_world(a, a.gt + f * J * 3, g);
            // mpjpe (loss.py:17-18) and its root-joint restriction (trainer.py:387)
            double e = 0, pp = 0, gp = 0;
            for (int j = 0; j < J; ++j) {
                double d2 = 0;
                for (int r = 0; r < 3; ++r) {
                    const double d = p[j][r] - g[j][r];
                    d2 += d * d;
                    pp += p[j][r] * p[j][r];
                    gp += g[j][r] * p[j][r];
                }
                const double d = sqrt(d2);
                e += d;
                if (j == 0) term[R3D_METRIC_ROOT] = d;
            }
            term[R3D_METRIC_MPJPE] = e / J;
            // n_mpjpe: scale = mean_j <g,p> / mean_j <p,p>   (loss.py:78-82)
            const double sc = (gp / J) / (pp / J);
            double en = 0;
            for (int j = 0; j < J; ++j) {
                double d2 = 0;
                for (int r = 0; r < 3; ++r) {
                    const double d = sc * p[j][r] - g[j][r];
                    d2 += d * d;
                }
                en += sqrt(d2);
            }
            term[R3D_METRIC_NMPJPE] = en / J;
            term[R3D_METRIC_PMPJPE] = procrustes_error(p, g, J, fit);
            // mean_velocity_error: first differences along the clip (loss.py:101-104)
            term[R3D_METRIC_VELOCITY] = 0.0;
            if (f + 1 < a.n) {
                double p1[MAX_J][3], g1[MAX_J][3];
                to_world(a, a.pred + (f + 1) * J * 3, p1);
                to_world(a, a.gt + (f + 1) * J * 3, g1);
                double ev = 0;
                for (int j = 0; j < J; ++j) {
                    double d2 = 0;
                    for (int r = 0; r < 3; ++r) {
                        const double d = (p1[j][r] - p[j][r]) - (g1[j][r] - g[j][r]);
                        d2 += d * d;
                    }
                    ev += sqrt(d2);
                }
                term[R3D_METRIC_VELOCITY] = ev / J;
            }
            for (int k = 0; k < R3D_METRIC_COUNT; ++k) acc[k] += term[k];
            if (a.frame)
                for (int k = 0; k < R3D_METRIC_COUNT; ++k) a.frame[f * R3D_METRIC_COUNT + k] = term[k];
        } else if (detail) {
            for (int j = 0; j < J; ++j)
                for (int r = 0; r < 3; ++r) p[j][r] = g[j][r] = 0.0;
            fit = Fit{};
        }
        if (detail) frame_detail(p, g, J, fit, live, cols[threadIdx.x >> 6], hist);
    }
    if (detail) {
        // the workgroup's detail row: its wavefronts' sums in index order, then the counts below each threshold
        __syncthreads();
        double *row = dpart;
        for (int c = threadIdx.x; c < R3D_DETAIL_DOUBLES; c += METRIC_THREADS) {
            double v = 0;
            if (c < JOINT_COLS) {
                for (int w = 0; w < METRIC_WAVES; ++w) v += cols[w][c];
            } else {
                unsigned long long below = 0;
                for (int k = 1; k <= c - JOINT_COLS; ++k) below += hist[k];
                v = (double)below;
            }
            row[c] = v;
        }
    }
    for (int k = 0; k < R3D_METRIC_COUNT; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = METRIC_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < R3D_METRIC_COUNT; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < R3D_METRIC_COUNT; ++k) part[k] = red[k][0];
}

__global__ __launch_bounds__(METRIC_THREADS) void r3d_clip_metrics_f64(MetricArgs a, ValidArgs valid, ClipsArgs clips) {
    __shared__ double red[R3D_METRIC_COUNT][METRIC_THREADS];
    __shared__ double cols[METRIC_WAVES][JOINT_COLS];
    __shared__ unsigned int hist[R3D_DETAIL_THRESHOLDS + 1];
    if (valid.out) {             // uniform: the whole launch is a validation-loss one, `a` is unused
        // r3d_clip_valid_losses: the clip of the arguments, every workgroup of the grid on it, partial rows behind the results
        int vwg = gridDim.x;
        double *row = valid.out + R3D_VALID_DOUBLES * (1 + (long long)blockIdx.x);
        if (clips.table) {
            // uniform: r3d_clips_valid_losses - clip blockIdx.y of the table, by the rule of r3d_clips_metrics below (rn2w / tn2w
            // are not read): the descriptor decides first, the shard's buffers are moved to the clip's first frame
            const r3d_clip_desc *d = clips.table + blockIdx.y;
            const long long first = uniform((long long)d->first_frame), n = uniform((long long)d->n_frames);
            if (!clip_desc_valid(first, n, clips)) return;
            vwg = (int)metric_blocks(n);
            if ((int)blockIdx.x >= vwg) return;
            valid.in.pos += first * valid.in.J * 3;
            valid.in.gt += first * valid.in.J * 3;
            if (valid.in.trj) valid.in.trj += first * 3;
            if (valid.frame) valid.frame += first * R3D_VALID_COUNT;
            valid.n = n;
            row = clips.part + ((long long)blockIdx.y * clips.blocks + blockIdx.x) * R3D_VALID_DOUBLES;
        }
        valid_block(valid, (int)blockIdx.x, vwg, row, &red[0][0]);
        return;
    }
    // r3d_clip_metrics(_detail): the clip of the arguments, every workgroup of the grid on it, partial rows behind the results
    int nwg = gridDim.x;
    double *part = a.out + R3D_METRIC_COUNT * (1 + (long long)blockIdx.x);
    double *dpart = a.detail ? a.detail + R3D_DETAIL_DOUBLES * (1 + (long long)blockIdx.x) : nullptr;
    if (clips.table) {
        // uniform: r3d_clips_metrics - clip blockIdx.y of the table; its descriptor is read once, by scalar loads (one address
        // for the workgroup), and decided on before anything else: an invalid one is not followed, a workgroup past the clip's
        // own count has nothing to do
        const r3d_clip_desc *d = clips.table + blockIdx.y;
        const long long first = uniform((long long)d->first_frame), n = uniform((long long)d->n_frames);
        if (!clip_desc_valid(first, n, clips)) return;
        nwg = (int)metric_blocks(n);
        if ((int)blockIdx.x >= nwg) return;
        a.pred = clips.pred + first * clips.J * 3;
        a.gt = clips.gt + first * clips.J * 3;
        a.n = n;
        a.J = clips.J;
        for (int i = 0; i < 9; ++i) a.R[i] = uniform(d->rn2w[i]);
        for (int i = 0; i < 3; ++i) a.T[i] = uniform(d->tn2w[i]);
        a.frame = clips.frame ? clips.frame + first * R3D_METRIC_COUNT : nullptr;
        a.detail = clips.dpart;  // (non-null: the detail mode; the rows themselves go to dpart)
        const long long slot = (long long)blockIdx.y * clips.blocks + blockIdx.x;
        part = clips.part + slot * R3D_METRIC_COUNT;
        dpart = clips.dpart ? clips.dpart + slot * R3D_DETAIL_DOUBLES : nullptr;
    }
    metrics_block(a, (int)blockIdx.x, nwg, part, dpart, red, cols, hist);
}

// One wavefront adds a clip's `blocks` partial rows (part: five sums each; dpart, optional: detail rows) in index order into
// out[0..4] and detail[0..R3D_DETAIL_DOUBLES): the second launch of both calls.
__device__ __forceinline__ void metrics_sum_rows(const double *part, const double *dpart, int blocks, long long n, double *out, double *detail) {
    const int k = threadIdx.x;
    if (k < R3D_METRIC_COUNT) {
        double s = 0;
        for (int b = 0; b < blocks; ++b) s += part[R3D_METRIC_COUNT * b + k];
        // n * mean over the n-1 differences (trainer.py:395 weights the clip's mean by its frame count); an empty mean
        // is NaN in NumPy
        if (k == R3D_METRIC_VELOCITY) s = n > 1 ? s * ((double)n / (double)(n - 1)) : nan("");
        out[k] = s;
    }
    if (detail)
        for (int c = threadIdx.x; c < R3D_DETAIL_DOUBLES; c += 64) {
            double s = 0;
            for (int b = 0; b < blocks; ++b) s += dpart[R3D_DETAIL_DOUBLES * b + c];
            detail[c] = s;
        }
}

__global__ __launch_bounds__(64) void r3d_clip_metrics_sum_f64(double *out, int blocks, long long n, double *detail, double *valid, ClipsArgs clips) {
    if (valid) {                 // the second launch of r3d_clip_valid_losses
        if (clips.table) {       // ... of r3d_clips_valid_losses: workgroup c is clip c's wavefront
            const r3d_clip_desc *d = clips.table + blockIdx.x;
            const long long first = uniform((long long)d->first_frame);
            n = uniform((long long)d->n_frames);
            double *row = clips.rows + (long long)blockIdx.x * clips.row_stride;
            if (!clip_desc_valid(first, n, clips)) {      // nothing of the clip was read: its results are NaN
                for (int c = threadIdx.x; c < R3D_VALID_DOUBLES; c += 64) row[c] = nan("");
                return;
            }
            valid_sum_rows(clips.part + (long long)blockIdx.x * clips.blocks * R3D_VALID_DOUBLES, (int)metric_blocks(n), row);
            return;
        }
        valid_sum_rows(valid + R3D_VALID_DOUBLES, blocks, valid);
        return;
    }
    if (clips.table) {           // ... of r3d_clips_metrics: workgroup c is clip c's wavefront
        const r3d_clip_desc *d = clips.table + blockIdx.x;
        const long long first = uniform((long long)d->first_frame);
        n = uniform((long long)d->n_frames);
        out = clips.rows + (long long)blockIdx.x * clips.row_stride;
        detail = clips.detail ? clips.detail + (long long)blockIdx.x * clips.detail_stride : nullptr;
        if (!clip_desc_valid(first, n, clips)) {      // nothing of the clip was read: its results are NaN
            if (threadIdx.x < R3D_METRIC_COUNT) out[threadIdx.x] = nan("");
            if (detail)
                for (int c = threadIdx.x; c < R3D_DETAIL_DOUBLES; c += 64) detail[c] = nan("");
            return;
        }
        const long long slot = (long long)blockIdx.x * clips.blocks;
        metrics_sum_rows(clips.part + slot * R3D_METRIC_COUNT, detail ? clips.dpart + slot * R3D_DETAIL_DOUBLES : nullptr, (int)metric_blocks(n), n, out, detail);
        return;
    }
    metrics_sum_rows(out + R3D_METRIC_COUNT, detail ? detail + R3D_DETAIL_DOUBLES : nullptr, blocks, n, out, detail);
}

}  // namespace

int launch_clip_metrics(const float *pred, const float *gt, long long n, int J, const double *Rn2w, const double *Tn2w,
                        double *out, double *frame, double *detail, hipStream_t stream) {
    MetricArgs a;
    a.pred = pred;
    a.gt = gt;
    a.out = out;
    a.frame = frame;
    a.detail = detail;
    a.n = n;
    a.J = J;
    for (int i = 0; i < 9; ++i) a.R[i] = Rn2w[i];
    for (int i = 0; i < 3; ++i) a.T[i] = Tn2w[i];
    const long long blocks = metric_blocks(n);
    hipLaunchKernelGGL(r3d_clip_metrics_f64, dim3((unsigned)blocks), dim3(METRIC_THREADS), 0, stream, a, ValidArgs{}, ClipsArgs{});
    hipLaunchKernelGGL(r3d_clip_metrics_sum_f64, dim3(1), dim3(64), 0, stream, out, (int)blocks, n, detail, (double *)nullptr, ClipsArgs{});
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

size_t clips_metrics_scratch_bytes(int num_clips, long long max_frames, bool detail) {
    return (size_t)num_clips * (size_t)metric_blocks(max_frames) * (R3D_METRIC_COUNT + (detail ? R3D_DETAIL_DOUBLES : 0)) * sizeof(double);
}

int launch_clips_metrics(const float *pred, const float *gt, long long total, int J, const r3d_clip_desc *table, int num_clips,
                         long long max_frames, double *rows, long long row_stride, double *detail, long long detail_stride,
                         double *frame, void *scratch, hipStream_t stream) {
    ClipsArgs c = {};
    c.table = table;
    c.pred = pred;
    c.gt = gt;
    c.total = total;
    c.max_frames = max_frames;
    c.J = J;
    c.blocks = (int)metric_blocks(max_frames);
    c.rows = rows;
    c.row_stride = row_stride;
    c.detail = detail;
    c.detail_stride = detail_stride;
    c.frame = frame;
    c.part = static_cast<double *>(scratch);
    c.dpart = detail ? c.part + (size_t)num_clips * c.blocks * R3D_METRIC_COUNT : nullptr;
    hipLaunchKernelGGL(r3d_clip_metrics_f64, dim3((unsigned)c.blocks, (unsigned)num_clips), dim3(METRIC_THREADS), 0, stream, MetricArgs{}, ValidArgs{}, c);
    hipLaunchKernelGGL(r3d_clip_metrics_sum_f64, dim3((unsigned)num_clips), dim3(64), 0, stream, (double *)nullptr, 0, 0ll, (double *)nullptr,
                       (double *)nullptr, c);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_clip_valid(const float *pos, const float *trj, const float *gt, long long n, int J, const int32_t *parents,
                      int flags, double *out, double *frame, hipStream_t stream) {
    MetricArgs a = {};
    ValidArgs v = {};
    v.in.pos = pos;
    v.in.trj = trj;
    v.in.gt = gt;
    v.in.J = J;
    v.in.flags = flags;
    v.in.bones = parents != nullptr;
    v.in.tree = parents ? valid_pack_tree(parents, J) : ValidTree{{0ull, 0ull}};
    v.out = out;
    v.frame = frame;
    v.n = n;
    long long blocks = (n + VALID_THREADS - 1) / VALID_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > R3D_METRIC_MAX_BLOCKS ? R3D_METRIC_MAX_BLOCKS : blocks);
    hipLaunchKernelGGL(r3d_clip_metrics_f64, dim3((unsigned)blocks), dim3(METRIC_THREADS), 0, stream, a, v, ClipsArgs{});
    hipLaunchKernelGGL(r3d_clip_metrics_sum_f64, dim3(1), dim3(64), 0, stream, (double *)nullptr, (int)blocks, n, (double *)nullptr, out, ClipsArgs{});
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

size_t clips_valid_scratch_bytes(int num_clips, long long max_frames) {
    return (size_t)num_clips * (size_t)metric_blocks(max_frames) * R3D_VALID_DOUBLES * sizeof(double);
}

int launch_clips_valid(const float *pos, const float *trj, const float *gt, long long total, int J, const int32_t *parents, int flags,
                       const r3d_clip_desc *table, int num_clips, long long max_frames, double *rows, long long row_stride,
                       double *frame, void *scratch, hipStream_t stream) {
    // both argument sets: ValidArgs the shard's buffers, the tree and the flags, ClipsArgs the table, the bounds, the rows and the scratch
    ValidArgs v = {};
    v.in.pos = pos;
    v.in.trj = trj;
    v.in.gt = gt;
    v.in.J = J;
    v.in.flags = flags;
    v.in.bones = parents != nullptr;
    v.in.tree = parents ? valid_pack_tree(parents, J) : ValidTree{{0ull, 0ull}};
    v.out = rows;
    v.frame = frame;
    ClipsArgs c = {};
    c.table = table;
    c.total = total;
    c.max_frames = max_frames;
    c.J = J;
    c.blocks = (int)metric_blocks(max_frames);
    c.rows = rows;
    c.row_stride = row_stride;
    c.part = static_cast<double *>(scratch);
    hipLaunchKernelGGL(r3d_clip_metrics_f64, dim3((unsigned)c.blocks, (unsigned)num_clips), dim3(METRIC_THREADS), 0, stream, MetricArgs{}, v, c);
    hipLaunchKernelGGL(r3d_clip_metrics_sum_f64, dim3((unsigned)num_clips), dim3(64), 0, stream, (double *)nullptr, 0, 0ll, (double *)nullptr,
                       rows, c);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace r3d
