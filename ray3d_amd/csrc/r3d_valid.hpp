// r3d_clip_valid_losses: the per-frame arithmetic of Trainer.test's validation losses (lib/train_val/trainer.py:187-223,
// lib/loss/loss.py:12-27, lib/skeleton/bone.py:43-100), __host__ __device__ so that the hooks build runs the very same
// routines on the CPU (r3d_debug_valid_losses_host).  The rounding contract of include/ray3d_hip.h: the reference's
// additions and subtractions - root-relative ground truth, pos + trj, prediction minus target, parent minus child - are
// float32 operations with one rounding each; their results are promoted and every norm, division and sum is float64 (IEEE
// divisions, no reciprocal approximations).  Nothing is kept in per-thread arrays: a joint's parent is looked up by a
// data-dependent index, so the routines read the two joints they need from memory (the frame's 2 * J * 12 bytes stay in
// cache) instead of indexing a register array, which would put it into scratch.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "ray3d_hip.h"

namespace r3d {

// parents[1 .. J-1], five bits each (values 0 .. 15), twelve to a word: a kernel argument, read with shifts
struct ValidTree {
    unsigned long long w[2];
};

__host__ __device__ inline int valid_parent(const ValidTree &t, int j) {
    const int k = j - 1;
    return (int)(((k < 12 ? t.w[0] : t.w[1]) >> (5 * (k < 12 ? k : k - 12))) & 31ull);
}

inline ValidTree valid_pack_tree(const int32_t *parents, int J) {
    ValidTree t{{0ull, 0ull}};
    for (int j = 1; j < J; ++j) {
        const int k = j - 1;
        t.w[k < 12 ? 0 : 1] |= (unsigned long long)parents[j] << (5 * (k < 12 ? k : k - 12));
    }
    return t;
}

struct ValidIn {
    const float *pos, *trj, *gt;   // (n, J, 3), (n, 3) or null, (n, J, 3)
    int J, flags;
    bool bones;                    // a parent table was given
    ValidTree tree;
};

// r3d_clips_valid_losses: a descriptor is followed only when its frames lie inside the shard's buffers and within the caller's bound -
// the rule of r3d_clips_metrics (r3d_metrics.hip: clip_desc_valid), shared by the kernels and the host hook
__host__ __device__ inline bool clip_range_valid(long long first, long long n, long long total, long long max_frames) {
    return n >= 1 && n <= max_frames && first >= 0 && first <= total - n;
}

__host__ __device__ inline double valid_norm3(float x, float y, float z) {
    const double a = (double)x, b = (double)y, c = (double)z;
    return sqrt(a * a + b * b + c * c);
}

// joint j of the root-relative prediction (what the pos network gives; R3D_VALID_POS_IS_SUM: pos_dev - trj, rounded once)
__host__ __device__ inline void valid_pos_joint(const ValidIn &a, const float *p, const float *t, int j, float o[3]) {
    for (int c = 0; c < 3; ++c) o[c] = (a.flags & R3D_VALID_POS_IS_SUM) ? p[3 * j + c] - t[c] : p[3 * j + c];
}

// joint j of the root-relative ground truth: gt_j - gt_0 rounded once, the root exactly 0 (trainer.py:193-194); without a
// trajectory the ground truth as it is unless R3D_VALID_GT_ROOT_RELATIVE (:195-197)
__host__ __device__ inline void valid_gt_rel_joint(const ValidIn &a, const float *g, int j, float o[3]) {
    const bool rel = a.trj != nullptr || (a.flags & R3D_VALID_GT_ROOT_RELATIVE);
    for (int c = 0; c < 3; ++c) o[c] = !rel ? g[3 * j + c] : (j == 0 ? 0.0f : g[3 * j + c] - g[c]);
}

// term[R3D_VALID_LOSS .. R3D_VALID_TRJ_DSUM] of frame f
__host__ __device__ inline void valid_frame_terms(const ValidIn &a, long long f, double *term) {
    const int J = a.J;
    const float *p = a.pos + f * J * 3, *g = a.gt + f * J * 3;
    const float *t = a.trj ? a.trj + f * 3 : nullptr;
    double loss = 0, pos = 0;
    for (int j = 0; j < J; ++j) {
        float pr[3], gr[3];
        valid_gt_rel_joint(a, g, j, gr);
        if (t) {
            valid_pos_joint(a, p, t, j, pr);
            // P_abs = pos + trj rounded once (trainer.py:215); with POS_IS_SUM the forward has already written that sum
            float pa[3];
            for (int c = 0; c < 3; ++c) pa[c] = (a.flags & R3D_VALID_POS_IS_SUM) ? p[3 * j + c] : p[3 * j + c] + t[c];
            loss += valid_norm3(pa[0] - g[3 * j], pa[1] - g[3 * j + 1], pa[2] - g[3 * j + 2]);      // :216
            pos += valid_norm3(pr[0] - gr[0], pr[1] - gr[1], pr[2] - gr[2]);                        // :200
        } else {
            loss += valid_norm3(p[3 * j] - gr[0], p[3 * j + 1] - gr[1], p[3 * j + 2] - gr[2]);      // :220 (= :200)
        }
    }
    term[R3D_VALID_LOSS] = loss / J;
    term[R3D_VALID_POS] = t ? pos / J : loss / J;
    term[R3D_VALID_TRJ_W] = term[R3D_VALID_TRJ_WSUM] = term[R3D_VALID_TRJ_DSUM] = 0.0;
    if (t) {
        const double w = fabs(1.0 / (double)g[2]);                                                 // :119 / :217
        const double d = valid_norm3(t[0] - g[0], t[1] - g[1], t[2] - g[2]);
        term[R3D_VALID_TRJ_W] = w * d;
        term[R3D_VALID_TRJ_WSUM] = w;
        term[R3D_VALID_TRJ_DSUM] = d;
    }
}

// bone b (joint parents[b+1] minus joint b+1, bone.py:51-68) of frame f: v = {|len_p - len_g|, len_p, len_p^2, len_g} - the
// R3D_VALID_BONE_ROWS per-bone terms - and dir = |bp / len_p - bg / len_g| (bone.py:97-99, trainer.py:207-209)
__host__ __device__ inline void valid_frame_bone(const ValidIn &a, long long f, int b, double v[4], double &dir) {
    const int J = a.J, j = b + 1, q = valid_parent(a.tree, j);
    const float *p = a.pos + f * J * 3, *g = a.gt + f * J * 3;
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const float *t = a.trj ? a.trj + f * 3 : zero;
    float pj[3], pq[3], gj[3], gq[3], bp[3], bg[3];
    valid_pos_joint(a, p, t, j, pj);
    valid_pos_joint(a, p, t, q, pq);
    valid_gt_rel_joint(a, g, j, gj);
    valid_gt_rel_joint(a, g, q, gq);
    for (int c = 0; c < 3; ++c) {
        bp[c] = pq[c] - pj[c];
        bg[c] = gq[c] - gj[c];
    }
    const double lp = valid_norm3(bp[0], bp[1], bp[2]), lg = valid_norm3(bg[0], bg[1], bg[2]);
    double d2 = 0;
    for (int c = 0; c < 3; ++c) {
        const double u = (double)bp[c] / lp - (double)bg[c] / lg;
        d2 += u * u;
    }
    v[0] = fabs(lp - lg);
    v[1] = lp;
    v[2] = lp * lp;
    v[3] = lg;
    dir = sqrt(d2);
}

}  // namespace r3d
