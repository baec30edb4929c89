// extern "C" entry points of libray3d_hip.so (contract: include/ray3d_hip.h).
#include <algorithm>

#include "r3d_internal.hpp"
#include "r3d_clips_repair.hpp"
#include "r3d_poses.hpp"
#include "r3d_streams.hpp"
#include "r3d_streams_assign.hpp"
#include "r3d_streams_fuse.hpp"
#include "r3d_streams_link.hpp"
#include "r3d_streams_peek.hpp"
#include "r3d_streams_poses.hpp"
#include "r3d_streams_repair.hpp"
#include "r3d_undistort.hpp"
#include "r3d_windows.hpp"

using namespace r3d;

// the ranges every call over a shard of clips allows: num_clips, then num_joints
static int clips_range_check(const char *what, int32_t num_clips, int32_t J) {
    if (num_clips < 1 || num_clips > R3D_CLIPS_MAX) { set_error("%s: num_clips must be in 1..%d (got %d)", what, R3D_CLIPS_MAX, num_clips); return R3D_ERR_ARG; }
    if (J < 1 || J > 17) { set_error("%s: num_joints must be in 1..17 (got %d)", what, J); return R3D_ERR_ARG; }
    return R3D_OK;
}

// mirror_perm (null: no flip pass) must be a permutation of the J joints
static int mirror_perm_check(const char *what, const int32_t *mirror_perm, int32_t J) {
    unsigned seen = 0;
    for (int j = 0; mirror_perm && j < J; ++j) {
        if (mirror_perm[j] < 0 || mirror_perm[j] >= J || (seen >> mirror_perm[j] & 1u)) {
            set_error("%s: mirror_perm must be a permutation of 0..%d (entry %d is %d)", what, J - 1, j, mirror_perm[j]);
            return R3D_ERR_ARG;
        }
        seen |= 1u << mirror_perm[j];
    }
    return R3D_OK;
}

// the argument rules of r3d_clips_metrics (every check on the host, before any HIP call)
static int clips_metrics_check_args(const char *what, const float *pred, const float *gt, int64_t total_frames, int32_t J,
                                    const r3d_clip_desc *clips, int32_t num_clips, int64_t max_frames, const double *rows,
                                    int64_t row_stride, const double *detail, int64_t detail_stride, const void *scratch) {
    if (!pred || !gt || !clips || !rows || !scratch) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (const int rc = clips_range_check(what, num_clips, J)) return rc;
    if (max_frames < 1) { set_error("%s: max_frames must be >= 1 (got %lld)", what, (long long)max_frames); return R3D_ERR_ARG; }
    if (total_frames < 1) { set_error("%s: total_frames must be >= 1 (got %lld)", what, (long long)total_frames); return R3D_ERR_ARG; }
    if (row_stride < R3D_METRIC_COUNT) { set_error("%s: row_stride must be >= %d (got %lld)", what, R3D_METRIC_COUNT, (long long)row_stride); return R3D_ERR_ARG; }
    if (detail && detail_stride < R3D_DETAIL_DOUBLES) {
        set_error("%s: detail_stride must be >= %d (got %lld)", what, R3D_DETAIL_DOUBLES, (long long)detail_stride);
        return R3D_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(clips) % 8 || reinterpret_cast<uintptr_t>(scratch) % 8) {
        set_error("%s: clips_dev and scratch_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    return R3D_OK;
}

// the argument rules of r3d_clip_valid_losses, shared with its host hook (`what`: the name in the message)
int r3d::valid_check_args(const char *what, const float *pos, const float *trj, const float *gt, int64_t n, int32_t J,
                          const int32_t *parents, int32_t flags, const double *out) {
    if (!pos || !gt || !out) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (n < 1) { set_error("%s: n_frames must be >= 1 (got %lld)", what, (long long)n); return R3D_ERR_ARG; }
    if (J < 1 || J > 17) { set_error("%s: num_joints must be in 1..17 (got %d)", what, J); return R3D_ERR_ARG; }
    if (flags & ~(R3D_VALID_POS_IS_SUM | R3D_VALID_GT_ROOT_RELATIVE)) { set_error("%s: unknown flags 0x%x", what, flags); return R3D_ERR_ARG; }
    if ((flags & R3D_VALID_POS_IS_SUM) && !trj) { set_error("%s: R3D_VALID_POS_IS_SUM needs trj_dev", what); return R3D_ERR_ARG; }
    if ((flags & R3D_VALID_GT_ROOT_RELATIVE) && trj) {
        set_error("%s: R3D_VALID_GT_ROOT_RELATIVE is for calls without trj_dev (with it the ground truth must be absolute)", what);
        return R3D_ERR_ARG;
    }
    if (parents) {
        if (parents[0] != -1) { set_error("%s: bad parent table: parents[0] must be -1 (got %d)", what, parents[0]); return R3D_ERR_ARG; }
        for (int j = 1; j < J; ++j)
            if (parents[j] < 0 || parents[j] >= j) {
                set_error("%s: bad parent table: parents[%d] must be in 0..%d (got %d)", what, j, j - 1, parents[j]);
                return R3D_ERR_ARG;
            }
    }
    return R3D_OK;
}

// the argument rules of r3d_clips_valid_losses, shared with its host hook: r3d_clip_valid_losses's on the buffers, the tree and the
// flags, r3d_clips_metrics's on the table and the bounds
int r3d::clips_valid_check_args(const char *what, const float *pos, const float *trj, const float *gt, int64_t total_frames, int32_t J,
                                const int32_t *parents, int32_t flags, const r3d_clip_desc *clips, int32_t num_clips, int64_t max_frames,
                                const double *rows, int64_t row_stride, const void *scratch, bool scratch_checked) {
    if (!clips || (scratch_checked && !scratch)) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (total_frames < 1) { set_error("%s: total_frames must be >= 1 (got %lld)", what, (long long)total_frames); return R3D_ERR_ARG; }
    const int rc = valid_check_args(what, pos, trj, gt, total_frames, J, parents, flags, rows);
    if (rc != R3D_OK) return rc;
    if (const int rc2 = clips_range_check(what, num_clips, J)) return rc2;      // (num_joints passed valid_check_args above)
    if (max_frames < 1) { set_error("%s: max_frames must be >= 1 (got %lld)", what, (long long)max_frames); return R3D_ERR_ARG; }
    if (row_stride < R3D_VALID_DOUBLES) { set_error("%s: row_stride must be >= %d (got %lld)", what, R3D_VALID_DOUBLES, (long long)row_stride); return R3D_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(clips) % 8 || (scratch_checked && reinterpret_cast<uintptr_t>(scratch) % 8)) {
        set_error("%s: the clip table and the scratch must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    return R3D_OK;
}

// the argument rules r3d_clips_encode and r3d_clips_project share: `src` the source buffer of total_frames rows, `clips` the table
static int clips_input_check(const char *what, const void *src, int64_t total_frames, int32_t J, int32_t encoding, const void *clips,
                             int32_t num_clips, int64_t max_rows, const float *x, int64_t out_rows, const float *x_mirror,
                             const int32_t *mirror_perm, const int32_t *status) {
    if (!src || !clips || !x || !status) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (const int rc = clips_range_check(what, num_clips, J)) return rc;
    if (encoding != R3D_ENCODE_RAY && encoding != R3D_ENCODE_INTRINSIC && encoding != R3D_ENCODE_SCREEN) {
        set_error("%s: unknown encoding %d", what, encoding);
        return R3D_ERR_ARG;
    }
    if (max_rows < 1 || total_frames < 1 || out_rows < 1) {
        set_error("%s: max_rows, total_frames and out_rows must be >= 1 (got %lld, %lld, %lld)", what, (long long)max_rows,
                  (long long)total_frames, (long long)out_rows);
        return R3D_ERR_ARG;
    }
    if (max_rows > R3D_ENCODE_MAX_POINTS / J || total_frames > R3D_ENCODE_MAX_POINTS || out_rows > R3D_ENCODE_MAX_POINTS) {
        set_error("%s: max_rows * num_joints, total_frames and out_rows must not exceed %d", what, R3D_ENCODE_MAX_POINTS);
        return R3D_ERR_ARG;
    }
    if ((x_mirror != nullptr) != (mirror_perm != nullptr)) {
        set_error("%s: x_mirror_dev and mirror_perm go together (both or neither)", what);
        return R3D_ERR_ARG;
    }
    if (const int rc = mirror_perm_check(what, mirror_perm, J)) return rc;
    if (reinterpret_cast<uintptr_t>(clips) % 8) { set_error("%s: the clip table must be 8-byte aligned", what); return R3D_ERR_ARG; }
    return R3D_OK;
}

// the argument rules of r3d_clips_encode, shared with its host hook (`what`: the name in the message)
int r3d::clips_encode_check_args(const char *what, const float *px, int64_t total_frames, int32_t J, int32_t encoding,
                                 const r3d_clip_input_desc *clips, int32_t num_clips, int64_t max_rows, const float *x, int64_t out_rows,
                                 const float *x_mirror, const int32_t *mirror_perm, const int32_t *status) {
    static_assert(sizeof(r3d_clip_input_desc) == 160, "r3d_clip_input_desc is documented as 160 bytes");
    return clips_input_check(what, px, total_frames, J, encoding, clips, num_clips, max_rows, x, out_rows, x_mirror, mirror_perm, status);
}

// the argument rules of r3d_clips_repair, shared with its host hook; fills the kernel's arguments
int r3d::clips_repair_check_args(const char *what, float *x, int64_t out_rows, int32_t J, int32_t F, float *x_mirror, const int32_t *mirror_perm,
                                 const r3d_clip_input_desc *clips, int32_t num_clips, int64_t max_rows, const float *conf, int64_t total_frames,
                                 float min_conf, int32_t max_gap, uint8_t *state, int32_t *stats, int32_t *status, ClipsRepairArgs *args) {
    if (!x || !clips || !status) { set_error("%s: null pointer (x_dev, clips_dev, status_dev)", what); return R3D_ERR_ARG; }
    if (F != 2 && F != 3) { set_error("%s: in_features must be 2 or 3 (got %d)", what, F); return R3D_ERR_ARG; }
    if (const int rc = clips_range_check(what, num_clips, J)) return rc;
    if (max_rows < 1 || max_rows > R3D_REPAIR_MAX_ROWS) {
        set_error("%s: max_rows must be in 1..%d (got %lld)", what, R3D_REPAIR_MAX_ROWS, (long long)max_rows);
        return R3D_ERR_ARG;
    }
    if (out_rows < 1 || out_rows > R3D_ENCODE_MAX_POINTS) {
        set_error("%s: out_rows must be in 1..%d (got %lld)", what, R3D_ENCODE_MAX_POINTS, (long long)out_rows);
        return R3D_ERR_ARG;
    }
    if (max_gap < 0 || max_gap > R3D_REPAIR_MAX_ROWS) { set_error("%s: max_gap must be in 0..%d (got %d)", what, R3D_REPAIR_MAX_ROWS, max_gap); return R3D_ERR_ARG; }
    if ((__builtin_bit_cast(uint32_t, min_conf) & 0x7f800000u) == 0x7f800000u) { set_error("%s: min_conf must be finite", what); return R3D_ERR_ARG; }
    if (conf && (total_frames < 1 || total_frames > R3D_ENCODE_MAX_POINTS)) {
        set_error("%s: total_frames must be in 1..%d with conf_dev (got %lld)", what, R3D_ENCODE_MAX_POINTS, (long long)total_frames);
        return R3D_ERR_ARG;
    }
    if ((x_mirror != nullptr) != (mirror_perm != nullptr)) {
        set_error("%s: x_mirror_dev and mirror_perm go together (both or neither)", what);
        return R3D_ERR_ARG;
    }
    if (const int rc = mirror_perm_check(what, mirror_perm, J)) return rc;
    if (reinterpret_cast<uintptr_t>(clips) % 8) { set_error("%s: the clip table must be 8-byte aligned", what); return R3D_ERR_ARG; }
    // the call works in place on x_dev / x_mirror_dev, and on nothing else: no other extent may overlap them, nor they each other
    // (address ranges; the sizes fit in 64 bits)
    const uintptr_t x_bytes = (uintptr_t)out_rows * J * F * sizeof(float);
    const char *io_name[2] = {"x_dev", "x_mirror_dev"};
    const uintptr_t io[2] = {reinterpret_cast<uintptr_t>(x), reinterpret_cast<uintptr_t>(x_mirror)};
    if (io[1] && io[0] < io[1] + x_bytes && io[1] < io[0] + x_bytes) { set_error("%s: x_dev overlaps x_mirror_dev", what); return R3D_ERR_ARG; }
    const char *name[5] = {"state_dev", "stats_dev", "status_dev", "conf_dev", "the clip table"};
    const uintptr_t at[5] = {reinterpret_cast<uintptr_t>(state), reinterpret_cast<uintptr_t>(stats), reinterpret_cast<uintptr_t>(status),
                             reinterpret_cast<uintptr_t>(conf), reinterpret_cast<uintptr_t>(clips)};
    const uintptr_t bytes[5] = {(uintptr_t)out_rows * J, (uintptr_t)num_clips * J * 4 * sizeof(int32_t), (uintptr_t)num_clips * sizeof(int32_t),
                                conf ? (uintptr_t)total_frames * J * sizeof(float) : 0, (uintptr_t)num_clips * sizeof(r3d_clip_input_desc)};
    for (int o = 0; o < 5; ++o)
        for (int i = 0; i < 2; ++i)
            if (at[o] && io[i] && at[o] < io[i] + x_bytes && io[i] < at[o] + bytes[o]) {
                set_error("%s: %s overlaps %s", what, name[o], io_name[i]);
                return R3D_ERR_ARG;
            }
    ClipsRepairArgs a = {};
    a.table = clips;
    a.x = reinterpret_cast<uint32_t *>(x);
    a.x_mirror = reinterpret_cast<uint32_t *>(x_mirror);
    a.conf = conf;
    a.state = state;
    a.stats = stats;
    a.status = status;
    a.out_rows = out_rows;
    a.max_rows = max_rows;
    a.total_frames = conf ? total_frames : 0;
    if (mirror_perm) mirror_pack_inverse(mirror_perm, J, a.mirror_inv);
    a.min_conf = min_conf;
    a.J = J;
    a.F = F;
    a.max_gap = max_gap;
    *args = a;
    return R3D_OK;
}

// the argument rules of r3d_clips_project, shared with its host hook: r3d_clips_encode's on the source, the table and the inputs it
// writes; then its own - the extent of gt_dev / px_dev when either is given, and the alignment of the float64 pixels
int r3d::clips_project_check_args(const char *what, const float *world, int64_t total_frames, int32_t J, int32_t encoding,
                                  const r3d_clip_project_desc *clips, int32_t num_clips, int64_t max_rows, const float *x, int64_t out_rows,
                                  const float *x_mirror, const int32_t *mirror_perm, const float *gt, const double *px, int64_t gt_rows,
                                  const int32_t *status) {
    static_assert(sizeof(r3d_clip_project_desc) == 360, "r3d_clip_project_desc is documented as 360 bytes");
    if (const int rc = clips_input_check(what, world, total_frames, J, encoding, clips, num_clips, max_rows, x, out_rows, x_mirror,
                                         mirror_perm, status))
        return rc;
    if ((gt || px) && (gt_rows < 1 || gt_rows > R3D_ENCODE_MAX_POINTS)) {
        set_error("%s: gt_rows must be in 1..%d when gt_dev or px_dev is given (got %lld)", what, R3D_ENCODE_MAX_POINTS, (long long)gt_rows);
        return R3D_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(px) % 8) { set_error("%s: px_dev must be 8-byte aligned", what); return R3D_ERR_ARG; }
    return R3D_OK;
}

// the argument rules of r3d_clips_poses, shared with its host hook (`what`: the name in the message)
int r3d::clips_poses_check_args(const char *what, const float *raw, const float *raw_mirror, int64_t raw_rows, int32_t J,
                                const int32_t *mirror_perm, const r3d_clip_desc *clips, const int64_t *raw_first, int32_t num_clips,
                                int64_t max_frames, const float *pred, const double *world, int64_t total_frames, const int32_t *status) {
    if (!raw || !clips || !raw_first || !status) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (!pred && !world) { set_error("%s: pred_dev and world_dev are both null: nothing to write", what); return R3D_ERR_ARG; }
    if (const int rc = clips_range_check(what, num_clips, J)) return rc;
    if (max_frames < 1 || total_frames < 1 || raw_rows < 1) {
        set_error("%s: max_frames, total_frames and raw_rows must be >= 1 (got %lld, %lld, %lld)", what, (long long)max_frames,
                  (long long)total_frames, (long long)raw_rows);
        return R3D_ERR_ARG;
    }
    if (max_frames > R3D_ENCODE_MAX_POINTS / J || total_frames > R3D_ENCODE_MAX_POINTS || raw_rows > R3D_ENCODE_MAX_POINTS) {
        set_error("%s: max_frames * num_joints, total_frames and raw_rows must not exceed %d", what, R3D_ENCODE_MAX_POINTS);
        return R3D_ERR_ARG;
    }
    if ((raw_mirror != nullptr) != (mirror_perm != nullptr)) {
        set_error("%s: raw_mirror_dev and mirror_perm go together (both or neither)", what);
        return R3D_ERR_ARG;
    }
    if (const int rc = mirror_perm_check(what, mirror_perm, J)) return rc;
    if (reinterpret_cast<uintptr_t>(clips) % 8 || reinterpret_cast<uintptr_t>(raw_first) % 8 || reinterpret_cast<uintptr_t>(world) % 8) {
        set_error("%s: the clip table, raw_first_dev and world_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    // in-place use is refused: an output extent may not overlap an input extent (address ranges; the sizes fit in 64 bits)
    const uintptr_t in_bytes = (uintptr_t)raw_rows * J * 3 * sizeof(float);
    const uintptr_t out_bytes[2] = {(uintptr_t)total_frames * J * 3 * sizeof(float), (uintptr_t)total_frames * J * 3 * sizeof(double)};
    const uintptr_t outs[2] = {reinterpret_cast<uintptr_t>(pred), reinterpret_cast<uintptr_t>(world)};
    const uintptr_t ins[2] = {reinterpret_cast<uintptr_t>(raw), reinterpret_cast<uintptr_t>(raw_mirror)};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 2; ++i)
            if (outs[o] && ins[i] && outs[o] < ins[i] + in_bytes && ins[i] < outs[o] + out_bytes[o]) {
                set_error("%s: %s overlaps %s: the call does not work in place", what, o ? "world_dev" : "pred_dev", i ? "raw_mirror_dev" : "raw_dev");
                return R3D_ERR_ARG;
            }
    return R3D_OK;
}

// the argument rules of r3d_clips_windows, shared with its host hook; fills the kernel's arguments
int r3d::clips_windows_check_args(const char *what, const float *src, int64_t total_frames, int32_t J, int32_t F, int32_t RF,
                                  const r3d_window_run_desc *runs, int32_t num_runs, const float *run_param, int32_t E, int64_t window0,
                                  int64_t batch, float *x, float *param, const int32_t *mirror_perm, int32_t *status, WindowsArgs *args) {
    static_assert(sizeof(r3d_window_run_desc) == 48, "r3d_window_run_desc is documented as 48 bytes");
    if (!src || !runs || !x || !status) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (const int rc = clips_range_check(what, num_runs, J)) return rc;
    if (F != 2 && F != 3) { set_error("%s: in_features must be 2 or 3 (got %d)", what, F); return R3D_ERR_ARG; }
    if (RF < 1 || total_frames < 1) {
        set_error("%s: receptive_field and total_frames must be >= 1 (got %d, %lld)", what, RF, (long long)total_frames);
        return R3D_ERR_ARG;
    }
    if (batch < 1 || batch > 65535) { set_error("%s: batch must be in 1..65535 (got %lld)", what, (long long)batch); return R3D_ERR_ARG; }
    if (window0 < 0 || window0 > (1ll << 62)) { set_error("%s: window0 must be in 0..2^62 (got %lld)", what, (long long)window0); return R3D_ERR_ARG; }
    if (RF > R3D_ENCODE_MAX_POINTS / J || total_frames > R3D_ENCODE_MAX_POINTS || batch > R3D_ENCODE_MAX_POINTS / ((int64_t)RF * J)) {
        set_error("%s: receptive_field * num_joints, total_frames and batch * receptive_field * num_joints must not exceed %d", what,
                  R3D_ENCODE_MAX_POINTS);
        return R3D_ERR_ARG;
    }
    if ((run_param != nullptr) != (param != nullptr)) {
        set_error("%s: run_param_dev and param_dev go together (both or neither)", what);
        return R3D_ERR_ARG;
    }
    if (run_param && E < 1) { set_error("%s: extrinsic_dim must be >= 1 with run_param_dev (got %d)", what, E); return R3D_ERR_ARG; }
    if (const int rc = mirror_perm_check(what, mirror_perm, J)) return rc;
    if (reinterpret_cast<uintptr_t>(runs) % 8) { set_error("%s: the run table must be 8-byte aligned", what); return R3D_ERR_ARG; }
    WindowsArgs a = {};
    a.runs = runs;
    a.src = reinterpret_cast<const uint32_t *>(src);
    a.run_param = reinterpret_cast<const uint32_t *>(run_param);
    a.x = reinterpret_cast<uint32_t *>(x);
    a.param = reinterpret_cast<uint32_t *>(param);
    a.status = status;
    a.total_frames = total_frames;
    a.window0 = window0;
    if (mirror_perm) window_pack_perm(mirror_perm, J, a.mirror_perm);
    a.num_runs = num_runs;
    a.RF = RF;
    a.J = J;
    a.F = F;
    a.E = run_param ? E : 0;
    a.has_perm = mirror_perm != nullptr;
    *args = a;
    return R3D_OK;
}

// the shape rules of r3d_streams_step that r3d_streams_state_bytes answers with 0 (no message) and the call with R3D_ERR_ARG
static bool streams_shape_ok(int32_t S, int32_t RF, int32_t J, int32_t F) {
    return S >= 1 && S <= R3D_CLIPS_MAX && J >= 1 && J <= 17 && RF >= 1 && (F == 2 || F == 3) && RF <= R3D_ENCODE_MAX_POINTS / J &&
           S <= R3D_ENCODE_MAX_POINTS / ((int64_t)RF * J);
}

// the rules of the arguments r3d_streams_step and r3d_streams_repair share (the pointers' null checks aside), in the step's order
static int streams_shared_check(const char *what, int32_t S, int32_t RF, int32_t lag, int32_t J, int32_t F, int32_t encoding, const double *cam) {
    static_assert(R3D_ENCODE_RAY == ENC_RAY && R3D_ENCODE_INTRINSIC == ENC_INTRINSIC && R3D_ENCODE_SCREEN == ENC_SCREEN, "encode_point_f32 takes them");
    if (S < 1 || S > R3D_CLIPS_MAX) { set_error("%s: num_streams must be in 1..%d (got %d)", what, R3D_CLIPS_MAX, S); return R3D_ERR_ARG; }
    if (J < 1 || J > 17) { set_error("%s: num_joints must be in 1..17 (got %d)", what, J); return R3D_ERR_ARG; }
    if (RF < 1) { set_error("%s: receptive_field must be >= 1 (got %d)", what, RF); return R3D_ERR_ARG; }
    if (lag < 0 || lag > RF - 1) { set_error("%s: lag must be in 0..receptive_field - 1 (got %d)", what, lag); return R3D_ERR_ARG; }
    const bool pixels = encoding == R3D_ENCODE_RAY || encoding == R3D_ENCODE_INTRINSIC || encoding == R3D_ENCODE_SCREEN;
    if (!pixels && encoding != R3D_ENCODE_NONE) { set_error("%s: unknown encoding %d", what, encoding); return R3D_ERR_ARG; }
    if (pixels ? F != enc_floats(encoding) : (F != 2 && F != 3)) {
        set_error("%s: in_features %d does not go with encoding %d", what, F, encoding);
        return R3D_ERR_ARG;
    }
    if (pixels && !cam) { set_error("%s: a pixel encoding needs cam_dev", what); return R3D_ERR_ARG; }
    return R3D_OK;
}

// the argument rules of r3d_streams_step, shared with its host hook; fills the kernel's arguments
int r3d::streams_check_args(const char *what, void *state, int32_t S, int32_t RF, int32_t lag, int32_t J, int32_t F, int32_t encoding,
                            const float *frame, const double *cam, const int32_t *action, float *x, float *x_mirror,
                            const int32_t *mirror_perm, int64_t *emit, int32_t *status, StreamsArgs *args) {
    static_assert(sizeof(r3d_stream_head) == 16, "r3d_stream_head is documented as 16 bytes");
    if (!state || !frame || !action || !x || !emit || !status) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (const int rc = streams_shared_check(what, S, RF, lag, J, F, encoding, cam)) return rc;
    const bool pixels = encoding != R3D_ENCODE_NONE;
    if ((x_mirror != nullptr) != (mirror_perm != nullptr)) {
        set_error("%s: x_mirror_dev and mirror_perm go together (both or neither)", what);
        return R3D_ERR_ARG;
    }
    if (const int rc = mirror_perm_check(what, mirror_perm, J)) return rc;
    if (!streams_shape_ok(S, RF, J, F)) {
        set_error("%s: receptive_field * num_joints and num_streams * receptive_field * num_joints must not exceed %d", what,
                  R3D_ENCODE_MAX_POINTS);
        return R3D_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(state) % 8 || reinterpret_cast<uintptr_t>(emit) % 8 || reinterpret_cast<uintptr_t>(cam) % 8) {
        set_error("%s: the state, emit_dev and cam_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    StreamsArgs a = {};
    a.heads = static_cast<r3d_stream_head *>(state);
    a.ring = reinterpret_cast<uint32_t *>(a.heads + S);
    a.frame = reinterpret_cast<const uint32_t *>(frame);
    a.cam = pixels ? cam : nullptr;
    a.action = action;
    a.x = reinterpret_cast<uint32_t *>(x);
    a.x_mirror = reinterpret_cast<uint32_t *>(x_mirror);
    a.emit = reinterpret_cast<long long *>(emit);
    a.status = status;
    if (mirror_perm) window_pack_perm(mirror_perm, J, a.mirror_perm);
    a.S = S;
    a.RF = RF;
    a.lag = lag;
    a.J = J;
    a.F = F;
    a.encoding = encoding;
    *args = a;
    return R3D_OK;
}

// the argument rules of r3d_streams_repair, shared with its host hook; fills the kernel's arguments
int r3d::streams_repair_check_args(const char *what, void *state, void *track, int32_t S, int32_t RF, int32_t lag, int32_t J, int32_t F,
                                   int32_t encoding, const float *frame, const float *conf, float min_conf, const double *cam,
                                   const int32_t *action, int32_t max_gap, float *frame_out, uint32_t *synthetic, StreamsRepairArgs *args) {
    if (!state || !frame || !action) { set_error("%s: null pointer (state_dev, frame_dev, action_dev)", what); return R3D_ERR_ARG; }
    if (!track) { set_error("%s: track_dev is null", what); return R3D_ERR_ARG; }
    if (!frame_out) { set_error("%s: frame_out_dev is null", what); return R3D_ERR_ARG; }
    if (!synthetic) { set_error("%s: synthetic_dev is null", what); return R3D_ERR_ARG; }
    if (const int rc = streams_shared_check(what, S, RF, lag, J, F, encoding, cam)) return rc;
    if (!streams_shape_ok(S, RF, J, F)) {
        set_error("%s: receptive_field * num_joints and num_streams * receptive_field * num_joints must not exceed %d", what,
                  R3D_ENCODE_MAX_POINTS);
        return R3D_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(state) % 8 || reinterpret_cast<uintptr_t>(cam) % 8) {
        set_error("%s: the state and cam_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(track) % 8) { set_error("%s: track_dev must be 8-byte aligned", what); return R3D_ERR_ARG; }
    if (max_gap < 0 || max_gap > RF - 1) { set_error("%s: max_gap must be in 0..receptive_field - 1 (got %d)", what, max_gap); return R3D_ERR_ARG; }
    if ((__builtin_bit_cast(uint32_t, min_conf) & 0x7f800000u) == 0x7f800000u) { set_error("%s: min_conf must be finite", what); return R3D_ERR_ARG; }
    // frame_out_dev may not overlap what the call reads or keeps (address ranges; the sizes fit in 64 bits)
    const int width = encoding == R3D_ENCODE_NONE ? F : 2;
    const uintptr_t row_bytes = (uintptr_t)S * J * width * sizeof(float), out = reinterpret_cast<uintptr_t>(frame_out);
    const char *in_name[4] = {"frame_dev", "conf_dev", "the state", "the track"};
    const uintptr_t ins[4] = {reinterpret_cast<uintptr_t>(frame), reinterpret_cast<uintptr_t>(conf), reinterpret_cast<uintptr_t>(state),
                              reinterpret_cast<uintptr_t>(track)};
    const uintptr_t in_bytes[4] = {row_bytes, (uintptr_t)S * J * sizeof(float), streams_state_bytes(S, RF, J, F), streams_track_bytes(S, RF, J, width)};
    for (int i = 0; i < 4; ++i)
        if (ins[i] && out < ins[i] + in_bytes[i] && ins[i] < out + row_bytes) {
            set_error("%s: frame_out_dev overlaps %s", what, in_name[i]);
            return R3D_ERR_ARG;
        }
    StreamsRepairArgs a = {};
    a.heads = static_cast<const r3d_stream_head *>(state);
    a.ring = reinterpret_cast<uint32_t *>(static_cast<r3d_stream_head *>(state) + S);
    a.age = static_cast<int32_t *>(track);
    a.last = reinterpret_cast<uint32_t *>(a.age + (size_t)S * J);
    a.missing = a.last + (size_t)S * J * width;
    a.frame = reinterpret_cast<const uint32_t *>(frame);
    a.conf = conf;
    a.cam = encoding == R3D_ENCODE_NONE ? nullptr : cam;
    a.action = action;
    a.frame_out = reinterpret_cast<uint32_t *>(frame_out);
    a.synthetic = synthetic;
    a.min_conf = min_conf;
    a.S = S;
    a.RF = RF;
    a.lag = lag;
    a.J = J;
    a.F = F;
    a.width = width;
    a.encoding = encoding;
    a.max_gap = max_gap;
    *args = a;
    return R3D_OK;
}

// the argument rules of r3d_streams_peek, shared with its host hook; fills the kernel's arguments
int r3d::streams_peek_check_args(const char *what, const void *state, int32_t S, int32_t RF, int32_t lag, int32_t J, int32_t F,
                                 const int32_t *looks, int32_t num_looks, const int32_t *action, const int32_t *status, float *x,
                                 float *x_mirror, const int32_t *mirror_perm, int64_t *emit, int32_t *peek_status, StreamsPeekArgs *args) {
    if (!state || !looks || !status || !x || !emit || !peek_status) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (S < 1 || S > R3D_CLIPS_MAX) { set_error("%s: num_streams must be in 1..%d (got %d)", what, R3D_CLIPS_MAX, S); return R3D_ERR_ARG; }
    if (J < 1 || J > 17) { set_error("%s: num_joints must be in 1..17 (got %d)", what, J); return R3D_ERR_ARG; }
    if (RF < 1) { set_error("%s: receptive_field must be >= 1 (got %d)", what, RF); return R3D_ERR_ARG; }
    if (lag < 0 || lag > RF - 1) { set_error("%s: lag must be in 0..receptive_field - 1 (got %d)", what, lag); return R3D_ERR_ARG; }
    if (F != 2 && F != 3) { set_error("%s: in_features must be 2 or 3 (got %d)", what, F); return R3D_ERR_ARG; }
    if (lag == 0) { set_error("%s: lag is 0 (a causal model): a look lies in 0..lag - 1, so none is admissible", what); return R3D_ERR_ARG; }
    if (num_looks < 1 || num_looks > R3D_STREAMS_PEEK_MAX) {
        set_error("%s: num_looks must be in 1..%d (got %d)", what, R3D_STREAMS_PEEK_MAX, num_looks);
        return R3D_ERR_ARG;
    }
    for (int k = 0; k < num_looks; ++k) {
        if (looks[k] < 0 || looks[k] >= lag) { set_error("%s: looks[%d] must be in 0..lag - 1 = %d (got %d)", what, k, lag - 1, looks[k]); return R3D_ERR_ARG; }
        if (k && looks[k] <= looks[k - 1]) { set_error("%s: looks must be strictly increasing (looks[%d] = %d after %d)", what, k, looks[k], looks[k - 1]); return R3D_ERR_ARG; }
    }
    if ((x_mirror != nullptr) != (mirror_perm != nullptr)) {
        set_error("%s: x_mirror_dev and mirror_perm go together (both or neither)", what);
        return R3D_ERR_ARG;
    }
    if (const int rc = mirror_perm_check(what, mirror_perm, J)) return rc;
    if (!streams_shape_ok(S, RF, J, F) || (int64_t)num_looks * S > R3D_ENCODE_MAX_POINTS / ((int64_t)RF * J)) {
        set_error("%s: receptive_field * num_joints and num_looks * num_streams * receptive_field * num_joints must not exceed %d", what,
                  R3D_ENCODE_MAX_POINTS);
        return R3D_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(state) % 8 || reinterpret_cast<uintptr_t>(emit) % 8) {
        set_error("%s: the state and emit_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    StreamsPeekArgs a = {};
    a.heads = static_cast<const r3d_stream_head *>(state);
    a.ring = reinterpret_cast<const uint32_t *>(a.heads + S);
    a.action = action;
    a.status = status;
    a.x = reinterpret_cast<uint32_t *>(x);
    a.x_mirror = reinterpret_cast<uint32_t *>(x_mirror);
    a.emit = reinterpret_cast<long long *>(emit);
    a.peek_status = peek_status;
    if (mirror_perm) window_pack_perm(mirror_perm, J, a.mirror_perm);
    for (int k = 0; k < num_looks; ++k) a.looks[k] = looks[k];
    a.S = S;
    a.RF = RF;
    a.lag = lag;
    a.J = J;
    a.F = F;
    a.K = num_looks;
    *args = a;
    return R3D_OK;
}

// the argument rules of r3d_streams_poses, shared with its host hook; fills the kernel's arguments
int r3d::streams_poses_check_args(const char *what, const float *raw, const float *raw_mirror, int32_t S, int32_t J,
                                  const int32_t *mirror_perm, const int64_t *emit, const int32_t *status, const r3d_stream_pose_desc *desc,
                                  const double *cam, const float *x, int32_t RF, int32_t lag, float *pred, double *world, double *reproj,
                                  double *quality, StreamsPosesArgs *args) {
    static_assert(sizeof(r3d_stream_pose_desc) == 112, "r3d_stream_pose_desc is documented as 112 bytes");
    if (!raw || !emit || !status) { set_error("%s: null pointer", what); return R3D_ERR_ARG; }
    if (!pred && !world && !reproj) { set_error("%s: pred_dev, world_dev and reproj_dev are all null: nothing to write", what); return R3D_ERR_ARG; }
    if (quality && !reproj) { set_error("%s: quality_dev needs reproj_dev", what); return R3D_ERR_ARG; }
    if ((world || reproj) && !desc) { set_error("%s: world_dev and reproj_dev need desc_dev", what); return R3D_ERR_ARG; }
    if (reproj && (!cam || !x)) { set_error("%s: reproj_dev needs cam_dev and x_dev", what); return R3D_ERR_ARG; }
    if (S < 1 || S > R3D_CLIPS_MAX) { set_error("%s: num_streams must be in 1..%d (got %d)", what, R3D_CLIPS_MAX, S); return R3D_ERR_ARG; }
    if (J < 1 || J > 17) { set_error("%s: num_joints must be in 1..17 (got %d)", what, J); return R3D_ERR_ARG; }
    if ((raw_mirror != nullptr) != (mirror_perm != nullptr)) {
        set_error("%s: raw_mirror_dev and mirror_perm go together (both or neither)", what);
        return R3D_ERR_ARG;
    }
    if (const int rc = mirror_perm_check(what, mirror_perm, J)) return rc;
    if (reproj) {
        if (RF < 1) { set_error("%s: receptive_field must be >= 1 (got %d)", what, RF); return R3D_ERR_ARG; }
        if (lag < 0 || lag > RF - 1) { set_error("%s: lag must be in 0..receptive_field - 1 (got %d)", what, lag); return R3D_ERR_ARG; }
        if (S > R3D_ENCODE_MAX_POINTS / ((int64_t)RF * J)) {
            set_error("%s: num_streams * receptive_field * num_joints must not exceed %d", what, R3D_ENCODE_MAX_POINTS);
            return R3D_ERR_ARG;
        }
    }
    if (reinterpret_cast<uintptr_t>(emit) % 8 || reinterpret_cast<uintptr_t>(desc) % 8 || reinterpret_cast<uintptr_t>(cam) % 8 ||
        reinterpret_cast<uintptr_t>(world) % 8 || reinterpret_cast<uintptr_t>(reproj) % 8 || reinterpret_cast<uintptr_t>(quality) % 8) {
        set_error("%s: emit_dev, desc_dev, cam_dev, world_dev, reproj_dev and quality_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    // in-place use is refused: an output extent may not overlap an input extent (address ranges; the sizes fit in 64 bits).  x_dev is
    // an input only with reproj_dev (its extent is known only then).
    const uintptr_t pts = (uintptr_t)S * J;
    const char *out_name[4] = {"pred_dev", "world_dev", "reproj_dev", "quality_dev"}, *in_name[3] = {"raw_dev", "raw_mirror_dev", "x_dev"};
    const uintptr_t outs[4] = {reinterpret_cast<uintptr_t>(pred), reinterpret_cast<uintptr_t>(world), reinterpret_cast<uintptr_t>(reproj),
                               reinterpret_cast<uintptr_t>(quality)};
    const uintptr_t out_bytes[4] = {pts * 3 * sizeof(float), pts * 3 * sizeof(double), pts * sizeof(double), (uintptr_t)S * 2 * sizeof(double)};
    const uintptr_t ins[3] = {reinterpret_cast<uintptr_t>(raw), reinterpret_cast<uintptr_t>(raw_mirror), reproj ? reinterpret_cast<uintptr_t>(x) : 0};
    const uintptr_t in_bytes[3] = {pts * 3 * sizeof(float), pts * 3 * sizeof(float), reproj ? pts * (uintptr_t)RF * 3 * sizeof(float) : 0};
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i < 3; ++i)
            if (outs[o] && ins[i] && outs[o] < ins[i] + in_bytes[i] && ins[i] < outs[o] + out_bytes[o]) {
                set_error("%s: %s overlaps %s: the call does not work in place", what, out_name[o], in_name[i]);
                return R3D_ERR_ARG;
            }
    StreamsPosesArgs a = {};
    a.raw = raw;
    a.raw_mirror = raw_mirror;
    a.emit = reinterpret_cast<const long long *>(emit);
    a.status = status;
    a.desc = (world || reproj) ? desc : nullptr;
    a.cam = reproj ? cam : nullptr;
    a.x = reproj ? x : nullptr;
    a.pred = pred;
    a.world = world;
    a.reproj = reproj;
    a.quality = quality;
    if (mirror_perm) pose_pack_perm(mirror_perm, J, a.mirror_perm);
    a.S = S;
    a.J = J;
    a.RF = reproj ? RF : 1;
    a.lag = reproj ? lag : 0;
    *args = a;
    return R3D_OK;
}

// the argument rules of r3d_streams_fuse, shared with its host hook; fills the kernel's arguments
int r3d::streams_fuse_check_args(const char *what, const double *world, const double *reproj, const int64_t *emit, const int32_t *status,
                                 const uint32_t *synthetic, int32_t S, int32_t J, const int32_t *member, int32_t G, int32_t M,
                                 double soft_px, double max_px, double max_dist, double *fused, double *spread, int32_t *count,
                                 uint32_t *used, StreamsFuseArgs *args) {
    if (!world || !emit || !status || !member || !fused) {
        set_error("%s: null pointer (world_dev, emit_dev, status_dev, member_dev, fused_dev)", what);
        return R3D_ERR_ARG;
    }
    if (S < 1 || S > R3D_CLIPS_MAX) { set_error("%s: num_streams must be in 1..%d (got %d)", what, R3D_CLIPS_MAX, S); return R3D_ERR_ARG; }
    if (G < 1 || G > R3D_CLIPS_MAX) { set_error("%s: num_groups must be in 1..%d (got %d)", what, R3D_CLIPS_MAX, G); return R3D_ERR_ARG; }
    if (J < 1 || J > 17) { set_error("%s: num_joints must be in 1..17 (got %d)", what, J); return R3D_ERR_ARG; }
    if (M < 1 || M > R3D_FUSE_MAX_MEMBERS) { set_error("%s: max_members must be in 1..%d (got %d)", what, R3D_FUSE_MAX_MEMBERS, M); return R3D_ERR_ARG; }
    if (!stream_finite_bits64(soft_px) || !(soft_px > 0.0)) { set_error("%s: soft_px must be finite and > 0", what); return R3D_ERR_ARG; }
    if (max_px != max_px || max_dist != max_dist) { set_error("%s: max_px and max_dist must not be NaN (<= 0 switches them off)", what); return R3D_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(world) % 8 || reinterpret_cast<uintptr_t>(reproj) % 8 || reinterpret_cast<uintptr_t>(emit) % 8 ||
        reinterpret_cast<uintptr_t>(fused) % 8 || reinterpret_cast<uintptr_t>(spread) % 8) {
        set_error("%s: world_dev, reproj_dev, emit_dev, fused_dev and spread_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    // an output extent may not overlap an input extent (address ranges; the sizes fit in 64 bits)
    const uintptr_t sj = (uintptr_t)S * J, gj = (uintptr_t)G * J, gm = (uintptr_t)G * M;
    const char *out_name[4] = {"fused_dev", "spread_dev", "count_dev", "used_dev"};
    const char *in_name[6] = {"world_dev", "reproj_dev", "emit_dev", "status_dev", "synthetic_dev", "member_dev"};
    const uintptr_t outs[4] = {reinterpret_cast<uintptr_t>(fused), reinterpret_cast<uintptr_t>(spread), reinterpret_cast<uintptr_t>(count),
                               reinterpret_cast<uintptr_t>(used)};
    const uintptr_t out_bytes[4] = {gj * 3 * sizeof(double), gj * sizeof(double), gj * sizeof(int32_t), gm * sizeof(uint32_t)};
    const uintptr_t ins[6] = {reinterpret_cast<uintptr_t>(world), reinterpret_cast<uintptr_t>(reproj), reinterpret_cast<uintptr_t>(emit),
                              reinterpret_cast<uintptr_t>(status), reinterpret_cast<uintptr_t>(synthetic), reinterpret_cast<uintptr_t>(member)};
    const uintptr_t in_bytes[6] = {sj * 3 * sizeof(double), sj * sizeof(double), (uintptr_t)S * sizeof(int64_t), (uintptr_t)S * sizeof(int32_t),
                                   (uintptr_t)S * sizeof(uint32_t), gm * sizeof(int32_t)};
    for (int o = 0; o < 4; ++o)
        for (int i = 0; i < 6; ++i)
            if (outs[o] && ins[i] && outs[o] < ins[i] + in_bytes[i] && ins[i] < outs[o] + out_bytes[o]) {
                set_error("%s: %s overlaps %s: the call does not work in place", what, out_name[o], in_name[i]);
                return R3D_ERR_ARG;
            }
    StreamsFuseArgs a = {};
    a.world = world;
    a.reproj = reproj;
    a.emit = reinterpret_cast<const long long *>(emit);
    a.status = status;
    a.synthetic = synthetic;
    a.member = member;
    a.fused = fused;
    a.spread = spread;
    a.count = count;
    a.used = used;
    a.soft_px = soft_px;
    a.max_px = max_px;
    a.max_dist = max_dist;
    a.S = S;
    a.J = J;
    a.G = G;
    a.M = M;
    *args = a;
    return R3D_OK;
}

// the shapes r3d_streams_assign takes: what r3d_streams_assign_bytes and the argument rules share
static bool streams_assign_shape_ok(int32_t C, int32_t P, int32_t J, int32_t width) {
    return C >= 1 && P >= 1 && P <= R3D_ASSIGN_MAX_SLOTS && (long long)C * P <= R3D_CLIPS_MAX && J >= 1 && J <= 17 && (width == 2 || width == 3);
}

// the argument rules of r3d_streams_assign, shared with its host hook; fills the kernel's arguments
int r3d::streams_assign_check_args(const char *what, void *state, const r3d_assign_params *prm, const float *det, const float *det_conf,
                                   const int32_t *det_count, int32_t *action, float *frame_out, float *conf_out, int32_t *match,
                                   int64_t *id, int32_t *stats, StreamsAssignArgs *args) {
    if (!state || !prm || !det || !det_count || !action || !frame_out || !match || !id) {
        set_error("%s: null pointer (assign_dev, prm, det_dev, det_count_dev, action_dev, frame_out_dev, match_dev, id_dev)", what);
        return R3D_ERR_ARG;
    }
    if (prm->struct_size != (int32_t)sizeof(r3d_assign_params)) {
        set_error("%s: prm->struct_size is %d, this library's r3d_assign_params has %d bytes", what, prm->struct_size, (int)sizeof(r3d_assign_params));
        return R3D_ERR_ARG;
    }
    const int32_t C = prm->num_cameras, P = prm->slots, D = prm->max_detections, J = prm->num_joints, width = prm->width;
    if (C < 1) { set_error("%s: num_cameras must be >= 1 (got %d)", what, C); return R3D_ERR_ARG; }
    if (P < 1 || P > R3D_ASSIGN_MAX_SLOTS) { set_error("%s: slots must be in 1..%d (got %d)", what, R3D_ASSIGN_MAX_SLOTS, P); return R3D_ERR_ARG; }
    if (D < 1 || D > R3D_ASSIGN_MAX_DETECTIONS) { set_error("%s: max_detections must be in 1..%d (got %d)", what, R3D_ASSIGN_MAX_DETECTIONS, D); return R3D_ERR_ARG; }
    if ((long long)C * P > R3D_CLIPS_MAX) { set_error("%s: num_cameras * slots must be <= %d (got %d * %d)", what, R3D_CLIPS_MAX, C, P); return R3D_ERR_ARG; }
    if (J < 1 || J > 17) { set_error("%s: num_joints must be in 1..17 (got %d)", what, J); return R3D_ERR_ARG; }
    if (width != 2 && width != 3) { set_error("%s: width must be 2 or 3 (got %d)", what, width); return R3D_ERR_ARG; }
    if (prm->lag < 0) { set_error("%s: lag must be >= 0 (got %d)", what, prm->lag); return R3D_ERR_ARG; }
    if (prm->min_joints < 1 || prm->min_joints > J || prm->min_common < 1 || prm->min_common > J) {
        set_error("%s: min_joints and min_common must be in 1..num_joints = %d (got %d, %d)", what, J, prm->min_joints, prm->min_common);
        return R3D_ERR_ARG;
    }
    if (prm->max_missed < 0) { set_error("%s: max_missed must be >= 0 (got %d)", what, prm->max_missed); return R3D_ERR_ARG; }
    if (prm->fill != R3D_ASSIGN_FILL_NAN && prm->fill != R3D_ASSIGN_FILL_HOLD) { set_error("%s: unknown fill %d", what, prm->fill); return R3D_ERR_ARG; }
    if (!stream_finite_bits(__builtin_bit_cast(uint32_t, prm->min_conf))) { set_error("%s: min_conf must be finite", what); return R3D_ERR_ARG; }
    if (!stream_finite_bits64(prm->max_cost) || !(prm->max_cost > 0.0)) { set_error("%s: max_cost must be finite and > 0", what); return R3D_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(state) % 8 || reinterpret_cast<uintptr_t>(id) % 8) {
        set_error("%s: assign_dev and id_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    // an output extent may not overlap an input extent, the state or another output (address ranges; the sizes fit in 64 bits)
    const uintptr_t S = (uintptr_t)C * P, cdj = (uintptr_t)C * D * J, sj = S * J;
    const char *name[10] = {"action_dev", "frame_out_dev", "conf_out_dev", "match_dev", "id_dev", "stats_dev",
                            "det_dev", "det_conf_dev", "det_count_dev", "assign_dev"};
    const uintptr_t ptr[10] = {reinterpret_cast<uintptr_t>(action), reinterpret_cast<uintptr_t>(frame_out), reinterpret_cast<uintptr_t>(conf_out),
                               reinterpret_cast<uintptr_t>(match), reinterpret_cast<uintptr_t>(id), reinterpret_cast<uintptr_t>(stats),
                               reinterpret_cast<uintptr_t>(det), reinterpret_cast<uintptr_t>(det_conf), reinterpret_cast<uintptr_t>(det_count),
                               reinterpret_cast<uintptr_t>(state)};
    const uintptr_t bytes[10] = {S * sizeof(int32_t), sj * width * sizeof(float), sj * sizeof(float), S * sizeof(int32_t), S * sizeof(int64_t),
                                 (uintptr_t)C * 4 * sizeof(int32_t), cdj * width * sizeof(float), cdj * sizeof(float), (uintptr_t)C * sizeof(int32_t),
                                 (uintptr_t)streams_assign_bytes(C, P, J, width)};
    for (int o = 0; o < 6; ++o)              // (the outputs come first)
        for (int i = o + 1; i < 10; ++i)
            if (ptr[o] && ptr[i] && ptr[o] < ptr[i] + bytes[i] && ptr[i] < ptr[o] + bytes[o]) {
                set_error("%s: %s overlaps %s: the call does not work in place", what, name[o], name[i]);
                return R3D_ERR_ARG;
            }
    StreamsAssignArgs a = {};
    a.state = state;
    a.det = reinterpret_cast<const uint32_t *>(det);
    a.det_conf = det_conf;
    a.det_count = det_count;
    a.action = action;
    a.frame_out = reinterpret_cast<uint32_t *>(frame_out);
    a.conf_out = reinterpret_cast<uint32_t *>(conf_out);
    a.match = match;
    a.id_out = reinterpret_cast<long long *>(id);
    a.stats = stats;
    a.max_cost = prm->max_cost;
    a.min_conf = prm->min_conf;
    a.C = C;
    a.P = P;
    a.D = D;
    a.J = J;
    a.width = width;
    a.lag = prm->lag;
    a.min_joints = prm->min_joints;
    a.min_common = prm->min_common;
    a.max_missed = prm->max_missed;
    a.fill = prm->fill;
    *args = a;
    return R3D_OK;
}

// the shapes r3d_streams_link's state takes: what r3d_streams_link_bytes and the argument rules share
static bool streams_link_shape_ok(int32_t N, int32_t C, int32_t G, int32_t J) {
    return N >= 1 && C >= 1 && C <= R3D_FUSE_MAX_MEMBERS && G >= 1 && G <= R3D_LINK_MAX_PEOPLE && (long long)N * C <= R3D_CLIPS_MAX &&
           (long long)N * G <= R3D_CLIPS_MAX && J >= 1 && J <= 17;
}

// the argument rules of r3d_streams_link, shared with its host hook; fills the kernel's arguments
int r3d::streams_link_check_args(const char *what, void *state, const r3d_link_params *prm, const double *world, const int64_t *emit,
                                 const int32_t *status, const int64_t *id, int32_t *member, int64_t *person, int32_t *group,
                                 int32_t *stats, StreamsLinkArgs *args) {
    if (!state || !prm || !world || !emit || !status || !id || !member || !person) {
        set_error("%s: null pointer (link_dev, prm, world_dev, emit_dev, status_dev, id_dev, member_dev, person_dev)", what);
        return R3D_ERR_ARG;
    }
    if (prm->struct_size != (int32_t)sizeof(r3d_link_params)) {
        set_error("%s: prm->struct_size is %d, this library's r3d_link_params has %d bytes", what, prm->struct_size, (int)sizeof(r3d_link_params));
        return R3D_ERR_ARG;
    }
    const int32_t N = prm->num_scenes, C = prm->num_cameras, P = prm->slots, G = prm->people, M = prm->max_members, J = prm->num_joints;
    if (N < 1) { set_error("%s: num_scenes must be >= 1 (got %d)", what, N); return R3D_ERR_ARG; }
    if (C < 1 || C > R3D_FUSE_MAX_MEMBERS) { set_error("%s: num_cameras must be in 1..%d (got %d)", what, R3D_FUSE_MAX_MEMBERS, C); return R3D_ERR_ARG; }
    if (P < 1 || P > R3D_ASSIGN_MAX_SLOTS) { set_error("%s: slots must be in 1..%d (got %d)", what, R3D_ASSIGN_MAX_SLOTS, P); return R3D_ERR_ARG; }
    if (G < 1 || G > R3D_LINK_MAX_PEOPLE) { set_error("%s: people must be in 1..%d (got %d)", what, R3D_LINK_MAX_PEOPLE, G); return R3D_ERR_ARG; }
    if (J < 1 || J > 17) { set_error("%s: num_joints must be in 1..17 (got %d)", what, J); return R3D_ERR_ARG; }
    if (M < C || M > R3D_FUSE_MAX_MEMBERS) { set_error("%s: max_members must be in num_cameras..%d (got %d)", what, R3D_FUSE_MAX_MEMBERS, M); return R3D_ERR_ARG; }
    if ((long long)N * C * P > R3D_CLIPS_MAX || (long long)N * G > R3D_CLIPS_MAX) {
        set_error("%s: num_scenes * num_cameras * slots and num_scenes * people must be <= %d (got %d * %d * %d, %d * %d)", what, R3D_CLIPS_MAX, N, C, P, N, G);
        return R3D_ERR_ARG;
    }
    if (prm->min_joints < 1 || prm->min_joints > J || prm->min_common < 1 || prm->min_common > J) {
        set_error("%s: min_joints and min_common must be in 1..num_joints = %d (got %d, %d)", what, J, prm->min_joints, prm->min_common);
        return R3D_ERR_ARG;
    }
    if (prm->max_missed < 0) { set_error("%s: max_missed must be >= 0 (got %d)", what, prm->max_missed); return R3D_ERR_ARG; }
    if (!stream_finite_bits64(prm->max_dist) || !(prm->max_dist > 0.0)) { set_error("%s: max_dist must be finite and > 0", what); return R3D_ERR_ARG; }
    if (prm->break_dist != prm->break_dist || (prm->break_dist > 0.0 && (!stream_finite_bits64(prm->break_dist) || prm->break_dist < prm->max_dist))) {
        set_error("%s: break_dist must be <= 0 (off) or finite and >= max_dist", what);
        return R3D_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(state) % 8 || reinterpret_cast<uintptr_t>(world) % 8 || reinterpret_cast<uintptr_t>(emit) % 8 ||
        reinterpret_cast<uintptr_t>(id) % 8 || reinterpret_cast<uintptr_t>(person) % 8) {
        set_error("%s: link_dev, world_dev, emit_dev, id_dev and person_dev must be 8-byte aligned", what);
        return R3D_ERR_ARG;
    }
    // an output extent may not overlap an input extent, the state or another output (address ranges; the sizes fit in 64 bits)
    const uintptr_t S = (uintptr_t)N * C * P, NG = (uintptr_t)N * G;
    const char *name[9] = {"member_dev", "person_dev", "group_dev", "stats_dev", "world_dev", "emit_dev", "status_dev", "id_dev", "link_dev"};
    const uintptr_t ptr[9] = {reinterpret_cast<uintptr_t>(member), reinterpret_cast<uintptr_t>(person), reinterpret_cast<uintptr_t>(group),
                              reinterpret_cast<uintptr_t>(stats), reinterpret_cast<uintptr_t>(world), reinterpret_cast<uintptr_t>(emit),
                              reinterpret_cast<uintptr_t>(status), reinterpret_cast<uintptr_t>(id), reinterpret_cast<uintptr_t>(state)};
    const uintptr_t bytes[9] = {NG * M * sizeof(int32_t), NG * sizeof(int64_t), S * sizeof(int32_t), (uintptr_t)N * 4 * sizeof(int32_t),
                                S * J * 3 * sizeof(double), S * sizeof(int64_t), S * sizeof(int32_t), S * sizeof(int64_t),
                                (uintptr_t)streams_link_bytes(N, C, G, J)};
    for (int o = 0; o < 4; ++o)              // (the outputs come first)
        for (int i = o + 1; i < 9; ++i)
            if (ptr[o] && ptr[i] && ptr[o] < ptr[i] + bytes[i] && ptr[i] < ptr[o] + bytes[o]) {
                set_error("%s: %s overlaps %s: the call does not work in place", what, name[o], name[i]);
                return R3D_ERR_ARG;
            }
    StreamsLinkArgs a = {};
    a.state = state;
    a.world = world;
    a.emit = reinterpret_cast<const long long *>(emit);
    a.status = status;
    a.id = reinterpret_cast<const long long *>(id);
    a.member = member;
    a.person = reinterpret_cast<long long *>(person);
    a.group = group;
    a.stats = stats;
    a.max_dist = prm->max_dist;
    a.break_dist = prm->break_dist;
    a.N = N;
    a.C = C;
    a.P = P;
    a.G = G;
    a.M = M;
    a.J = J;
    a.min_joints = prm->min_joints;
    a.min_common = prm->min_common;
    a.max_missed = prm->max_missed;
    *args = a;
    return R3D_OK;
}

extern "C" {

int r3d_create(const r3d_config *cfg, r3d_model **out) {
    if (!cfg || !out) { set_error("r3d_create: null argument"); return R3D_ERR_ARG; }
    if (cfg->struct_size != (int32_t)sizeof(r3d_config)) {
        set_error("r3d_create: r3d_config.struct_size is %d, this library's r3d_config has %d bytes (ABI version %d): the "
                  "binding was written against another include/ray3d_hip.h", cfg->struct_size, (int)sizeof(r3d_config), R3D_ABI_VERSION);
        return R3D_ERR_ARG;
    }
    Model *m = model_create(*cfg);
    if (!m) return R3D_ERR_ARG;
    *out = reinterpret_cast<r3d_model *>(m);
    return R3D_OK;
}

int r3d_destroy(r3d_model *m) {
    delete reinterpret_cast<Model *>(m);
    return R3D_OK;
}

int r3d_num_weights(const r3d_model *m) {
    return m ? (int)reinterpret_cast<const Model *>(m)->specs.size() : R3D_ERR_ARG;
}

const char *r3d_weight_key(const r3d_model *m, int index) {
    const Model *mm = reinterpret_cast<const Model *>(m);
    if (!mm || index < 0 || index >= (int)mm->specs.size()) return nullptr;
    return mm->specs[index].key.c_str();
}

int r3d_weight_shape(const r3d_model *m, int index, int64_t shape[4], int *rank) {
    const Model *mm = reinterpret_cast<const Model *>(m);
    if (!mm || !shape || !rank || index < 0 || index >= (int)mm->specs.size()) { set_error("r3d_weight_shape: bad argument"); return R3D_ERR_ARG; }
    *rank = mm->specs[index].rank;
    for (int i = 0; i < 4; ++i) shape[i] = mm->specs[index].shape[i];
    return R3D_OK;
}

int r3d_set_weight(r3d_model *m, const char *key, const float *host, const int64_t *shape, int rank) {
    return model_set_weight(reinterpret_cast<Model *>(m), key, host, shape, rank);
}

int r3d_finalize(r3d_model *m) { return model_finalize(reinterpret_cast<Model *>(m)); }

int r3d_finalize_dev(r3d_model *m, const float *const *weights_dev, const int64_t *numel, int32_t count, void *hip_stream) {
    return model_finalize_dev(reinterpret_cast<Model *>(m), weights_dev, numel, count, hip_stream);
}

size_t r3d_workspace_bytes(const r3d_model *pos, const r3d_model *trj, int64_t B) {
    const auto [a, b] = model_pair(pos, trj);
    if (!a || B <= 0) return 0;
    return workspace_bytes_pair(a, b, B);
}

size_t r3d_input_workspace_bytes(const r3d_model *pos, const r3d_model *trj, const r3d_input *in, int64_t B) {
    const auto [a, b] = model_pair(pos, trj);
    if (!a || !in || B <= 0) { set_error("r3d_input_workspace_bytes: no model, no input or B <= 0"); return 0; }
    switch (in->mode) {
        case R3D_INPUT_RAYS:
        case R3D_INPUT_UV: return workspace_bytes_pair(a, b, B);
        case R3D_INPUT_UV_DIST:
        case R3D_INPUT_PX_INTRINSIC:
        case R3D_INPUT_PX_SCREEN:
            if (dist_check(a, in, false) != R3D_OK) return 0;
            return (workspace_bytes_pair(a, b, B) + 255) / 256 * 256 + dist_ray_bytes(a, in, B);
        default: set_error("r3d_input_workspace_bytes: bad input mode %d", in->mode); return 0;
    }
}

int r3d_prepare(r3d_model *pos, r3d_model *trj, int64_t B) {
    const auto [a, b] = model_pair(pos, trj);
    if (!a || B <= 0) { set_error("r3d_prepare: no model given or B <= 0"); return R3D_ERR_ARG; }
    for (Model *m : {a, b})
        if (m && (!m->finalized || m->dirty)) { set_error("r3d_prepare called before r3d_finalize (or weights changed since)"); return R3D_ERR_STATE; }
    if (b && !same_input_shape(a, b)) { set_error("pos and trj models disagree on J / F / levels / extrinsic_dim"); return R3D_ERR_ARG; }
    const FwdKeys keys = forward_keys(a, b);
    for (int k = 0; k < keys.nlanes; ++k)  // (R3D_OPT_LANES: every lane's schedule of this size)
        if (!schedule_get(plan_get(a, b, plan_kind(B)), B, keys.nwg, /*pin=*/true, keys.lane_key0 + k)) return R3D_ERR_HIP;
    return R3D_OK;
}

int r3d_release(r3d_model *pos, r3d_model *trj, int64_t B) {
    const auto [a, b] = model_pair(pos, trj);
    if (!a || B <= 0) { set_error("r3d_release: no model given or B <= 0"); return R3D_ERR_ARG; }
    Plan *pl = plan_get(a, b, plan_kind(B));
    bool any = false;
    for (int k = 0; k <= 4; ++k) {         // (the handle without lanes: key 0; lane k: key k + 1)
        auto it = pl->schedules.find(schedule_key(B, k));
        if (it != pl->schedules.end() && it->second->pinned) { it->second->pinned = false; any = true; }
    }
    if (!any) { set_error("r3d_release: %lld windows were never prepared for this pair", (long long)B); return R3D_ERR_ARG; }
    return R3D_OK;
}

int r3d_forward(r3d_model *m, const r3d_input *in, int64_t B, float *out_dev, void *ws, size_t ws_bytes, void *stream) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm) { set_error("r3d_forward: null model"); return R3D_ERR_ARG; }
    return forward_run(mm, nullptr, in, B, out_dev, nullptr, ws, ws_bytes, stream);
}

int r3d_forward_pair(r3d_model *pos, r3d_model *trj, const r3d_input *in, int64_t B, float *out_dev, float *out_trj_dev,
                     void *ws, size_t ws_bytes, void *stream) {
    Model *p = reinterpret_cast<Model *>(pos), *t = reinterpret_cast<Model *>(trj);
    if (!p || !t) { set_error("r3d_forward_pair: both models are required"); return R3D_ERR_ARG; }
    if (p->cfg.kind != R3D_KIND_POS || t->cfg.kind != R3D_KIND_TRJ) { set_error("r3d_forward_pair: (pos, trj) expected in that order"); return R3D_ERR_ARG; }
    return forward_run(p, t, in, B, out_dev, out_trj_dev, ws, ws_bytes, stream);
}

int r3d_forward_pair_split(r3d_model *pos, r3d_model *trj, const r3d_input *in, int64_t B, float *out_pos_dev, float *out_trj_dev,
                           void *ws, size_t ws_bytes, void *stream) {
    Model *p = reinterpret_cast<Model *>(pos), *t = reinterpret_cast<Model *>(trj);
    if (!p || !t) { set_error("r3d_forward_pair_split: both models are required"); return R3D_ERR_ARG; }
    if (!out_pos_dev || !out_trj_dev) { set_error("r3d_forward_pair_split: both outputs are required"); return R3D_ERR_ARG; }
    if (p->cfg.kind != R3D_KIND_POS || t->cfg.kind != R3D_KIND_TRJ) { set_error("r3d_forward_pair_split: (pos, trj) expected in that order"); return R3D_ERR_ARG; }
    return forward_run(p, t, in, B, out_pos_dev, out_trj_dev, ws, ws_bytes, stream, /*split=*/true);
}

int r3d_profile_enable(r3d_model *m, int on) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm) { set_error("r3d_profile_enable: null model"); return R3D_ERR_ARG; }
    mm->profiling = on != 0;
    mm->nrec = 0;
    return R3D_OK;
}

int r3d_profile_read(r3d_model *m, r3d_launch_record *records, int capacity) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm) { set_error("r3d_profile_read: null model"); return R3D_ERR_ARG; }
    int n = 0;
    for (int i = 0; i < mm->nrec; ++i) {
        Model::Rec &r = mm->recs[i];
        hipError_t e = hipEventSynchronize(r.e1);
        if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
        if ((e = hipEventElapsedTime(&r.r.ms, r.e0, r.e1)) != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
        if (records && n < capacity) records[n] = r.r;
        ++n;
    }
    return n;
}

int r3d_clip_valid_losses(const float *pos_dev, const float *trj_dev, const float *gt_dev, int64_t n_frames,
                          int32_t num_joints, const int32_t *parents, int32_t flags,
                          double *out_dev, double *frame_dev, void *stream) {
    const int rc = valid_check_args("r3d_clip_valid_losses", pos_dev, trj_dev, gt_dev, n_frames, num_joints, parents, flags, out_dev);
    if (rc != R3D_OK) return rc;
    if (r3d::launch_clip_valid(pos_dev, trj_dev, gt_dev, n_frames, num_joints, parents, flags, out_dev, frame_dev, (hipStream_t)stream)) {
        r3d::set_error("r3d_clip_valid_losses: launch failed: %s", hipGetErrorString(hipGetLastError()));
        return R3D_ERR_HIP;
    }
    return 0;
}

size_t r3d_clips_valid_scratch_bytes(int32_t num_clips, int64_t max_frames) {
    if (num_clips < 1 || max_frames < 1) return 0;
    return r3d::clips_valid_scratch_bytes(num_clips, max_frames);
}

int r3d_clips_valid_losses(const float *pos_dev, const float *trj_dev, const float *gt_dev, int64_t total_frames, int32_t num_joints,
                           const int32_t *parents, int32_t flags, const r3d_clip_desc *clips_dev, int32_t num_clips, int64_t max_frames,
                           double *rows_dev, int64_t row_stride, double *frame_dev, void *scratch_dev, size_t scratch_bytes, void *stream) {
    // (every check on the host, before any HIP call)
    const int rc = clips_valid_check_args("r3d_clips_valid_losses", pos_dev, trj_dev, gt_dev, total_frames, num_joints, parents, flags,
                                          clips_dev, num_clips, max_frames, rows_dev, row_stride, scratch_dev, true);
    if (rc != R3D_OK) return rc;
    const size_t need = r3d::clips_valid_scratch_bytes(num_clips, max_frames);
    if (scratch_bytes < need) {
        r3d::set_error("r3d_clips_valid_losses: scratch of %zu bytes, %zu needed (r3d_clips_valid_scratch_bytes)", scratch_bytes, need);
        return R3D_ERR_WORKSPACE;
    }
    if (r3d::launch_clips_valid(pos_dev, trj_dev, gt_dev, total_frames, num_joints, parents, flags, clips_dev, num_clips, max_frames,
                                rows_dev, row_stride, frame_dev, scratch_dev, (hipStream_t)stream)) {
        r3d::set_error("r3d_clips_valid_losses: launch failed: %s", hipGetErrorString(hipGetLastError()));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_clip_metrics(const float *pred_dev, const float *gt_dev, int64_t n_frames, int32_t num_joints,
                     const double *rn2w, const double *tn2w, double *out_dev, void *stream) {
    if (!pred_dev || !gt_dev || !rn2w || !tn2w || !out_dev) { r3d::set_error("r3d_clip_metrics: null pointer"); return R3D_ERR_ARG; }
    if (n_frames < 1) { r3d::set_error("r3d_clip_metrics: n_frames must be >= 1 (got %lld)", (long long)n_frames); return R3D_ERR_ARG; }
    if (num_joints < 1 || num_joints > 17) { r3d::set_error("r3d_clip_metrics: num_joints must be in 1..17 (got %d)", num_joints); return R3D_ERR_ARG; }
    if (r3d::launch_clip_metrics(pred_dev, gt_dev, n_frames, num_joints, rn2w, tn2w, out_dev, nullptr, nullptr, (hipStream_t)stream)) {
        r3d::set_error("r3d_clip_metrics: launch failed: %s", hipGetErrorString(hipGetLastError()));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_clip_metrics_detail(const float *pred_dev, const float *gt_dev, int64_t n_frames, int32_t num_joints,
                            const double *rn2w, const double *tn2w, double *out_dev, double *frame_dev, double *detail_dev,
                            void *stream) {
    if (!pred_dev || !gt_dev || !rn2w || !tn2w || !out_dev || !detail_dev) { r3d::set_error("r3d_clip_metrics_detail: null pointer"); return R3D_ERR_ARG; }
    if (n_frames < 1) { r3d::set_error("r3d_clip_metrics_detail: n_frames must be >= 1 (got %lld)", (long long)n_frames); return R3D_ERR_ARG; }
    if (num_joints < 1 || num_joints > 17) { r3d::set_error("r3d_clip_metrics_detail: num_joints must be in 1..17 (got %d)", num_joints); return R3D_ERR_ARG; }
    if (r3d::launch_clip_metrics(pred_dev, gt_dev, n_frames, num_joints, rn2w, tn2w, out_dev, frame_dev, detail_dev, (hipStream_t)stream)) {
        r3d::set_error("r3d_clip_metrics_detail: launch failed: %s", hipGetErrorString(hipGetLastError()));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_clips_encode(const float *px_dev, int64_t total_frames, int32_t num_joints, int32_t encoding,
                     const r3d_clip_input_desc *clips_dev, int32_t num_clips, int64_t max_rows, float *x_dev, int64_t out_rows,
                     float *x_mirror_dev, const int32_t *mirror_perm, int32_t *status_dev, void *stream) {
    // (every check on the host, before any HIP call)
    const int rc = clips_encode_check_args("r3d_clips_encode", px_dev, total_frames, num_joints, encoding, clips_dev, num_clips, max_rows,
                                           x_dev, out_rows, x_mirror_dev, mirror_perm, status_dev);
    if (rc != R3D_OK) return rc;
    r3d::ClipsEncArgs a = {};
    a.table = clips_dev;
    a.px = px_dev;
    a.x = x_dev;
    a.x_mirror = x_mirror_dev;
    a.status = status_dev;
    a.total_frames = total_frames;
    a.out_rows = out_rows;
    a.max_rows = max_rows;
    if (mirror_perm) r3d::mirror_pack_inverse(mirror_perm, num_joints, a.mirror_inv);
    a.J = num_joints;
    a.encoding = encoding;
    const hipError_t err = r3d::launch_clips_encode(a, num_clips, (hipStream_t)stream);   // (the launcher consumed the error: print what it returned)
    if (err != hipSuccess) {
        set_error("r3d_clips_encode: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_clips_repair(float *x_dev, int64_t out_rows, int32_t num_joints, int32_t in_features, float *x_mirror_dev, const int32_t *mirror_perm,
                     const r3d_clip_input_desc *clips_dev, int32_t num_clips, int64_t max_rows, const float *conf_dev, int64_t total_frames,
                     float min_conf, int32_t max_gap, uint8_t *state_dev, int32_t *stats_dev, int32_t *status_dev, void *stream) {
    // (every check on the host, before any HIP call)
    r3d::ClipsRepairArgs a;
    const int rc = clips_repair_check_args("r3d_clips_repair", x_dev, out_rows, num_joints, in_features, x_mirror_dev, mirror_perm, clips_dev,
                                           num_clips, max_rows, conf_dev, total_frames, min_conf, max_gap, state_dev, stats_dev, status_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_clips_repair(a, num_clips, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_clips_repair: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_clips_poses(const float *raw_dev, const float *raw_mirror_dev, int64_t raw_rows, int32_t num_joints, const int32_t *mirror_perm,
                    const r3d_clip_desc *clips_dev, const int64_t *raw_first_dev, int32_t num_clips, int64_t max_frames,
                    float *pred_dev, double *world_dev, int64_t total_frames, int32_t *status_dev, void *stream) {
    // (every check on the host, before any HIP call)
    const int rc = clips_poses_check_args("r3d_clips_poses", raw_dev, raw_mirror_dev, raw_rows, num_joints, mirror_perm, clips_dev,
                                          raw_first_dev, num_clips, max_frames, pred_dev, world_dev, total_frames, status_dev);
    if (rc != R3D_OK) return rc;
    r3d::ClipsPosesArgs a = {};
    a.table = clips_dev;
    a.raw_first = reinterpret_cast<const long long *>(raw_first_dev);
    a.raw = raw_dev;
    a.raw_mirror = raw_mirror_dev;
    a.pred = pred_dev;
    a.world = world_dev;
    a.status = status_dev;
    a.raw_rows = raw_rows;
    a.total_frames = total_frames;
    a.max_frames = max_frames;
    if (mirror_perm) r3d::pose_pack_perm(mirror_perm, num_joints, a.mirror_perm);
    a.J = num_joints;
    const hipError_t err = r3d::launch_clips_poses(a, num_clips, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_clips_poses: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_clips_project(const float *world_dev, int64_t total_frames, int32_t num_joints, int32_t encoding,
                      const r3d_clip_project_desc *clips_dev, int32_t num_clips, int64_t max_rows, float *x_dev, int64_t out_rows,
                      float *x_mirror_dev, const int32_t *mirror_perm, float *gt_dev, double *px_dev, int64_t gt_rows,
                      int32_t *outside_dev, int32_t *status_dev, void *stream) {
    // (every check on the host, before any HIP call)
    const int rc = clips_project_check_args("r3d_clips_project", world_dev, total_frames, num_joints, encoding, clips_dev, num_clips,
                                            max_rows, x_dev, out_rows, x_mirror_dev, mirror_perm, gt_dev, px_dev, gt_rows, status_dev);
    if (rc != R3D_OK) return rc;
    r3d::ClipsProjectArgs a = {};
    a.table = clips_dev;
    a.world = world_dev;
    a.x = x_dev;
    a.x_mirror = x_mirror_dev;
    a.gt = gt_dev;
    a.px = px_dev;
    a.outside = outside_dev;
    a.status = status_dev;
    a.total_frames = total_frames;
    a.out_rows = out_rows;
    a.max_rows = max_rows;
    a.gt_rows = gt_rows;
    if (mirror_perm) r3d::mirror_pack_inverse(mirror_perm, num_joints, a.mirror_inv);
    a.J = num_joints;
    a.encoding = encoding;
    const hipError_t err = r3d::launch_clips_project(a, num_clips, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_clips_project: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_clips_windows(const float *src_dev, int64_t total_frames, int32_t num_joints, int32_t in_features, int32_t receptive_field,
                      const r3d_window_run_desc *runs_dev, int32_t num_runs, const float *run_param_dev, int32_t extrinsic_dim,
                      int64_t window0, int64_t batch, float *x_dev, float *param_dev, const int32_t *mirror_perm, int32_t *status_dev,
                      void *stream) {
    // (every check on the host, before any HIP call)
    r3d::WindowsArgs a;
    const int rc = clips_windows_check_args("r3d_clips_windows", src_dev, total_frames, num_joints, in_features, receptive_field, runs_dev,
                                            num_runs, run_param_dev, extrinsic_dim, window0, batch, x_dev, param_dev, mirror_perm, status_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_clips_windows(a, (int)batch, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_clips_windows: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

size_t r3d_streams_state_bytes(int32_t num_streams, int32_t receptive_field, int32_t num_joints, int32_t in_features) {
    if (!streams_shape_ok(num_streams, receptive_field, num_joints, in_features)) return 0;
    return r3d::streams_state_bytes(num_streams, receptive_field, num_joints, in_features);
}

int r3d_streams_step(void *state_dev, int32_t num_streams, int32_t receptive_field, int32_t lag, int32_t num_joints, int32_t in_features,
                     int32_t encoding, const float *frame_dev, const double *cam_dev, const int32_t *action_dev, float *x_dev,
                     float *x_mirror_dev, const int32_t *mirror_perm, int64_t *emit_dev, int32_t *status_dev, void *stream) {
    // (every check on the host, before any HIP call)
    r3d::StreamsArgs a;
    const int rc = streams_check_args("r3d_streams_step", state_dev, num_streams, receptive_field, lag, num_joints, in_features, encoding,
                                      frame_dev, cam_dev, action_dev, x_dev, x_mirror_dev, mirror_perm, emit_dev, status_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_streams_step(a, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_streams_step: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_streams_poses(const float *raw_dev, const float *raw_mirror_dev, int32_t num_streams, int32_t num_joints, const int32_t *mirror_perm,
                      const int64_t *emit_dev, const int32_t *status_dev, const r3d_stream_pose_desc *desc_dev, const double *cam_dev,
                      const float *x_dev, int32_t receptive_field, int32_t lag, float *pred_dev, double *world_dev, double *reproj_dev,
                      double *quality_dev, void *stream) {
    // (every check on the host, before any HIP call)
    r3d::StreamsPosesArgs a;
    const int rc = streams_poses_check_args("r3d_streams_poses", raw_dev, raw_mirror_dev, num_streams, num_joints, mirror_perm, emit_dev,
                                            status_dev, desc_dev, cam_dev, x_dev, receptive_field, lag, pred_dev, world_dev, reproj_dev,
                                            quality_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_streams_poses(a, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_streams_poses: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

size_t r3d_streams_track_bytes(int32_t num_streams, int32_t receptive_field, int32_t num_joints, int32_t width) {
    if (!streams_shape_ok(num_streams, receptive_field, num_joints, width)) return 0;
    return r3d::streams_track_bytes(num_streams, receptive_field, num_joints, width);
}

int r3d_streams_repair(void *state_dev, void *track_dev, int32_t num_streams, int32_t receptive_field, int32_t lag, int32_t num_joints,
                       int32_t in_features, int32_t encoding, const float *frame_dev, const float *conf_dev, float min_conf,
                       const double *cam_dev, const int32_t *action_dev, int32_t max_gap, float *frame_out_dev, uint32_t *synthetic_dev,
                       void *stream) {
    // (every check on the host, before any HIP call)
    r3d::StreamsRepairArgs a;
    const int rc = streams_repair_check_args("r3d_streams_repair", state_dev, track_dev, num_streams, receptive_field, lag, num_joints,
                                             in_features, encoding, frame_dev, conf_dev, min_conf, cam_dev, action_dev, max_gap,
                                             frame_out_dev, synthetic_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_streams_repair(a, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_streams_repair: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_streams_peek(const void *state_dev, int32_t num_streams, int32_t receptive_field, int32_t lag, int32_t num_joints,
                     int32_t in_features, const int32_t *looks, int32_t num_looks, const int32_t *action_dev, const int32_t *status_dev,
                     float *x_dev, float *x_mirror_dev, const int32_t *mirror_perm, int64_t *emit_dev, int32_t *peek_status_dev,
                     void *stream) {
    // (every check on the host, before any HIP call)
    r3d::StreamsPeekArgs a;
    const int rc = streams_peek_check_args("r3d_streams_peek", state_dev, num_streams, receptive_field, lag, num_joints, in_features, looks,
                                           num_looks, action_dev, status_dev, x_dev, x_mirror_dev, mirror_perm, emit_dev, peek_status_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_streams_peek(a, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_streams_peek: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_streams_fuse(const double *world_dev, const double *reproj_dev, const int64_t *emit_dev, const int32_t *status_dev,
                     const uint32_t *synthetic_dev, int32_t num_streams, int32_t num_joints, const int32_t *member_dev, int32_t num_groups,
                     int32_t max_members, double soft_px, double max_px, double max_dist, double *fused_dev, double *spread_dev,
                     int32_t *count_dev, uint32_t *used_dev, void *stream) {
    // (every check on the host, before any HIP call)
    r3d::StreamsFuseArgs a;
    const int rc = streams_fuse_check_args("r3d_streams_fuse", world_dev, reproj_dev, emit_dev, status_dev, synthetic_dev, num_streams,
                                           num_joints, member_dev, num_groups, max_members, soft_px, max_px, max_dist, fused_dev,
                                           spread_dev, count_dev, used_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_streams_fuse(a, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_streams_fuse: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

size_t r3d_streams_assign_bytes(int32_t num_cameras, int32_t slots, int32_t num_joints, int32_t width) {
    if (!streams_assign_shape_ok(num_cameras, slots, num_joints, width)) return 0;
    return r3d::streams_assign_bytes(num_cameras, slots, num_joints, width);
}

int r3d_streams_assign(void *assign_dev, const r3d_assign_params *prm, const float *det_dev, const float *det_conf_dev,
                       const int32_t *det_count_dev, int32_t *action_dev, float *frame_out_dev, float *conf_out_dev, int32_t *match_dev,
                       int64_t *id_dev, int32_t *stats_dev, void *stream) {
    // (every check on the host, before any HIP call)
    r3d::StreamsAssignArgs a;
    const int rc = streams_assign_check_args("r3d_streams_assign", assign_dev, prm, det_dev, det_conf_dev, det_count_dev, action_dev,
                                             frame_out_dev, conf_out_dev, match_dev, id_dev, stats_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_streams_assign(a, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_streams_assign: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

size_t r3d_streams_link_bytes(int32_t num_scenes, int32_t num_cameras, int32_t people, int32_t num_joints) {
    if (!streams_link_shape_ok(num_scenes, num_cameras, people, num_joints)) return 0;
    return r3d::streams_link_bytes(num_scenes, num_cameras, people, num_joints);
}

int r3d_streams_link(void *link_dev, const r3d_link_params *prm, const double *world_dev, const int64_t *emit_dev, const int32_t *status_dev,
                     const int64_t *id_dev, int32_t *member_dev, int64_t *person_dev, int32_t *group_dev, int32_t *stats_dev, void *stream) {
    // (every check on the host, before any HIP call)
    r3d::StreamsLinkArgs a;
    const int rc = streams_link_check_args("r3d_streams_link", link_dev, prm, world_dev, emit_dev, status_dev, id_dev, member_dev, person_dev,
                                           group_dev, stats_dev, &a);
    if (rc != R3D_OK) return rc;
    const hipError_t err = r3d::launch_streams_link(a, (hipStream_t)stream);
    if (err != hipSuccess) {
        set_error("r3d_streams_link: launch failed: %s", hipGetErrorString(err));
        return R3D_ERR_HIP;
    }
    return 0;
}

size_t r3d_clips_metrics_scratch_bytes(int32_t num_clips, int64_t max_frames, int detail) {
    if (num_clips < 1 || max_frames < 1) return 0;
    return r3d::clips_metrics_scratch_bytes(num_clips, max_frames, detail != 0);
}

int r3d_clips_metrics(const float *pred_dev, const float *gt_dev, int64_t total_frames, int32_t num_joints,
                      const r3d_clip_desc *clips_dev, int32_t num_clips, int64_t max_frames, double *rows_dev, int64_t row_stride,
                      double *detail_dev, int64_t detail_stride, double *frame_dev, void *scratch_dev, size_t scratch_bytes, void *stream) {
    const int rc = clips_metrics_check_args("r3d_clips_metrics", pred_dev, gt_dev, total_frames, num_joints, clips_dev, num_clips, max_frames,
                                            rows_dev, row_stride, detail_dev, detail_stride, scratch_dev);
    if (rc != R3D_OK) return rc;
    const size_t need = r3d::clips_metrics_scratch_bytes(num_clips, max_frames, detail_dev != nullptr);
    if (scratch_bytes < need) {
        r3d::set_error("r3d_clips_metrics: scratch of %zu bytes, %zu needed (r3d_clips_metrics_scratch_bytes)", scratch_bytes, need);
        return R3D_ERR_WORKSPACE;
    }
    if (r3d::launch_clips_metrics(pred_dev, gt_dev, total_frames, num_joints, clips_dev, num_clips, max_frames, rows_dev, row_stride,
                                  detail_dev, detail_stride, frame_dev, scratch_dev, (hipStream_t)stream)) {
        r3d::set_error("r3d_clips_metrics: launch failed: %s", hipGetErrorString(hipGetLastError()));
        return R3D_ERR_HIP;
    }
    return 0;
}

int r3d_set_option(r3d_model *m, int32_t option, int64_t value) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm) { r3d::set_error("r3d_set_option: null model"); return R3D_ERR_ARG; }
    switch (option) {
        case R3D_OPT_STAGED: mm->opt_staged = value != 0; return R3D_OK;
        case R3D_OPT_SPIN_TIMEOUT_MS:
            if (value < 1 || value > 600000) { r3d::set_error("r3d_set_option: spin timeout must be 1 .. 600000 ms (got %lld)", (long long)value); return R3D_ERR_ARG; }
            mm->spin_timeout_ms = (int)value;
            return R3D_OK;
        case R3D_OPT_CU_LIMIT:
            if (value < 0 || value > 4096) { r3d::set_error("r3d_set_option: CU limit must be 0 .. 4096 (got %lld)", (long long)value); return R3D_ERR_ARG; }
            if (mm->cu_limit != (int)value) {
                // The cached schedules were packed for another workgroup count: they are dropped - which must not happen under a
                // captured graph (r3d_prepare pins the schedules a graph's kernels point into) or while a capture is being recorded.
                if (r3d::plans_pinned(mm)) {
                    r3d::set_error("r3d_set_option(R3D_OPT_CU_LIMIT): the handle has prepared (pinned) schedules - r3d_release them first; "
                                   "a captured hipGraph would be left with dangling tile lists");
                    return R3D_ERR_STATE;
                }
                // ... and their launches may still be in flight on the handle's device
                int cur = 0;
                const bool have_dev = mm->device >= 0 && hipGetDevice(&cur) == hipSuccess;
                if (have_dev && cur != mm->device) (void)hipSetDevice(mm->device);
                if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
                if (have_dev && cur != mm->device) (void)hipSetDevice(cur);
                r3d::plans_drop(mm);
                mm->cu_limit = (int)value;
                mm->last_fwd_stream = nullptr;
            }
            return R3D_OK;
        case R3D_OPT_LANES: {
            if (value != 0 && value != 1 && value != 2 && value != 4) { r3d::set_error("r3d_set_option: R3D_OPT_LANES is 0, 1, 2 or 4 (got %lld)", (long long)value); return R3D_ERR_ARG; }
            const int n = value <= 1 ? 0 : (int)value;
            if (n == mm->lanes) return R3D_OK;
            if (!mm->finalized) { r3d::set_error("r3d_set_option(R3D_OPT_LANES): r3d_finalize the handle first (the lanes live on its device)"); return R3D_ERR_STATE; }
            if (r3d::plans_pinned(mm)) {
                r3d::set_error("r3d_set_option(R3D_OPT_LANES): the handle has prepared (pinned) schedules - r3d_release them first");
                return R3D_ERR_STATE;
            }
            int cur = 0;
            const bool have_dev = mm->device >= 0 && hipGetDevice(&cur) == hipSuccess;
            if (have_dev && cur != mm->device) (void)hipSetDevice(mm->device);
            if (hipDeviceSynchronize() != hipSuccess) (void)hipGetLastError();
            r3d::plans_drop(mm);
            r3d::lanes_destroy(mm);
            mm->lanes = 0;
            int rc = R3D_OK;
            if (n > 1 && (rc = r3d::lanes_create(mm, n)) == R3D_OK) mm->lanes = n;
            if (rc != R3D_OK) r3d::lanes_destroy(mm);
            if (have_dev && cur != mm->device) (void)hipSetDevice(cur);
            return rc;
        }
        default: r3d::set_error("r3d_set_option: unknown option %d", option); return R3D_ERR_ARG;
    }
}

int r3d_lane_stream(r3d_model *m, int32_t lane, void **stream) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm || !stream) { r3d::set_error("r3d_lane_stream: null argument"); return R3D_ERR_ARG; }
    if (lane < 0 || lane >= mm->lanes) { r3d::set_error("r3d_lane_stream: lane %d of %d", lane, mm->lanes); return R3D_ERR_ARG; }
    *stream = mm->lane[lane].stream;
    return R3D_OK;
}

int r3d_lanes_join(r3d_model *m, void *stream) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm) { r3d::set_error("r3d_lanes_join: null model"); return R3D_ERR_ARG; }
    for (int k = 0; k < mm->lanes; ++k) {
        r3d::Model::Lane &ln = mm->lane[k];
        if (ln.waiters.empty()) continue;
        // (every lane somebody still has to join: `stream` waits for more than its own forwards at most - never for less)
        hipError_t e = hipStreamWaitEvent((hipStream_t)stream, ln.done, 0);
        if (e != hipSuccess) return r3d::hip_fail(e, "hipStreamWaitEvent(lane)");
        ln.waiters.erase(std::remove(ln.waiters.begin(), ln.waiters.end(), stream), ln.waiters.end());
    }
    return R3D_OK;
}

int r3d_last_clock(r3d_model *m, void *stream, double *ghz) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm || !ghz) { r3d::set_error("r3d_last_clock: null argument"); return R3D_ERR_ARG; }
    *ghz = 0.0;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return r3d::hip_fail(e, "hipStreamSynchronize");
    if (!mm->last_clk_dev) return R3D_OK;
    unsigned w[2] = {0u, 0u};
    if ((e = hipMemcpy(w, mm->last_clk_dev, sizeof w, hipMemcpyDeviceToHost)) != hipSuccess) return r3d::hip_fail(e, "hipMemcpy(clock stamp)");
    if (w[1] > 0u) *ghz = (double)w[0] / ((double)w[1] * 10.0);      // cycles per 10 ns tick
    return R3D_OK;
}

int r3d_status(r3d_model *m, void *stream) {
    Model *mm = reinterpret_cast<Model *>(m);
    if (!mm) { r3d::set_error("r3d_status: null model"); return R3D_ERR_ARG; }
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return r3d::hip_fail(e, "hipStreamSynchronize");
    for (int k = 0; k < mm->lanes; ++k)            // (R3D_OPT_LANES: the forwards ran on the lanes' streams)
        if ((e = hipStreamSynchronize(mm->lane[k].stream)) != hipSuccess) return r3d::hip_fail(e, "hipStreamSynchronize(lane)");
    if (mm->status_host && *reinterpret_cast<volatile unsigned *>(mm->status_host) != 0u) {
        *reinterpret_cast<volatile unsigned *>(mm->status_host) = 0u;
        r3d::set_error("a dependency wait of the single-launch forward gave up after %d ms (workgroups not co-resident: the GPU is shared "
                       "with another persistent kernel, or CUs are masked): the outputs of that forward are NaN.  Run the handle "
                       "level by level: r3d_set_option(m, R3D_OPT_STAGED, 1)", mm->spin_timeout_ms);
        return R3D_ERR_ABORTED;
    }
    return R3D_OK;
}

const char *r3d_last_error(void) { return r3d::last_error(); }
const char *r3d_version(void) { return "ray3d_hip 0.6 (gfx950, ABI 6)"; }
int r3d_abi_version(void) { return R3D_ABI_VERSION; }
int r3d_precision(const r3d_model *m) {
    if (!m) { r3d::set_error("r3d_precision: null model"); return R3D_ERR_ARG; }
    return reinterpret_cast<const Model *>(m)->use_b3 ? 1 : 0;
}

}  // extern "C"
