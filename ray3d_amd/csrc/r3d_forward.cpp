// The forward driver: one call of r3d_forward / r3d_forward_pair as a sequence of steps over one call context.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "r3d_internal.hpp"
#include "r3d_undistort.hpp"

namespace r3d {

// output joint slot -> (body part, index inside the part), lib/model/rie.py:426-431 (quirk Q2:
// for J = 14 / 15 this is not the inverse of the input grouping).  Fills slot[] such that the
// o-th output of part g (flat index first[g] + o) lands in element slot[first[g] + o] of (J,3).
static void output_slots(int J, const int *first, int *slot) {
    int s = 0;
    auto put = [&](int part, int idx) {
        for (int f = 0; f < 3; ++f) slot[first[part] + idx * 3 + f] = s * 3 + f;
        ++s;
    };
    enum { T = 0, LA = 1, RA = 2, LL = 3, RL = 4 };
    if (J == 17) {
        put(T, 0);
        for (int i = 0; i < 3; ++i) put(LL, i);
        for (int i = 0; i < 3; ++i) put(RL, i);
        for (int i = 1; i < 5; ++i) put(T, i);
        for (int i = 0; i < 3; ++i) put(RA, i);
        for (int i = 0; i < 3; ++i) put(LA, i);
    } else if (J == 15) {
        put(T, 0); put(T, 1);
        for (int i = 0; i < 3; ++i) put(LL, i);
        for (int i = 0; i < 3; ++i) put(RL, i);
        for (int i = 0; i < 3; ++i) put(RA, i);
        for (int i = 0; i < 3; ++i) put(LA, i);
        put(T, 2);
    } else {
        put(T, 0);
        for (int i = 0; i < 3; ++i) put(LL, i);
        for (int i = 0; i < 3; ++i) put(RL, i);
        for (int i = 0; i < 3; ++i) put(RA, i);
        for (int i = 0; i < 3; ++i) put(LA, i);
        put(T, 1);
    }
}

bool same_input_shape(const Model *a, const Model *b) {
    return a->cfg.num_joints == b->cfg.num_joints && a->cfg.in_features == b->cfg.in_features &&
           a->cfg.num_levels == b->cfg.num_levels && a->cfg.extrinsic_dim == b->cfg.extrinsic_dim;
}

// activations (the input is read in place in both modes: UV mode encodes the rays inside the gather), then - 256-byte
// aligned - the single-launch forward's control region: ready counters + abort flag, the call's problem table
size_t workspace_act_bytes(const Plan *pl, int64_t B) {
    const size_t act = ((size_t)pl->floats_per_window * (size_t)B + (size_t)pl->tail_floats + 64) * sizeof(float);
    return (act + 255) / 256 * 256;
}
static size_t workspace_need(const Plan *pl, int64_t B) { return workspace_act_bytes(pl, B) + fwd_ctrl_bytes(pl, B); }

// r3d_workspace_bytes of a pair (a = pos or the single model, b = trj of a pair)
size_t workspace_bytes_pair(Model *a, Model *b, int64_t B) {
    // monotonic in B: the plan kind switches with the window count and the less fused plans of small calls keep larger
    // intermediates, so a call of fewer windows may need MORE bytes than one of B - the answer covers every size <= B
    size_t need = workspace_need(plan_get(a, b, plan_kind(B)), B);
    for (int64_t edge : plan_kind_edges())
        if (edge < B) need = std::max(need, workspace_need(plan_get(a, b, plan_kind(edge)), edge));
    return need;
}

// R3D_INPUT_UV_DIST, R3D_INPUT_PX_INTRINSIC, R3D_INPUT_PX_SCREEN - the modes with a pixel pre-pass: it writes the model's
// input (3-float rays, or 2 floats per point for the in_features == 2 models) behind r3d_workspace_bytes(B) of the call's
// own B (<= that of any larger B, so a workspace sized for the largest call serves every smaller one).  Layout: one point
// per input frame, in the input's own window stride - unless windows overlap AND have their own cameras: a frame then has
// one point per window that holds it, and the windows are materialised as (B, RF, J, F), read with window_stride = RF.
static bool px_mode(int mode) { return mode == R3D_INPUT_UV_DIST || mode == R3D_INPUT_PX_INTRINSIC || mode == R3D_INPUT_PX_SCREEN; }
static int px_encoding(int mode) { return mode == R3D_INPUT_PX_INTRINSIC ? ENC_INTRINSIC : mode == R3D_INPUT_PX_SCREEN ? ENC_SCREEN : ENC_RAY; }
static const char *px_name(int mode) {
    return mode == R3D_INPUT_PX_INTRINSIC ? "R3D_INPUT_PX_INTRINSIC" : mode == R3D_INPUT_PX_SCREEN ? "R3D_INPUT_PX_SCREEN" : "R3D_INPUT_UV_DIST";
}
static bool dist_materialised(const Model *a, const r3d_input *in) { return in->cam_stride != 0 && in->window_stride < a->RF; }
static int64_t dist_ray_frames(const Model *a, const r3d_input *in, int64_t B) {
    return dist_materialised(a, in) ? B * a->RF : (B - 1) * in->window_stride + a->RF;
}
size_t dist_ray_bytes(const Model *a, const r3d_input *in, int64_t B) {
    const size_t F = (size_t)enc_floats(px_encoding(in->mode));
    return ((size_t)dist_ray_frames(a, in, B) * (size_t)a->cfg.num_joints * F * sizeof(float) + 255) / 256 * 256;
}
int dist_check(const Model *a, const r3d_input *in, bool need_cam) {
    const char *name = px_name(in->mode);
    const int F = enc_floats(px_encoding(in->mode));
    if (a->cfg.in_features != F) { set_error("%s needs in_features == %d (got %d)", name, F, a->cfg.in_features); return R3D_ERR_ARG; }
    if (need_cam && !in->cam_dev) { set_error("%s needs cam_dev (rows of 16 doubles)", name); return R3D_ERR_ARG; }
    if (in->cam_stride != 0 && in->cam_stride < UNDIST_ROW_DOUBLES) {
        set_error("%s: cam_stride must be 0 or >= %d doubles (got %lld)", name, UNDIST_ROW_DOUBLES, (long long)in->cam_stride);
        return R3D_ERR_ARG;
    }
    if (in->window_stride <= 0) { set_error("window_stride must be positive"); return R3D_ERR_ARG; }
    return R3D_OK;
}

// The size limits of one call (include/ray3d_hip.h, "Size limits of one forward"), judged on shapes alone - check_call and
// redirect_px ask here, and so does r3d_debug_call_check.  The first-level gathers address the whole raw input through one
// buffer descriptor with 32-bit byte offsets, and a problem's row count is an int.
int call_size_check(const Model *a, int64_t window_stride, int64_t B) {
    if (((B - 1) * window_stride + a->RF) * (int64_t)(a->cfg.num_joints * 3) * 4 >= 0x7fffffffLL || B * (int64_t)(a->RF / 3) >= 0x7fffffffLL) {
        set_error("B too large for one call (the raw input must stay below 2 GiB)");
        return R3D_ERR_ARG;
    }
    return R3D_OK;
}
// ... of the pixel modes: the windows the pre-pass materialises (overlapping windows with a camera row each)
int px_size_check(const Model *a, int64_t window_stride, int64_t cam_stride, int64_t B) {
    if (cam_stride != 0 && window_stride < a->RF && B * (int64_t)a->RF * (int64_t)(a->cfg.num_joints * 3) * 4 >= 0x7fffffffLL) {
        set_error("B too large for one call (the materialised rays of overlapping windows must stay below 2 GiB)");
        return R3D_ERR_ARG;
    }
    return R3D_OK;
}

// The kernels a forward launches, as its launch records name them (r3d_profile_read) - every name a record can carry comes from here
const char *stage_kernel_name(int kind, bool uv_launch, bool b3_launch) {
    return kind == STAGE_ENC ? (uv_launch ? "r3d_gemm_enc_uv_f32" : "r3d_gemm_enc_f32")
         : b3_launch ? (uv_launch ? "r3d_gemm_uv_b3" : "r3d_gemm_b3") : (uv_launch ? "r3d_gemm_uv_f32" : "r3d_gemm_f32");
}
const char *decode_kernel_name(int64_t B) { return B >= 128 ? "r3d_decode_w4_f32" : "r3d_decode_f32"; }   // (launch_decode picks by the same test)
const char *bind_kernel_name() { return "r3d_bind_f32"; }
const char *undistort_kernel_name() { return "r3d_undistort_rays_f64"; }
std::vector<const char *> launch_kernel_names() {
    std::vector<const char *> v;
    for (int k = 0; k < FWD_KERNEL_COUNT; ++k)
        for (int uv = 0; uv < 2; ++uv) v.push_back(forward_kernel_name(k, uv != 0));
    for (int kind : {STAGE_BIG, STAGE_ENC})
        for (int b3 = 0; b3 < (kind == STAGE_BIG ? 2 : 1); ++b3)
            for (int uv = 0; uv < 2; ++uv) v.push_back(stage_kernel_name(kind, uv != 0, b3 != 0));
    v.push_back(bind_kernel_name());
    v.push_back(decode_kernel_name(1));
    v.push_back(decode_kernel_name(128));
    v.push_back(undistort_kernel_name());
    return v;
}

// Whether a call's fused first levels read the per-frame buffer (CallShape::shared).
// Clip calls (window stride one frame, lib/train_val/trainer.py:47-58): consecutive windows share all but one of their
// frames, and expand_conv is linear - its pre-activations are evaluated once per FRAME by a launch of gathered GEMMs
// ahead of the forward (Plan::frame_probs) and the first-level tiles read them instead of gathering and multiplying
// (r3d_kernels.hip, first_level_shared).  Where it pays (four times fewer rows), one camera for the
// clip, fp32 tiles.  `frame_tiles`: the schedule has the per-frame launch's tile lists.
bool call_shares_first_layers(const Plan *pl, const Model *a, int64_t B, bool uv, int64_t window_stride, int64_t cam_stride, long long frames,
                              bool frame_tiles) {
    bool b3_call = false;
    for (const Model *mm : pl->m) b3_call = b3_call || (mm && mm->use_b3 && B >= b3_min_batch());
    // (the per-frame buffer is addressed with 32-bit byte offsets in first_level_shared - row tables, descriptor bound: a
    //  clip whose buffer would reach 4 GiB, ~349 k windows for a pos + trj pair, keeps the gathered path, which has 64-bit tile bases)
    return pl->frame_buf >= 0 && frame_tiles && window_stride == 1 && !b3_call && (frames - 2) * 4 <= B * (int64_t)(a->RF / 3) &&
           !(uv && cam_stride != 0) && !hook_on("R3D_NO_SHARED_L0") &&
           (unsigned long long)frames * (unsigned long long)pl->frame_ld * 4ull < 0xffffffffull;
}

// Whether a call runs as ONE persistent launch: `grid` / `kernel` of the schedule's single-launch lists (0: it has none),
// `has_table`: the relative problem table of the call's variant exists
bool call_is_single(const Model *a, const Model *b, int grid, bool has_table, int kernel, bool shared) {
    return forward_single_launch() && !a->opt_staged && !(b && b->opt_staged) && grid > 0 && has_table && !(shared && kernel != FWD_KERNEL_F32);
}

struct Recorder {
    Model *m;
    hipStream_t stream;
    size_t n = 0;
    bool on() const { return m->profiling; }
    hipError_t begin(const char *kernel, int stage, int blocks, double flops, double bytes) {
        if (!on()) return hipSuccess;
        if (n == m->recs.size()) {
            Model::Rec r;
            hipError_t e = hipEventCreate(&r.e0);
            if (e != hipSuccess) return e;
            if ((e = hipEventCreate(&r.e1)) != hipSuccess) return e;
            m->recs.push_back(r);
        }
        Model::Rec &r = m->recs[n];
        memset(&r.r, 0, sizeof r.r);
        strncpy(r.r.kernel, kernel, sizeof r.r.kernel - 1);
        r.r.stage = stage;
        r.r.blocks = blocks;
        r.r.flops = flops;
        r.r.bytes = bytes;
        return hipEventRecord(r.e0, stream);
    }
    hipError_t end() {
        if (!on()) return hipSuccess;
        return hipEventRecord(m->recs[n++].e1, stream);
    }
};

// One GEMM problem of the plan for a call of B windows.  `tags` (optional, BIND_NPTR entries): the base of every pointer field.
int fill_prob(const Plan *pl, const ProbSpec &q, int64_t B, const Model *a, const Bases &bs, const CallShape &cs, GemmProb &g,
              unsigned char *tags) {
    memset(&g, 0, sizeof g);
    unsigned char tg[BIND_NPTR] = {0};
    const Model *m = pl->m[q.model];
    const Layer &L = m->layers[q.layer];
    const int JF = frame_floats(a, cs.uv);
    auto ws_ptr = [&](int buf, int col) {
        return reinterpret_cast<float *>(const_cast<char *>(bs.ws) + ((size_t)pl->buffers[buf].offset_per_window * (size_t)B + (size_t)col) * sizeof(float));
    };
    auto arena_ptr = [&](size_t off) { return reinterpret_cast<const float *>(bs.arena[q.model] + off * sizeof(float)); };
    const unsigned char TA = (unsigned char)(BIND_ARENA0 + q.model), TI = (unsigned char)(BIND_IARENA0 + q.model);
    int kend = 0;
    for (int s = 0; s < MAX_SEG; ++s) {
        if (s < q.nseg) {
            if (pl->buffers[q.seg[s].buf].external == 3) {      // the caller's camera-parameter rows
                g.a[s] = reinterpret_cast<const float *>(bs.param);
                g.lda[s] = (int)cs.param_stride;
                tg[s] = BIND_PARAM;
            } else {
                g.a[s] = ws_ptr(q.seg[s].buf, q.seg[s].col);
                g.lda[s] = q.seg[s].ld;
                tg[s] = BIND_WS;
            }
            kend += q.seg[s].width;
        } else {
            g.a[s] = g.a[0];
            g.lda[s] = g.lda[0];
            tg[s] = tg[0];
        }
        g.kend[s] = s < q.nseg ? kend : 0x7fffffff;
    }
    // the last real segment absorbs the rest - unless it is narrower than the padded K (embedder.w1 on
    // the 2-wide parameter rows): its true width bounds the buffer descriptor, the rest reads as zeros
    if (q.nseg > 0 && !(q.nseg == 1 && kend < L.Kpad)) g.kend[q.nseg - 1] = 0x7fffffff;
    if (q.enc_lut >= 0) {
        if (cs.uv && q.enc_lut_uv < 0) { set_error("internal: no UV tables for an encoded operand"); return R3D_ERR_STATE; }
        g.lut = reinterpret_cast<const int *>(bs.iarena[q.model] + (size_t)(cs.uv ? q.enc_lut_uv : q.enc_lut) * sizeof(int));
        tg[15] = TI;
        g.x = reinterpret_cast<const float *>(bs.x);
        tg[16] = BIND_X;
        g.cam = cs.uv ? reinterpret_cast<const double *>(bs.cam) : nullptr;
        tg[17] = cs.uv ? BIND_CAM : BIND_NULL;
        g.cam_stride = cs.cam_stride;
        g.enc_ws = cs.window_stride * JF;
        g.enc_rows = q.enc_rows;
        g.enc_step = q.enc_step;
        g.enc_jf = JF;
        g.enc_cur = (a->RF / a->cfg.in_features) * JF;   // quirk Q1: "current" frame is RF // in_features
        g.enc_bytes = (unsigned)((size_t)cs.frames * JF * sizeof(float));
        g.res_tap = 1 + m->cfg.causal;
        if (cs.shared && q.layer3 >= 0 && q.frame_col >= 0) {
            // clip call: the tile reads its expand_conv pre-activations from the per-frame buffer (Plan::frame_buf, written by
            // the launch ahead of the forward) - `x` is this branch's [E | V] block, a row per input frame of enc_jf floats,
            // enc_ws / enc_cur the window stride and the current frame's offset in those rows; no tables, no camera
            g.lut = nullptr;
            tg[15] = BIND_NULL;
            g.x = ws_ptr(pl->frame_buf, q.frame_col);
            tg[16] = BIND_WS;
            g.cam = nullptr;
            tg[17] = BIND_NULL;
            g.cam_stride = 0;
            g.enc_jf = pl->frame_ld;
            g.enc_ws = cs.window_stride * pl->frame_ld;
            g.enc_cur = (a->RF / a->cfg.in_features) * pl->frame_ld;
            g.enc_bytes = (unsigned)(((size_t)cs.frames * pl->frame_ld - (size_t)q.frame_col) * sizeof(float));
        }
    }
    g.w = arena_ptr(L.w_off);
    tg[4] = TA;
    const bool b3 = B >= b3_min_batch();
    if (b3 && L.bf3 && q.layer2 < 0 && q.enc_lut < 0) { g.wb3 = arena_ptr(L.wb3_off); tg[10] = TA; }
    g.bias = arena_ptr(L.b_off);
    tg[5] = TA;
    if (q.res_buf >= 0) { g.res = ws_ptr(q.res_buf, q.res_col); tg[6] = BIND_WS; }
    g.ldr = q.res_ld;
    g.c = ws_ptr(q.c_buf, q.c_col);
    tg[7] = BIND_WS;
    g.ldc = q.c_ld;
    g.M = (int)(B * q.rows_per_window);
    g.N = L.N;
    g.K = L.Kpad;
    g.slope = L.slope;
    if (q.layer2 >= 0) {
        const Layer &L2 = m->layers[q.layer2];
        if (b3 && q.layer3 < 0 && L.bf3_conv && L2.bf3_conv && q.nseg == 1) {   // gemm_tile_b3t
            g.wb3 = arena_ptr(L.wb3_off);
            g.w2b3 = arena_ptr(L2.wb3_off);
            tg[10] = tg[11] = TA;
        }
        g.w2 = arena_ptr(L2.w_off);
        g.bias2 = arena_ptr(L2.b_off);
        tg[8] = tg[9] = TA;
        g.K2 = L2.Kpad;
        g.slope2 = L2.slope;
    }
    if (q.layer3 >= 0) {
        const Layer &L3 = m->layers[q.layer3];
        const Layer &L2b = m->layers[q.layer2];
        if (b3 && L.bf3_conv && L2b.bf3_conv && L3.bf3_conv) {   // first_level_taps_b3
            g.wb3 = arena_ptr(L.wb3_off);
            g.w2b3 = arena_ptr(L2b.wb3_off);
            g.w3b3 = arena_ptr(L3.wb3_off);
            tg[10] = tg[11] = tg[12] = TA;
        }
        g.w3 = arena_ptr(L3.w_off);
        g.bias3 = arena_ptr(L3.b_off);
        tg[13] = tg[14] = TA;
        g.K3 = L3.Kpad;
        g.slope3 = L3.slope;
    }
    if (tags) memcpy(tags, tg, sizeof tg);
    return R3D_OK;
}

// The workgroup count and the Plan::schedules lane keys a forward of (a, b) runs under.  r3d_prepare pins what the driver
// fetches - a graph captured after it is only safe because both ask here.
// (R3D_OPT_CU_LIMIT: a CU-masked stream - fewer workgroups, and no ordering against other streams' forwards)
FwdKeys forward_keys(const Model *a, const Model *b) {
    FwdKeys k;
    k.cu_limit = a->lanes > 1 ? device_cu_count() / a->lanes : std::max(a->cu_limit, b ? b->cu_limit : 0);
    k.nwg = k.cu_limit > 0 ? std::min(k.cu_limit, device_cu_count()) : device_cu_count();
    k.lane_key0 = a->lanes > 1 ? 1 : 0;    // schedules of lane k live under key k + 1 (0: the handle without lanes)
    k.nlanes = a->lanes > 1 ? a->lanes : 1;
    return k;
}

namespace {

// What the steps of one forward share.  One per call, on the driver's stack; every step takes it by reference.
struct Call {
    Model *a, *b;                          // a = pos or the single model, b = trj of a pair
    const r3d_input *in;                   // what the forward reads: the caller's input, or `in_rays` (redirect_px)
    int64_t B;
    float *out, *out_trj;
    void *ws;
    size_t ws_bytes;
    void *caller_stream;                   // the stream the caller passed ...
    hipStream_t stream;                    // ... and the one the forward runs on (a relayed call: the lane's)
    const r3d_input *in_px = nullptr;      // (the caller's pixels and camera rows: what the pre-pass reads)
    r3d_input in_rays;
    Plan *pl = nullptr;
    Schedule *sched = nullptr;
    size_t ws_need = 0;                    // r3d_workspace_bytes(B), asked once per call (redirect_px, or pick_plan)
    long long frames = 0;
    int JF = 0;                            // floats per input frame of the call
    bool uv = false, shared = false, single = false;
    int variant = 0;                       // which of the schedule's relative tables: UV input + 2 * shared
    int lane = 0;                          // R3D_OPT_LANES: the lane that runs this forward (0 without lanes)
    Model::Lane *relay = nullptr;          // round-robin: the lane this call is relayed to
    int cu_limit = 0;
    Bases bases;
    CallShape shape;
    float *act_base = nullptr;             // (poll mode: the schedule's own activation bank of this call)
    const unsigned *abort_flag = nullptr;
    Recorder rec{nullptr, nullptr};
    int stage_no = 0;
    bool split = false;                    // r3d_forward_pair_split: the decode keeps pos and trj apart

    // the profile record around a launch: begin .. launch .. end
    int begin(const char *kernel, int blocks, double flops, double bytes) {
        const hipError_t e = rec.begin(kernel, stage_no, blocks, flops, bytes);
        return e == hipSuccess ? R3D_OK : hip_fail(e, "hipEventRecord");
    }
    int end() {
        const hipError_t e = rec.end();
        if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
        ++stage_no;
        return R3D_OK;
    }
};

// ---- 1. what is wrong with the call itself
int check_call(const Call &c) {
    const Model *a = c.a, *b = c.b;
    const r3d_input *in = c.in;
    if (!a) { set_error("forward: no model given"); return R3D_ERR_ARG; }
    if (!in || !in->x_dev || !c.out || c.B <= 0) { set_error("forward: null input/output or B <= 0"); return R3D_ERR_ARG; }
    // the 2-feature pixel modes: what is wrong with the arguments themselves (they are judged against the configuration
    // only) is reported whatever state the handle is in - a binding can validate its call before anything is uploaded
    if (in->mode == R3D_INPUT_PX_INTRINSIC || in->mode == R3D_INPUT_PX_SCREEN)
        if (const int rc = dist_check(a, in, true); rc != R3D_OK) return rc;
    for (const Model *m : {a, b})
        if (m && (!m->finalized || m->dirty)) {
            set_error("forward called before r3d_finalize (or weights changed since)");
            return R3D_ERR_STATE;
        }
    if (b && !same_input_shape(a, b)) { set_error("pos and trj models disagree on J / F / levels / extrinsic_dim"); return R3D_ERR_ARG; }
    if (in->mode != R3D_INPUT_RAYS && in->mode != R3D_INPUT_UV && !px_mode(in->mode)) { set_error("bad input mode %d", in->mode); return R3D_ERR_ARG; }
    if (in->mode == R3D_INPUT_UV && (a->cfg.in_features != 3 || !in->cam_dev)) {
        set_error("R3D_INPUT_UV needs in_features == 3 and cam_dev");
        return R3D_ERR_ARG;
    }
    if (in->mode == R3D_INPUT_UV_DIST)
        if (const int rc = dist_check(a, in, true); rc != R3D_OK) return rc;
    const bool needs_param = a->cfg.embed_dim > 0 || (b && b->cfg.embed_dim > 0);
    if (needs_param && !in->param_dev) { set_error("param_dev is required when the camera embedding is on"); return R3D_ERR_ARG; }
    if (in->window_stride <= 0) { set_error("window_stride must be positive"); return R3D_ERR_ARG; }
    return call_size_check(a, in->window_stride, c.B);
}

// ---- 2. the pixel modes: the forward is the R3D_INPUT_RAYS one, on the input the pre-pass writes into the workspace's tail
int redirect_px(Call &c) {
    const Model *a = c.a;
    const r3d_input *in = c.in;
    if (!px_mode(in->mode)) return R3D_OK;
    if (const int rc = px_size_check(a, in->window_stride, in->cam_stride, c.B); rc != R3D_OK) return rc;
    c.ws_need = workspace_bytes_pair(c.a, c.b, c.B);
    const size_t dist_off = (c.ws_need + 255) / 256 * 256;
    const size_t need = dist_off + dist_ray_bytes(a, in, c.B);
    if (!c.ws || c.ws_bytes < need) {
        set_error("workspace too small for %s (r3d_input_workspace_bytes): need %zu bytes, got %zu", px_name(in->mode), need, c.ws_bytes);
        return R3D_ERR_WORKSPACE;
    }
    c.in_px = in;
    c.in_rays = *in;
    c.in_rays.mode = R3D_INPUT_RAYS;
    c.in_rays.x_dev = reinterpret_cast<const float *>(reinterpret_cast<const char *>(c.ws) + dist_off);
    c.in_rays.window_stride = dist_materialised(a, in) ? a->RF : in->window_stride;
    c.in_rays.cam_dev = nullptr;
    c.in_rays.cam_stride = 0;
    c.in = &c.in_rays;
    return R3D_OK;
}

// ---- 3. the plan of a call of B windows, and whether the workspace holds it
int pick_plan(Call &c) {
    c.pl = plan_get(c.a, c.b, plan_kind(c.B));
    c.frames = (c.B - 1) * c.in->window_stride + c.a->RF;
    // the bound is what r3d_workspace_bytes(B) answers - the size formula and this check are one function - which is
    // >= workspace_need(c.pl, B): the plans of smaller calls may need more than this call's own (1025 windows: 1023's)
    const size_t need = c.ws_need ? c.ws_need : (c.ws_need = workspace_bytes_pair(c.a, c.b, c.B));
    if (!c.ws || c.ws_bytes < need) {
        set_error("workspace too small: need %zu bytes (r3d_workspace_bytes), got %zu", need, c.ws_bytes);
        return R3D_ERR_WORKSPACE;
    }
    c.act_base = (float *)c.ws;
    return R3D_OK;
}

// ---- 4. R3D_OPT_LANES: which lane runs this forward - the one whose stream the caller passed, or the next one round-robin (then the
// lane's stream waits for the caller's, runs the forward, and the caller's stream joins later: r3d_lanes_join)
int pick_lane(Call &c) {
    Model *a = c.a, *b = c.b;
    const int lanes = a->lanes;
    if (b && b->lanes != lanes) { set_error("pos and trj handles disagree on R3D_OPT_LANES (%d / %d): set it on both", a->lanes, b->lanes); return R3D_ERR_STATE; }
    if (lanes <= 1) return R3D_OK;
    int lane = -1;
    for (int k = 0; k < lanes; ++k)
        if (a->lane[k].stream == c.stream) lane = k;
    if (lane < 0) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(c.stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            set_error("a handle with R3D_OPT_LANES cannot be captured from a caller's stream: capture on a lane's own stream (r3d_lane_stream)");
            return R3D_ERR_STATE;
        }
        lane = a->next_lane;
        a->next_lane = (a->next_lane + 1) % lanes;
        c.relay = &a->lane[lane];
        hipError_t e0;
        // (the lane is in order: a forward still pending on it for another stream simply runs first)
        // (a caller on the legacy default stream: the lanes' streams are blocking ones and behind its work as they are - an
        //  event recorded there would also be behind the other lanes' forwards, and the lanes would take turns)
        if (c.stream != nullptr &&
            ((e0 = hipEventRecord(c.relay->in, c.stream)) != hipSuccess || (e0 = hipStreamWaitEvent(c.relay->stream, c.relay->in, 0)) != hipSuccess))
            return hip_fail(e0, "hipStreamWaitEvent(lane)");
        c.stream = c.relay->stream;
    }
    c.lane = lane;
    return R3D_OK;
}

// ---- 5. profiling: an empty bracket first - what two event records cost by themselves on this stream (stage -1)
int empty_bracket(Call &c) {
    c.rec = Recorder{c.a, c.stream};       // (the stream is final: pick_lane)
    hipError_t e;
    if ((e = c.rec.begin("r3d_event_pair", -1, 0, 0.0, 0.0)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    if ((e = c.rec.end()) != hipSuccess) return hip_fail(e, "hipEventRecord");
    return R3D_OK;
}

// ---- 6. the pixel modes: the pre-pass, on the stream the forward runs on (a relayed call: the lane's, behind the caller's work)
int px_prepass(Call &c) {
    if (!c.in_px) return R3D_OK;
    const Model *a = c.a;
    const r3d_input *in_px = c.in_px;
    UndistArgs ua;
    memset(&ua, 0, sizeof ua);
    ua.uv = in_px->x_dev;
    ua.cam = in_px->cam_dev;
    ua.cam_stride = in_px->cam_stride;
    ua.rays = const_cast<float *>(c.in->x_dev);
    ua.J = a->cfg.num_joints;
    ua.npts = (int)(dist_ray_frames(a, in_px, c.B) * a->cfg.num_joints);
    ua.pts_per_window = dist_materialised(a, in_px) ? a->RF * a->cfg.num_joints : 0;
    ua.window_stride = (int)in_px->window_stride;
    ua.last_window = (int)(c.B - 1);
    ua.encoding = px_encoding(in_px->mode);
    if (const int rc = c.begin(undistort_kernel_name(), (ua.npts + 255) / 256, 0.0, (double)ua.npts * (2 + enc_floats(ua.encoding)) * sizeof(float)); rc != R3D_OK)
        return rc;
    if (const hipError_t e = launch_undistort(ua, c.stream); e != hipSuccess) return hip_fail(e, "launch r3d_undistort_rays_f64");
    return c.end();
}

// ---- 7. the schedule of this call, whether its first levels read the per-frame buffer (`shared`), and whether it is one launch (`single`)
int pick_schedule(Call &c) {
    const Model *a = c.a, *b = c.b;
    const r3d_input *in = c.in;
    const Plan *pl = c.pl;
    // UV mode: the kernels read pixel keypoints (frames, J, 2) and encode the rays while gathering them
    c.uv = in->mode == R3D_INPUT_UV;
    c.JF = frame_floats(a, c.uv);
    c.bases.ws = reinterpret_cast<const char *>(c.ws);
    for (int mi = 0; mi < 2; ++mi)
        if (pl->m[mi]) {
            c.bases.arena[mi] = reinterpret_cast<const char *>(pl->m[mi]->d_arena);
            c.bases.iarena[mi] = reinterpret_cast<const char *>(pl->m[mi]->d_iarena);
        }
    c.bases.x = reinterpret_cast<const char *>(in->x_dev);
    c.bases.param = reinterpret_cast<const char *>(in->param_dev);
    c.bases.cam = reinterpret_cast<const char *>(in->cam_dev);
    c.shape.uv = c.uv;
    c.shape.window_stride = in->window_stride;
    c.shape.param_stride = in->param_stride;
    c.shape.cam_stride = in->cam_stride;
    c.shape.frames = c.frames;

    const FwdKeys keys = forward_keys(a, b);
    c.cu_limit = keys.cu_limit;
    c.sched = schedule_get(c.pl, c.B, keys.nwg, false, keys.lane_key0 + c.lane);
    if (!c.sched) return R3D_ERR_HIP;
    const Schedule *sched = c.sched;
    // clip calls: the per-frame first layers where they pay (call_shares_first_layers)
    c.shared = call_shares_first_layers(pl, a, c.B, c.uv, in->window_stride, in->cam_stride, c.frames, sched->d_frame_tiles != nullptr);
    c.shape.shared = c.shared;
    c.variant = (c.uv ? 1 : 0) + (c.shared ? 2 : 0);
    c.single = call_is_single(a, b, sched->fwd.grid, sched->fwd.d_rel[c.variant] != nullptr, sched->fwd.kernel, c.shared);
    return R3D_OK;
}

// ---- 8. a clip call's launch of per-frame first layers, ahead of the forward
int frame_stage(Call &c) {
    if (!c.shared) return R3D_OK;
    const Plan *pl = c.pl;
    const r3d_input *in = c.in;
    const bool uv = c.uv;
    const StageSchedule &fs = c.sched->frame_stage;
    LaunchArgs la;
    memset(&la, 0, sizeof la);
    la.tiles = c.sched->d_frame_tiles;
    la.wg_off = c.sched->d_frame_wgoff;
    la.nprob = (int)pl->frame_probs.size();
    la.ks = fs.ks;
    float *fbase = reinterpret_cast<float *>(c.ws) + (size_t)pl->buffers[pl->frame_buf].offset_per_window * (size_t)c.B;
    for (int i = 0; i < la.nprob; ++i) {
        const Plan::FrameProb &f = pl->frame_probs[i];
        const Model *mm = pl->m[f.model];
        const Layer &L = mm->layers[f.layer];
        GemmProb &g = la.p[i];
        for (int sg = 0; sg < MAX_SEG; ++sg) g.kend[sg] = 0x7fffffff;
        g.w = mm->d_arena + L.w_off;
        g.bias = mm->d_arena + L.b_off;
        g.c = fbase + f.col;
        g.ldc = pl->frame_ld;
        g.M = (int)(c.frames - 2);
        g.N = L.N;
        g.K = L.Kpad;
        g.slope = 1.0f;
        g.lut = mm->d_iarena + (uv ? f.lut_uv : f.lut);
        g.x = reinterpret_cast<const float *>(in->x_dev);
        g.cam = uv ? reinterpret_cast<const double *>(in->cam_dev) : nullptr;
        g.cam_stride = 0;
        g.enc_ws = 0;
        g.enc_rows = g.M;                    // (one "window": operand row r starts at frame r)
        g.enc_step = 1;
        g.enc_jf = c.JF;
        g.enc_cur = 0;
        g.enc_bytes = (unsigned)((size_t)c.frames * c.JF * sizeof(float));
        g.res_tap = 1;
    }
    if (const int rc = c.begin(stage_kernel_name(STAGE_BIG, uv, false), fs.nwg, 0.0, 0.0); rc != R3D_OK) return rc;
    if (const hipError_t e = launch_gemm_stage(la, fs.nwg, STAGE_BIG, uv, c.stream); e != hipSuccess)
        return hip_fail(e, "launch r3d_gemm_f32 (per-frame first layers)");
    return c.end();
}

// ---- 9 a. the whole forward as ONE persistent launch: bind (zero the ready counters, resolve the problem table), run

// Where one call's single launch keeps its control data, and whether the table there is bound to this call already
struct Single {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    bool own = false;          // the schedule's own control region (the stream is not being captured)
    bool poll = false;         // ... and its own activation banks, data as its own ready flag
    bool bound = false;        // the table is bound to this call's buffers: no r3d_bind_f32
    char *ctrl = nullptr;
    size_t bank_bytes = 0;
    GemmProb *tables = nullptr;
    int bank = 0;
    unsigned *cnt = nullptr;
    BoundKey key;
};

void resolve_single(const Call &c, Single &s) {
    const Schedule::Fwd &fw = c.sched->fwd;
    const r3d_input *in = c.in;
    // Control region: the caller's workspace while the stream is being captured (the graph binds for itself), the
    // schedule's own otherwise - there a call on the buffers of the previous one finds the table bound and a zeroed
    // bank of counters, and skips r3d_bind_f32 (4-5 us per call; R3D_BIND_ALWAYS=1: never)
    if (hipStreamIsCapturing(c.stream, &s.cap) != hipSuccess) { (void)hipGetLastError(); s.cap = hipStreamCaptureStatusActive; }
    s.own = s.cap == hipStreamCaptureStatusNone && fw.d_ctrl != nullptr;
    s.ctrl = s.own ? fw.d_ctrl : reinterpret_cast<char *>(c.ws) + workspace_act_bytes(c.pl, c.B);
    s.bank_bytes = ((size_t)(fw.ncnt + 4) * sizeof(unsigned) + 255) / 256 * 256;
    s.tables = reinterpret_cast<GemmProb *>(s.ctrl + (s.own ? 2 : 1) * s.bank_bytes);   // (own: one table per activation bank)
    // calls of a few windows, not captured: activations in the schedule's own two banks, data as its own ready flag
    s.poll = s.own && fw.d_act != nullptr;
    s.key.variant = c.variant;
    s.key.base[BIND_WS] = c.ws;              // (the key of the bound state: what the caller passed)
    s.key.base[BIND_ARENA0] = c.bases.arena[0];
    s.key.base[BIND_ARENA1] = c.bases.arena[1];
    s.key.base[BIND_IARENA0] = c.bases.iarena[0];
    s.key.base[BIND_IARENA1] = c.bases.iarena[1];
    s.key.base[BIND_X] = in->x_dev;
    s.key.base[BIND_PARAM] = in->param_dev;
    s.key.base[BIND_CAM] = in->cam_dev;
    s.key.enc_ws = in->window_stride * c.JF;
    s.key.cam_stride = in->cam_stride;
    s.key.enc_bytes = (unsigned)((size_t)c.frames * c.JF * sizeof(float));
    s.key.param_stride = (int)in->param_stride;
    const Schedule::Fwd::Bound &bd = fw.bound;
    s.bound = s.own && bd.valid && bd.key == s.key;
    s.bank = s.bound ? bd.bank ^ 1 : 0;
    s.cnt = reinterpret_cast<unsigned *>(s.ctrl + (s.own ? s.bank : 0) * s.bank_bytes);
}

int bind_if_needed(Call &c, const Single &s) {
    if (s.bound) return R3D_OK;
    const Schedule::Fwd &fw = c.sched->fwd;
    BindArgs ba;
    memset(&ba, 0, sizeof ba);
    ba.rel = fw.d_rel[c.variant];
    ba.tags = fw.d_tags[c.variant];
    ba.out = s.tables;
    ba.nprob = fw.nprob;
    for (int k = 0; k < BIND_NBASE; ++k) ba.base[k] = s.key.base[k];
    ba.enc_ws = s.key.enc_ws;
    ba.cam_stride = s.key.cam_stride;
    ba.enc_bytes = s.key.enc_bytes;
    ba.param_stride = s.key.param_stride;
    ba.cnt = reinterpret_cast<unsigned *>(s.ctrl);
    ba.ncnt = s.own ? (int)(2 * s.bank_bytes / sizeof(unsigned)) - 4 : fw.ncnt;      // (the kernel zeroes ncnt + 4 words: both banks)
    if (s.poll) {                 // both activation banks armed, bank 0's table
        ba.base[BIND_WS] = fw.d_act;
        ba.arm = fw.d_act;
        ba.canon = 1;             // (every producer of a polled operand, the throughput tiles included: r3d_tiles.hpp, act_canon)
        ba.arm_vec4 = (long long)(2 * fw.act_bytes / 16);
    }
    hipError_t e;
    if (const int rc = c.begin(bind_kernel_name(), 1, 0.0, 0.0); rc != R3D_OK) return rc;
    if ((e = launch_bind(ba, c.stream)) != hipSuccess) return hip_fail(e, "launch r3d_bind_f32");
    if (s.poll) {                 // ... and bank 1's
        BindArgs b1 = ba;
        b1.base[BIND_WS] = fw.d_act + fw.act_bytes;
        b1.out = s.tables + fw.nprob;
        b1.ncnt = -4;
        b1.arm = nullptr;
        if ((e = launch_bind(b1, c.stream)) != hipSuccess) return hip_fail(e, "launch r3d_bind_f32");
    }
    return c.end();
}

// the launch itself; its profile record stays open (the caller closes it once the launch lock is released)
int launch_tiles(Call &c, const Single &s, FwdArgs &fa) {
    Schedule::Fwd &fw = c.sched->fwd;
    const GemmProb *table = s.tables + (s.poll ? s.bank * fw.nprob : 0);
    if (s.poll) c.act_base = reinterpret_cast<float *>(fw.d_act + (size_t)s.bank * fw.act_bytes);
    fw.bound.valid = false;    // (until this call's launch is on the stream: it is what zeroes the bank the next call runs on)
    memset(&fa, 0, sizeof fa);
    fa.tiles = fw.d_tiles;
    fa.wg_off = fw.d_wgoff;
    fa.probs = table;
    fa.cnt = s.cnt;
    fa.cnt_next = s.own ? reinterpret_cast<unsigned *>(s.ctrl + (s.bank ^ 1) * s.bank_bytes) : nullptr;
    fa.ncnt = fw.ncnt;
    if (s.poll) {
        fa.poll = 1;
        fa.arm = fw.d_act + (size_t)(s.bank ^ 1) * fw.act_bytes;
        fa.arm_vec4 = (long long)(fw.act_bytes / 16);
    }
    fa.spin_ticks = (long long)std::max(c.a->spin_timeout_ms, 1) * 100000LL;          // 100 MHz wall clock
    if (const char *ft = hook_env("R3D_FAULT_TILE")) fa.fault_tile1 = atoi(ft) + 1;   // (hooks build only: see FwdArgs)
    const bool uv_launch = c.uv && fw.uses_gather;
    const int fwd_kernel = c.shared ? FWD_KERNEL_CLIP : fw.kernel;           // (shared: fw.kernel is FWD_KERNEL_F32 - `single`, pick_schedule)
    if (const int rc = c.begin(forward_kernel_name(fwd_kernel, uv_launch), fw.grid, fw.flops, fw.bytes); rc != R3D_OK) return rc;
#ifdef R3D_TIMING
    timing_arm_forward(fw, fa, c.stream);
#endif
    if (const hipError_t e = launch_forward(fa, fw.grid, fwd_kernel, uv_launch, c.stream); e != hipSuccess) return hip_fail(e, "launch r3d_forward_f32");
    c.a->last_clk_dev = s.cap == hipStreamCaptureStatusNone ? s.cnt + fw.ncnt + 2 : nullptr;   // (a captured call runs later, maybe never)
    return R3D_OK;
}

// (handles of different threads: the waits below, the launch and the note of whose forward was last are one critical section -
//  two threads that both passed the waits before either had launched would put two whole-device forwards on the chip together)
int launch_in_order(Call &c, const Single &s, FwdArgs &fa) {
    Model *a = c.a;
    hipError_t e;
    std::lock_guard<std::mutex> launch_lock(g_fwd_launch_mu);
    if ((e = order_single_launch(c.stream, true, c.cu_limit > 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    // one handle on two masked streams: its counter banks and control region are one per handle - the second stream waits for the first
    if (c.cu_limit > 0 && a->lanes <= 1 && a->last_fwd_stream && a->last_fwd_stream != c.stream) {
        if ((e = wait_behind(c.stream, (hipStream_t)a->last_fwd_stream, a->order_ev)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    }
    a->last_fwd_stream = c.stream;
    if (const int rc = bind_if_needed(c, s); rc != R3D_OK) return rc;
    if (const int rc = launch_tiles(c, s, fa); rc != R3D_OK) return rc;
    if ((e = order_single_launch(c.stream, false, c.cu_limit > 0)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    return R3D_OK;
}

int single_launch(Call &c) {
    Schedule::Fwd &fw = c.sched->fwd;
    Single s;
    resolve_single(c, s);
    FwdArgs fa;
    if (const int rc = launch_in_order(c, s, fa); rc != R3D_OK) return rc;
    if (s.own) {                     // the next call on these buffers needs no bind
        fw.bound.valid = true;
        fw.bound.bank = s.bank;
        fw.bound.key = s.key;
    }
#ifdef R3D_TIMING
    timing_report_forward(c.pl, fw, fa, c.B, c.stream);
#endif
    if (const int rc = c.end(); rc != R3D_OK) return rc;
    c.abort_flag = s.cnt + fw.ncnt;
    return R3D_OK;
}

// ---- 9 b. (staged form) persistent GEMM launches, one per DAG level
int staged_level(Call &c, size_t si) {
    const Plan *pl = c.pl;
    const auto &st = (*c.sched->levels)[si];
    const StageSchedule &ss = c.sched->stages[si];
    LaunchArgs la;
    memset(&la, 0, sizeof la);
    la.tiles = c.sched->d_tiles + ss.tiles_off;
    la.wg_off = c.sched->d_wgoff + ss.wgoff_off;
    la.nprob = (int)st.size();
    la.ks = ss.ks;
    int n_enc = 0;
    for (int i = 0; i < la.nprob; ++i) {
        const ProbSpec &q = pl->probs[st[i] & ~STAGE_SPILL_IN];      // (a spilled tail uses the problem as it is: tiles carry absolute rows)
        if (q.enc_lut >= 0 && q.enc_kernel) ++n_enc;                 // (with a fused first level these run in the GEMM kernel)
        const int rc = fill_prob(pl, q, c.B, c.a, c.bases, c.shape, la.p[i], nullptr);
        if (rc != R3D_OK) return rc;
    }
    if (n_enc != 0 && n_enc != la.nprob) { set_error("internal: launch mixes encoded and plain operands"); return R3D_ERR_STATE; }
    if ((n_enc != 0) != (ss.kind == STAGE_ENC)) { set_error("internal: schedule and plan disagree on the launch kind"); return R3D_ERR_STATE; }
    bool uv_launch = false;                             // UV mode: only the launches that gather from the input
    for (int i = 0; i < la.nprob; ++i) uv_launch = uv_launch || la.p[i].cam != nullptr;
    bool b3_launch = false;                             // (launch_gemm_stage picks the kernel by the same test)
    for (int i = 0; i < la.nprob; ++i) b3_launch = b3_launch || la.p[i].wb3 != nullptr;
    const char *kname = stage_kernel_name(ss.kind, uv_launch, b3_launch);
    if (const int rc = c.begin(kname, ss.nwg, ss.flops, ss.bytes); rc != R3D_OK) return rc;
#ifdef R3D_TIMING
    const bool timed = timing_arm_stage(si, la, c.stream);
#endif
    if (const hipError_t e = launch_gemm_stage(la, ss.nwg, ss.kind, uv_launch, c.stream); e != hipSuccess) return hip_fail(e, "launch r3d_gemm_f32");
#ifdef R3D_TIMING
    if (timed) timing_report_stage(si, ss, c.stream);
#endif
    return c.end();
}

int staged_levels(Call &c) {
    c.a->last_clk_dev = nullptr;
    for (size_t si = 0; si < c.sched->levels->size(); ++si)
        if (const int rc = staged_level(c, si); rc != R3D_OK) return rc;
    return R3D_OK;
}

// ---- 10. fused decoder tail
int decoder_tail(Call &c) {
    const Model *a = c.a;
    const Plan *pl = c.pl;
    auto buf_ptr = [&](int id) -> float * { return c.act_base + (size_t)pl->buffers[id].offset_per_window * (size_t)c.B; };
    DecodeArgs da;
    memset(&da, 0, sizeof da);
    da.B = c.B;
    da.J = a->cfg.num_joints;
    da.has_pos = pl->pos_model >= 0;
    da.has_trj = pl->trj_model >= 0;
    da.out = c.out;
    da.out_trj = da.has_pos ? c.out_trj : nullptr;
    da.split = c.split && da.has_pos && da.has_trj && da.out_trj != nullptr;
    da.abort_flag = c.abort_flag;
    da.status = a->status_host;
    double dec_flops = 0;
    int first = 0;
    // plan.decs lists the pos parts (Torso, LArm, RArm, LLeg, RLeg) then the trajectory decoder
    std::vector<Plan::Dec> order;
    for (const auto &d : pl->decs) if (pl->m[d.model]->cfg.kind == R3D_KIND_POS) order.push_back(d);
    for (const auto &d : pl->decs) if (pl->m[d.model]->cfg.kind == R3D_KIND_TRJ) order.push_back(d);
    int firsts[MAX_DEC] = {0};
    for (const auto &d : order) {
        const Model *m = pl->m[d.model];
        const Layer &L = m->layers[d.layer];
        const int sidx = da.nsrc++;
        da.h[sidx] = buf_ptr(d.hbuf);
        da.w[sidx] = m->d_arena + L.w_off;
        da.bias[sidx] = m->d_arena + L.b_off;
        da.n_out[sidx] = L.N;
        da.first[sidx] = first;
        firsts[sidx] = first;
        if (m->cfg.kind == R3D_KIND_POS) first += L.N;
        dec_flops += 2.0 * (double)c.B * L.K * L.N;
    }
    if (da.has_pos) output_slots(da.J, firsts, da.slot);
    if (const int rc = c.begin(decode_kernel_name(c.B), 0, dec_flops, (double)c.B * da.nsrc * MLP_HIDDEN * 4.0); rc != R3D_OK) return rc;
    if (const hipError_t e = launch_decode(da, c.stream); e != hipSuccess) return hip_fail(e, "launch r3d_decode_f32");
    if (const int rc = c.end(); rc != R3D_OK) return rc;
    if (c.rec.on()) c.a->nrec = (int)c.rec.n;
    return R3D_OK;
}

// ---- 11. a relayed call: the caller's stream sees the outputs once it has joined this lane (r3d_lanes_join)
int relay_done(Call &c) {
    Model::Lane *relay = c.relay;
    if (!relay) return R3D_OK;
    if (const hipError_t e = hipEventRecord(relay->done, relay->stream); e != hipSuccess) return hip_fail(e, "hipEventRecord(lane)");
    if (std::find(relay->waiters.begin(), relay->waiters.end(), c.caller_stream) == relay->waiters.end()) relay->waiters.push_back(c.caller_stream);
    return R3D_OK;
}

}  // namespace

// One forward of (a, b) - r3d_forward / r3d_forward_pair / r3d_forward_pair_split - as the steps above, in this order
int forward_run(Model *a, Model *b, const r3d_input *in, int64_t B, float *out, float *out_trj, void *ws, size_t ws_bytes,
                void *stream, bool split) {
    Call c{a, b, in, B, out, out_trj, ws, ws_bytes, stream, (hipStream_t)stream};
    c.split = split;
    int rc = check_call(c);
    if (rc == R3D_OK) rc = redirect_px(c);
    if (rc == R3D_OK) rc = pick_plan(c);
    if (rc == R3D_OK) rc = pick_lane(c);
    if (rc == R3D_OK) rc = empty_bracket(c);
    if (rc == R3D_OK) rc = px_prepass(c);
    if (rc == R3D_OK) rc = pick_schedule(c);
    if (rc == R3D_OK) rc = frame_stage(c);
    if (rc == R3D_OK) rc = c.single ? single_launch(c) : staged_levels(c);
    if (rc == R3D_OK) rc = decoder_tail(c);
    if (rc == R3D_OK) rc = relay_done(c);
    return rc;
}

}  // namespace r3d
