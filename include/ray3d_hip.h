/*
 * ray3d_hip.h - C ABI of libray3d_hip.so: the MI355X (gfx950) implementation of Ray3D's
 * 2D->3D lifting forward pass.
 *
 * The reference (YxZhxn/Ray3D) has no FFI for this path; its seam is the Python nn.Module
 * contract.  Each entry point below names the reference interface it
 * replaces; INTEGRATION.md shows the ctypes stub a maintainer would add on the reference side.
 *
 * Conventions: plain C, int status codes (0 = ok, <0 = error, text via r3d_last_error()),
 * no exceptions cross the boundary.  All *_dev pointers are device (HBM) pointers owned by the
 * caller; the library owns only its packed weights.  A handle is bound to the HIP device that
 * was current at r3d_finalize().  Threading: a handle - and a (pos, trj) pair used together - must
 * be driven by one thread at a time (its launch plans, per-batch-size tile schedules and profiling
 * records are unguarded caches); different handles are independent and may be used concurrently
 * (the registry that maps handle pairs to plans is mutex-guarded, r3d_last_error() is thread-local; the ordering of whole-device
 * forwards - two of them must never share the chip - and the launch it protects are one critical section across threads).
 * Every call enqueues on the given hipStream_t (passed as void*) and returns without syncing.
 * The first forward of a new batch size builds and uploads a tile schedule (hipMalloc + blocking
 * hipMemcpy): call r3d_prepare() for that size beforehand when the forward is to be captured into
 * a hipGraph or must not stall.
 */
#ifndef RAY3D_HIP_H
#define RAY3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3D_OK 0
#define R3D_ERR_ARG (-1)        /* bad argument / unsupported configuration            */
#define R3D_ERR_KEY (-2)        /* unknown, duplicate or missing state_dict key         */
#define R3D_ERR_SHAPE (-3)      /* tensor shape does not match the configuration         */
#define R3D_ERR_STATE (-4)      /* call order violated (e.g. forward before finalize)    */
#define R3D_ERR_HIP (-5)        /* a HIP runtime call failed                             */
#define R3D_ERR_WORKSPACE (-6)  /* workspace too small                                   */
#define R3D_ERR_ABORTED (-7)    /* r3d_status: a forward gave up waiting for its own tiles: its outputs are NaN */

#define R3D_KIND_POS 0 /* lib/model/rie.py:172  RIEModel            -> (B,1,J,3) */
#define R3D_KIND_TRJ 1 /* lib/model/rie.py:437  RIETrajectoryModel  -> (B,1,1,3) */

/* Mirrors the constructor arguments the reference factory passes
 * (lib/model/__init__.py:23-46 -> lib/model/rie.py:178-181 / :443-446). */
#define R3D_ABI_VERSION 6 /* bumped whenever a struct below changes size or layout: r3d_abi_version() returns the
                           * library's; a binding compares it with the header it was written against       */

typedef struct {
    int32_t struct_size;   /* sizeof(r3d_config) of the CALLER's header: r3d_create rejects any other size, so a
                            * binding built against an older (shorter) struct fails loudly instead of having
                            * r3d_create read past its buffer                                             */
    int32_t kind;          /* R3D_KIND_POS | R3D_KIND_TRJ                               */
    int32_t num_joints;    /* NUM_KPTS: 14, 15 or 17                                    */
    int32_t in_features;   /* INPUT_DIM: 3 (rays) or 2                                  */
    int32_t num_levels;    /* len(ARCHITECTURE); every filter width must be 3           */
    int32_t channels;      /* CHANNELS (multiple of 32)                                 */
    int32_t latent;        /* LATENT_FEATURES_DIM (multiple of 32)                      */
    int32_t stage;         /* STAGE (pos only; 1 = no FuseBlocks)                       */
    int32_t extrinsic_dim; /* EXTRINSIC_DIM, or 0 when CAMERA_EMBDDING is False         */
    int32_t embed_dim;     /* EMBEDD_DIM (multiple of 32), or 0 when CAMERA_EMBDDING off */
    int32_t causal;        /* CAUSAL with DISABLE_OPTIMIZATIONS: each level's residual is the
                            * last of its three input frames instead of the centre one
                            * (rie.py:43-47,88-92).  CAUSAL with the strided convolutions is
                            * not a configuration the reference can run (rie.py:94-97 raises);
                            * DISABLE_OPTIMIZATIONS alone computes the same function for an
                            * RF-long window and needs no flag.                             */
    int32_t dense;         /* DENSE with DISABLE_OPTIMIZATIONS (the dense-convolution ablation,
                            * rie.py:49-53): level i's convolution has 2*3^i + 1 taps, stride 1,
                            * and every level is evaluated at all RF positions of a window
                            * (cost grows with RF^2: meant for the short receptive fields the
                            * ablation is run at).  DENSE without DISABLE_OPTIMIZATIONS is
                            * ignored by the reference constructor (:54-55): pass 0.          */
    int32_t bf16x3;        /* 0: fp32 matrix cores (v_mfma_f32_32x32x2_f32).  1: the large GEMMs on the
                            * bf16 matrix cores with every fp32 operand split exactly into three bf16
                            * terms (six products, fp32 accumulate): fp32-equivalent results - 1.1 to 1.4
                            * times the fp32 path's error against a float64 evaluation, both ~1e-6 of the
                            * output magnitude - at 6/16 of the matrix time.  Not a
                            * reference key.  The environment variable R3D_BF16X3=1 / =0 at r3d_create
                            * overrides the field.                                                     */
} r3d_config;

typedef struct r3d_model r3d_model;

/* ---- construction: replaces RIEModel(...)/RIETrajectoryModel(...) + load_state_dict ---- */

/* lib/model/rie.py:178-253 / :443-494 (module construction). */
int r3d_create(const r3d_config *cfg, r3d_model **out);
int r3d_destroy(r3d_model *m);

/* The float tensors of the reference state_dict this configuration expects (SURVEY.md A.4;
 * int64 num_batches_tracked buffers are not part of the ABI).  Lets a binding enumerate keys. */
int r3d_num_weights(const r3d_model *m);
const char *r3d_weight_key(const r3d_model *m, int index);
int r3d_weight_shape(const r3d_model *m, int index, int64_t shape[4], int *rank);

/* nn.Module.load_state_dict(strict=True) equivalent (lib/train_val/trainer.py:161-164,
 * lib/utils/utils.py:208-218, but loud: unknown key -> R3D_ERR_KEY, wrong shape ->
 * R3D_ERR_SHAPE).  `host` is float32 row-major in torch layout (Conv1d (Cout,Cin,k),
 * Linear (out,in)); it is copied.  A leading "module." (nn.DataParallel checkpoints,
 * lib/model/__init__.py:52) is stripped.  May be called again after finalize to update. */
int r3d_set_weight(r3d_model *m, const char *key, const float *host, const int64_t *shape, int rank);

/* model.eval() + device placement: folds eval-mode BatchNorm (eps 1e-5) into the preceding
 * Conv1d/Linear in float64, repacks every layer into the GEMM layout the kernels read and
 * uploads to the current HIP device.  R3D_ERR_KEY (message lists the first missing key) if any
 * tensor was not set. */
int r3d_finalize(r3d_model *m);

/* r3d_finalize from DEVICE-resident tensors: the same fold and repack, run on the device on `hip_stream` - for a model whose
 * parameters live in device memory and change (a validation pass after every epoch).  `weights_dev` and `numel` are HOST arrays
 * of `count` entries: entry i is the device pointer and the element count of tensor r3d_weight_key(m, i), contiguous float32 in
 * torch layout, on the current HIP device.  No weight is copied to the host, nothing waits for the device, and the number of
 * launches (two, of the kernel r3d_k_pack, behind one small copy of the pointer table) does not depend on
 * the number of layers.  The packed image is BIT FOR BIT what r3d_finalize produces from the same values (the same float64
 * arithmetic, per element, without contraction); non-finite inputs are outside that promise (NaN payloads may differ).
 * Checked on the host before any device call: count != r3d_num_weights, a null argument or a null entry -> R3D_ERR_ARG; a numel[i]
 * that is not the tensor's element count -> R3D_ERR_SHAPE; r3d_last_error names the key.  A stream that is being captured is
 * refused with R3D_ERR_STATE (the call may allocate, and it copies the pointer table from a staging buffer it reuses).
 * Works on a fresh handle - it allocates the packed arena, zero-fills it on the stream and uploads the gather tables - and on a
 * finalized one, where it packs IN PLACE: the arena does not move, so plans, prepared (pinned) schedules and captured graphs stay
 * valid.  r3d_set_weight + r3d_finalize keep working afterwards; the last finalize of either kind wins.  The tensors are only read,
 * and must stay alive and unchanged until the stream has passed the call.
 * Ordering: the pack is ordered on `hip_stream`.  Forwards of this handle issued on the same stream before the call see the old
 * weights, those issued after it the new ones.  With R3D_OPT_LANES > 1 the call first makes `hip_stream` wait for the lanes (the
 * events r3d_lanes_join waits for; the stream counts as joined afterwards), and a forward relayed to a lane later waits for its
 * caller's stream as always - so forwards issued from `hip_stream` are ordered around the pack with lanes too.  Forwards in
 * flight on OTHER caller streams (or issued directly on a lane's stream) are the caller's to order against the call, as for any
 * buffer two streams share.  There is no device-wide synchronisation on this path. */
int r3d_finalize_dev(r3d_model *m, const float *const *weights_dev, const int64_t *numel, int32_t count, void *hip_stream);

/* ---- forward: replaces pos_model(inputs_2d, inputs_param) [+ trj_model(...)] ---- */

#define R3D_INPUT_RAYS 0 /* x is what the reference feeds the model: ray-encoded keypoints  */
#define R3D_INPUT_UV 1   /* x is pixel keypoints; rays are computed on the fly from `cam`   */
/* x is RAW pixel keypoints of a distorted camera (CameraInfoPacket(..., undistort=True), the H36M / HumanEva loaders'
 * default: lib/dataset/h36m_dataset.py:383-385).  A pre-pass kernel (r3d_undistort_rays_f64) computes in float64, per
 * keypoint, what lib/camera/camera.py:412-441 does on the host - cv2.undistortPoints(uv, K, dist, P=K), i.e. five
 * fixed-point iterations and the re-projection with K - then the ray encoding (:460-471), casts once to float32
 * (lib/train_val/trainer.py:298) and writes the rays into the TAIL of the workspace (size it with
 * r3d_input_workspace_bytes); the R3D_INPUT_RAYS forward then reads them.  Needs in_features == 3 and cam_dev; cam_stride
 * is 0 (one camera) or >= 16.  Rows whose five coefficients are all 0 skip the iteration and the re-projection (the
 * reference's undistort=False): the outputs are then bit-identical to R3D_INPUT_UV.  Layout of the rays: one per input
 * frame (frame f with the row of window min(f / window_stride, B - 1)) for one camera or window_stride >= RF; windows
 * that overlap AND have their own cameras get a materialised (B, RF, J, 3) copy.  The pre-pass is enqueued on the
 * stream the forward runs on (with R3D_OPT_LANES: the lane's, after the relay - workspace and inputs belong to the lane
 * until r3d_lanes_join as always), is captured with the forward into a hipGraph, and is a record of its own in
 * r3d_profile_read.  PARITY UNPINNED against cv2 itself (OpenCV is not a dependency): the arithmetic restates OpenCV's
 * documented algorithm and is pinned to the project's other restatements (ray3d_amd/camera.py, the CPU oracle, the
 * fixture generator's five-iteration grid), INTEGRATION.md section 5. */
#define R3D_INPUT_UV_DIST 2
/* The inputs of the 2-feature models (INPUT_DIM 2, RAY_ENCODING False: the cfg_rie_* baselines) from RAW pixel keypoints.
 * The same pre-pass kernel (r3d_undistort_rays_f64, one launch, same record name in r3d_profile_read) writes 2 floats per
 * keypoint into the workspace tail - size it with r3d_input_workspace_bytes - and the R3D_INPUT_RAYS forward reads them.
 * Both need in_features == 2 and cam_dev rows of 16 doubles (cam_stride 0 or >= 16); layouts, stream / lane / hipGraph
 * behaviour and the 2 GiB limits are those of R3D_INPUT_UV_DIST; r3d_forward (pos or trj alone) and r3d_forward_pair take
 * them with every window_stride.  Rounding contract of both: the float32 pixels are promoted to float64, the expressions
 * below are evaluated in float64 in the written operation order with IEEE division, and the result is cast ONCE to float32
 * (lib/train_val/trainer.py:298).
 *   R3D_INPUT_PX_INTRINSIC replaces CameraInfoPacket.encode_uv_with_intrinsic (lib/camera/camera.py:423-441, called at load
 *     time from lib/dataset/__init__.py:180-189 when INTRINSIC_ENCODING is set): the undistortion of R3D_INPUT_UV_DIST
 *     (skipped for rows whose five coefficients are 0: undistort=False), then ((u - cx) / fx, (v - cy) / fy).  Slots 4-7 of
 *     the row are not read.
 *   R3D_INPUT_PX_SCREEN replaces normalize_screen_coordinates (lib/camera/camera.py:11-18, called from
 *     lib/dataset/__init__.py:167-178): no undistortion - the reference normalises raw pixels - and
 *     (u / w * 2 - 1, v / w * 2 - h / w) with w = res_w, h = res_h from slots 6 / 7 of the row (both must be set; the
 *     other slots are not read).  The reference evaluates `X / w * 2` in the dtype of the keypoint archive it loaded, so
 *     its own result depends on whether that archive is float32 or float64; this mode is the float64 evaluation, i.e. it
 *     equals the reference bit for bit (before the cast) for a float64 archive holding these pixels. */
#define R3D_INPUT_PX_INTRINSIC 3
#define R3D_INPUT_PX_SCREEN 4

typedef struct {
    int32_t mode;          /* R3D_INPUT_RAYS | R3D_INPUT_UV | R3D_INPUT_UV_DIST | R3D_INPUT_PX_INTRINSIC | R3D_INPUT_PX_SCREEN */
    const float *x_dev;    /* RAYS: float32 (frames, J, F);  UV, UV_DIST, PX_*: float32 (frames, J, 2) pixels */
    int64_t window_stride; /* frames between the starts of consecutive windows:
                              RF for a (B,RF,J,F) batch (lib/train_val/trainer.py:47-58 output),
                              1 to slide over an edge-padded clip in place (replaces
                              eval_data_prepare: window i = frames [i, i+RF))                */
    const float *param_dev;/* float32 [height, pitch] rows (lib/train_val/trainer.py:297);
                              ignored (may be NULL) when the camera embedding is off         */
    int64_t param_stride;  /* floats between consecutive windows' rows: extrinsic_dim for a
                              (B,E) tensor, 0 to broadcast one row to every window           */
    const double *cam_dev; /* UV mode only: float64 rows {fx, fy, cx, cy, cos(pitch),
                              sin(pitch), 0, 0} (lib/camera/camera.py:423-471);
                              UV_DIST: rows of 16 doubles {fx, fy, cx, cy, cos(pitch), sin(pitch), 0, 0,
                              k1, k2, p1, p2, k3, 0, 0, 0} (dist_coeff order of h36m_dataset.py:378-380);
                              PX_INTRINSIC, PX_SCREEN: the same 16 doubles with slots 6 / 7 = {res_w, res_h}, the
                              image size in pixels (read by PX_SCREEN only; UV and UV_DIST never read them)      */
    int64_t cam_stride;    /* doubles between consecutive windows' rows: 8 (UV_DIST, PX_*: >= 16), or 0 = broadcast */
} r3d_input;

/* Bytes of scratch HBM that suffice for every forward of AT MOST B windows (either model may be NULL): the maximum over
 * the launch plans calls of 1..B windows can select (small calls run less fused plans with larger intermediates), so a
 * caller may size its workspace once for its largest batch.
 * Exactly this many bytes are enough: a forward reads and writes nothing past workspace_dev + workspace_bytes, and a
 * call of B windows given fewer than r3d_workspace_bytes(B) bytes returns R3D_ERR_WORKSPACE before anything is launched.
 * `workspace_dev` must be 256-byte aligned (the library rounds its regions to 256 bytes relative to that base).  The
 * float pointers of a call - x_dev, param_dev, out_dev, out_trj_dev - need the 4-byte alignment of their type and no
 * more (a slice x + k windows of a larger tensor is fine as it is: what reads them several floats at a time does so
 * with buffer loads, which need dword alignment only); cam_dev the 8 bytes of a double.  Each buffer is
 * read or written inside its stated extent only: x_dev the (B - 1) * window_stride + RF frames of the call, param_dev
 * and cam_dev B rows (one row with stride 0), out_dev / out_trj_dev B rows.
 * The workspace is scratch: nothing in it has to survive between calls, the caller may use it for something else
 * between them, and what it holds when a call starts - zeros, NaN, anything - has no effect on the outputs.  (What a
 * forward needs ACROSS calls - the ready counters and the bound problem table of the single-launch forward, and for
 * calls of <= 16 windows two banks of activations - lives in device memory the library owns, per cached batch size.)
 * A forward that is being captured into a hipGraph keeps all of that inside the workspace instead and sets it up
 * inside the graph on every replay.  So a graph's workspace must exist, and be left alone by other work, WHILE the
 * graph runs - as any captured buffer; BETWEEN replays it may hold anything, like the workspace of an eager call. */
size_t r3d_workspace_bytes(const r3d_model *pos, const r3d_model *trj, int64_t B);

/* ... for forwards of AT MOST B windows with inputs shaped as `in` (mode, window_stride and cam_stride are read; the pointers
 * are not): r3d_workspace_bytes for R3D_INPUT_RAYS and R3D_INPUT_UV; for R3D_INPUT_UV_DIST that plus the ray buffer of the
 * pre-pass, which starts at r3d_workspace_bytes(B) rounded up to 256 bytes; for R3D_INPUT_PX_INTRINSIC / _SCREEN the same
 * with 2 floats per point instead of 3.  A forward of these modes given less returns R3D_ERR_WORKSPACE.  0 on bad
 * arguments (r3d_last_error says which). */
size_t r3d_input_workspace_bytes(const r3d_model *pos, const r3d_model *trj, const r3d_input *in, int64_t B);

/* Everything a forward of B windows needs besides its arguments - the launch plan of the pair and the tile schedule
 * of this batch size, uploaded - so that the forward itself only enqueues kernels (hipGraph capture, latency).
 * Either model may be NULL.
 * Lifetime rule: the library caches the tile schedules (device memory) of the 64 most recently used batch sizes per
 * pair and frees the least recently used one beyond that - EXCEPT sizes named in r3d_prepare, which stay resident
 * until r3d_release (or until either model is destroyed): a hipGraph that captured a forward holds pointers into its
 * size's schedule and never calls the library again, so prepare every size you capture and release it only after the
 * graph is destroyed.  Never call r3d_prepare / a first forward of a new size while a stream is capturing.
 * A captured forward also holds the handle's status word (pinned host memory, freed by r3d_destroy): destroy every
 * graph that captured a forward of a handle BEFORE the handle - a replay after r3d_destroy writes to freed memory. */
int r3d_prepare(r3d_model *pos, r3d_model *trj, int64_t B);
int r3d_release(r3d_model *pos, r3d_model *trj, int64_t B);   /* un-pins the size; R3D_ERR_ARG if it was never prepared */

/* One network, exactly the reference module's forward:
 *   pos: out_dev (B,1,J,3)   lib/model/rie.py:284-434
 *   trj: out_dev (B,1,1,3)   lib/model/rie.py:518-559
 * Non-finite input (a detector's NaN / Inf for a missed joint; any NaN payload, signalling ones included), in every input
 * mode and for r3d_forward_pair alike: an element of x_dev, param_dev or a pixel coordinate that is NaN or +-Inf makes every
 * output of the windows that read it NaN (non-finite at least) - as the reference's forward does - and leaves every other
 * window's output bits exactly what they are without it.  It is not an error: nothing is reported through r3d_status, and
 * the call takes no longer than on finite input (tests/test_gpu_nonfinite.py).
 * Size limits of one forward (r3d_forward, r3d_forward_pair, r3d_forward_pair_split; every input mode).  With
 * frames = (B - 1) * window_stride + RF and J = num_joints, a call is refused with R3D_ERR_ARG ("B too large for one call"),
 * before any HIP call, unless all of
 *   frames * J * 3 * 4 < 2^31 - 1   the raw input, counted at three floats per keypoint whatever the mode: the first-level
 *                                   gathers address it through one buffer descriptor with 32-bit byte offsets;
 *   B * (RF / 3)       < 2^31 - 1   the rows of the first level (a problem's row count is an int);
 *   B * RF * J * 3 * 4 < 2^31 - 1   R3D_INPUT_UV_DIST / PX_* with cam_stride != 0 and window_stride < RF only: the windows
 *                                   the pre-pass materialises
 * hold ("the 2 GiB limits").  Workspace buffers may be of any size: they are addressed from 64-bit tile bases.  One buffer is
 * not: the per-frame buffer of a clip call (window_stride 1, one camera) is read with 32-bit byte offsets, so a
 * call whose frames * (floats per frame of that buffer) * 4 reaches 2^32 - 1 bytes runs the gathered first levels instead -
 * the same poses to rounding, more arithmetic; nothing is refused. */
int r3d_forward(r3d_model *m, const r3d_input *in, int64_t B, float *out_dev,
                void *workspace_dev, size_t workspace_bytes, void *hip_stream);

/* Both networks in one pass over the input: out_dev (B,1,J,3) = pos + trj broadcast over
 * joints (lib/train_val/trainer.py:337,346,353); out_trj_dev (B,1,1,3) optional (may be NULL). */
int r3d_forward_pair(r3d_model *pos, r3d_model *trj, const r3d_input *in, int64_t B,
                     float *out_dev, float *out_trj_dev, void *workspace_dev,
                     size_t workspace_bytes, void *hip_stream);

/* r3d_forward_pair with the two networks' outputs kept apart, for callers that follow the reference's evaluation to the
 * letter (lib/train_val/trainer.py:337-353): it calls pos(x), pos(x_flip), trj(x), trj(x_flip), averages the flip pass
 * per network and only then adds the trajectory to the pose - so it needs both outputs of one pass separately.
 *   out_pos_dev (B,1,J,3): the pos network alone;  out_trj_dev (B,1,1,3): the trj network - required.
 * Everything else is r3d_forward_pair: the same plan, tile schedule, launches and r3d_workspace_bytes, every input mode and
 * window_stride, the single-launch / staged / bf16x3 / <= 32-window forms, the hipGraph capture and lanes rules, the
 * non-finite-input contract, and R3D_ERR_ABORTED through r3d_status with BOTH outputs NaN.  Only the decode kernel's last
 * add differs (a mode of the same two kernels).  Either model NULL or either output NULL: R3D_ERR_ARG, before any HIP call.
 * Contract:
 *   - out_trj_dev has the bits of r3d_forward_pair's out_trj_dev;
 *   - out_pos_dev + out_trj_dev (a float32 add, the trajectory broadcast over the joints) has the bits of r3d_forward_pair's
 *     out_dev: (v + bj) + 0 followed by + trj rounds like (v + bj) + trj;
 *   - against r3d_forward(pos, ...) alone the plan and the order of summation differ: out_pos_dev agrees with it within the
 *     library's usual bound against the reference, not bit for bit. */
int r3d_forward_pair_split(r3d_model *pos, r3d_model *trj, const r3d_input *in, int64_t B,
                           float *out_pos_dev, float *out_trj_dev, void *workspace_dev,
                           size_t workspace_bytes, void *hip_stream);

/* ---- errors of a forward that surface on the device; per-handle options ---- */

/* The reference's seam reports errors as Python exceptions.  A forward is asynchronous, so what can only
 * be found out on the device is reported here: r3d_status synchronises `hip_stream` and returns R3D_ERR_ABORTED when a
 * forward of this handle (for a pair: ask the pos handle) since the last call gave up waiting for its own tiles - the
 * single-launch forward needs all its workgroups resident, which another process's persistent kernel on the same GPU or
 * a CU mask can prevent; such a forward ends after the spin timeout with NaN outputs, never hangs.  The flag is cleared
 * by the call.  Remedy: R3D_OPT_STAGED (the Python mirror's checked entry points do exactly that, once, before raising). */
int r3d_status(r3d_model *m, void *hip_stream);

#define R3D_OPT_STAGED 1          /* value != 0: this handle's forwards run as one launch per level of the network (no
                                   * co-residency assumption; a few percent slower) instead of one persistent launch    */
#define R3D_OPT_SPIN_TIMEOUT_MS 2 /* how long a tile of the single-launch forward waits for its producers before the
                                   * forward gives up (default 1000)                                                    */
#define R3D_OPT_CU_LIMIT 3        /* value = n > 0: this handle's forwards are launched on a CU-masked stream that can use n CUs
                                   * (hipExtStreamCreateWithCUMask): the single-launch forward uses at most n workgroups and is
                                   * NOT ordered against masked forwards of OTHER streams (two half-chip forwards side by side:
                                   * DESIGN.md 5.2).  The caller guarantees:
                                   *  - streams used concurrently have DISJOINT masks;
                                   *  - a mask enables at least ceil(n / 8) CUs in EVERY XCD (workgroups are dealt round-robin to
                                   *    the eight XCDs: n enabled CUs anywhere are not enough for n co-resident workgroups);
                                   *  - one handle (pair) per masked stream: a handle has ONE control region; used on a second
                                   *    masked stream its forwards are ordered behind those on the first one.
                                   * The library orders whole-device forwards (n = 0 handles) behind every masked forward issued
                                   * before them and masked forwards behind the last whole-device forward, so the two kinds never
                                   * share the chip.  A violated guarantee ends in the bounded spin (R3D_OPT_SPIN_TIMEOUT_MS), NaN
                                   * outputs and R3D_ERR_ABORTED from r3d_status - never in a hang.  0 (default): the whole device.
                                   * Changing the value waits for the handle's device and drops its cached tile schedules; it
                                   * fails with R3D_ERR_STATE while the handle has prepared (pinned) schedules - r3d_release them
                                   * first.  For a pair set it on both handles.                                              */
#define R3D_OPT_LANES 4           /* value = n in {2, 4} (0 / 1: off): the LIBRARY creates n CU-masked streams on the handle's device -
                                   * lane k: the CUs c of every XCD with c % n == k, so every lane spans all eight XCDs - each with
                                   * its own tile schedules and control regions; the packed weights stay ONE image per handle.  n
                                   * independent forwards then share the chip side by side (a level that holds 192 - 224 tiles
                                   * leaves a quarter of 256 CUs idle and runs as two full rounds on 128): the throughput mode for
                                   * callers with independent batches in flight - the clip evaluation has 240 clips
                                   * (lib/train_val/trainer.py:295-353).  How a forward finds its lane:
                                   *  - `stream` IS a lane's stream (r3d_lane_stream): it runs there, in order with whatever else the
                                   *    caller enqueues on that stream (the metrics of the clip, ...);
                                   *  - any other stream: lanes are served round-robin; the lane's stream waits for everything the
                                   *    caller's stream holds so far, runs the forward, and the caller's stream sees the outputs
                                   *    after r3d_lanes_join(m, stream) - NOT at return as without lanes.
                                   *    Until that join the forward's inputs, workspace and outputs belong to the lane: the
                                   *    caller's stream must not overwrite or free them (it is not ordered behind the lane).
                                   *    (a caller on the LEGACY DEFAULT stream: the lanes' streams are blocking streams - they are
                                   *    behind the default stream's work without an event, and none is recorded there, because an
                                   *    event on the default stream is behind every blocking stream's work: the lanes would take
                                   *    turns.  For the same reason any work issued on the default stream between two lanes'
                                   *    forwards serialises them - drive a lane loop from a stream of your own.)
                                   * One workspace per lane in flight (the caller's, as always).  Set it on both handles of a pair,
                                   * after r3d_finalize; it waits for the device, drops cached schedules and fails with
                                   * R3D_ERR_STATE while prepared (pinned) schedules exist.  r3d_prepare prepares every lane.
                                   * hipGraphs: a forward issued on a lane's OWN stream can be captured there (after r3d_prepare); a
                                   * forward on a capturing stream that is no lane's would have to be relayed inside the capture
                                   * and is refused with R3D_ERR_STATE.
                                   * Abort contract as without lanes: a lane's forward that cannot get its workgroups resident
                                   * ends in NaN outputs and R3D_ERR_ABORTED from r3d_status (which waits for the lanes too).    */
int r3d_set_option(r3d_model *m, int32_t option, int64_t value);

/* R3D_OPT_LANES: the stream of lane `lane` (0 .. n - 1) of the handle (for a pair: the pos handle's lanes are the pair's) - a
 * hipStream_t the library owns; replaces nothing in the reference (its evaluation loop is sequential: trainer.py:295-353). */
int r3d_lane_stream(r3d_model *m, int32_t lane, void **stream);
/* ... and: make `stream` wait (device-side) for every forward that was relayed to a lane and not joined yet by the stream that
 * issued it.  Afterwards the forwards `stream` itself issued count as joined; those of other streams still wait for THEIR join. */
int r3d_lanes_join(r3d_model *m, void *stream);

/* ---- instrumentation (bench.py / tests) ---- */

/* When enabled, the next forward brackets every kernel launch with hipEvents on the launch
 * stream; r3d_profile_read then synchronises and returns per-launch records.  The first record
 * ("r3d_event_pair", stage -1) is an empty bracket: the cost of the two event records themselves,
 * which every other record's `ms` includes. */
typedef struct {
    char kernel[48];  /* kernel family name as rocprofv3 shows it (prefix)                  */
    int32_t stage;    /* position in the launch sequence                                     */
    int32_t blocks;   /* workgroups launched                                                 */
    float ms;         /* elapsed milliseconds between the bracketing events                  */
    double flops;     /* algorithmic FLOPs (2*M*K*N over the reference's layers) in launch   */
    double bytes;     /* algorithmic HBM bytes (operands read once + result written once)    */
} r3d_launch_record;
int r3d_profile_enable(r3d_model *m, int on);
int r3d_profile_read(r3d_model *m, r3d_launch_record *records, int capacity);

/* The shader clock the handle's last single-launch forward ran at, in GHz (for a pair: ask the pos handle): the kernel's
 * first workgroup stamps its cycle counter and the 100 MHz wall clock at both ends.  Synchronises `hip_stream`.  The
 * first forwards after an idle period run below the clock a busy chip settles at, so a roofline wants it
 * next to the rate (north_star: counters against the gfx950 peak - there is no reference counterpart).  *ghz = 0 when the last forward ran level by level (R3D_OPT_STAGED, plans the single launch
 * cannot hold) or none ran yet. */
int r3d_last_clock(r3d_model *m, void *hip_stream, double *ghz);

/* ---- per-clip error sums: the host side of Trainer.evaluate_core after the forward ---- */

/* lib/train_val/trainer.py:355-397 for one clip: prediction and ground truth (float32, (n_frames, J, 3), normalised
 * frame, device memory) go to world coordinates in float64 (camera.py:401-410: p @ Rn2w^T + Tn2w^T; `rn2w` is the
 * row-major 3x3 Rn2w, `tn2w` its translation, host pointers), then
 *   out[R3D_METRIC_MPJPE]    = sum over frames of mean_j |pred - gt|                (loss.py:12-18,  trainer.py:386)
 *   out[R3D_METRIC_PMPJPE]   = ... after the per-frame similarity (Procrustes) fit  (loss.py:30-69,  :393)
 *   out[R3D_METRIC_NMPJPE]   = ... after the per-frame scale fit                    (loss.py:72-82,  :388)
 *   out[R3D_METRIC_VELOCITY] = n_frames * mean |first difference of the error|      (loss.py:95-104, :395; NaN if n < 2)
 *   out[R3D_METRIC_ROOT]     = sum over frames of |pred - gt| of joint 0                             (:387)
 * i.e. the clip's contribution to each epoch_loss_* accumulator, in metres.  `out_dev` is device memory of
 * R3D_METRIC_OUT_DOUBLES doubles: the five sums first, the rest is scratch for the workgroups' partial sums.
 * Deterministic (fixed summation order); enqueued on `stream`, no synchronisation. */
#define R3D_METRIC_MPJPE 0
#define R3D_METRIC_PMPJPE 1
#define R3D_METRIC_NMPJPE 2
#define R3D_METRIC_VELOCITY 3
#define R3D_METRIC_ROOT 4
#define R3D_METRIC_COUNT 5
#define R3D_METRIC_MAX_BLOCKS 128
#define R3D_METRIC_OUT_DOUBLES (R3D_METRIC_COUNT * (1 + R3D_METRIC_MAX_BLOCKS))
int r3d_clip_metrics(const float *pred_dev, const float *gt_dev, int64_t n_frames, int32_t num_joints,
                     const double *rn2w, const double *tn2w, double *out_dev, void *stream);

/* The same call (same arguments, checks and five sums in `out_dev`, bit for bit) that also keeps what those sums are made
 * of.  It extends trainer.py:386-397 and loss.py:30-69; the reference has no counterpart - it reports the five clip means
 * only - so the quantities below are this project's definition, all in the world frame, float64, metres:
 *   frame_dev (optional, may be NULL): (n_frames, R3D_METRIC_COUNT) doubles, row f = the frame's MPJPE, P-MPJPE, N-MPJPE,
 *     mean_j |first difference of the error| against frame f+1 (0.0 in the last row) and root-joint error, i.e. the
 *     terms of the five sums (the velocity sum is the column's sum times n/(n-1)).
 *   detail_dev: R3D_DETAIL_OUT_DOUBLES doubles; the first R3D_DETAIL_DOUBLES are the results, the rest is scratch for the
 *     workgroups' partial rows.  Results: R3D_DETAIL_JOINT_ROWS rows of R3D_DETAIL_MAX_JOINTS columns (columns >=
 *     num_joints are 0), each the sum over frames of a per-joint distance -
 *       row 0: |pred_j - gt_j|
 *       row 1: the same after the frame's similarity (Procrustes) fit: the per-joint term P-MPJPE averages
 *       row 2: root-relative, |(pred_j - pred_0) - (gt_j - gt_0)|
 *     then R3D_DETAIL_THRESHOLDS counts (exact integers stored as doubles): count[k] = the number of (frame, joint)
 *     pairs with joint >= 1 whose root-relative distance is STRICTLY below 0.005 * k metres, k = 0..30 (0, 5, ..., 150 mm;
 *     count[0] is 0).  The root joint - distance 0 by construction - is excluded: a caller that counts it adds n_frames
 *     to every count with k >= 1.  PCK at a threshold is count / (n_frames * joints counted), PCK@150mm the last one (the
 *     headline figure of MPI-INF-3DHP), AUC the mean of PCK over the R3D_DETAIL_THRESHOLDS thresholds.
 * Deterministic (fixed summation order, integer counts); enqueued on `stream`, no synchronisation. */
#define R3D_DETAIL_THRESHOLDS 31
#define R3D_DETAIL_JOINT_ROWS 3
#define R3D_DETAIL_MAX_JOINTS 17
#define R3D_DETAIL_DOUBLES (R3D_DETAIL_JOINT_ROWS * R3D_DETAIL_MAX_JOINTS + R3D_DETAIL_THRESHOLDS)
#define R3D_DETAIL_OUT_DOUBLES (R3D_DETAIL_DOUBLES * (1 + R3D_METRIC_MAX_BLOCKS))
int r3d_clip_metrics_detail(const float *pred_dev, const float *gt_dev, int64_t n_frames, int32_t num_joints,
                            const double *rn2w, const double *tn2w, double *out_dev, double *frame_dev, double *detail_dev,
                            void *stream);

/* ---- a whole shard of clips in one call ---- */

/* lib/train_val/trainer.py:355-403 for every clip of a shard at once: r3d_clip_metrics / r3d_clip_metrics_detail over a table of
 * clips that lives in DEVICE memory (uploaded once per data set; the host never sees a descriptor during the call), in exactly
 * two kernel launches on `stream` - no copy, no allocation, no synchronisation.  pred_dev and gt_dev are (total_frames, J, 3)
 * float32; clip c is rows [first_frame, first_frame + n_frames) of both (and of frame_dev), measured through ITS rigid
 * transform (rn2w row-major, tn2w: as r3d_clip_metrics takes them).  Clips may lie in the buffers in any order, with gaps;
 * the velocity term never crosses a clip's end.
 *   rows_dev:   clip c's five sums (R3D_METRIC_* order) at rows_dev + c * row_stride, row_stride >= R3D_METRIC_COUNT: a
 *               pointer to column 3 of a (k, 8) matrix of partial rows and stride 8 fills columns 3..7 in place; nothing else
 *               of the matrix is written.
 *   detail_dev: optional (NULL: none): clip c's R3D_DETAIL_DOUBLES results at detail_dev + c * detail_stride,
 *               detail_stride >= R3D_DETAIL_DOUBLES.
 *   frame_dev:  optional (NULL: none): (total_frames, R3D_METRIC_COUNT) doubles, row first_frame + f the terms of the clip's
 *               frame f; rows no valid clip covers are left untouched.
 * BIT-FOR-BIT EQUALITY WITH THE PER-CLIP CALLS.  For every clip the five sums equal r3d_clip_metrics on that clip alone,
 * the detail row and the clip's rows of frame_dev equal r3d_clip_metrics_detail on that clip alone, bit for bit - the NaN
 * velocity of a one-frame clip and clips above R3D_METRIC_MAX_BLOCKS * 256 frames (where the per-clip call wraps around its
 * workgroups) included: both run one and the same workgroup body with the same frame-to-workgroup assignment and add the
 * partial rows in the same order.  A caller may switch between the two paths without its numbers moving.
 * GRID.  max_frames is the caller's bound on any clip's length and sizes the grid: (min(ceil(max_frames / 256),
 * R3D_METRIC_MAX_BLOCKS), num_clips) workgroups; a workgroup past its clip's own count returns at once.
 * INVALID DESCRIPTORS - THE WHOLE BOUNDS STORY.  A descriptor is invalid when n_frames < 1, n_frames > max_frames, or
 * [first_frame, first_frame + n_frames) is not inside [0, total_frames).  The kernels never follow an invalid descriptor:
 * nothing of that clip is read, its five sums and its detail row are all NaN, its rows of frame_dev are left untouched.
 * Beyond the descriptors the kernels read pred_dev / gt_dev within total_frames * num_joints * 3 floats, the table within
 * num_clips descriptors, and write the strided rows, frame_dev within total_frames rows and the scratch within
 * r3d_clips_metrics_scratch_bytes: no input can make them touch memory outside these extents.
 * SCRATCH.  The workgroups' partial rows: num_clips * min(ceil(max_frames / 256), R3D_METRIC_MAX_BLOCKS) *
 * (R3D_METRIC_COUNT + (detail ? R3D_DETAIL_DOUBLES : 0)) doubles - r3d_clips_metrics_scratch_bytes returns exactly that
 * (0 for num_clips < 1 or max_frames < 1), exactly that many bytes suffice, and what the scratch holds at entry has no effect
 * on the outputs.  With less the call returns R3D_ERR_WORKSPACE before anything is launched.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (pred_dev, gt_dev, clips_dev, rows_dev,
 * scratch_dev), num_clips outside 1..R3D_CLIPS_MAX, num_joints outside 1..17, max_frames < 1, total_frames < 1,
 * row_stride < R3D_METRIC_COUNT, detail_dev with detail_stride < R3D_DETAIL_DOUBLES, a table or scratch pointer that is
 * not 8-byte aligned.  Deterministic (fixed summation order, integer counts). */
typedef struct {
    int64_t first_frame;  /* row of the clip's first frame in pred_dev / gt_dev / frame_dev */
    int64_t n_frames;
    double  rn2w[9];      /* row-major, as r3d_clip_metrics takes it */
    double  tn2w[3];
} r3d_clip_desc;          /* 112 bytes, 8-byte aligned; lives in DEVICE memory */
#define R3D_CLIPS_MAX 65535 /* clips per call (the grid's second dimension) */
size_t r3d_clips_metrics_scratch_bytes(int32_t num_clips, int64_t max_frames, int detail);
int r3d_clips_metrics(const float *pred_dev, const float *gt_dev, int64_t total_frames, int32_t num_joints,
                      const r3d_clip_desc *clips_dev, int32_t num_clips, int64_t max_frames,
                      double *rows_dev, int64_t row_stride,          /* clip c: 5 sums at rows_dev + c*row_stride */
                      double *detail_dev, int64_t detail_stride,     /* optional (NULL): R3D_DETAIL_DOUBLES per clip */
                      double *frame_dev,                             /* optional (NULL): (total_frames, R3D_METRIC_COUNT) */
                      void *scratch_dev, size_t scratch_bytes, void *stream);

/* ---- a shard's model inputs from raw pixels: pad, encode and mirror every clip in one call ---- */

/* The input side of a clip evaluation on the device - the counterpart of what the reference does once per data set at load
 * time (lib/dataset/__init__.py:167-189: every sequence encoded) and per sequence in its generator
 * (lib/dataloader/generators.py:213-216: np.pad(..., 'edge')).  ONE launch turns a shard's raw pixel archive px_dev
 * (total_frames, J, 2) float32 into the edge-padded, encoded float32 inputs x_dev (out_rows, J, F) that a R3D_INPUT_RAYS
 * forward with window_stride 1 reads (F = 3 for R3D_ENCODE_RAY, 2 for the other two), clip by clip over a table of
 * descriptors in DEVICE memory.  Clip c writes output rows [out_first, out_first + pad_front + n_frames + pad_back); its
 * row r is the encoding of source frame first_frame + clamp(r - pad_front, 0, n_frames - 1) through the clip's camera row
 * `cam` (the 16 doubles of R3D_INPUT_UV_DIST / R3D_INPUT_PX_*).  pad_back may carry, on top of the receptive field's pad,
 * the surplus rows of a rounded-up batch size.  Rows that no valid clip covers are left untouched.  Clips may lie in the
 * buffers in any order, with gaps; overlapping OUTPUT ranges of two valid clips are the caller's error (either value may
 * win, nothing leaves the extents).
 *   x_mirror_dev / mirror_perm: both NULL, or both given: the flip pass's inputs (lib/train_val/trainer.py:299-302 on the
 *               ENCODED input - also right for distorted cameras, whose pixels have no exact mirror image):
 *               x_mirror_dev[row, j] = x_dev[row, mirror_perm[j]] with component 0 negated, same layout and extents as
 *               x_dev.  mirror_perm is a HOST array of J entries, a permutation of 0..J-1; it travels as a kernel argument.
 *   status_dev: num_clips int32 words, required: 0 for a clip that was followed, 1 for an invalid descriptor.
 * BIT-FOR-BIT WITH THE PRE-PASS.  Every value is what the pre-pass of a R3D_INPUT_UV_DIST / R3D_INPUT_PX_INTRINSIC /
 * R3D_INPUT_PX_SCREEN forward writes for that pixel and camera row: the same float64 routines, the same single cast to
 * float32 (zero coefficients: R3D_INPUT_UV's values).  A padding row is encoded again from the frame it repeats and has its
 * bits; the negation of the mirrored copy is exact.
 * GRID.  max_rows is the caller's bound on any clip's pad_front + n_frames + pad_back and sizes the grid:
 * (ceil(max_rows * num_joints / 256), num_clips) workgroups, one output point per thread; a workgroup past its clip's points
 * returns at once.
 * INVALID DESCRIPTORS - THE WHOLE BOUNDS STORY.  A descriptor is invalid when n_frames < 1, a pad is < 0, pad_front +
 * n_frames + pad_back > max_rows, [first_frame, first_frame + n_frames) is not inside [0, total_frames), or the output rows
 * are not inside [0, out_rows).  The kernel never follows an invalid descriptor: nothing of that clip is read or written,
 * status_dev[c] = 1.  Beyond the descriptors it reads px_dev within total_frames * num_joints * 2 floats and the table within
 * num_clips descriptors, and writes x_dev / x_mirror_dev within out_rows * num_joints * F floats and status_dev within
 * num_clips words: no input can make it touch memory outside these extents.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (px_dev, clips_dev, x_dev, status_dev),
 * num_clips outside 1..R3D_CLIPS_MAX, num_joints outside 1..17, an unknown encoding, max_rows, total_frames or out_rows < 1,
 * max_rows * num_joints, total_frames or out_rows above R3D_ENCODE_MAX_POINTS (index arithmetic), exactly one of
 * x_mirror_dev / mirror_perm, a mirror_perm that is not a permutation, a table pointer that is not 8-byte aligned.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
typedef struct {
    int64_t first_frame;  /* row of the clip's first frame in px_dev                       */
    int64_t n_frames;
    int64_t out_first;    /* row of the clip's first OUTPUT row in x_dev / x_mirror_dev     */
    int32_t pad_front;    /* output rows in front that repeat frame 0                       */
    int32_t pad_back;     /* output rows behind that repeat frame n_frames - 1              */
    double  cam[16];      /* the 16-double camera row of R3D_INPUT_UV_DIST / PX_*           */
} r3d_clip_input_desc;    /* 160 bytes, 8-byte aligned; lives in DEVICE memory */
#define R3D_ENCODE_RAY 0        /* 3 floats, as the R3D_INPUT_UV_DIST pre-pass writes them  */
#define R3D_ENCODE_INTRINSIC 1  /* 2 floats, R3D_INPUT_PX_INTRINSIC                          */
#define R3D_ENCODE_SCREEN 2     /* 2 floats, R3D_INPUT_PX_SCREEN                             */
#define R3D_ENCODE_MAX_POINTS 2147483391 /* 2^31 - 257: max_rows * num_joints (the grid), total_frames, out_rows */
int r3d_clips_encode(const float *px_dev, int64_t total_frames, int32_t num_joints, int32_t encoding,
                     const r3d_clip_input_desc *clips_dev, int32_t num_clips, int64_t max_rows,
                     float *x_dev, int64_t out_rows,
                     float *x_mirror_dev, const int32_t *mirror_perm,   /* both NULL: no mirrored copy */
                     int32_t *status_dev, void *stream);

/* ---- a shard's model inputs repaired: dropped keypoints held, back-filled and interpolated before the first forward ---- */

/* The archive-side counterpart of r3d_streams_repair.  One NaN keypoint in a shard's pixel archive makes r3d_clips_encode write a
 * non-finite input row, and by the non-finite contract every window that reads it comes out NaN.  This call repairs x_dev
 * (out_rows, J, F), F = 2 | 3, IN PLACE, enqueued behind r3d_clips_encode on the same stream with the same table, out_rows and
 * max_rows, before the first forward reads the buffer.  The reference's archives are complete, so the rule is this library's; an
 * archive knows both ends of every gap, so - unlike the live rule, which never revises an emitted window - every gap of at most
 * max_gap rows is interpolated from both sides and a late first observation is back-filled over the whole clip.
 * A clip's rows are its local rows r in [0, R), R = pad_front + n_frames + pad_back, starting at out_first; local row r belongs
 * to source frame first_frame + clamp(r - pad_front, 0, n_frames - 1), as in r3d_clips_encode.  The descriptors' `cam` is not read.
 * OBSERVED(r, j): every one of the F components of x_dev[out_first + r, j] is finite (judged on the exponent bits), and - with
 * conf_dev, (total_frames, J) float32 over SOURCE frames - conf[source frame, j] >= min_conf; a NaN confidence is not observed.
 * Only x_dev is judged, never the mirrored copy.
 * THE RULE per clip and joint, decided on the contents at entry.  O: the observed local rows of (clip, j).  A missing row r gets
 * (all F components):
 *   O empty:                                    the canonical quiet NaN 0x7FC00000                                   state 4
 *   r < min O:                                  the bits of row min O - the back-fill, the per-joint analogue of
 *                                               the front edge padding                                              state 3
 *   p = max{o in O, o < r}, q = min{o in O, o > r} exists and g = q - p - 1 <= max_gap:
 *                                               per component fl32(a + (e - a) * ((r - p) / (g + 1))) in float64,
 *                                               a = x[p], e = x[q], every operation rounded once, a NaN result the
 *                                               canonical quiet NaN: the routine, and the bits, of r3d_streams_repair  state 1
 *   otherwise:                                  the bits of row p - the hold                                        state 2
 * Observed points have state 0 and are NEVER written; a missing point's value depends on observed points only: the call is in
 * place and its result does not depend on any order of execution.
 *   x_mirror_dev / mirror_perm: both NULL, or both given (HOST perm), as in r3d_clips_encode: x_mirror_dev[row, dest(j)] of every
 *               REWRITTEN point gets the new value with the sign bit of component 0 turned (also of the canonical NaN), the
 *               other components bit for bit; points that were observed keep what r3d_clips_encode wrote.
 *   state_dev:  (out_rows, J) uint8 or NULL: the state of every point of every row of a followed clip.
 *   stats_dev:  (num_clips, J, 4) int32 or NULL: {interpolated, held, back-filled, never-observed} point counts over the clip's
 *               OWN frames only (pad_front <= r < pad_front + n_frames), exact integers; written whole for a followed clip -
 *               nothing needs to be zeroed beforehand.
 *   status_dev: num_clips int32 words, required: 0 for a clip that was followed, 1 for an invalid descriptor.
 * WHAT FOLLOWS.  A clip without a missing point is not written at all.  Padding rows repeat an edge frame, so the repair of a
 * padded clip is the padding of the repaired clip, bit for bit, whatever the pads (the surplus rows of a rounded-up batch
 * included).  If every joint of a clip was observed at least once, every value of the clip is finite afterwards - with ONE
 * exception: an interpolation between endpoints near FLT_MAX may round to an infinity.
 * ONE LAUNCH of the call's own kernel, r3d_k_clips_repair: (num_joints, num_clips)
 * workgroups of 256 threads.  A workgroup builds the bitmap of its clip-joint's observed rows in LDS (R3D_REPAIR_MAX_ROWS bits),
 * then every missing point finds p and q in it; the work per point is bounded by max_gap / 64 + 2 bitmap words whatever the
 * pattern.  No atomics.
 * INVALID DESCRIPTORS - THE WHOLE BOUNDS STORY.  A descriptor is invalid when n_frames < 1, a pad is < 0, R > max_rows, R >
 * R3D_REPAIR_MAX_ROWS, the output rows are not inside [0, out_rows), or - with conf_dev, the only thing read by source frame -
 * [first_frame, first_frame + n_frames) is not inside [0, total_frames) (without conf_dev first_frame is not read).  The kernel
 * never follows an invalid descriptor: status_dev[c] = 1 and nothing else of that clip is read or written.  No index comes from a
 * float: p and q are bit positions of a bitmap indexed by r < R <= R3D_REPAIR_MAX_ROWS, so rows p and q lie inside the clip; a
 * source frame is a clamped index of a descriptor that passed the rule.  Beyond the descriptors the call reads the table within
 * num_clips descriptors and conf_dev within total_frames * num_joints floats, and touches x_dev / x_mirror_dev within out_rows *
 * num_joints * F floats, state_dev within out_rows * num_joints bytes, stats_dev within num_clips * num_joints * 4 words and
 * status_dev within num_clips words: no input can make it touch memory outside these extents.  Overlapping OUTPUT ranges of two
 * valid clips are the caller's error, as in r3d_clips_encode.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (x_dev, clips_dev, status_dev), in_features
 * other than 2 or 3, num_joints outside 1..17, num_clips outside 1..R3D_CLIPS_MAX, max_rows outside 1..R3D_REPAIR_MAX_ROWS,
 * out_rows outside 1..R3D_ENCODE_MAX_POINTS, max_gap outside 0..R3D_REPAIR_MAX_ROWS, a min_conf that is not finite, conf_dev with
 * total_frames outside 1..R3D_ENCODE_MAX_POINTS, exactly one of x_mirror_dev / mirror_perm, a mirror_perm that is not a
 * permutation, a table pointer that is not 8-byte aligned, state_dev / stats_dev / status_dev / conf_dev / the table overlapping
 * x_dev or x_mirror_dev (address ranges), x_dev overlapping x_mirror_dev.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
#define R3D_REPAIR_MAX_ROWS 65536   /* rows (pad_front + n_frames + pad_back) of one clip */
int r3d_clips_repair(float *x_dev, int64_t out_rows, int32_t num_joints, int32_t in_features,   /* (out_rows, J, F), F = 2 | 3: IN PLACE */
                     float *x_mirror_dev, const int32_t *mirror_perm,    /* both NULL, or both given (HOST perm), as r3d_clips_encode */
                     const r3d_clip_input_desc *clips_dev, int32_t num_clips, int64_t max_rows,   /* the table r3d_clips_encode read */
                     const float *conf_dev, int64_t total_frames, float min_conf,   /* (total_frames, J) over SOURCE frames, or NULL */
                     int32_t max_gap,                                    /* 0 .. R3D_REPAIR_MAX_ROWS: longest gap that is interpolated */
                     uint8_t *state_dev,                                 /* (out_rows, J), may be NULL */
                     int32_t *stats_dev,                                 /* (num_clips, J, 4), may be NULL */
                     int32_t *status_dev, void *stream);                 /* (num_clips): 0 followed, 1 invalid descriptor */

/* ---- per-clip validation losses: Trainer.test after the forwards ---- */

/* lib/train_val/trainer.py:187-223 for one clip of n_frames frames, in the NORMALISED frame (no world transform): the
 * terms of losses_3d_valid - the figure that selects best_epoch.bin and is stored as `best_performance` (:235) - and of
 * the logged test_pos / test_trj / test_bone.  Device memory: pos_dev (n, J, 3) float32, the pos network's output;
 * trj_dev (n, 3) float32 or NULL (configurations without a trajectory model); gt_dev (n, J, 3) float32, the ABSOLUTE
 * ground truth in the frame of the predictions.  `parents` is a HOST array of J entries (parents[0] == -1, 0 <= parents[j]
 * < j otherwise; it travels as a kernel argument, nothing is copied to the device): bone j-1 is joint parents[j] minus
 * joint j, the column order of lib/skeleton/bone.py:51-68; NULL: no bone terms (they are 0).
 *   out[R3D_VALID_LOSS]      = sum_f mean_j |P_abs - G|                           (:216, without trj :220)
 *   out[R3D_VALID_POS]       = sum_f mean_j |pos - G_rel|                         (:200)
 *   out[R3D_VALID_TRJ_W]     = sum_f w_f d_f,  w_f = |1 / gt_root_z|, d_f = |trj - gt_root|   (weighted_mpjpe,
 *                              lib/loss/loss.py:21-27 with the weights of :119-120)
 *   out[R3D_VALID_TRJ_WSUM]  = sum_f w_f       out[R3D_VALID_TRJ_DSUM] = sum_f d_f
 *   out[R3D_VALID_BONE_LEN]  = sum_f mean_b | |bp| - |bg| |                       (bone.py:80-88,  :203-205)
 *   out[R3D_VALID_BONE_DIR]  = sum_f mean_b | bp/|bp| - bg/|bg| |                 (bone.py:91-100, :207-209)
 * then R3D_VALID_BONE_ROWS rows of R3D_VALID_MAX_BONES columns, out[R3D_VALID_COUNT + row * R3D_VALID_MAX_BONES + b], the
 * sums over frames of bone b's |len_p - len_g|, len_p, len_p^2 and len_g (columns >= J-1 and, without `parents`, all of
 * them are 0): per-bone error, mean lengths and the temporal deviation of a predicted bone's length.  Each sum is the
 * clip's contribution to an epoch accumulator of :200-222 (mean times frame count), in metres.
 * ROUNDING CONTRACT.  The reference takes its sums and differences in float32 before any norm; so does this call, with one
 * float32 rounding each:
 *   with trj_dev:            G_rel = fl32(gt_j - gt_0) with the root exactly 0 (:193-194), P_abs = fl32(pos + trj) (:215),
 *                            G = gt;
 *   R3D_VALID_POS_IS_SUM:    pos_dev holds what r3d_forward_pair writes (pos + trj): P_abs = pos_dev, and the
 *                            root-relative prediction is recovered as fl32(pos_dev - trj) - which differs from the
 *                            separately computed pos by at most one float32 rounding of the sum (2^-24 |pos + trj| per
 *                            coordinate, and as much again for the rounding of the difference);
 *   without trj_dev:         P_abs = pos, G = gt - or G_rel with R3D_VALID_GT_ROOT_RELATIVE (the models that are not fed
 *                            rays, :195-197); POS equals LOSS and the three TRJ sums are 0;
 *   bones:                   parent minus child, fl32, of `pos` and of G_rel as defined above (:203-204);
 *   differences prediction - target (and trj - gt_root): fl32.
 * Everything after these steps is float64: the values are promoted, norms, divisions (IEEE) and sums are float64.  A
 * zero-length bone or a zero root depth gives Inf / NaN exactly as the reference does; so does the empty bone mean of a
 * one-joint tree.
 * THE test_trj QUIRK.  Trainer.test passes the weights with shape (B,1) against a norm of shape (B,1,1) (:217-218):
 * broadcasting makes the product an outer product, so the figure it logs as test_trj is mean(w) * mean(d) of the clip, not
 * mean(w * d).  TRJ_W is the elementwise definition of Trainer.train (:119-120); TRJ_WSUM * TRJ_DSUM / n_frames is the
 * clip's contribution to the figure as logged.
 * `out_dev`: R3D_VALID_OUT_DOUBLES doubles, the R3D_VALID_DOUBLES results first, the rest scratch for the workgroups'
 * partial rows.  `frame_dev` (optional, may be NULL): (n_frames, R3D_VALID_COUNT) doubles, row f the frame's seven terms.
 * The inputs are only read (the reference overwrites its own in place, :193-194, :215).  R3D_ERR_ARG: a null required
 * pointer, n_frames < 1, num_joints outside 1..17, a bad parent table, unknown flags, POS_IS_SUM without trj_dev,
 * GT_ROOT_RELATIVE together with trj_dev.  Deterministic (fixed summation order, no atomics); enqueued on `stream`, no
 * synchronisation. */
#define R3D_VALID_POS_IS_SUM 1        /* flags */
#define R3D_VALID_GT_ROOT_RELATIVE 2
#define R3D_VALID_LOSS 0
#define R3D_VALID_POS 1
#define R3D_VALID_TRJ_W 2
#define R3D_VALID_TRJ_WSUM 3
#define R3D_VALID_TRJ_DSUM 4
#define R3D_VALID_BONE_LEN 5
#define R3D_VALID_BONE_DIR 6
#define R3D_VALID_COUNT 7
#define R3D_VALID_MAX_BONES 16
#define R3D_VALID_BONE_ROWS 4 /* per bone: sum |len_p - len_g|, sum len_p, sum len_p^2, sum len_g */
#define R3D_VALID_DOUBLES (R3D_VALID_COUNT + R3D_VALID_BONE_ROWS * R3D_VALID_MAX_BONES)
#define R3D_VALID_OUT_DOUBLES (R3D_VALID_DOUBLES * (1 + R3D_METRIC_MAX_BLOCKS))
int r3d_clip_valid_losses(const float *pos_dev, const float *trj_dev, const float *gt_dev, int64_t n_frames,
                          int32_t num_joints, const int32_t *parents, int32_t flags,
                          double *out_dev, double *frame_dev, void *stream);

/* lib/train_val/trainer.py:187-225 for every clip of a shard at once: what Trainer.test does per batch between its forwards and
 * its epoch accumulators - root-relative ground truth, the losses of :200-222 - as r3d_clip_valid_losses over the table of clips
 * r3d_clips_metrics reads (r3d_clip_desc, DEVICE memory; rn2w / tn2w are NOT read: the losses live in the normalised frame, so a
 * caller that both evaluates and validates uploads one table), in exactly two kernel launches on `stream` - no copy, no
 * allocation, no synchronisation (it can be captured into a hipGraph).  pos_dev and gt_dev are (total_frames, J, 3) float32,
 * trj_dev (total_frames, 3) float32 or NULL; clip c is rows [first_frame, first_frame + n_frames) of all three (and of
 * frame_dev).  Clips may lie in the buffers in any order, with gaps.  `parents` and `flags` are r3d_clip_valid_losses's, one tree
 * and one flag set per call; the rounding contract is that call's.
 *   rows_dev:   clip c's R3D_VALID_DOUBLES sums at rows_dev + c * row_stride, row_stride >= R3D_VALID_DOUBLES: a pointer to
 *               column 3 of a (k, 3 + R3D_VALID_DOUBLES) matrix of partial rows and that stride fills columns 3.. in place;
 *               nothing else of the matrix is written.
 *   frame_dev:  optional (NULL: none): (total_frames, R3D_VALID_COUNT) doubles, row first_frame + f the seven terms of the
 *               clip's frame f; rows no valid clip covers are left untouched.
 * BIT-FOR-BIT EQUALITY WITH THE PER-CLIP CALL.  For every valid clip the R3D_VALID_DOUBLES results and the clip's rows of
 * frame_dev equal r3d_clip_valid_losses on that clip alone, bit for bit - clips above R3D_METRIC_MAX_BLOCKS * 256 frames (where
 * the per-clip call wraps around its workgroups) and the Inf / NaN of a zero root depth, a zero-length bone or a one-joint tree
 * included: both run one and the same workgroup body, assign frames to workgroups from the clip's own n_frames and add the
 * partial rows in the same order.  A caller may switch between the two paths without its numbers moving.
 * GRID.  max_frames is the caller's bound on any clip's length and sizes the grid: (min(ceil(max_frames / 256),
 * R3D_METRIC_MAX_BLOCKS), num_clips) workgroups, then num_clips wavefronts; a workgroup past its clip's own count returns at once.
 * INVALID DESCRIPTORS - THE WHOLE BOUNDS STORY.  The rule of r3d_clips_metrics: a descriptor is invalid when n_frames < 1,
 * n_frames > max_frames, or [first_frame, first_frame + n_frames) is not inside [0, total_frames).  The kernels never follow an
 * invalid descriptor: nothing of that clip is read, its R3D_VALID_DOUBLES results are all NaN, its rows of frame_dev are left
 * untouched.  Beyond the descriptors the kernels read pos_dev / gt_dev within total_frames * num_joints * 3 floats, trj_dev
 * within total_frames * 3, the table within num_clips descriptors, and write the strided rows (R3D_VALID_DOUBLES doubles per
 * clip, nothing between rows), frame_dev within total_frames rows and the scratch within r3d_clips_valid_scratch_bytes: no
 * input can make them touch memory outside these extents.
 * SCRATCH.  The workgroups' partial rows: num_clips * min(ceil(max_frames / 256), R3D_METRIC_MAX_BLOCKS) * R3D_VALID_DOUBLES
 * doubles - r3d_clips_valid_scratch_bytes returns exactly that (0 for num_clips < 1 or max_frames < 1), exactly that many bytes
 * suffice, and what the scratch holds at entry has no effect on the outputs.  With less the call returns R3D_ERR_WORKSPACE
 * before anything is launched.
 * R3D_ERR_ARG (checked on the host before any HIP call): what r3d_clip_valid_losses rejects - a null required pointer (pos_dev,
 * gt_dev, rows_dev; here also clips_dev, scratch_dev), num_joints outside 1..17, a bad parent table, unknown flags, POS_IS_SUM
 * without trj_dev, GT_ROOT_RELATIVE together with trj_dev - what r3d_clips_metrics rejects - num_clips outside
 * 1..R3D_CLIPS_MAX, max_frames < 1, total_frames < 1, a table or scratch pointer that is not 8-byte aligned - and
 * row_stride < R3D_VALID_DOUBLES.  Deterministic (fixed summation order, no atomics). */
size_t r3d_clips_valid_scratch_bytes(int32_t num_clips, int64_t max_frames);
int r3d_clips_valid_losses(const float *pos_dev, const float *trj_dev, const float *gt_dev,
                           int64_t total_frames, int32_t num_joints,
                           const int32_t *parents, int32_t flags,          /* as r3d_clip_valid_losses: one tree, one flag set per call */
                           const r3d_clip_desc *clips_dev, int32_t num_clips, int64_t max_frames,
                           double *rows_dev, int64_t row_stride,           /* clip c: R3D_VALID_DOUBLES sums at rows_dev + c*row_stride */
                           double *frame_dev,                              /* optional (NULL): (total_frames, R3D_VALID_COUNT) */
                           void *scratch_dev, size_t scratch_bytes, void *stream);

/* ---- a shard's finished poses: flip average and world coordinates of every clip in one call ---- */

/* What lies between a shard's forwards and its measurement, on the device and in ONE launch: the flip average of
 * lib/train_val/trainer.py:340-346 and - what the reference hands to its renderer, Trainer.render, trainer.py:505-526 through
 * cam.normalized2world / cam.camera2world, lib/camera/camera.py:347-410 - the poses in world coordinates.  raw_dev and
 * raw_mirror_dev are (raw_rows, J, 3) float32: what the forwards wrote, the straight pass and the pass over the mirrored input.
 * Clip c is its row of the r3d_clip_desc table that r3d_clips_metrics reads (a caller uploads ONE table) and raw_first_dev[c], a
 * device array of num_clips int64: it reads raw rows [raw_first, raw_first + n_frames) - the rows behind them, up to the clip's
 * rounded-up call sizes, are surplus and are never read - and writes rows [first_frame, first_frame + n_frames) of pred_dev
 * (total_frames, J, 3) float32 and world_dev (total_frames, J, 3) float64; either output may be NULL, not both.  Clips may lie in
 * any order, with gaps, in both layouts.  A trajectory buffer (rows, 3) is the J = 1 case with mirror_perm = {0}.
 *   raw_mirror_dev / mirror_perm: both NULL, or both given.  mirror_perm is a HOST array of J entries, a permutation of 0..J-1
 *               (left and right joints trade places); it travels as a kernel argument.
 *   status_dev: num_clips int32 words, required: 0 for a clip that was followed, 1 for an invalid descriptor.
 * ROUNDING CONTRACT.  Per output point (frame, joint j), p its three float32 components:
 *   without raw_mirror_dev: p is the raw value, bits copied (NaN payloads included);
 *   with raw_mirror_dev:    m = raw_mirror[row, mirror_perm[j]] with component 0 negated (exact), p = fl32(fl32(raw + m) * 0.5f):
 *                           one float32 rounding each, in that operand order - the bits of
 *                           torch.add(dst, mirror_output(pred_m)); dst.mul_(0.5), the per-clip sequence it replaces;
 *   pred_dev receives p;
 *   world_dev is computed from that same p promoted to float64, whether or not pred_dev is given: component r is
 *                           ((R[3r] * x + R[3r+1] * y) + R[3r+2] * z) + T[r] with R = rn2w, T = tn2w of the clip's descriptor,
 *                           every product and every sum rounded once (no fused multiply-add: the one routine the kernel and the
 *                           host hook share is compiled with floating-point contraction off, so the two agree bit for bit).
 * A NaN that the arithmetic produces is stored as the canonical quiet NaN (float32 0x7fc00000, float64 0x7ff8000000000000).
 * NON-FINITE VALUES.  A NaN or Inf in a raw element makes exactly the output point(s) that read it non-finite - all three world
 * components of that point included - and every other output keeps the bits it would have had without it.  Not an error.
 * GRID.  max_frames is the caller's bound on any clip's length and sizes the grid: (ceil(max_frames * num_joints / 256),
 * num_clips) workgroups, one output point per thread; a workgroup past its clip's points returns at once.
 * INVALID DESCRIPTORS - THE WHOLE BOUNDS STORY.  A descriptor is invalid when n_frames < 1, n_frames > max_frames,
 * [first_frame, first_frame + n_frames) is not inside [0, total_frames), raw_first < 0, or raw_first + n_frames > raw_rows.  The
 * kernel never follows an invalid descriptor: nothing of that clip is read or written, status_dev[c] = 1.  Rows no valid clip
 * covers are left untouched.  Beyond the descriptors it reads raw_dev / raw_mirror_dev within raw_rows * num_joints * 3 floats,
 * the table within num_clips descriptors and raw_first_dev within num_clips words, and writes pred_dev / world_dev within
 * total_frames * num_joints * 3 elements and status_dev within num_clips words: no input can make it touch memory outside these
 * extents.  Overlapping output rows of two valid clips are the caller's error (either value may win, nothing leaves the extents).
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (raw_dev, clips_dev, raw_first_dev,
 * status_dev), both outputs null, exactly one of raw_mirror_dev / mirror_perm, a mirror_perm that is not a permutation,
 * num_clips outside 1..R3D_CLIPS_MAX, num_joints outside 1..17, max_frames, total_frames or raw_rows < 1, max_frames *
 * num_joints, total_frames or raw_rows above R3D_ENCODE_MAX_POINTS (index arithmetic), a table, raw_first_dev or world_dev
 * pointer that is not 8-byte aligned, an output extent (pred_dev, world_dev) that overlaps the extent of raw_dev or
 * raw_mirror_dev - compared as address ranges: in-place use is refused rather than given rules.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph).  The launch is of the
 * call's own kernel, r3d_k_clips_poses. */
int r3d_clips_poses(const float *raw_dev, const float *raw_mirror_dev, int64_t raw_rows, int32_t num_joints,
                    const int32_t *mirror_perm,                 /* HOST, J entries; given exactly when raw_mirror_dev is */
                    const r3d_clip_desc *clips_dev, const int64_t *raw_first_dev, int32_t num_clips, int64_t max_frames,
                    float *pred_dev, double *world_dev, int64_t total_frames,   /* either may be NULL, not both */
                    int32_t *status_dev, void *stream);

/* ---- a virtual-camera sweep's model inputs and ground truth from world poses: project, encode and mirror in one call ---- */

/* The input side of a synthetic camera sweep on the device - what the reference does per virtual camera on the host:
 * data/camera_augmentation.py:626-846 projects the world-frame ground truth through each camera of a grid
 * (CameraInfoPacket.project, lib/camera/camera.py:485-496, no distortion) and drops the cameras that put a keypoint outside the
 * frame (check_in_frame); lib/dataset/__init__.py:96-110, 191-203 then turns the pixels into the model's input
 * (get_cam_ray_given_uv / encode_uv_with_intrinsic / normalize_screen_coordinates) and the world poses into the frame of the
 * ground truth (world2normalized / world2camera).  ONE launch does all of it for every (clip, camera) pair of a table of
 * descriptors in DEVICE memory, from world_dev (total_frames, J, 3) float32 - the archive's world poses in metres, uploaded once:
 * many descriptors (one per camera) may name the same frames.  Descriptor c writes output rows [out_first, out_first + pad_front +
 * n_frames + pad_back) of x_dev (out_rows, J, F) float32 - what a R3D_INPUT_RAYS forward with window_stride 1 reads, F = 3 for
 * R3D_ENCODE_RAY and 2 for the other two - and, for its n_frames unpadded frames, rows [gt_first, gt_first + n_frames) of gt_dev
 * (gt_rows, J, 3) float32 and px_dev (gt_rows, J, 2) float64.  pad_front / pad_back are r3d_clip_input_desc's (pad_back may carry
 * the surplus rows of a rounded-up batch size).  Descriptors may lie in the buffers in any order, with gaps; overlapping OUTPUT
 * ranges of two valid descriptors are the caller's error (either value may win, nothing leaves the extents).
 * ARITHMETIC per output point (row r, joint j).  The source frame is first_frame + clamp(r - pad_front, 0, n_frames - 1); its
 * point (x, y, z) is promoted to float64.
 *   pixel:      h_k = ((P[4k] * x + P[4k+1] * y) + P[4k+2] * z) + P[4k+3] for k = 0, 1, 2 with P = proj, every product and every
 *               sum rounded once (no fused multiply-add: the routine the kernel and the host hook share is compiled with
 *               floating-point contraction off, as r3d_clips_poses's world transform is); u = h0 / h2, v = h1 / h2, IEEE
 *               divisions.  This is CameraInfoPacket.project on catesian2homogenous of the float32 pose.
 *   x_dev:      the FLOAT64 pixel through the routine r3d_clips_encode writes with, and the camera row `cam` (16 doubles, as
 *               R3D_INPUT_UV_DIST / R3D_INPUT_PX_*): the same float64 encoding, the same single cast to float32.  The reference's
 *               chain (lib/dataset/__init__.py:191-203, then lib/train_val/trainer.py:298) rounds to float32 there and nowhere
 *               before; a float32 pixel archive in between rounds once more.  Zero distortion coefficients are the synthetic
 *               sets' case (undistort=False); non-zero coefficients are simply followed.  A padding row is computed again from
 *               the frame it repeats and has its bits.
 *   x_mirror_dev / mirror_perm: both NULL, or both given: r3d_clips_encode's rule - x_mirror_dev[row, j] = x_dev[row,
 *               mirror_perm[j]] with component 0 negated (exact).  mirror_perm is a HOST array of J entries, a permutation of
 *               0..J-1; it travels as a kernel argument.
 *   gt_dev:     optional (NULL: none).  Written by the threads of rows pad_front <= r < pad_front + n_frames only, so every source
 *               frame once: gt_dev[gt_first + f, j], component k, is the float32 cast of ((R[3k] * x + R[3k+1] * y) + R[3k+2] * z)
 *               + T[k], R = rw2g, T = tw2g - the world -> normalised transform (Rw2n, Tw2n: world2normalized), or world -> camera
 *               (Rw2c, Tw2c: world2camera) for a ground truth in the camera frame - in the rounding of r3d_clips_poses's world_dev.
 *   px_dev:     optional (NULL: none), the same rows: (u, v) as float64.
 *   outside_dev: optional (NULL: none), num_clips int32: outside_dev[c] has ADDED to it the number of those points (rows pad_front
 *               <= r < pad_front + n_frames) with !(u >= 0 && u <= res_w && v >= 0 && v <= res_h), res_w / res_h slots 6 / 7 of
 *               `cam`.  The CALLER zeroes it.  Integer adds (one atomic per wavefront with a non-zero count): their order does
 *               not matter, the count is deterministic.  A NaN pixel counts as OUTSIDE - the reference's check_in_frame (`u < 0 or
 *               u > w or ...`) is false for a NaN and would call it inside.
 *   status_dev: num_clips int32 words, required: 0 for a descriptor that was followed, 1 for an invalid one.
 * A NaN that the arithmetic produces is stored as the canonical quiet NaN (float32 0x7fc00000, float64 0x7ff8000000000000).
 * NON-FINITE VALUES.  A NaN or Inf in a world element, a point in the camera's plane (h2 == 0: u, v = +-Inf or NaN) or behind it
 * makes exactly the outputs that read it non-finite (or, behind the camera, a mirrored pixel); every other output keeps the bits
 * it would have had without it.  Not an error.
 * GRID.  max_rows is the caller's bound on any descriptor's pad_front + n_frames + pad_back and sizes the grid:
 * (ceil(max_rows * num_joints / 256), num_clips) workgroups, one output point per thread; a workgroup past its clip's points
 * returns at once.
 * INVALID DESCRIPTORS - THE WHOLE BOUNDS STORY.  A descriptor is invalid when n_frames < 1, a pad is < 0, pad_front + n_frames +
 * pad_back > max_rows, [first_frame, first_frame + n_frames) is not inside [0, total_frames), the output rows are not inside
 * [0, out_rows), or - in a call that writes gt_dev or px_dev - [gt_first, gt_first + n_frames) is not inside [0, gt_rows) (without
 * the two, gt_first and gt_rows are not read).  The kernel never follows an invalid descriptor: nothing of it is read or written -
 * outside_dev[c] stays what the caller put there - and status_dev[c] = 1.  Rows no valid descriptor covers are left untouched.
 * Beyond the descriptors it reads world_dev within total_frames * num_joints * 3 floats and the table within num_clips
 * descriptors, and writes x_dev / x_mirror_dev within out_rows * num_joints * F floats, gt_dev within gt_rows * num_joints * 3
 * floats, px_dev within gt_rows * num_joints * 2 doubles and outside_dev / status_dev within num_clips words: no input can make
 * it touch memory outside these extents.
 * R3D_ERR_ARG (checked on the host before any HIP call): the rules of r3d_clips_encode - a null required pointer (world_dev,
 * clips_dev, x_dev, status_dev), num_clips outside 1..R3D_CLIPS_MAX, num_joints outside 1..17, an unknown encoding, max_rows,
 * total_frames or out_rows < 1, max_rows * num_joints, total_frames or out_rows above R3D_ENCODE_MAX_POINTS (index arithmetic),
 * exactly one of x_mirror_dev / mirror_perm, a mirror_perm that is not a permutation, a table pointer that is not 8-byte aligned -
 * and, with gt_dev or px_dev given, gt_rows < 1 or above R3D_ENCODE_MAX_POINTS; a px_dev that is not 8-byte aligned.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph).  The launch is of the
 * call's own kernel, r3d_k_clips_project. */
typedef struct {
    int64_t first_frame;  /* row of the clip's first frame in world_dev (many descriptors may name the same frames)        */
    int64_t n_frames;
    int64_t out_first;    /* first OUTPUT row in x_dev / x_mirror_dev (pad_front + n_frames + pad_back rows)                */
    int64_t gt_first;     /* first row in gt_dev / px_dev (n_frames rows, no padding)                                      */
    int32_t pad_front;    /* as r3d_clip_input_desc                                                                        */
    int32_t pad_back;
    double  proj[12];     /* P = K [R|t], row-major 3x4 (lib/camera/camera.py:231)                                         */
    double  cam[16];      /* the camera row r3d_clips_encode reads; slots 6 / 7 = res_w / res_h                            */
    double  rw2g[9];      /* row-major: world -> frame of the ground truth (Rw2n, or Rw2c for a camera-frame ground truth) */
    double  tw2g[3];
} r3d_clip_project_desc;  /* 360 bytes, 8-byte aligned; lives in DEVICE memory */
int r3d_clips_project(const float *world_dev, int64_t total_frames, int32_t num_joints, int32_t encoding,
                      const r3d_clip_project_desc *clips_dev, int32_t num_clips, int64_t max_rows,
                      float *x_dev, int64_t out_rows,
                      float *x_mirror_dev, const int32_t *mirror_perm,   /* both NULL or both given */
                      float *gt_dev, double *px_dev, int64_t gt_rows,    /* each optional (NULL) */
                      int32_t *outside_dev,                              /* optional (NULL) */
                      int32_t *status_dev, void *stream);

/* ---- a batch of materialised windows gathered from a pool of windows drawn from many clips ---- */

/* The step that lets a shard of SHORT clips be lifted in full, uniform batches of the plain (B, RF, J, F) forward: the reference's
 * np.pad(..., 'edge') (lib/dataloader/generators.py:213-216) plus eval_data_prepare (lib/train_val/trainer.py:47-58), for windows of
 * many clips at once, each with its camera-parameter row beside it - and, with one-window runs, ChunkedGenerator's (sequence, start,
 * flip) chunks.  src_dev holds model-input rows (total_frames, J, F) float32, F = 2 or 3: the rays of a data set, or what
 * r3d_clips_encode writes with pads 0.  The shard's windows form one POOLED list, cut into runs: run r is windows [win_first,
 * win_first + n_windows) of the list, all from one clip (source rows [first_frame, first_frame + n_frames)).  One call writes the
 * pooled windows [window0, window0 + batch) into x_dev (batch, RF, J, F) - what a R3D_INPUT_RAYS forward with window_stride = RF
 * reads - and their parameter rows into param_dev (batch, E).
 * ARITHMETIC (integers only; nothing rounds).  Pooled window g is looked up in the LAST run of the table with win_first <= g (run 0
 * when there is none): a table sorted by win_first, as evaluate.clip_window_table builds it, finds the run that holds g.  When that
 * run is valid and win_first <= g < win_first + n_windows, then with k = g - win_first row i (0 <= i < RF) of the window is source
 * frame first_frame + clamp(start + k * step + i, 0, n_frames - 1), in int64: the clamp IS the edge padding, no padded copy exists
 * anywhere.  Values are copied as 32-bit patterns, NaN payloads included.  A run with flip = 1 writes x[.., j, :] = src[..,
 * mirror_perm[j], :] with the sign bit of component 0 turned (the exact negation): r3d_clips_encode's rule, trainer.py:299-302.
 * param_dev[g - window0] = run_param_dev[r] (E 32-bit patterns).  Rows of x_dev / param_dev whose window no valid run holds are
 * left untouched.
 *   status_dev: num_runs int32 words, required.  Each window of the launch reports on the run it was looked up in: 1 when that
 *               descriptor is invalid, 0 when it is valid and holds the window; a valid run that does not hold the window is not
 *               reported on.  So every run with a window in [window0, window0 + batch) of a sorted table has its word written; the
 *               words of the other runs keep what they held.
 *   mirror_perm: HOST array of J entries, a permutation of 0..J-1, or NULL; it travels as a kernel argument.  Without it a flip
 *               run is invalid.
 * GRID.  (ceil(RF * J / 256), batch) workgroups, one output point (row, joint) per thread; the workgroup bisects the table and
 * validates the descriptor, uniformly, before any thread follows it.
 * INVALID DESCRIPTORS - THE WHOLE BOUNDS STORY.  A run is invalid when n_frames < 1, n_windows < 1, step < 1, flip is not 0 or 1,
 * flip is 1 and mirror_perm is NULL, [first_frame, first_frame + n_frames) is not inside [0, total_frames), win_first < 0,
 * n_windows > R3D_ENCODE_MAX_POINTS, start is outside [-R3D_ENCODE_MAX_POINTS, R3D_ENCODE_MAX_POINTS], or the last window's first
 * frame start + (n_windows - 1) * step exceeds R3D_ENCODE_MAX_POINTS (with these limits no product or sum of the index arithmetic
 * can overflow 64 bits).  The kernel never follows an invalid run: nothing of its clip is read, nothing is written for a window
 * that was looked up in it, its status word is 1.  Whatever the table holds - unsorted, overlapping, garbage - the bisection ends on
 * an index inside [0, num_runs), and that descriptor is validated like any other.  Beyond the descriptors the kernel reads src_dev
 * within total_frames * J * F floats, the table within num_runs descriptors and run_param_dev within num_runs * E words, and writes
 * x_dev within batch * RF * J * F floats, param_dev within batch * E words and status_dev within num_runs words: no input can make
 * it touch memory outside these extents.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (src_dev, runs_dev, x_dev, status_dev), num_runs
 * outside 1..R3D_CLIPS_MAX, num_joints outside 1..17, in_features other than 2 or 3, receptive_field < 1, total_frames < 1, batch
 * outside 1..65535 (the grid's second dimension), window0 outside [0, 2^62], receptive_field * num_joints, total_frames or batch *
 * receptive_field * num_joints above R3D_ENCODE_MAX_POINTS (index arithmetic), exactly one of run_param_dev / param_dev,
 * extrinsic_dim < 1 with run_param_dev given, a mirror_perm that is not a permutation, a table pointer that is not 8-byte aligned.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph).  The launch is of the
 * call's own kernel, r3d_k_clips_windows. */
typedef struct {
    int64_t first_frame;  /* row of the run's source clip in src_dev                                  */
    int64_t n_frames;     /* frames of that clip (>= 1)                                               */
    int64_t win_first;    /* index of the run's first window in the shard's pooled window list        */
    int64_t n_windows;    /* windows of the run (>= 1)                                                */
    int64_t start;        /* frame, relative to the clip's frame 0, of window 0's first frame; may be
                             negative: -(pad + causal_shift) for an evaluation clip                   */
    int32_t step;         /* frames between the starts of consecutive windows (>= 1; 1 for a clip)    */
    int32_t flip;         /* 0 | 1: the mirrored input (component 0 negated, joints permuted)         */
} r3d_window_run_desc;    /* 48 bytes, 8-byte aligned; lives in DEVICE memory */
int r3d_clips_windows(const float *src_dev, int64_t total_frames, int32_t num_joints, int32_t in_features,
                      int32_t receptive_field,
                      const r3d_window_run_desc *runs_dev, int32_t num_runs,
                      const float *run_param_dev, int32_t extrinsic_dim,   /* (num_runs, E) float32, or NULL / 0 */
                      int64_t window0, int64_t batch,                      /* pooled windows [window0, window0 + batch) */
                      float *x_dev,                                        /* (batch, RF, J, F) */
                      float *param_dev,                                    /* (batch, E), or NULL with run_param_dev */
                      const int32_t *mirror_perm,                          /* HOST, J entries; required if any run may flip */
                      int32_t *status_dev, void *stream);

/* ---- live streams lifted a frame at a time: a head and a ring of RF frames per stream, one call per tick ---- */

/* The input side of a LIVE caller: S streams (cameras) each deliver at most one new frame of J keypoints per tick and want the pose
 * of the newest frame their window is complete for.  The state - caller-owned DEVICE memory of r3d_streams_state_bytes bytes, 8-byte
 * aligned - holds S heads (r3d_stream_head) followed by S rings of (RF, J, F) float32; an all-zero state is S freshly reset streams.
 * One call advances every stream by its action word and writes, for every stream that emits a frame this tick, that frame's window
 * into row s of x_dev (S, RF, J, F) - what a R3D_INPUT_RAYS forward with window_stride = RF and batch = S reads: the reference's
 * np.pad(..., 'edge') (lib/dataloader/generators.py:213-216) plus eval_data_prepare (lib/train_val/trainer.py:47-58), one window
 * at a time, without a history buffer that grows and without re-encoding the RF - 1 frames the window shares with the last tick.
 *   frame_dev:  encoding R3D_ENCODE_RAY / R3D_ENCODE_INTRINSIC / R3D_ENCODE_SCREEN: (S, J, 2) float32 raw pixels; stream s's go
 *               through row s of cam_dev (S, 16) float64 - the camera rows of R3D_INPUT_UV_DIST / R3D_INPUT_PX_* - by the routine
 *               r3d_clips_encode writes with: the same bits; in_features is 3, 2, 2.  R3D_ENCODE_NONE: (S, J, F) float32
 *               model-input rows, F = in_features = 2 or 3, copied as 32-bit patterns, NaN payloads included; cam_dev may be NULL.
 *               Rows of streams that do not PUSH or RESTART this tick are not read.
 *   lag:        in [0, RF - 1]: the future frames a window needs - the reference's pad - causal_shift: 0 for a CAUSAL model (the
 *               pose of the newest frame), pad = (RF - 1) / 2 for a centred one (the pose of frame newest - pad).
 *   action_dev: S int32 words, R3D_STREAM_IDLE | R3D_STREAM_PUSH | R3D_STREAM_RESTART | R3D_STREAM_DRAIN.
 *   x_mirror_dev / mirror_perm: both NULL, or both given: x_mirror_dev[s, i, j] = x_dev[s, i, mirror_perm[j]] with the sign bit of
 *               component 0 turned (r3d_clips_windows's flip rule, trainer.py:299-302).  mirror_perm is a HOST array of J entries,
 *               a permutation of 0..J-1; it travels as a kernel argument.
 *   emit_dev:   S int64 words: the index (from 0, in PUSH order since the last RESTART) of the frame whose window was written into
 *               row s this tick, or -1.
 *   status_dev: S int32 words: 0 followed, 1 refused.
 * ARITHMETIC PER STREAM AND TICK (integers only; nothing rounds).  c is the head's count, k the drain step.
 *   IDLE     nothing happens (the head is not looked at): emit -1, status 0.
 *   PUSH     the new frame goes to ring slot c % RF; c += 1; k = 0.
 *   RESTART  the head is zeroed - whatever it held -, then the action is a PUSH: how a stream starts on a state that was not zeroed.
 *   DRAIN    c == 0 or drained == lag: a valid no-op, emit -1.  Otherwise drained += 1, k = drained: the stream has ended and
 *            the frames whose windows lack future frames are emitted one per tick, `lag` of them.
 * After a PUSH, RESTART or DRAIN that took effect n = c - 1 - lag + k.  n < 0: nothing is emitted, emit -1.  Otherwise emit = n and
 * row i of x_dev[s] is the ring's copy of frame clamp(n - (RF - 1 - lag) + i, 0, c - 1), found at slot frame % RF.  The clamp at 0
 * is the reference's front edge padding, the clamp at c - 1 (during a drain) its back edge padding; the oldest frame a window can
 * name is c - RF, which the ring still holds.  A stream fed N frames and then drained emits the frames 0 .. N - 1 once each, in order.
 * Rows of x_dev / x_mirror_dev of streams that emit nothing this tick are left untouched.
 * REFUSED STREAMS.  status 1, emit -1, and NOTHING else of the stream is written - not its head, not its ring, not its rows - when
 * the action word is unknown; when a PUSH comes after a drain began (drained > 0: RESTART starts the next clip); when the head a
 * PUSH or DRAIN meets is invalid: count < 0, count > 2^62, drained < 0 or drained > lag; when a PUSH meets count == 2^62 (the
 * counter is full).
 * TWO LAUNCHES, of the call's own kernels r3d_k_streams_advance and r3d_k_streams_gather.  Advance: S workgroups; each
 * reads and judges its stream's head and action uniformly, puts the J points of the new frame into the ring slot, and one thread
 * writes the head, emit and status.  Gather: (ceil(RF * J / 256), S) workgroups, one output point (row, joint) per thread, from the
 * head, emit and status words the advance launch wrote: no head is written by the launch other workgroups read it in.
 * THE WHOLE BOUNDS STORY.  Whatever the state and the action words hold, the kernel reads frame_dev, cam_dev and action_dev within
 * their S rows, and writes the state within r3d_streams_state_bytes, x_dev and x_mirror_dev within S * RF * J * F floats, emit_dev
 * and status_dev within S words: a ring slot is a remainder modulo RF of a non-negative number, a frame index is clamped into
 * [0, c - 1] of a head that passed the rule above, and the gather follows no head that fails it.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (state_dev, frame_dev, action_dev, x_dev, emit_dev,
 * status_dev), num_streams outside 1..R3D_CLIPS_MAX, num_joints outside 1..17, receptive_field < 1, lag outside [0,
 * receptive_field - 1], an unknown encoding, in_features that does not go with it, cam_dev NULL with a pixel encoding, exactly one
 * of x_mirror_dev / mirror_perm, a mirror_perm that is not a permutation, receptive_field * num_joints or num_streams *
 * receptive_field * num_joints above R3D_ENCODE_MAX_POINTS (index arithmetic), a state, emit_dev or cam_dev pointer that is not
 * 8-byte aligned.  r3d_streams_state_bytes returns 0 for shapes the call refuses.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
typedef struct {
    int64_t count;        /* frames pushed since the stream's last RESTART                            */
    int64_t drained;      /* DRAIN ticks that took effect since the last PUSH (0 .. lag)              */
} r3d_stream_head;        /* 16 bytes, 8-byte aligned; lives in DEVICE memory */
#define R3D_ENCODE_NONE 3       /* r3d_streams_step only: frame_dev holds model-input rows, copied bit for bit */
#define R3D_STREAM_IDLE 0
#define R3D_STREAM_PUSH 1
#define R3D_STREAM_RESTART 2
#define R3D_STREAM_DRAIN 3
size_t r3d_streams_state_bytes(int32_t num_streams, int32_t receptive_field, int32_t num_joints, int32_t in_features);
int r3d_streams_step(void *state_dev, int32_t num_streams, int32_t receptive_field, int32_t lag,
                     int32_t num_joints, int32_t in_features, int32_t encoding,
                     const float *frame_dev,          /* (S, J, 2) pixels, or (S, J, F) model-input rows        */
                     const double *cam_dev,           /* (S, 16) camera rows; NULL with R3D_ENCODE_NONE          */
                     const int32_t *action_dev,       /* (S) R3D_STREAM_IDLE | PUSH | RESTART | DRAIN            */
                     float *x_dev,                    /* (S, RF, J, F): stream s owns row s                      */
                     float *x_mirror_dev, const int32_t *mirror_perm,   /* both NULL, or both given (HOST perm)  */
                     int64_t *emit_dev,               /* (S) frame index of the window written this tick, or -1  */
                     int32_t *status_dev,             /* (S) 0 followed, 1 refused                               */
                     void *stream);

/* ---- a live tick's finished poses: flip average, world coordinates and a quality signal without ground truth, one call ---- */

/* The output side of a LIVE caller, between a tick's forward(s) and its consumer: for every stream that FINISHED a frame this tick -
 * status_dev[s] == 0 && emit_dev[s] >= 0, the words r3d_streams_step wrote - the flip average of lib/train_val/trainer.py:340-346,
 * the world transform every prediction gets (cam.normalized2world, lib/camera/camera.py:401-410; trainer.py:358-359, :514-523), and
 * the one check a stream without ground truth has: the predicted absolute pose taken back to the camera (normalized2camera,
 * camera.py:379-388), projected, and compared with the keypoints that were fed in (get_uv_given_cam_ray, camera.py:473-483 - the
 * overlay of trainer.py:535-537).  For every other stream nothing of rows s is read - apart from those two words - and nothing of
 * rows s is written in any output.
 *   raw_dev / raw_mirror_dev: (S, J, 3) float32, what the forward of x_dev and of x_mirror_dev wrote (pos + trj, normalised frame).
 *   mirror_perm: HOST array of J entries, a permutation of 0..J-1 (the output joints' left <-> right); given exactly when
 *               raw_mirror_dev is; it travels as a kernel argument.
 *   desc_dev:   S r3d_stream_pose_desc in device memory, 8-byte aligned: rn2w / tn2w as r3d_clip_desc, `height` the camera height
 *               in metres (Tc2n = (0, -height, 0), camera.py:340-343).  NULL only if world_dev and reproj_dev are NULL.
 *   cam_dev:    (S, 16) float64 camera rows (those of r3d_streams_step); slots 0, 1 (fx, fy) and 4, 5 (cos, sin of the pitch) are read.
 *   x_dev, receptive_field, lag: the (S, RF, J, 3) windows r3d_streams_step wrote this tick and its lag: row RF - 1 - lag of a
 *               window is the frame the pose belongs to (the step's clamp never touches it: 0 <= emit <= count - 1).  reproj_dev is
 *               defined for 3-feature (ray) inputs only.
 * ARITHMETIC PER FINISHED STREAM s, JOINT j.
 *   p           without a mirrored pass the bits of raw[s, j]; with one fl32(fl32(raw + m) * 0.5f), m = raw_mirror[s, mirror_perm[j]]
 *               with component 0 negated: r3d_clips_poses's rule, the bits of torch.add(...).mul_(0.5) in float32.
 *   pred_dev[s, j]  = p.
 *   world_dev[s, j] = rn2w p + tn2w in float64, p promoted; component r = ((R[3r] x + R[3r+1] y) + R[3r+2] z) + T[r], every product
 *               and every sum rounded once (r3d_clips_poses's rule).
 *   reproj_dev[s, j], float64, no contraction, c = cam[4], sn = cam[5], fx = cam[0], fy = cam[1], h = height:
 *               predicted  yy = (double)p[1] + h;  Xc = (double)p[0];  Yc = c * yy - sn * z;  Zc = sn * yy + c * z  (z = (double)p[2]);
 *                          a = Xc / Zc;  b = Yc / Zc  (IEEE divisions)
 *               observed   r = x_dev[s, RF - 1 - lag, j, 0..2];  xo = (double)r[0];  yo = c * r[1] - sn * r[2]  (the reference does
 *                          not divide by the third component either)
 *               residual   du = fx * (a - xo);  dv = fy * (b - yo);  reproj = sqrt(du * du + dv * dv), the correctly rounded sqrt:
 *               a distance in UNDISTORTED pixels; the principal point cancels and is not read.
 *   quality_dev[s]  word 0 the mean of row s of reproj (summed in joint order j = 0 .. J - 1 from zero, then one division by J),
 *               word 1 its maximum; both the canonical quiet NaN if any residual of the row is NaN.
 * NON-FINITE VALUES.  A NaN the arithmetic produces leaves as the canonical quiet NaN; raw bits that are only copied (pred_dev
 * without a mirrored pass) keep their payload.  A point behind the camera or in its plane (Zc <= 0) is simply followed, as
 * r3d_clips_project does: a mirrored, infinite or NaN residual, not an error.  A non-finite raw element touches its own point's
 * outputs and its stream's quality words, nothing else.
 * ONE LAUNCH of the call's own kernel, r3d_k_streams_poses: S workgroups of one wavefront;
 * each reads its stream's emit and status words uniformly before anything else; thread j < J finishes joint j; one thread sums the
 * residuals it finds parked in LDS.  Launch-latency-bound by construction.
 * THE WHOLE BOUNDS STORY.  Whatever emit_dev, status_dev, the descriptors and the inputs hold, the kernel reads emit_dev and
 * status_dev within S words, raw_dev / raw_mirror_dev within S * J * 3 floats (a mirrored joint is an entry of a checked
 * permutation), desc_dev within S descriptors, cam_dev within S rows, x_dev within S * RF * J * 3 floats (row RF - 1 - lag of
 * window s, lag checked on the host), and writes pred_dev and world_dev within S * J * 3, reproj_dev within S * J and quality_dev
 * within S * 2 elements: no index depends on a value read from device memory.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (raw_dev, emit_dev, status_dev; desc_dev with
 * world_dev or reproj_dev; cam_dev and x_dev with reproj_dev), pred_dev, world_dev and reproj_dev all NULL, exactly one of
 * raw_mirror_dev / mirror_perm, a mirror_perm that is not a permutation, num_streams outside 1..R3D_CLIPS_MAX, num_joints outside
 * 1..17, quality_dev without reproj_dev, and with reproj_dev: receptive_field < 1, lag outside [0, receptive_field - 1], num_streams *
 * receptive_field * num_joints above R3D_ENCODE_MAX_POINTS; emit_dev, desc_dev, cam_dev, world_dev, reproj_dev or quality_dev not
 * 8-byte aligned; an output extent that overlaps raw_dev, raw_mirror_dev or (with reproj_dev) x_dev, compared as address ranges.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
typedef struct {
    double rn2w[9];       /* row-major, normalised -> world rotation (as r3d_clip_desc)               */
    double tn2w[3];
    double height;        /* camera height in metres: Tc2n = (0, -height, 0), camera.py:340-343       */
    double reserved;      /* 0                                                                        */
} r3d_stream_pose_desc;   /* 112 bytes, 8-byte aligned; lives in DEVICE memory */
int r3d_streams_poses(const float *raw_dev, const float *raw_mirror_dev,   /* (S, J, 3): the forwards' outputs */
                      int32_t num_streams, int32_t num_joints,
                      const int32_t *mirror_perm,              /* HOST, J entries; given exactly when raw_mirror_dev is */
                      const int64_t *emit_dev, const int32_t *status_dev,   /* (S): what r3d_streams_step wrote this tick */
                      const r3d_stream_pose_desc *desc_dev,    /* (S); NULL only if world_dev and reproj_dev are NULL */
                      const double *cam_dev,                   /* (S, 16) camera rows; required with reproj_dev */
                      const float *x_dev, int32_t receptive_field, int32_t lag,   /* (S, RF, J, 3); required with reproj_dev */
                      float *pred_dev,       /* (S, J, 3) float32, may be NULL */
                      double *world_dev,     /* (S, J, 3) float64, may be NULL */
                      double *reproj_dev,    /* (S, J) float64 pixels, may be NULL */
                      double *quality_dev,   /* (S, 2) float64: mean, max of the stream's row of reproj; NULL unless reproj_dev */
                      void *stream);

/* ---- live streams that survive dropped keypoints: one call in front of a tick's r3d_streams_step ---- */

/* A 2D detector does not deliver every joint of every frame.  r3d_streams_step copies or encodes whatever it is handed into the
 * ring, and a non-finite keypoint then makes the stream's pose NaN for the next RF ticks.  r3d_streams_repair is enqueued BEFORE
 * r3d_streams_step of the same tick, on the same stream, with the same state, shape, camera rows and action words: it reads the
 * tick's new frames, decides per joint whether the keypoint was OBSERVED, writes a repaired frame for the step to push
 * (frame_out_dev: the step is then given frame_out_dev as its frame_dev), rewrites the few ring entries a closing gap lets it
 * improve, keeps a small per-stream track record, and reports which joints of the frame the step emits this tick are synthetic.
 * A stream without gaps is left bit for bit what it is without the call.  The reference's archives are complete, so it has no
 * behaviour to copy here; a repaired stream equals the reference's windows (np.pad 'edge' + eval_data_prepare) of the clip
 * repaired offline by the same rules, wherever that is well defined.  Windows already emitted are never revised: a frame's window
 * uses the best repair known at the tick it is emitted.
 *   state_dev:   the state of r3d_streams_step.  The heads are READ, never written; ring entries may be rewritten.
 *   track_dev:   caller-owned DEVICE memory of r3d_streams_track_bytes bytes, 8-byte aligned; all-zero is "freshly reset".  LAYOUT,
 *                with width = 2 for the pixel encodings and in_features for R3D_ENCODE_NONE (as the frame rows of r3d_streams_step):
 *                  int32    age[S][J]            0: the joint was never observed since the stream's last RESTART; k >= 1: it was
 *                                                observed k - 1 frames ago; saturates at INT32_MAX; a value below 0 (a track nobody
 *                                                zeroed) reads as 0
 *                  float32  last[S][J][width]    the joint's last observed input, as delivered (32-bit patterns)
 *                  uint32   missing[S][RF]       per ring slot the mask (bit j: joint j) of the joints not observed in that frame
 *                in that order, the total rounded up to a multiple of 8 bytes.
 *   frame_dev:   (S, J, width) float32: what the caller would have given the step; may hold non-finite entries.
 *   conf_dev / min_conf: NULL, or (S, J) float32 detector confidences and the threshold.
 *   max_gap:     in [0, RF - 1]: the longest gap that is interpolated when it closes (0: zero-order hold only).
 *   frame_out_dev: (S, J, width) float32, written for the streams that PUSH or RESTART this tick.
 *   synthetic_dev: (S) uint32: bit j set = joint j of the frame the step emits this tick was not observed - however good its repair.
 * PER STREAM.  The head and the action word are judged by the very routine the step uses, on the head as it stands before the step.
 *   NO PUSH (IDLE, DRAIN, a stream the step will refuse): nothing of the stream's track, ring or frame_out row is written;
 *            synthetic[s] is the `missing` word of the frame the step will emit (a DRAIN that emits), or 0.
 *   RESTART  the stream's track is zeroed first - whatever it held -, then the action is a PUSH with c = 0.
 *   PUSH, joint j, c the head's count before the push:
 *     OBSERVED means every one of the `width` input components is finite (tested on the exponent bits) and, with conf_dev,
 *            conf >= min_conf (a NaN confidence is not observed).
 *     not observed, age == 0   frame_out = the canonical quiet NaN (0x7FC00000) in every component; age stays 0.
 *     not observed, age >= 1   frame_out = last[j]: zero-order hold in INPUT space (the step encodes it to the bits it encoded
 *            before); age += 1.
 *     observed   frame_out = the input bits, last[j] = the input bits, age = 1.  Before that, with e the joint's encoding - for a
 *            pixel encoding the routine and bits the step will push (through the stream's camera row), for R3D_ENCODE_NONE the
 *            row itself:
 *            BACK-FILL  the old age was 0 and c >= 1: every frame in max(0, c - (RF - 1)) .. c - 1 gets e for joint j in the ring
 *              (the per-joint analogue of the reference's front edge padding).
 *            INTERPOLATION  the old age was k >= 2, g = k - 1, 1 <= g <= max_gap and g + 1 <= c: with a the ring's entry of frame
 *              c - 1 for joint j (the held copy of the last observation), frame c - 1 - g + m, m = 1 .. g, gets per component
 *                fl32((double)a + ((double)e - (double)a) * ((double)m / (double)(g + 1)))
 *              every operation rounded once, no contraction; a NaN result leaves as the canonical quiet NaN.  The encodings are
 *              affine in the (undistorted) pixel: this is linear interpolation in undistorted pixel space.
 *            Otherwise the held values stay.
 *     after the joints   missing[c % RF] = the mask of the joints not observed in the new frame (interpolated or back-filled
 *            frames keep their bits); synthetic[s] = missing[(c - lag) % RF] if c - lag >= 0 - the frame the step will emit - else 0.
 * ONE LAUNCH of the call's own kernel, r3d_k_streams_repair: S workgroups of one wavefront;
 * thread j < J owns joint j and is the only one that writes the joint's frame_out row, age, last and ring entries; one thread
 * forms the mask from the wavefront's ballot and writes the two mask words.  Launch-latency-bound by construction.
 * THE WHOLE BOUNDS STORY.  Whatever the track, the state and the action words hold, the kernel reads the heads, frame_dev,
 * conf_dev, cam_dev and action_dev within their S rows and writes the rings within r3d_streams_state_bytes, the track within
 * r3d_streams_track_bytes, frame_out_dev within S * J * width floats and synthetic_dev within S words: ring and `missing` indices
 * are remainders modulo RF of frames in [0, c] of a head that passed the step's head rule (rewritten ring entries: frames in
 * [0, c - 1]); g is used only after g <= max_gap <= RF - 1 and g + 1 <= c; no index comes from `last` or `missing`, and an age only
 * ever bounds a loop that those two comparisons have bounded first.
 * R3D_ERR_ARG (checked on the host before any HIP call): everything r3d_streams_step refuses for the arguments the two share
 * (state_dev, the shape, lag, encoding and in_features, frame_dev, cam_dev, action_dev); a null track_dev, frame_out_dev or
 * synthetic_dev; max_gap outside [0, receptive_field - 1]; a non-finite min_conf; a track_dev that is not 8-byte aligned;
 * frame_out_dev overlapping frame_dev, conf_dev, the state or the track, compared as address ranges.  r3d_streams_track_bytes
 * returns 0 for shapes the call refuses (`width` 2 or 3, the rest as r3d_streams_state_bytes).
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
size_t r3d_streams_track_bytes(int32_t num_streams, int32_t receptive_field, int32_t num_joints, int32_t width);
int r3d_streams_repair(void *state_dev,              /* the state of r3d_streams_step: heads READ, rings rewritten */
                       void *track_dev,              /* r3d_streams_track_bytes, 8-byte aligned; all-zero = fresh   */
                       int32_t num_streams, int32_t receptive_field, int32_t lag,
                       int32_t num_joints, int32_t in_features, int32_t encoding,
                       const float *frame_dev,       /* (S, J, width): what the caller would have given the step    */
                       const float *conf_dev, float min_conf,   /* (S, J) or NULL: detector confidences             */
                       const double *cam_dev,        /* (S, 16); NULL with R3D_ENCODE_NONE                          */
                       const int32_t *action_dev,    /* (S): the words the step will read                           */
                       int32_t max_gap,              /* 0 .. RF - 1: longest gap that is interpolated when it closes */
                       float *frame_out_dev,         /* (S, J, width): what the step is given as frame_dev          */
                       uint32_t *synthetic_dev,      /* (S): bit j set = joint j of the frame emitted this tick was not observed */
                       void *stream);

/* ---- early poses for live streams of centred models: one read-only call behind a tick's r3d_streams_step ---- */

/* A centred model's pose of a frame is emitted `lag` ticks after the frame arrived.  r3d_streams_peek is enqueued AFTER
 * r3d_streams_step of the same tick, on the same stream, with the same state and shape, and writes for every look L of `looks`
 * the window the reference builds when the clip ENDS at this tick's frame - back edge padding in place of the frames that have not
 * arrived - for the frame L ticks old: a pose now, superseded by the stream's final pose of that frame `lag - L` ticks later.
 * Nothing of the state is written: the streams go on as if the call had not been made.
 *   looks:      HOST array of num_looks entries, 1 <= num_looks <= R3D_STREAMS_PEEK_MAX, strictly increasing, each in [0, lag): they
 *               travel as a kernel argument.  A small look is early and sees little of the future (look 0: none at all, the newest
 *               frame); a look of lag - 1 lacks one future frame only.  lag == 0 (a causal model) has no admissible look.
 *   action_dev, status_dev: the action words this tick's step read and the status words it wrote.  action_dev NULL: every stream
 *               counts as pushed.
 *   x_dev / x_mirror_dev / mirror_perm: (K, S, RF, J, F) float32, K = num_looks; the mirrored copy as r3d_streams_step takes it.
 *   emit_dev:   (K, S) int64: the frame the window of row block (k, s) belongs to, or -1.
 *   peek_status_dev: (K, S) int32: 1 when status_dev[s] != 0 or the head is invalid (r3d_streams_step's rule), 0 otherwise.
 * PER LOOK k AND STREAM s (integers only).  c is the head's count after the step, L = looks[k], p = c - 1 - L.  The stream PREVIEWS
 * when status_dev[s] == 0, the action word is PUSH or RESTART (or action_dev is NULL), the head is valid, drained == 0, c >= 1 and
 * p >= 0.  Then emit = p and row i of x_dev[k, s] is the ring's copy of frame clamp(p - (RF - 1 - lag) + i, 0, c - 1), found at slot
 * frame % RF - r3d_streams_step's rule with p in place of n: the window a drain started now would emit at its (lag - L)-th tick, and
 * window p of the reference's np.pad(..., 'edge') + eval_data_prepare on the stream's c frames so far.  The oldest frame it names
 * is c - RF + lag - L > c - RF, which the ring holds.  Otherwise emit = -1 and nothing of row block (k, s) is read or written.
 * ONE LAUNCH of the call's own kernel, r3d_k_streams_peek: (ceil(RF * J / 256), S, K)
 * workgroups, one output point (row, joint) per thread; each workgroup reads its stream's head, action and status word uniformly and
 * decides before anything is written; nothing the launch writes is read by another of its workgroups.
 * THE WHOLE BOUNDS STORY.  Whatever the state and the words hold, the kernel reads the state within r3d_streams_state_bytes,
 * action_dev and status_dev within S words, and writes x_dev and x_mirror_dev within K * S * RF * J * F floats, emit_dev and
 * peek_status_dev within K * S words: a ring slot is a remainder modulo RF of a non-negative number, a frame index is clamped into
 * [0, c - 1] of a head that passed the rule, and no head that fails it is followed.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (state_dev, looks, status_dev, x_dev, emit_dev,
 * peek_status_dev), num_streams outside 1..R3D_CLIPS_MAX, num_joints outside 1..17, receptive_field < 1, lag outside [0,
 * receptive_field - 1], in_features other than 2 or 3, lag == 0, num_looks outside 1..R3D_STREAMS_PEEK_MAX, a look outside
 * [0, lag), looks that are not strictly increasing, exactly one of x_mirror_dev / mirror_perm, a mirror_perm that is not a
 * permutation, receptive_field * num_joints or num_looks * num_streams * receptive_field * num_joints above R3D_ENCODE_MAX_POINTS, a
 * state or emit_dev pointer that is not 8-byte aligned.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
#define R3D_STREAMS_PEEK_MAX 8
int r3d_streams_peek(const void *state_dev,           /* the state of r3d_streams_step: READ, never written     */
                     int32_t num_streams, int32_t receptive_field, int32_t lag,
                     int32_t num_joints, int32_t in_features,
                     const int32_t *looks, int32_t num_looks,   /* HOST, strictly increasing, 0 <= look < lag    */
                     const int32_t *action_dev,       /* (S) the words of this tick's step, or NULL: all pushed  */
                     const int32_t *status_dev,       /* (S) what this tick's step wrote                         */
                     float *x_dev,                    /* (K, S, RF, J, F): look k, stream s own row block (k, s) */
                     float *x_mirror_dev, const int32_t *mirror_perm,   /* both NULL, or both given (HOST perm)  */
                     int64_t *emit_dev,               /* (K, S) the preview frame of the row block, or -1        */
                     int32_t *peek_status_dev,        /* (K, S) 0, or 1: refused by the step / invalid head      */
                     void *stream);

/* ---- one world skeleton per person from several cameras: one call behind a tick's r3d_streams_poses ---- */

/* Several cameras watch the same person; each is a live stream.  r3d_streams_poses writes, per stream and tick, the pose in WORLD
 * coordinates and the per-joint re-projection residual: the model predicts in a camera-independent frame, so the streams' world
 * poses are directly comparable.  r3d_streams_fuse is enqueued AFTER r3d_streams_poses of the same tick, on the same stream, and
 * combines them: per GROUP of streams (one person) and joint a gated, weighted mean over the group's members that finished a frame
 * this tick.  The reference is monocular and has nothing to copy here: what follows is this library's definition, held bit for bit
 * between the device and the host hook.
 *   world_dev:  (S, J, 3) float64, what r3d_streams_poses wrote.  Rows of streams that did not finish a frame are never read.
 *   reproj_dev: (S, J) float64 residuals in pixels (r3d_streams_poses), or NULL: every weight is 1.
 *   emit_dev, status_dev: (S) the words r3d_streams_step wrote this tick.
 *   synthetic_dev: (S) the mask words of r3d_streams_repair (bit j: joint j of the emitted frame was not observed), or NULL.
 *   member_dev: (G, M) int32 in DEVICE memory: the stream index in slot m of group g; a negative word is an empty slot.  The
 *               table may be rewritten between ticks.  The same stream in two slots counts as two candidates.
 *   soft_px > 0, max_px (<= 0: off), max_dist in metres (<= 0: off).
 * THE RULE PER GROUP g AND JOINT j.  Integers decide first; after that the arithmetic is float64, no contraction, every operation
 * rounded once, slots visited in ascending slot order, every sum started from zero.
 *   1. CANDIDATES.  Slot m, s = member[g, m], is a candidate when 0 <= s < S (an index outside that range is not followed: nothing
 *      of it is read); the stream finished this tick (status[s] == 0 and emit[s] >= 0, r3d_streams_poses's rule); the three
 *      components of world[s, j] are finite (tested on the exponent bits); and, with reproj_dev, r = reproj[s, j] is finite and
 *      r <= max_px when max_px > 0.  TIERS, with synthetic_dev: if at least one candidate has bit j of synthetic[s] clear, the
 *      candidates with bit j set are dropped - a held or interpolated keypoint does not vote against an observed one; if all
 *      candidates are synthetic, all stay.
 *   2. WEIGHT.  w = 1.0 / (soft_px * soft_px + r * r); 1.0 without reproj_dev.
 *   3. GATE, only with max_dist > 0 and at least two candidates (after the tiers).  d(a, b) = sqrt(((dx*dx) + (dy*dy)) + (dz*dz)),
 *      the correctly rounded sqrt.  The cost of candidate m is c_m = the sum of w_t * d(x_m, x_t) over the other candidates t.  The
 *      medoid is the first candidate, replaced by a later one only when c < c_best: ties and NaN costs keep the earlier slot.  The
 *      inliers are the candidates with d(x_medoid, x_m) <= max_dist (the medoid is one).  Without the gate every candidate is an
 *      inlier.  Two cameras that disagree by more than max_dist thus keep the one with the smaller residual.
 *   4. OUTPUTS.  den = sum of w over the inliers.  fused_dev[g, j, r] = (sum of w * x[r]) / den.  spread_dev[g, j] =
 *      sqrt((sum of w * q(fused, x)) / den), q the squared distance formed as inside d, `fused` the value just computed: the
 *      weighted RMS distance of the inliers from the fused point, in metres.  count_dev[g, j] = the number of inliers.  Bit j of
 *      used_dev[g, m] is set when slot m was an inlier for joint j (bits J .. 31 are 0).  No inlier: fused and spread are the
 *      canonical quiet NaN (0x7FF8000000000000), count is 0.  Any NaN the arithmetic produces (an overflowing sum, a weight that
 *      underflows the denominator to 0) leaves as the canonical quiet NaN.
 * EVERY row of every output given is written on every call, also those of a group whose slots are all empty (NaN, NaN, 0, 0).
 * ONE LAUNCH of the call's own kernel, r3d_k_streams_fuse: G workgroups of one wavefront;
 * the workgroup reads its M member words uniformly, once; thread j < J owns joint j, stages its candidates' points and weights in
 * LDS (at most 16 x 17 x 32 bytes per group) and runs the gate out of it; a `used` word is the wavefront's ballot for its slot,
 * written by one thread.  Launch-latency-bound by construction.
 * THE WHOLE BOUNDS STORY.  The only index taken from device memory is a member word, and it is used only after 0 <= s < S held.
 * Whatever the inputs hold, the kernel reads member_dev within G * M words, emit_dev, status_dev and synthetic_dev within S words,
 * world_dev within S * J * 3 and reproj_dev within S * J doubles, and writes fused_dev within G * J * 3 doubles, spread_dev and
 * count_dev within G * J elements and used_dev within G * M words; the staging area is indexed by slot m < M <= 16 and joint
 * j < J <= 17 only.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (world_dev, emit_dev, status_dev, member_dev,
 * fused_dev), num_streams or num_groups outside 1..R3D_CLIPS_MAX, num_joints outside 1..17, max_members outside
 * 1..R3D_FUSE_MAX_MEMBERS, a soft_px that is not finite or <= 0, a NaN max_px or max_dist, world_dev, reproj_dev, emit_dev,
 * fused_dev or spread_dev not 8-byte aligned, an output extent (fused_dev, spread_dev, count_dev, used_dev) that overlaps an input
 * extent (world_dev, reproj_dev, emit_dev, status_dev, synthetic_dev, member_dev), compared as address ranges.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
#define R3D_FUSE_MAX_MEMBERS 16
int r3d_streams_fuse(const double *world_dev,          /* (S, J, 3) float64: what r3d_streams_poses wrote          */
                     const double *reproj_dev,         /* (S, J) float64 px, or NULL: every weight is 1            */
                     const int64_t *emit_dev, const int32_t *status_dev,   /* (S): this tick's step words            */
                     const uint32_t *synthetic_dev,    /* (S) r3d_streams_repair's masks, or NULL                  */
                     int32_t num_streams, int32_t num_joints,
                     const int32_t *member_dev,        /* (G, M) stream index per slot, < 0: empty slot; DEVICE    */
                     int32_t num_groups, int32_t max_members,              /* G in 1..R3D_CLIPS_MAX, M in 1..16     */
                     double soft_px, double max_px, double max_dist,       /* > 0; <= 0: off; <= 0: off             */
                     double *fused_dev,                /* (G, J, 3) float64                                        */
                     double *spread_dev,               /* (G, J) float64 metres, may be NULL                       */
                     int32_t *count_dev,               /* (G, J) contributors, may be NULL                         */
                     uint32_t *used_dev,               /* (G, M): bit j = slot m contributed to joint j; may be NULL */
                     void *stream);

/* ---- detections to live streams: one call in front of a tick's r3d_streams_repair / r3d_streams_step ---- */

/* r3d_streams_step expects row s of its frame to be the same person on every tick, and its caller to know when to RESTART and when
 * to DRAIN a stream.  A 2D detector delivers neither: per camera and tick an unordered list of 0 .. D skeletons with joints
 * missing; people enter, are missed for a few frames, and leave.  r3d_streams_assign is enqueued BEFORE r3d_streams_repair /
 * r3d_streams_step of the same tick, on the same stream.  Per camera it associates the tick's detections with that camera's P
 * stream slots (stream s = c * P + p), starts new tracks, ends lost ones and writes exactly what repair and step read: the action
 * words, the frame rows and the confidence rows.  The reference works on complete, pre-associated archives and has nothing to copy
 * here: what follows is this library's definition, held bit for bit between the device and the host hook.
 *   det_dev:       (C, D, J, width) float32 keypoints, width 2 or 3 as the frame rows of r3d_streams_step; components 0 and 1 are
 *                  what the rule measures with.  Detections d >= det_count[c] are never read.
 *   det_conf_dev:  (C, D, J) float32 detector confidences, or NULL.
 *   det_count_dev: (C) int32, read clamped into [0, D].
 * THE STATE.  assign_dev is caller-owned DEVICE memory of r3d_streams_assign_bytes bytes, 8-byte aligned; all-zero means "no
 * tracks".  In this order, the total rounded up to 8 bytes: int64 next_id[C], int64 id[S], int32 phase[S] (0 free, 1 live, 2
 * draining; any other value - and 2 when lag == 0 - reads as 0), int32 missed[S] (a value below 0 reads as 0), int32 left[S] (read
 * clamped into [1, lag]), uint32 seen[S] (bit j set: ref[j] holds an observation; bits J .. 31 are not read), float32
 * ref[S][J][width] (the per-joint last observation).
 * THE RULE PER CAMERA c.  Integers decide first; the arithmetic is float64, no contraction, every operation rounded once, joints
 * visited in ascending order, every sum started from zero, sqrt and / the correctly rounded ones.
 *   1. DETECTIONS.  n = clamp(det_count[c], 0, D).  Joint j of detection d < n is OBSERVED when all `width` components are finite
 *      (tested on the exponent bits) and - with det_conf_dev - conf >= min_conf (a NaN confidence is not observed).  size(d) =
 *      max(max x - min x, max y - min y) over the observed joints, components 0 and 1 widened to float64.  The detection is VALID
 *      when it has at least min_joints observed joints and size > 0.
 *   2. COST.  For a live slot p (phase 1 at entry) and a valid detection d the COMMON joints are those observed in d and set in
 *      seen[p].  Fewer than min_common: the pair is inadmissible.  Otherwise cost = (sum over the common joints of
 *      sqrt((dx*dx) + (dy*dy)) / their number) / size(d), dx and dy components 0 and 1 of det - ref[p].  The pair is admissible
 *      when cost <= max_cost; a NaN cost fails.
 *   3. GREEDY MATCHING.  Repeatedly the admissible pair with the smallest cost among the unmatched slots and the unmatched
 *      detections is matched; ties go to the smaller p, then the smaller d.  It stops when no admissible pair is left.
 *   4. LIVE SLOTS.  MATCHED with d: action PUSH; the frame_out row is the detection's bits (unobserved joints included: they are
 *      what r3d_streams_repair repairs); the conf_out row its confidences, or 1.0 without det_conf_dev; missed = 0; per observed
 *      joint ref[j] takes the detection's bits and bit j of seen is set; match = d.  UNMATCHED with missed + 1 <= max_missed:
 *      action PUSH; the frame row is the canonical quiet NaN (0x7FC00000) with R3D_ASSIGN_FILL_NAN - r3d_streams_repair holds or
 *      interpolates it - and with R3D_ASSIGN_FILL_HOLD ref[j] where seen, else the canonical NaN; the conf_out row is 0.0;
 *      missed += 1.  UNMATCHED BEYOND max_missed: the track ends.  lag > 0: action DRAIN, left = lag - 1, the slot goes to phase 2,
 *      or to 0 when left == 0.  lag == 0: action IDLE, phase 0.
 *   5. DRAINING SLOTS.  action DRAIN; left -= 1; phase 0 when left reaches 0.  An ended track thus gets exactly `lag` DRAIN ticks.
 *   6. BIRTHS.  The valid unmatched detections, in ascending d, take the slots that were FREE AT ENTRY, in ascending p (a slot
 *      freed in this call is not reused in it).  A born slot: action RESTART; id = next_id[c], then next_id[c] += 1; phase 1;
 *      missed = 0; seen and ref from the detection's observed joints; the frame_out and conf_out rows as for a match; match = d.
 *      A detection that finds no free slot is counted in stats[c][3] and otherwise ignored.
 *   7. REMAINING FREE SLOTS.  action IDLE.
 * OUTPUTS.  EVERY element of every output given is written on every call.  The frame_out rows of slots that neither PUSH nor
 * RESTART are the canonical NaN, their conf_out rows 0.0, their match -1.  id_dev[s] is the track's identity on every tick the
 * slot is live or draining - the tick the track ends included -, -1 for a slot that is free and stays free.  Identities count from
 * the state's next_id[c] per camera: (c, id) names a track.  stats_dev[c] = the valid detections, the matched ones, the births
 * and the valid detections that found no slot.  Copied keypoints and confidences travel as 32-bit patterns.
 * ONE LAUNCH of the call's own kernel, r3d_k_streams_assign: C workgroups of one wavefront.
 * Lanes own detections for step 1; the P x D pairs are dealt over the lanes for step 2, the cost keys in LDS; step 3 is at most
 * min(P, D) rounds of a wavefront-wide arg-min over (cost, p * D + d) with taken-row and taken-column masks; ballots and
 * popcounts rank step 6's detections and slots; then lanes own slots.  Launch-latency-bound by construction.
 * THE WHOLE BOUNDS STORY.  Nothing in the state is ever used as an index: phase, missed, left and seen are compared and masked,
 * ref is subtracted and copied, the identities are copied and counted.  The only value taken from device memory that bounds a
 * loop or forms an index is det_count[c], after its clamp into [0, D]: a matched or born slot copies detection d < n <= D.
 * Whatever the inputs and the state hold, the kernel reads det_dev within C * D * J * width floats, det_conf_dev within C * D * J,
 * det_count_dev within C words, reads and writes the state within r3d_streams_assign_bytes bytes, and writes action_dev, match_dev
 * and id_dev within S elements, frame_out_dev within S * J * width, conf_out_dev within S * J and stats_dev within C * 4; the LDS
 * keys are indexed by p * D + d < P * D <= 1024 only.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (assign_dev, prm, det_dev, det_count_dev,
 * action_dev, frame_out_dev, match_dev, id_dev), a struct_size other than sizeof(r3d_assign_params), num_cameras < 1, slots outside
 * 1..R3D_ASSIGN_MAX_SLOTS, max_detections outside 1..R3D_ASSIGN_MAX_DETECTIONS, num_cameras * slots > R3D_CLIPS_MAX, num_joints
 * outside 1..17, a width other than 2 or 3, lag < 0, min_joints or min_common outside 1..num_joints, max_missed < 0, an unknown
 * fill, a non-finite min_conf, a max_cost that is not finite and > 0, assign_dev or id_dev not 8-byte aligned, an output extent
 * (action_dev, frame_out_dev, conf_out_dev, match_dev, id_dev, stats_dev) that overlaps an input extent (det_dev, det_conf_dev,
 * det_count_dev), the state or another output, compared as address ranges.  r3d_streams_assign_bytes returns 0 for shapes the
 * call refuses.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
#define R3D_ASSIGN_MAX_SLOTS 32        /* P: stream slots per camera      */
#define R3D_ASSIGN_MAX_DETECTIONS 32   /* D: detections per camera & tick */
#define R3D_ASSIGN_FILL_NAN  0         /* an unmatched live slot pushes canonical NaNs (for r3d_streams_repair) */
#define R3D_ASSIGN_FILL_HOLD 1         /* ... pushes the per-joint last observation (a caller without repair)   */
typedef struct {
    int32_t struct_size;               /* sizeof of the CALLER's struct; any other size is R3D_ERR_ARG */
    int32_t num_cameras, slots, max_detections;   /* C, P, D: stream s = c * P + p; S = C * P <= R3D_CLIPS_MAX */
    int32_t num_joints, width;         /* J in 1..17; width 2 or 3: the frame rows of r3d_streams_step */
    int32_t lag;                       /* the step's lag: how many DRAIN ticks an ended track gets */
    int32_t min_joints, min_common;    /* 1..J each */
    int32_t max_missed;                /* >= 0: consecutive unmatched ticks a track survives */
    int32_t fill;                      /* R3D_ASSIGN_FILL_* */
    float   min_conf;                  /* finite; used only with det_conf_dev */
    double  max_cost;                  /* finite, > 0 */
} r3d_assign_params;
size_t r3d_streams_assign_bytes(int32_t num_cameras, int32_t slots, int32_t num_joints, int32_t width);
int r3d_streams_assign(void *assign_dev, const r3d_assign_params *prm /* HOST */,
                       const float *det_dev,        /* (C, D, J, width) */
                       const float *det_conf_dev,   /* (C, D, J) or NULL */
                       const int32_t *det_count_dev,/* (C): read clamped into [0, D] */
                       int32_t *action_dev,         /* (S) R3D_STREAM_* for this tick's repair / step */
                       float *frame_out_dev,        /* (S, J, width): what repair / step get as frame_dev */
                       float *conf_out_dev,         /* (S, J) or NULL */
                       int32_t *match_dev,          /* (S): detection index matched or born from, or -1 */
                       int64_t *id_dev,             /* (S): the slot's track identity this tick, or -1 */
                       int32_t *stats_dev,          /* (C, 4) or NULL: valid, matched, born, dropped */
                       void *stream);

/* ---- one person across cameras: one call between a tick's r3d_streams_poses and its r3d_streams_fuse ---- */

/* r3d_streams_assign keeps tracks per camera and r3d_streams_fuse combines the streams a (G, M) member table names; which camera's
 * track is which person is what r3d_streams_link decides, on the device: it keeps a table of people, G slots per scene, in
 * caller-owned device memory, links each camera's tracks to people by the distance of their world poses, starts and ends people and
 * writes the member table r3d_streams_fuse reads.  It is enqueued AFTER r3d_streams_poses and BEFORE r3d_streams_fuse of the same
 * tick, on the same stream.  The reference is monocular and pre-associated and has nothing to copy here: what follows is this
 * library's definition, held bit for bit between the device and the host hook.
 * SHAPES.  N scenes (a scene is a room whose cameras see the same people), C cameras per scene, P slots per camera, G people per
 * scene.  Stream s = (n * C + c) * P + p - as r3d_streams_assign numbers them with num_cameras = N * C -, S = N * C * P; person
 * n * G + g.  M = max_members is the member table's row length, C <= M <= R3D_FUSE_MAX_MEMBERS.
 *   world_dev:             (S, J, 3) float64, what r3d_streams_poses wrote this tick.
 *   emit_dev, status_dev:  (S) this tick's words of r3d_streams_step.  A stream FINISHED when status == 0 and emit >= 0, as for
 *                          r3d_streams_poses.
 *   id_dev:                (S) int64 track identities: what r3d_streams_assign wrote this tick (a caller without it supplies its
 *                          own); < 0: no track.
 * THE STATE.  link_dev is caller-owned DEVICE memory of r3d_streams_link_bytes bytes, 8-byte aligned; all-zero means "no people".
 * In this order, the total rounded up to 8 bytes: int64 next_id[N], int64 pid[N*G], int64 link_id[N*G][C], double ref[N*G][J][3],
 * int32 phase[N*G] (0 free, 1 live; any other value reads as 0), int32 missed[N*G] (a value below 0 reads as 0), int32 link[N*G][C]
 * (the slot PLUS ONE; 0: none; a value outside 0..P reads as 0), uint32 seen[N*G] (bit j set: ref[j] holds a point; bits J .. 31
 * are not read).
 * THE RULE PER SCENE n.  Integers decide first; the arithmetic is float64, no contraction, every operation rounded once, joints
 * visited in ascending order, every sum started from zero, sqrt and / the correctly rounded ones.  Joint j of a finished stream is
 * PRESENT when its three world components are finite (tested on the exponent bits).  cost(g, s), over the COMMON joints - present
 * in s and set in seen[g] -, is (sum of sqrt(((dx*dx) + (dy*dy)) + (dz*dz))) / their number, d = world[s][j] - ref[g][j]; it is
 * defined with at least one common joint.
 *   A. VALIDATE, people in ascending g, cameras in ascending c.  The link p of live person g in camera c, s its stream, is DROPPED
 *      when id_dev[s] < 0 or id_dev[s] != link_id[g][c] (the track ended or the slot was reused; a draining track keeps its
 *      identity and stays linked through its drain); when, with break_dist > 0, the stream finished, has a common joint and
 *      cost(g, s) > break_dist (a NaN cost keeps the link); when a smaller g holds the same stream after its own tests (only a
 *      state nobody zeroed has that).
 *   B. PER CAMERA, ascending c, strictly in that order.  CANDIDATES are the slots p with id >= 0, finished this tick, held by no
 *      person, with at least min_joints present joints.  ELIGIBLE are the live people - those born earlier in this call included -
 *      without a link in camera c and with a non-empty seen.  A pair is ADMISSIBLE with at least min_common common joints and
 *      cost <= max_dist (a NaN cost fails).  GREEDY MATCHING: repeatedly the admissible pair with the smallest cost among the
 *      unmatched people and candidates is matched; ties go to the smaller g, then the smaller p; it stops when no admissible pair
 *      is left.  A matched pair sets link = p + 1 and link_id = id_dev[s].  BIRTHS: the unmatched candidates, in ascending p, take
 *      the people that are free now, in ascending g: pid = next_id[n], then next_id[n] += 1; phase 1; missed 0; seen is the
 *      stream's present mask and ref[j] its point for every present joint (the other joints' ref stays); camera c's link is set
 *      as for a match, the person's other links are none.  A candidate that finds no free person is counted in stats[n][3] and
 *      stays unlinked: it is a candidate again on the next tick.  During B the ref of a person alive at entry is its value at
 *      entry; camera c + 1 sees the people camera c bore.
 *   C. PER LIVE PERSON.  Per joint, over the linked members that finished and have the joint present, cameras in ascending order:
 *      ref[j] = (sum of their points, per component) / their number, and bit j of seen is set; with no such member the joint's
 *      ref and bit stay.  With at least one link missed = 0.  With none: when missed + 1 > max_missed the person is FREED - phase
 *      0, not reused within this call -, else missed += 1; until then it keeps its ref, so a track re-born after an occlusion,
 *      with a new track identity, re-joins the same pid.
 * Every link word of the state is written on every call, 0 for a person that is not live after step B; link_id only where a link is
 * made; the other words of a person only where the rule changes them.
 * OUTPUTS.  EVERY element of every output given is written on every call.  member_dev[g][c] = the absolute stream index of the
 * person's link in camera c, or -1; slots C .. M - 1 hold -1: r3d_streams_fuse takes the table as it is, with num_groups = N * G.
 * person_dev[g] = the pid of a person live after the call, else -1.  group_dev[s] = the absolute person index that holds stream
 * s, or -1.  stats_dev[n] = the people live after the call, the links step B's matching made, the births and the candidates that
 * found no free person.
 * ONE LAUNCH of the call's own kernel, r3d_k_streams_link: N workgroups of one wavefront.
 * Lane g owns person g in step A and for the words of step C, whose joint means are dealt over the lanes by joint; in step B lane p
 * summarises slot p, the G x P pairs are dealt over the lanes, their cost keys in LDS, the matching at most min(G, P) rounds of a
 * wavefront-wide arg-min, births ranked by ballots and popcounts.  The cameras are visited one after the other: the launch's time
 * grows with C.
 * THE WHOLE BOUNDS STORY.  ONE state word becomes an index: a link word, and only after its range check - a value outside 1..P
 * reads as "none", so the slot p = link - 1 < P and the stream (n * C + c) * P + p < S.  Everything else in the state is compared
 * and masked (phase, missed, seen), subtracted, averaged and copied (ref) or copied and counted (the identities).  The inputs
 * form no index at all.  Whatever the inputs and the state hold, the kernel reads world_dev within S * J * 3 doubles and emit_dev,
 * status_dev and id_dev within S words, reads and writes the state within r3d_streams_link_bytes bytes, and writes member_dev
 * within N * G * M words, person_dev within N * G, group_dev within S and stats_dev within N * 4; the LDS keys are indexed by
 * g * P + p < G * P <= 1024 only, step C's member rows by g * C + c < G * C <= 512.
 * R3D_ERR_ARG (checked on the host before any HIP call): a null required pointer (link_dev, prm, world_dev, emit_dev, status_dev,
 * id_dev, member_dev, person_dev), a struct_size other than sizeof(r3d_link_params), num_scenes < 1, num_cameras outside
 * 1..R3D_FUSE_MAX_MEMBERS, slots outside 1..R3D_ASSIGN_MAX_SLOTS, people outside 1..R3D_LINK_MAX_PEOPLE, num_joints outside 1..17,
 * max_members outside num_cameras..R3D_FUSE_MAX_MEMBERS, num_scenes * num_cameras * slots or num_scenes * people above
 * R3D_CLIPS_MAX, min_joints or min_common outside 1..num_joints, max_missed < 0, a max_dist that is not finite and > 0, a
 * break_dist that is NaN or - when > 0 - not finite or below max_dist, link_dev, world_dev, emit_dev, id_dev or person_dev not
 * 8-byte aligned, an output extent (member_dev, person_dev, group_dev, stats_dev) that overlaps an input extent (world_dev,
 * emit_dev, status_dev, id_dev), the state or another output, compared as address ranges.  r3d_streams_link_bytes returns 0 for
 * shapes the call refuses.
 * Enqueued on `stream`: no copy, no allocation, no synchronisation (it can be captured into a hipGraph). */
#define R3D_LINK_MAX_PEOPLE 32         /* G: people per scene */
typedef struct {
    int32_t struct_size;               /* sizeof of the CALLER's struct; any other size is R3D_ERR_ARG */
    int32_t num_scenes, num_cameras, slots;       /* N, C, P: stream s = (n * C + c) * P + p; S = N * C * P <= R3D_CLIPS_MAX */
    int32_t people, max_members;       /* G in 1..R3D_LINK_MAX_PEOPLE; M in C..R3D_FUSE_MAX_MEMBERS: the member table is (N * G, M) */
    int32_t num_joints;                /* J in 1..17 */
    int32_t min_joints, min_common;    /* 1..J each */
    int32_t max_missed;                /* >= 0: consecutive ticks without a link a person survives */
    double  max_dist;                  /* metres; finite, > 0 */
    double  break_dist;                /* metres; <= 0: off; else finite and >= max_dist */
} r3d_link_params;
size_t r3d_streams_link_bytes(int32_t num_scenes, int32_t num_cameras, int32_t people, int32_t num_joints);
int r3d_streams_link(void *link_dev, const r3d_link_params *prm /* HOST */,
                     const double *world_dev,     /* (S, J, 3) float64: what r3d_streams_poses wrote */
                     const int64_t *emit_dev,     /* (S) */
                     const int32_t *status_dev,   /* (S) */
                     const int64_t *id_dev,       /* (S): the track identities of this tick, < 0: no track */
                     int32_t *member_dev,         /* (N * G, M): what r3d_streams_fuse gets as member_dev */
                     int64_t *person_dev,         /* (N * G): the pid of a live person, or -1 */
                     int32_t *group_dev,          /* (S) or NULL: the person index that holds the stream, or -1 */
                     int32_t *stats_dev,          /* (N, 4) or NULL: live, linked, born, dropped */
                     void *stream);

const char *r3d_last_error(void);
const char *r3d_version(void);
int r3d_abi_version(void);                 /* R3D_ABI_VERSION the library was built with */
/* The arithmetic the handle's large GEMMs actually run in: 0 = fp32 matrix cores, 1 = bf16x3 (r3d_config.bf16x3, or
 * the R3D_BF16X3 environment override read at r3d_create).  bench.py labels its line with this, not with the field. */
int r3d_precision(const r3d_model *m);

/* ---- test hooks: ONLY in libray3d_hip_hooks.so (the same sources built with -DR3D_TEST_HOOKS; tests/test_host.py, host
 * only, no device needed).  That build also reads the development switches (plan / tile-kind A/Bs, schedule dumps, fault
 * injection) from the environment; the product library has neither. ---- */
#ifdef R3D_TEST_HOOKS

/* Builds the static tile schedule of ONE launch for `nprob` GEMM problems (rows M[i], columns N[i], nk[i] K tiles of
 * 32, largest split-K factor max_ks[i], cap on 32-row units per tile max_units[i]) on `nwg` workgroups and verifies
 * that the tiles cover every (32-row unit, 32-column granule) exactly once within the kernel's tile-shape rules.
 * Returns 0, or a negative code naming the first violated rule. */
int r3d_debug_schedule_check(int nprob, const int *M, const int *N, const int *nk, const int *max_ks,
                             const int *max_units, int nwg, int enc, int *out_grid, int *out_tiles,
                             double *out_imbalance);

/* The whole forward's tile lists for `batch` windows on `nwg` CUs: every cell of every problem computed exactly once
 * over all launches, every consumer's launch after all of its producers' tiles.  *spilled = first-level rows that
 * run one launch late (row spill).  Returns 0 or a negative code. */
int r3d_debug_plan_check(r3d_model *pos, r3d_model *trj, int64_t batch, int nwg, int *launches, int *spilled);

/* The single-launch form of the forward (one persistent kernel for all levels, tiles ordered by ready counters), built
 * and executed on the host as a dependency machine: every tile gets to run, every counter ends full, and whenever a tile
 * runs every earlier problem that touches the same buffer columns is complete for the tile's windows.  Returns 0, 1 when
 * the plan of this batch size runs launch by launch (nothing to check), or a negative code. */
int r3d_debug_forward_check(r3d_model *pos, r3d_model *trj, int64_t batch, int nwg, int *tiles, int *counters);

/* Census of kernel specialisations: the launches one forward of `batch` windows on `nwg` CUs would make, in order, and for
 * each the tile kinds its tiles select in the persistent loop's dispatch (r3d_tiles.hpp, gemm_persistent) - host only, no
 * device.  Plan, tile lists, kernel choice and call form come from the code the driver itself runs; only the in-kernel
 * dispatch is restated (r3d_hooks.cpp, census_tile_kind).  The call shape: `uv` pixel keypoints (R3D_INPUT_UV) or rays,
 * `cam_stride` 0 = one camera row (as r3d_input), `window_stride` in frames (1: a clip call), `staged` as R3D_OPT_STAGED,
 * `captured` as on a stream under capture.  An eager call is reported as the FIRST one on its buffers (with r3d_bind_f32;
 * a repeat on the same buffers skips it).  Assumes every workgroup resident and no CU mask, as on the device the lists are
 * built for.  One row per (launch, tile kind), launches in order; a launch without tile lists (r3d_bind_f32, the decoder
 * tail) has one row with an empty tile kind.  `blocks` is what the launch record reports.  Returns the number of rows
 * (which may exceed `cap`: nothing is written past it), or a negative code. */
typedef struct r3d_census_row {
    int32_t launch;          /* index of the launch in the call, from 0 */
    int32_t blocks;          /* r3d_launch_record.blocks of that launch */
    int32_t tiles;           /* tiles of this kind in the launch */
    char kernel[48];         /* as r3d_profile_read names it */
    char tile_kind[48];      /* e.g. "gemm_tile<3,1>", "first_level_taps_b3<2,K>64,UV>" */
} r3d_census_row;
int r3d_debug_forward_census(r3d_model *pos, r3d_model *trj, int64_t batch, int nwg, int32_t uv, int64_t cam_stride,
                             int64_t window_stride, int32_t staged, int32_t captured, r3d_census_row *rows, int32_t cap);
/* Every (kernel, tile kind) the dispatch instantiates, by the same restatement run over all header values; and with
 * tile_kind empty, every kernel name a forward's launch record can carry.  Same return convention. */
int r3d_debug_census_domain(r3d_census_row *rows, int32_t cap);

/* The largest window count of every plan kind that has one, ascending (what r3d_workspace_bytes walks): a call of edge + 1
 * windows runs the next kind's plan.  Returns their number (which may exceed `cap`: nothing is written past it). */
int r3d_debug_plan_kind_edges(int64_t *edges, int32_t cap);

/* The workspace layout of a call of `batch` windows: one row per buffer of the plan that call runs, in workspace order, then
 * "(tail)" (the slack behind the last buffer, up to the next multiple of 256 bytes) and "(control)" (the single-launch
 * forward's ready counters and problem table).  Offsets and sizes are in bytes from workspace_dev; a buffer's bytes are
 * batch * floats_per_window * 4.  The per-frame buffer of clip calls (per_frame = 1; floats_per_window is then its floats
 * per input FRAME) is the last buffer: a clip call uses (batch - 1) * window_stride + RF rows of it, the ones beyond `batch`
 * lying in the tail.  *workspace_bytes (optional) = the sum of the rows' bytes = what this plan needs; r3d_workspace_bytes is
 * the maximum of that over the plans of smaller calls.  No device call.  Returns the number of rows (which may exceed `cap`:
 * nothing is written past it), or a negative code. */
typedef struct r3d_plan_buffer_row {
    char name[48];
    int64_t floats_per_window;
    uint64_t offset_bytes;
    uint64_t bytes;
    int32_t per_frame;
    int32_t reserved;
} r3d_plan_buffer_row;
int r3d_debug_plan_buffers(r3d_model *pos, r3d_model *trj, int64_t batch, r3d_plan_buffer_row *rows, int32_t cap,
                           uint64_t *workspace_bytes);

/* What a forward decides from the SHAPE of its call, with no pointer and on handles in any state: the size limits (above,
 * "Size limits of one forward": the functions the forward itself asks) - 0, or R3D_ERR_ARG with r3d_last_error set - and, in
 * *per_frame (optional), whether a call of this shape runs the per-frame first layers.  `mode`, `window_stride` and
 * `cam_stride` as in r3d_input.  No device call. */
int r3d_debug_call_check(r3d_model *pos, r3d_model *trj, int32_t mode, int64_t window_stride, int64_t cam_stride,
                         int64_t batch, int32_t *per_frame);

/* The per-keypoint routine of the R3D_INPUT_UV_DIST pre-pass, run on the host: `row16` one camera row of 16 doubles, `uv`
 * n pixel pairs; out_uv (n, 2) the undistorted pixels, out_rays (n, 3) the float64 rays before the cast (either may be
 * NULL).  Returns 0 or R3D_ERR_ARG. */
int r3d_debug_undistort_host(const double *row16, const double *uv, int64_t n, double *out_uv, double *out_rays);

/* ... and its two 2-float encodings (R3D_INPUT_PX_INTRINSIC: encoding 1, R3D_INPUT_PX_SCREEN: encoding 2): `out2` (n, 2) the
 * float64 values before the cast.  Returns 0 or R3D_ERR_ARG (null pointer, any other encoding). */
int r3d_debug_encode_px_host(const double *row16, const double *uv, int64_t n, int32_t encoding, double *out2);

/* The per-frame routines of r3d_clip_valid_losses run on the host (HOST pointers throughout, the same arguments and checks),
 * the frames added up by a plain index-order sum: `out` R3D_VALID_DOUBLES doubles, `frame` (n, R3D_VALID_COUNT) or NULL. */
int r3d_debug_valid_losses_host(const float *pos, const float *trj, const float *gt, int64_t n_frames, int32_t num_joints,
                                const int32_t *parents, int32_t flags, double *out, double *frame);
/* r3d_clips_encode on the host (HOST pointers throughout): the same argument checks, the same descriptor rules and
 * row-to-source mapping, the same per-keypoint routines and cast, clips in table order. */
int r3d_debug_clips_encode_host(const float *px, int64_t total_frames, int32_t num_joints, int32_t encoding,
                                const r3d_clip_input_desc *clips, int32_t num_clips, int64_t max_rows, float *x, int64_t out_rows,
                                float *x_mirror, const int32_t *mirror_perm, int32_t *status);
/* r3d_clips_repair on the host (HOST pointers throughout, no stream): the same argument checks and return codes, the same
 * descriptor rule, observed test, bitmap searches and per-point routine, clips in table order, joints in order. */
int r3d_debug_clips_repair_host(float *x, int64_t out_rows, int32_t num_joints, int32_t in_features, float *x_mirror,
                                const int32_t *mirror_perm, const r3d_clip_input_desc *clips, int32_t num_clips, int64_t max_rows,
                                const float *conf, int64_t total_frames, float min_conf, int32_t max_gap, uint8_t *state, int32_t *stats,
                                int32_t *status);
/* r3d_clips_valid_losses on the host (HOST pointers throughout, no scratch): the same argument checks, the same descriptor rule,
 * per valid clip exactly r3d_debug_valid_losses_host on the clip's slice; an invalid clip's row is NaN, its frame rows stay. */
int r3d_debug_clips_valid_losses_host(const float *pos, const float *trj, const float *gt, int64_t total_frames, int32_t num_joints,
                                      const int32_t *parents, int32_t flags, const r3d_clip_desc *clips, int32_t num_clips,
                                      int64_t max_frames, double *rows, int64_t row_stride, double *frame);
/* r3d_clips_poses on the host (HOST pointers throughout, no stream): the same argument checks, the same descriptor rule and the
 * same per-point routines, clips in table order. */
int r3d_debug_clips_poses_host(const float *raw, const float *raw_mirror, int64_t raw_rows, int32_t num_joints,
                               const int32_t *mirror_perm, const r3d_clip_desc *clips, const int64_t *raw_first, int32_t num_clips,
                               int64_t max_frames, float *pred, double *world, int64_t total_frames, int32_t *status);
/* r3d_clips_project on the host (HOST pointers throughout, no stream): the same argument checks, the same descriptor rule and the
 * same per-point routines, descriptors in table order; `outside` is added to, as on the device. */
int r3d_debug_clips_project_host(const float *world, int64_t total_frames, int32_t num_joints, int32_t encoding,
                                 const r3d_clip_project_desc *clips, int32_t num_clips, int64_t max_rows, float *x, int64_t out_rows,
                                 float *x_mirror, const int32_t *mirror_perm, float *gt, double *px, int64_t gt_rows,
                                 int32_t *outside, int32_t *status);
/* r3d_clips_windows on the host (HOST pointers throughout, no stream): the same argument checks, the same bisection, descriptor rule
 * and per-point routine, windows of the batch in order. */
int r3d_debug_clips_windows_host(const float *src, int64_t total_frames, int32_t num_joints, int32_t in_features,
                                 int32_t receptive_field, const r3d_window_run_desc *runs, int32_t num_runs, const float *run_param,
                                 int32_t extrinsic_dim, int64_t window0, int64_t batch, float *x, float *param,
                                 const int32_t *mirror_perm, int32_t *status);
/* r3d_streams_step on the host (HOST pointers throughout, no stream): the same argument checks, the same head rule, action step,
 * slot index and point routines, every stream advanced and then every stream gathered, as the two launches do. */
int r3d_debug_streams_step_host(void *state, int32_t num_streams, int32_t receptive_field, int32_t lag, int32_t num_joints,
                                int32_t in_features, int32_t encoding, const float *frame, const double *cam, const int32_t *action,
                                float *x, float *x_mirror, const int32_t *mirror_perm, int64_t *emit, int32_t *status);
/* r3d_streams_poses on the host (HOST pointers throughout, no stream): the same argument checks, the same finished-stream rule and
 * the same per-point and quality routines, streams in order. */
int r3d_debug_streams_poses_host(const float *raw, const float *raw_mirror, int32_t num_streams, int32_t num_joints,
                                 const int32_t *mirror_perm, const int64_t *emit, const int32_t *status, const r3d_stream_pose_desc *desc,
                                 const double *cam, const float *x, int32_t receptive_field, int32_t lag, float *pred, double *world,
                                 double *reproj, double *quality);
/* r3d_streams_repair on the host (HOST pointers throughout, no stream): the same argument checks, the same head and action
 * verdict, observed test, per-joint step, interpolation arithmetic and mask words, streams in order, joints in order. */
int r3d_debug_streams_repair_host(void *state, void *track, int32_t num_streams, int32_t receptive_field, int32_t lag,
                                  int32_t num_joints, int32_t in_features, int32_t encoding, const float *frame, const float *conf,
                                  float min_conf, const double *cam, const int32_t *action, int32_t max_gap, float *frame_out,
                                  uint32_t *synthetic);
/* r3d_streams_peek on the host (HOST pointers throughout, no stream): the same argument checks, the same verdict per look and
 * stream and the same point routine, looks in order, streams in order. */
int r3d_debug_streams_peek_host(const void *state, int32_t num_streams, int32_t receptive_field, int32_t lag, int32_t num_joints,
                                int32_t in_features, const int32_t *looks, int32_t num_looks, const int32_t *action,
                                const int32_t *status, float *x, float *x_mirror, const int32_t *mirror_perm, int64_t *emit,
                                int32_t *peek_status);
/* r3d_streams_fuse on the host (HOST pointers throughout, no stream): the same argument checks and the same per-joint routine on
 * a staging area of its own, groups in order, joints in order; the `used` words from the joints' inlier masks. */
int r3d_debug_streams_fuse_host(const double *world, const double *reproj, const int64_t *emit, const int32_t *status,
                                const uint32_t *synthetic, int32_t num_streams, int32_t num_joints, const int32_t *member,
                                int32_t num_groups, int32_t max_members, double soft_px, double max_px, double max_dist, double *fused,
                                double *spread, int32_t *count, uint32_t *used);
/* r3d_streams_assign on the host (HOST pointers throughout, no stream): the same argument checks and the same per-detection,
 * per-pair, per-slot and per-camera routines, cameras in order; the greedy matching as plain loops over the same keys in the
 * same order. */
int r3d_debug_streams_assign_host(void *assign, const r3d_assign_params *prm, const float *det, const float *det_conf,
                                  const int32_t *det_count, int32_t *action, float *frame_out, float *conf_out, int32_t *match,
                                  int64_t *id, int32_t *stats);
/* r3d_streams_link on the host (HOST pointers throughout, no stream): the same argument checks and the same per-link, per-slot,
 * per-pair and per-person routines, scenes, cameras and people in order; the greedy matching as plain loops over the same keys in
 * the same order. */
int r3d_debug_streams_link_host(void *link, const r3d_link_params *prm, const double *world, const int64_t *emit, const int32_t *status,
                                const int64_t *id, int32_t *member, int64_t *person, int32_t *group, int32_t *stats);
/* The device path's tables and per-element routines run on the CPU: packs the handle's host weights (every r3d_set_weight done) the
 * way r3d_finalize does, then once more through the descriptor / inverse / segment tables of r3d_finalize_dev and the routines its
 * kernel runs, work item by work item, and compares the two images as 32-bit patterns: *mismatches differing floats, *first_index
 * the first one's index (-1: none).  No device call.  Returns 0, R3D_ERR_KEY (a weight is missing) or R3D_ERR_ARG. */
int r3d_debug_pack_replay_host(r3d_model *m, int64_t *mismatches, int64_t *first_index);
/* The packed image as it is on the device, copied back after a device synchronise: *need_floats its size (always written);
 * `out` receives it when cap_floats suffices (else R3D_ERR_WORKSPACE).  R3D_ERR_STATE before a finalize. */
int r3d_debug_weights_image(r3d_model *m, float *out, size_t cap_floats, size_t *need_floats);
#endif /* R3D_TEST_HOOKS */

#ifdef __cplusplus
}
#endif
#endif
