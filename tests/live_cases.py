"""What tests/test_live_pixels_host.py and tests/test_gpu_live_pixels.py share: the end-to-end layer of the live path - raw pixels
from distorted cameras in, every option of OnlineLifter on at once.  Nothing is restated here a second time: the tick-wise rules
are the restatements already in the tree (tests/streams_assign_cases.py, tests/streams_repair_cases.py, tests/streams_peek_cases.py),
the cameras, pixels and the host encode chain are those of tests/test_clips_encode_host.py.  Three parts: the fixtures (model
pairs, camera rows), the scenes (a clip scene and a tracking scene, both in PIXELS), and the helpers - `device_rows` (one
r3d_clips_encode call: what a row-fed lifter is given, so that pixel-fed and row-fed runs are compared device against device) and
`oracle_poses` (the restated, repaired, HOST-encoded history of every emitted frame through oracle/torch_port.py: compared under
the literal 1e-4 only, never by bits - the device encode and the host chain agree to one float32 ulp)."""
import functools
import types

import numpy as np
import torch

import streams_assign_cases as ac
import streams_peek_cases as pk
import streams_repair_cases as rc
from conftest import case_out_scale, load_model_fixture, synth_states
from ray3d_amd import _capi, evaluate
from streams_cases import DRAIN, IDLE, PUSH, RESTART, garbage_frame
from test_clips_encode_host import KPS, cameras, host_encode, pixels

# ------------------------------------------------------------------------------------ fixtures

# name -> the pixel encodings its pair takes.  j17_rf9_s1: RF 9, lag 4, camera embedding, centred; j17_f2_rf27_noemb_s3: RF 27, lag
# 13, two features, no embedding; j14_rf9_dense_causal_s2: RF 9, lag 0, 14 joints (left / right from KPS[14]).
FIXTURES = {"j17_rf9_s1": ("ray",), "j17_f2_rf27_noemb_s3": ("intrinsic", "screen"), "j14_rf9_dense_causal_s2": ("ray",)}
CENTRED, TWO_FEATURE, CAUSAL = FIXTURES
REPAIR, MIN_CONF = 2, 0.3
FUSE = dict(fuse_soft_px=2.0, fuse_max_px=2000.0, fuse_max_dist=0.5)     # (a residual of two image widths; half a metre)


@functools.lru_cache(maxsize=None)
def states(name):
    """-> ((pos config, pos state), (trj config, trj state)): the deterministic weights of the golden fixtures."""
    _, mc = load_model_fixture(name)
    return synth_states(mc, case_out_scale(name))


def shape_of(name):
    """-> (RF, lag, J, F)."""
    cp = states(name)[0][0]
    rf = cp.receptive_field
    return rf, (0 if cp.causal else (rf - 1) // 2), cp.num_joints, cp.in_features


def looks_of(name):
    lag = shape_of(name)[1]
    return (0, lag - 1) if lag else None


def stream_cameras(indices):
    """The cameras of tests/test_clips_encode_host.py by index: 0 .. 3 distorted H36M rows, 4 .. 7 the same with zero coefficients."""
    cams = [cameras()[i] for i in indices]
    assert any(np.abs(c.cam_row(distortion=True)[8:13]).max() > 0 for c in cams)
    assert any(np.abs(c.cam_row(distortion=True)[8:13]).max() == 0 for c in cams)     # an undistorting row beside an identity row
    return cams


def camera_rows(name, cams):
    """What set_cameras takes for these streams: cam_rows (with res_w / res_h in slots 6 / 7: the screen encoding reads them),
    transforms, and params for a pair with a camera embedding."""
    rows = dict(cam_rows=np.stack([c.cam_row(distortion=True) for c in cams]), transforms=np.stack([c.stream_pose_row() for c in cams]))
    if states(name)[0][0].camera_embedding:
        rows["params"] = np.stack([c.param() for c in cams])
    return rows


# ------------------------------------------------------------------------------------ the clip scene

CLIP_CAMERAS = (5, 2, 2, 1)        # stream 0 an identity row, streams 1 and 2 share a distorted camera, stream 3 stays IDLE
LIFT_CAMERAS = (1, 5, 2, 6)        # lift_clips: distorted, identity, distorted, and the idle stream
S_CLIPS = 4
GROUPS = [[1, 2], [0, 3]]          # the shared-camera pair; a group that is empty whenever stream 0 has no pose (3 never has one)
SECOND_CLIP = 7                    # frames of the clip that RESTARTs stream 0 after its drain


def pixel_clips(name, tag):
    """Pixel clips of 1, 5 and 2 RF + 3 frames (the longest wraps the ring twice)."""
    rf, _, J, _ = shape_of(name)
    return [pixels("live.%s.%s.%d" % (name, tag, k), (n, J, 2)) for k, n in enumerate((1, 5, 2 * rf + 3))]


HOLE_KINDS = ("nan", "+inf", "-inf", "nan0", "nan1")


def punch_pixels(clips, holes):
    """The entries of `holes` - (clip, joint or None = every joint, first frame, last frame) - made non-finite, the kind rotating:
    a NaN pixel, +Inf or -Inf in one component, a NaN in component 0 only, in component 1 only.  -> (clips, observed per clip)."""
    clips = [c.copy() for c in clips]
    observed = [np.ones(c.shape[:2], bool) for c in clips]
    for h, (s, j, f0, f1) in enumerate(holes):
        for f in range(f0, min(f1, clips[s].shape[0] - 1) + 1):
            for jj in (range(clips[s].shape[1]) if j is None else [j]):
                kind = HOLE_KINDS[(h + f) % len(HOLE_KINDS)]
                if kind == "nan":
                    clips[s][f, jj] = np.nan
                elif kind in ("+inf", "-inf"):
                    clips[s][f, jj, (f + jj) % 2] = np.inf if kind == "+inf" else -np.inf
                else:
                    clips[s][f, jj, int(kind[-1])] = np.nan
                observed[s][f, jj] = False
    return clips, observed


def clip_holes(rf):
    """Gaps on the long clip (index 2), all behind its first five frames - gaps of 1 and REPAIR frames (interpolated), of REPAIR + 1
    (held), a gap across ring slot RF - 1 -> 0, a frame with every joint missing, a gap still open at the end - one on the clip of 5
    frames, and on the clip that restarts stream 0 (index 3) a leading gap (back-filled) and a gap of two."""
    n = 2 * rf + 3
    return [(2, 3, 6, 6), (2, 1, 5, 5 + REPAIR - 1), (2, 5, 8, 8 + REPAIR), (2, 6, 12, 12), (2, 8, rf - 1, rf), (2, None, rf + 2, rf + 2),
            (2, 7, 2 * rf - 2, 2 * rf), (2, 9, n - 2, n - 1), (1, 2, 2, 2), (3, 4, 0, 0), (3, 11, 3, 4)]


@functools.lru_cache(maxsize=None)
def clip_scene(name, with_conf):
    """The clips side by side on streams 0 .. 2 (RESTART, PUSH ..., DRAIN x lag, IDLE), stream 3 IDLE throughout, and a second clip
    RESTARTed on stream 0 one tick after its drain.  The long clip begins with the frames of the clip of 5, gap included: streams 1
    and 2 share a camera, so the window of frame 0 - and without confidences its pose - is the same on both, and the group of the
    two is fused from both cameras there; every later window differs.  -> dict(ticks [(frame (S, J, 2), action (S,), conf (S, J) or None)], clips,
    observed); the frame rows of streams that deliver nothing hold NaNs with a payload, their confidences NaN."""
    rf, lag, J, _ = shape_of(name)
    clips = pixel_clips(name, "scene") + [pixels("live.%s.scene.second" % name, (SECOND_CLIP, J, 2))]
    clips, observed = punch_pixels(clips, clip_holes(rf))
    assert observed[2][:5].all()
    clips[2][:5], observed[2][:5] = clips[1], observed[1]
    start2 = 1 + lag + 1
    first = [0, 0, 0, start2]                              # (clip k starts at tick first[k])
    stream_of = [0, 1, 2, 0]
    T = max(f + c.shape[0] for f, c in zip(first, clips)) + lag + 1
    rng = np.random.RandomState(71)
    ticks = []
    for t in range(T):
        frame, act = garbage_frame(S_CLIPS, J, 2), np.full(S_CLIPS, IDLE, np.int32)
        conf = np.full((S_CLIPS, J), np.nan, np.float32) if with_conf else None
        for k, (c, f0, s) in enumerate(zip(clips, first, stream_of)):
            n = t - f0
            if 0 <= n < c.shape[0]:
                frame[s], act[s] = c[n], (RESTART if n == 0 else PUSH)
                if with_conf:               # a tenth of the joints below min_conf, one in forty with a NaN confidence
                    conf[s] = rng.uniform(0.5, 1.0, J)
                    conf[s][rng.uniform(size=J) < 0.1] = 0.2
                    conf[s][rng.uniform(size=J) < 0.025] = np.nan
            elif c.shape[0] <= n < c.shape[0] + lag:
                act[s] = DRAIN
        ticks.append((frame, act, conf))
    return dict(ticks=ticks, clips=clips, observed=observed, S=S_CLIPS, cameras=CLIP_CAMERAS)


# ------------------------------------------------------------------------------------ the tracking scene

C_LIVE, P_LIVE, D_LIVE = 2, 3, 4
S_LIVE = C_LIVE * P_LIVE
TICKS = 40
MAX_MISSED = 2
TRACK_CAMERAS = (1, 1, 1, 6, 6, 6)     # camera 0 a distorted row, camera 1 an identity row, each repeated over its slots
TRACK_GROUPS = [[0, 3], [1, 4], [2, 5]]
HOMES = {"A": (200, 250), "B": (500, 300), "E": (800, 250), "F": (250, 700), "G": (600, 720), "H": (800, 780)}
SPANS = {"A": (0, TICKS), "B": (2, 15), "E": (25, TICKS), "F": (27, 33), "G": (28, 33), "H": (29, 33)}
LATE_JOINT = 5                          # of person E on camera 0: first delivered lag + 3 ticks after the birth


@functools.lru_cache(maxsize=None)
def tracking_scene(name, holes, with_conf):
    """Per tick (det (C, D, J, 2) pixels, counts (C,), conf (C, D, J) or None), in the style of tests/test_gpu_streams_assign.py but
    in pixel units: skeletons of 200 px that drift 2 px a tick, 1 px of detector noise.  Per camera person A all the way with a
    miss of two ticks, B from tick 2 to 14 (the track ends, drains and frees its slot), E from tick 25 (the slot is reused); on
    camera 1 also F, G and H for a few ticks - five people, D = 4, three slots: overflow, and births with no free slot.  The rows
    are shuffled every tick.  `holes`: 15 % of the joints are missing, and joint LATE_JOINT of E on camera 0 is first delivered
    lag + 3 ticks after the birth - the poses of E's first frames are legitimately NaN.  `with_conf`: detector confidences, a tenth
    below MIN_CONF."""
    _, lag, J, _ = shape_of(name)
    rng = np.random.RandomState(43)
    shape = 200.0 * ac.BONES[:J]
    out = []
    for t in range(TICKS):
        det = np.full((C_LIVE, D_LIVE, J, 2), np.nan, np.float32)
        conf = np.full((C_LIVE, D_LIVE, J), np.nan, np.float32) if with_conf else None
        counts = np.zeros(C_LIVE, np.int32)
        for c in range(C_LIVE):
            rows = []
            for who, (a, b) in SPANS.items():
                if not a <= t < b or (who == "A" and t in (10, 11)) or (who in "FGH" and c == 0):
                    continue
                xy = np.array(HOMES[who], np.float64) + 2.0 * t * np.array([1.0, -0.5]) + shape + rng.normal(0, 1.0, (J, 2))
                row = xy.astype(np.float32)
                assert row.min() > 0 and row.max() < 1000
                if holes:
                    row[rng.uniform(size=J) < 0.15] = np.nan
                    if who == "E" and c == 0 and t < SPANS["E"][0] + lag + 3:
                        row[LATE_JOINT] = np.nan
                cf = rng.uniform(0.5, 1.0, J).astype(np.float32)
                cf[rng.uniform(size=J) < 0.1] = 0.2
                rows.append((row, cf))
            order = rng.permutation(len(rows))
            for d, k in enumerate(order[:D_LIVE]):
                det[c, d] = rows[k][0]
                if with_conf:
                    conf[c, d] = rows[k][1]
            counts[c] = len(rows)                                    # (camera 1 at ticks 29 - 32: five people, D = 4 - read clamped)
        out.append((det, counts, conf))
    assert max(int(n[1]) for _, n, _ in out) == 5
    return tuple(out)


def member_table(groups):
    """The (G, 16) int32 member table r3d_streams_fuse reads: stream indices, empty slots -1."""
    table = np.full((len(groups), _capi.FUSE_MAX_MEMBERS), -1, np.int32)
    for g, row in enumerate(groups):
        table[g, :len(row)] = row
    return table


def assign_params(name, fill, min_conf):
    _, lag, J, _ = shape_of(name)
    return dict(C=C_LIVE, P=P_LIVE, D=D_LIVE, J=J, width=2, lag=lag, min_joints=4, min_common=3, max_missed=MAX_MISSED,
                fill=ac.FILL_NAN if fill == "nan" else ac.FILL_HOLD, min_conf=min_conf, max_cost=0.5)


def assigned(name, scene, fill, min_conf):
    """tests/streams_assign_cases.restate over the scene -> per tick its outputs (action, frame_out, conf_out, match, id, stats)."""
    prm = assign_params(name, fill, min_conf)
    st = ac.unpack_state(np.zeros(ac.state_bytes(C_LIVE, P_LIVE, prm["J"], 2), np.uint8), C_LIVE, P_LIVE, prm["J"], 2)
    return [ac.restate(st, prm, det, conf, counts) for det, counts, conf in scene]


def assigned_ticks(wants, repair):
    """The (frame, action, conf) a lifter without cameras= is stepped with: what the assign call wrote."""
    return [(w["frame_out"].view(np.float32), w["action"], w["conf_out"].view(np.float32) if repair is not None else None) for w in wants]


# ------------------------------------------------------------------------------------ the restated history

def fresh_model(S, rf, lag, J, F, perm, max_gap, min_conf, encode):
    """tests/streams_repair_cases.Restatement on a zeroed state and track."""
    heads = np.zeros(S, _capi.stream_head_dtype())
    rig = types.SimpleNamespace(S=S, rf=rf, lag=lag, J=J, F=F, width=2, perm=perm, max_gap=max_gap or 0, min_conf=min_conf,
                                state=lambda: (heads, np.zeros((S, rf, J, F), np.uint32)),
                                track=lambda: (np.zeros((S, J), np.int32), np.zeros((S, J, 2), np.uint32), np.zeros((S, rf), np.uint32)))
    return rc.Restatement(rig, encode)


def host_encoder(cams, encoding):
    """`encode` of the restatement through the HOST chain (Camera.rays_from_uv / intrinsic_from_uv / screen_from_uv in float64,
    one cast)."""
    cache = {}

    def encode(s, row):
        key = (s, int(row[0]), int(row[1]))
        if key not in cache:
            with np.errstate(all="ignore"):
                cache[key] = rc.bits(host_encode(cams[s], np.asarray(row, np.uint32).view(np.float32), encoding)).copy()
        return cache[key]
    return encode


def history(name, encoding, cams, ticks, repair, min_conf=0.0, looks=None, encode=None):
    """The tick-wise restatements over `ticks` [(frame (S, J, 2) pixels, action, conf or None)] on host-encoded rows (`encode`:
    another encoder) -> per tick dict(emit (S,), status, synthetic (S,) or None, observed (S, J) bool or None, pushed,
    x {s: the emitted frame's reference window (RF, J, F) float32}, finite {s: bool}, previews [per look dict(frames (S,),
    x {s: window}, finite {s: bool})], ring, count).  `repair` None: the step alone."""
    rf, lag, J, F = shape_of(name)
    S = len(cams)
    model = fresh_model(S, rf, lag, J, F, None, repair, np.float32(min_conf), encode or host_encoder(cams, encoding))
    out = []
    for frame, action, conf in ticks:
        fb = rc.bits(np.asarray(frame, np.float32))
        rec = dict(synthetic=None, observed=None)
        if repair is not None:
            rows, syn, pushed = model.repair(frame, action, conf)
            obs = np.array([[all(rc.finite_bits(b) for b in fb[s, j]) and (conf is None or bool(np.float32(conf[s][j]) >= np.float32(min_conf)))
                             for j in range(J)] for s in range(S)])
            rec.update(synthetic=syn.copy(), observed=obs)
        else:
            rows = fb
        x, _, emit, status = model.step(rows, action)
        rec.update(emit=emit, status=status, action=np.asarray(action).copy(), x={s: w.view(np.float32) for s, w in x.items()},
                   ring=model.ring.copy(), count=list(model.count))
        rec["finite"] = {s: bool(np.isfinite(w).all()) for s, w in rec["x"].items()}
        rec["previews"] = []
        for L in looks or ():
            frames, wins = np.full(S, -1, np.int64), {}
            for s in range(S):
                p, _ = pk.verdict(model.count[s], model.drained[s], int(action[s]), int(status[s]), L, lag)
                frames[s] = p
                if p >= 0:
                    wins[s] = pk.window_of_ring(model.ring[s], p, model.count[s], rf, lag).view(np.float32)
            rec["previews"].append(dict(look=L, frames=frames, x=wins, finite={s: bool(np.isfinite(w).all()) for s, w in wins.items()}))
        out.append(rec)
    return out


def finite_share(hist):
    """-> (emitting (tick, stream) pairs, those with an all-finite reference window)."""
    flags = [ok for rec in hist for ok in rec["finite"].values()]
    return len(flags), int(np.sum(flags))


def gap_census(hist, max_gap):
    """From the restated observations alone: how many gaps were closed by interpolation, how many were only held, how many joints
    were back-filled, how many joints a pushed frame lacked - per joint the run of missing frames since the stream's RESTART."""
    S, J = hist[0]["observed"].shape
    age = np.zeros((S, J), np.int64)        # 0: never observed since the RESTART; k: observed k - 1 frames ago
    frames = np.zeros(S, np.int64)
    n = dict(interpolated=0, held=0, backfilled=0, missing=0, closures=[])
    for t, rec in enumerate(hist):
        for s in range(S):
            a = int(rec["action"][s])
            if rec["status"][s] != 0 or a not in (PUSH, RESTART):
                continue
            if a == RESTART:
                age[s], frames[s] = 0, 0
            for j in range(J):
                if rec["observed"][s, j]:
                    gap = age[s, j] - 1
                    if age[s, j] == 0 and frames[s] >= 1:
                        n["backfilled"] += 1
                    elif 1 <= gap <= max_gap and gap + 1 <= frames[s]:
                        n["interpolated"] += 1
                        n["closures"].append((t, s, j, int(gap)))
                    elif gap >= 1:
                        n["held"] += 1
                    age[s, j] = 1
                else:
                    n["missing"] += 1
                    age[s, j] += age[s, j] > 0
            frames[s] += 1
    return n


# ------------------------------------------------------------------------------------ the runs both suites look at

CLIP_CASES = [(True, REPAIR), (False, 0)]                            # (confidences, repair): the clip scene on the centred fixture
TRACK_CASES = [(CENTRED, "nan", REPAIR, True), (CENTRED, "hold", None, False), (CAUSAL, "nan", REPAIR, False), (CAUSAL, "hold", None, False)]
TRACK_IDS = ["centred-nan-repair-conf", "centred-hold", "causal-nan-repair", "causal-hold"]       # (fixture, fill, repair, confidences)


@functools.lru_cache(maxsize=None)
def clip_history(with_conf, repair):
    """-> (scene, cameras, history on host-encoded rows) of the clip scene on the centred fixture."""
    scn = clip_scene(CENTRED, with_conf)
    cams = stream_cameras(scn["cameras"])
    return scn, cams, history(CENTRED, "ray", cams, scn["ticks"], repair, MIN_CONF if with_conf else 0.0, looks_of(CENTRED))


@functools.lru_cache(maxsize=None)
def track_history(name, fill, repair, with_conf):
    """-> (scene, cameras, the assign restatement's outputs per tick, history on host-encoded rows) of the tracking scene."""
    scene = tracking_scene(name, repair is not None, with_conf)
    cams = stream_cameras(TRACK_CAMERAS)
    min_conf = MIN_CONF if with_conf else 0.0
    wants = assigned(name, scene, fill, min_conf)
    return scene, cams, wants, history(name, "ray", cams, assigned_ticks(wants, repair), repair, min_conf, looks_of(name))


# ------------------------------------------------------------------------------------ the oracle

@functools.lru_cache(maxsize=None)
def _state_dicts(name):
    (cp, sp), (ct, st) = states(name)
    return cp, ct, [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]


def lift(name, windows, params, flip):
    """oracle/torch_port.forward (pos + trj) on `windows` (n, RF, J, F), and with `flip` on their mirrored twins, then the flip
    average - exactly as `oracle_chain` of tests/test_gpu_streams.py does it.  -> (n, J, 3) float32."""
    from oracle import torch_port
    cp, ct, sds = _state_dicts(name)
    left, right = KPS[cp.num_joints]
    windows = np.ascontiguousarray(windows, np.float32)
    n = windows.shape[0]

    def run(w):
        with torch.no_grad():
            xw, pw = torch.from_numpy(w), (torch.from_numpy(np.ascontiguousarray(params, np.float32)) if params is not None else None)
            return (torch_port.forward(cp, sds[0], xw, pw) + torch_port.forward(ct, sds[1], xw, pw)).numpy().reshape(n, -1, 3)
    ref = run(windows)
    if not flip:
        return ref
    wm = windows.copy()
    wm[..., 0] *= -1
    wm[:, :, left + right] = wm[:, :, right + left]
    refm = run(wm)
    refm[..., 0] *= -1
    refm[:, left + right] = refm[:, right + left]
    return (0.5 * (ref.astype(np.float64) + refm)).astype(np.float32)


def oracle_poses(name, hist, cams, flip=True):
    """Every all-finite reference window of `hist` (:func:`history` on host-encoded rows) - the emitted frames' and every look's -
    through :func:`lift`, in ONE batch.  -> per tick dict(poses {s: (J, 3)}, previews [per look {s: (J, 3)}]); a pair whose window is
    not all finite is absent: the device's pose must be non-finite there."""
    embed = states(name)[0][0].camera_embedding
    wins, prm, where = [], [], []
    for t, rec in enumerate(hist):
        for s, w in rec["x"].items():
            if rec["finite"][s]:
                wins.append(w), prm.append(cams[s].param()), where.append((t, None, s))
        for k, pv in enumerate(rec["previews"]):
            for s, w in pv["x"].items():
                if pv["finite"][s]:
                    wins.append(w), prm.append(cams[s].param()), where.append((t, k, s))
    poses = lift(name, np.stack(wins), np.stack(prm) if embed else None, flip)
    out = [dict(poses={}, previews=[{} for _ in rec["previews"]]) for rec in hist]
    for (t, k, s), p in zip(where, poses):
        (out[t]["poses"] if k is None else out[t]["previews"][k])[s] = p
    return out


# ------------------------------------------------------------------------------------ the device's own rows

def device_rows(px, cam_row, encoding, device="cuda:0"):
    """One r3d_clips_encode call: `px` (N, J, 2) float32 pixels through one 16-double camera row -> (N, J, F) float32, the bits the
    step's ring holds for them (test_pixel_rings_hold_what_clips_encode_writes).  A keypoint that is not finite in the pixels is
    NaN in the rows: to a row-fed lifter it is then as little observed as it is to a pixel-fed one."""
    dev = torch.device(device)
    px = np.ascontiguousarray(px, np.float32)
    N, J = px.shape[:2]
    enc = evaluate.ENCODINGS[encoding]
    F = _capi.ENCODE_FLOATS[enc]
    table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
    table[0]["n_frames"], table[0]["cam"] = N, cam_row
    x = torch.full((N, J, F), -7.0, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    p_dev, t_dev = torch.from_numpy(px).to(dev), torch.from_numpy(table.view(np.uint8)).to(dev)
    _capi.clips_encode(p_dev.data_ptr(), N, J, enc, t_dev.data_ptr(), 1, N, x.data_ptr(), N, None, None, status.data_ptr(),
                       torch.cuda.current_stream(dev).cuda_stream)
    rows = x.cpu().numpy()
    assert status.tolist() == [0]
    rows[~np.isfinite(px).all(-1)] = np.nan
    return rows
