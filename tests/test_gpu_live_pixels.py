"""GPU suite of the end-to-end layer: OnlineLifter fed RAW PIXELS from distorted cameras, with every option on at once, on the scenes
of tests/live_cases.py (tests/test_live_pixels_host.py proves from the restatements that they hold every case).  The rule that keeps
the bit comparisons honest: the device encode and the float64 host chain agree to one float32 ulp, not to the bit (DESIGN 4.7 /
4.10), so nothing downstream of a pixel encode is compared bit for bit with something that went through the host encode.  Bits are
compared device against device - a pixel-fed lifter against a row-fed one (encoding=None) whose rows are what r3d_clips_encode
writes on the device for the same pixels and camera row; an eager tick against a captured one; a lifter with every option against
one with fewer.  The host chain enters twice: under the one-ulp rule for the encoded rows themselves, and under the literal 1e-4
(conftest.check_parity) for the poses against the oracle chain on the restated, repaired, host-encoded history.  World poses,
residuals, quality and the fused skeletons are the NumPy restatements applied to the device's own poses and extras."""
import functools
import time

import numpy as np
import pytest
import torch

import live_cases as lc
import streams_fuse_cases as fc
import streams_poses_cases as pc
import streams_repair_cases as rc
from conftest import check_parity
from live_cases import CAUSAL, CENTRED, FUSE, MIN_CONF
from test_clips_encode_host import KPS, host_encode, ulps
from test_gpu_streams import pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAPTURE_AFTER = 7                  # the all-on clip run is captured after tick 7, in the middle of every clip
FINISH = ("world", "reproj", "quality")
FUSED = ("fused", "fused_spread", "fused_count", "fused_used")


def _online(name, S, encoding, **kw):
    import ray3d_amd
    lifter, _ = pair(name)
    left, right = KPS[lifter.pos.num_joints_in]
    return ray3d_amd.OnlineLifter(lifter, S, encoding=encoding, kps_left=left, kps_right=right, device=DEV, **kw)


def _done(name):
    pair(name)[0].check_status(torch.device(DEV))


def _cpu(res):
    """What step() / track() returned, as NumPy copies: dict(poses, frames, and the extras' keys; previews a list of dicts)."""
    poses, frames, *rest = res
    out = dict(poses=poses.cpu().numpy(), frames=frames.cpu().numpy())
    for k, v in (rest[0] if rest else {}).items():
        out[k] = [{kk: (vv.cpu().numpy() if hasattr(vv, "cpu") else vv) for kk, vv in pv.items()} for pv in v] if k == "previews" else v.cpu().numpy()
    return out


def _rows_agree(a, b, live, keys, what, any_nan=False):
    for k in keys:
        x, y = a[k][live], b[k][live]
        assert a[k].dtype == b[k].dtype and x.shape == y.shape, (what, k)
        if any_nan and k == "poses":
            nan = np.isnan(x)
            assert np.array_equal(nan, np.isnan(y)) and np.array_equal(pc.bits(x)[~nan], pc.bits(y)[~nan]), (what, k)
        else:
            assert pc.same_bits(x, y), (what, k)


def _agree(a, b, what, keys=None, any_nan=False):
    """Two ticks are the same bits: frames; poses, world, reproj and quality on the live rows (rows of streams without a pose keep
    what an earlier tick left); synthetic, the fused outputs and the tracking words whole; every look's frames and live rows.
    `any_nan` (a pixel-fed lifter against a row-fed one): a float32 pose that is not a number is not one in both - for a joint never
    observed the one ring holds the encoding of a NaN pixel, the other a NaN row, and the payload of what the network makes of
    either is not part of the comparison; every number is, and so are the float64 outputs, whose NaN is canonical by contract."""
    keys = set(a) if keys is None else set(keys)
    assert keys <= set(a) and keys <= set(b), (what, sorted(a), sorted(b))
    assert np.array_equal(a["frames"], b["frames"]), (what, "frames")
    live = a["frames"] >= 0
    _rows_agree(a, b, live, [k for k in ("poses",) + FINISH if k in keys], what, any_nan)
    for k in keys - {"poses", "frames", "previews"} - set(FINISH):
        assert a[k].dtype == b[k].dtype and pc.same_bits(a[k], b[k]), (what, k)
    if "previews" in keys:
        assert [p["look"] for p in a["previews"]] == [p["look"] for p in b["previews"]], what
        for pa, pb in zip(a["previews"], b["previews"]):
            assert set(pa) == set(pb) and np.array_equal(pa["frames"], pb["frames"]), (what, "look", pa["look"])
            _rows_agree(pa, pb, pa["frames"] >= 0, [k for k in pa if k not in ("look", "frames")], (what, "look", pa["look"]), any_nan)


def _check_finish(rec, rows, ray, what, table=None, repair=True):
    """world / reproj / quality (and the fused outputs) of one tick - or of one look - are the restatements applied to the device's
    own poses: tests/streams_poses_cases.world_of within 1e-12, reproj_of and quality_of and tests/streams_fuse_cases.restate by
    bits.  `ray`: the centre rows of the device's own windows - the keypoints the residuals are measured against."""
    live = rec["frames"] >= 0
    p = rec["poses"]
    world = pc.world_of(rows["transforms"], p)
    assert np.allclose(rec["world"][live], world[live], rtol=0, atol=1e-12, equal_nan=True), (what, "world")
    assert np.array_equal(np.isnan(rec["world"][live]), np.isnan(world[live])), (what, "world")
    res = pc.reproj_of(rows["transforms"], rows["cam_rows"], p, ray)
    assert pc.same_bits(rec["reproj"][live], res[live]), (what, "reproj")
    assert pc.same_bits(rec["quality"][live], pc.quality_of(res)[live]), (what, "quality")
    if table is None:
        return None
    S = p.shape[0]
    want = fc.restate(rec["world"], rec["reproj"], rec["frames"], np.zeros(S, np.int32), rec["synthetic"].view(np.uint32) if repair else None,
                      table, FUSE["fuse_soft_px"], FUSE["fuse_max_px"], FUSE["fuse_max_dist"])
    fc.agree(dict(fused=fc.bits64(rec["fused"]), spread=fc.bits64(rec["fused_spread"]), count=rec["fused_count"],
                  used=fc.bits32(rec["fused_used"])), want, what)
    return want


def _candidates(rec, table, want):
    """-> (how many (group, joint) pairs have two members with a pose and a finite world joint this tick, how many of them a GATE
    cut down to one member or none: both residuals finite and both joints observed or both synthetic, so that neither a missing
    residual nor the rule that a synthetic keypoint does not vote against an observed one explains it)."""
    n = gated = 0
    for g, row in enumerate(table):
        members = [s for s in row if s >= 0 and rec["frames"][s] >= 0]
        if len(members) == 2:
            both = np.isfinite(rec["world"][members]).all(-1).all(0)
            syn = np.array([[(int(w) >> j) & 1 for j in range(both.size)] for w in rec["synthetic"][members].view(np.uint32)])
            clean = both & np.isfinite(rec["reproj"][members]).all(0) & (syn[0] == syn[1])
            n, gated = n + int(both.sum()), gated + int((clean & (want["count"][g] < 2)).sum())
    return n, gated


def _against_the_oracle(name, recs, hist, cams, what):
    """Final poses and every look's against :func:`live_cases.oracle_poses`, the literal 1e-4: every (tick, stream) pair that emits,
    but those whose restated reference window is not all finite - there the device's pose must be non-finite too.  -> the line
    for the summary."""
    oracle = lc.oracle_poses(name, hist, cams, flip=True)
    got, ref, pgot, pref, pairs, skipped = [], [], [], [], 0, 0
    for t, (rec, h, o) in enumerate(zip(recs, hist, oracle)):
        assert np.array_equal(rec["frames"], h["emit"]), (what, t)
        for s in h["x"]:
            pairs += 1
            if s in o["poses"]:
                got.append(rec["poses"][s]), ref.append(o["poses"][s])
            else:
                skipped += 1
                assert not np.isfinite(rec["poses"][s]).all(), (what, t, s)
        for k, pv in enumerate(h["previews"]):
            assert np.array_equal(rec["previews"][k]["frames"], pv["frames"]), (what, t, pv["look"])
            for s in pv["x"]:
                if s in o["previews"][k]:
                    pgot.append(rec["previews"][k]["poses"][s]), pref.append(o["previews"][k][s])
                else:
                    assert not np.isfinite(rec["previews"][k]["poses"][s]).all(), (what, t, pv["look"], s)
    assert (pairs, pairs - skipped) == lc.finite_share(hist)                       # the host suite's number
    err = check_parity(np.stack(got), np.stack(ref), "%s final poses vs the oracle chain" % what)
    line = "%s: %d of %d emitting pairs compared, worst pose error %.3e" % (what, pairs - skipped, pairs, err)
    if pgot:
        perr = check_parity(np.stack(pgot), np.stack(pref), "%s preview poses vs the oracle chain" % what)
        line += "; %d previews, worst %.3e" % (len(pgot), perr)
    return line


# ------------------------------------------------------------------ 1. lift_clips from pixels

LIFT_CASES = [(name, enc) for name, encs in lc.FIXTURES.items() for enc in encs]


def _lift_rows(name):
    cams = lc.stream_cameras(lc.LIFT_CAMERAS)
    return cams, lc.camera_rows(name, cams)


@functools.lru_cache(maxsize=None)
def _row_fed_lift(name, encoding, flip):
    """-> (the device's rows per clip, the poses per clip of a row-fed lifter on them, eager) - computed once per case."""
    _, rows = _lift_rows(name)
    clips = lc.pixel_clips(name, "lift")
    dev_rows = [lc.device_rows(c, rows["cam_rows"][s], encoding, DEV) for s, c in enumerate(clips)]
    ol = _online(name, len(lc.LIFT_CAMERAS), None, flip=flip)
    if "params" in rows:
        ol.set_cameras(params=rows["params"])
    return dev_rows, [p.cpu().numpy() for p in ol.lift_clips(dev_rows)]


@functools.lru_cache(maxsize=None)
def _lift_oracle(name, encoding, flip):
    """The oracle chain on the HOST-encoded clips: the reference's windows (edge padding + slicing), pos + trj, the flip average."""
    cams, rows = _lift_rows(name)
    rf, lag, _, _ = lc.shape_of(name)
    out = []
    for s, c in enumerate(lc.pixel_clips(name, "lift")):
        windows = rc.reference_windows(host_encode(cams[s], c, encoding), rf, lag)
        out.append(lc.lift(name, windows, np.tile(rows["params"][s], (c.shape[0], 1)) if "params" in rows else None, flip))
    return out


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("name,encoding", LIFT_CASES, ids=["%s-%s" % c for c in LIFT_CASES])
def test_lift_clips_from_pixels(name, encoding, flip, captured):
    """Pixel clips of 1, 5 and 2 RF + 3 frames and an idle stream, distorted and zero-coefficient camera rows side by side: the
    poses are bit-equal to a row-fed lifter on the device's own rows; those rows are within one ulp of the host chain; the poses are
    within 1e-4 of the oracle chain on the host-encoded clips."""
    t0 = time.time()
    cams, rows = _lift_rows(name)
    clips = lc.pixel_clips(name, "lift")
    dev_rows, want = _row_fed_lift(name, encoding, flip)
    ol = _online(name, len(lc.LIFT_CAMERAS), encoding, flip=flip)
    assert ol.width == 2 and tuple(ol.frame.shape) == (4, clips[0].shape[1], 2)
    try:
        ol.set_cameras(cam_rows=rows["cam_rows"], params=rows.get("params"))
        if captured:
            ol.capture()
        got = [p.cpu().numpy() for p in ol.lift_clips(clips)]
        _done(name)
    finally:
        ol.release()
    equal = total = 0
    for s, (c, g, w, d, ref) in enumerate(zip(clips, got, want, dev_rows, _lift_oracle(name, encoding, flip))):
        assert g.shape == (c.shape[0], c.shape[1], 3) and pc.same_bits(g, w), ("pixel-fed against row-fed", s)
        host = host_encode(cams[s], c, encoding)
        assert ulps(d, host) <= 1, ("device rows against the host chain", s)
        equal, total = equal + int((d == host).sum()), total + d.size
        check_parity(g, ref, "clip of %d frames vs the oracle chain" % c.shape[0])
    print("lift_clips %s %s flip=%s captured=%s: %.6f of %d encoded elements equal to the host chain; %.2f s"
          % (name, encoding, flip, captured, equal / total, total, time.time() - t0))


# ------------------------------------------------------------------ 2. every option on, step()

def _clip_rows():
    cams = lc.stream_cameras(lc.CLIP_CAMERAS)
    return cams, lc.camera_rows(CENTRED, cams)


def _all_on(with_conf, repair, encoding="ray", **over):
    kw = dict(flip=True, world=True, quality=True, repair=repair, min_conf=MIN_CONF if with_conf else 0.0, previews=lc.looks_of(CENTRED),
              groups=lc.GROUPS, **FUSE)
    kw.update(over)
    ol = _online(CENTRED, lc.S_CLIPS, encoding, **kw)
    ol.set_cameras(**_clip_rows()[1])
    return ol


def _play(ol, ticks, frames=None, capture_after=None):
    """step() over the scene's ticks (`frames`: other frame rows for them) -> per tick :func:`_cpu` of the result, and the centre
    rows of the lifter's own windows (`ray`, per look `pray`)."""
    out, c = [], ol.rf - 1 - ol.lag
    for t, (frame, act, conf) in enumerate(ticks):
        f = frame if frames is None else frames[t]
        rec = _cpu(ol.step(f, act, conf=conf) if conf is not None else ol.step(f, act))
        rec["ray"] = ol.x[:, c].cpu().numpy()
        if ol.looks:
            rec["pray"] = ol.px[:, :, c].cpu().numpy()
        out.append(rec)
        if t == capture_after:
            ol.capture()
    return out


@functools.lru_cache(maxsize=None)
def _all_on_run(with_conf, repair):
    """The clip scene through the pixel-fed lifter with every option on, eager -> per tick what :func:`_play` keeps."""
    return tuple(_play(_all_on(with_conf, repair), lc.clip_scene(CENTRED, with_conf)["ticks"]))


@pytest.mark.parametrize("with_conf,repair", lc.CLIP_CASES, ids=["conf-repair2", "repair0"])
def test_every_option_on_step(with_conf, repair):
    """encoding="ray", flip, world, quality, repair, min_conf with confidences, previews (0, lag - 1), a shared-camera pair and a
    group that is empty at times, the fuse gates on - over the clip scene, RESTART after the drain included.  Pixel-fed eager,
    pixel-fed captured (after tick 7) and row-fed agree bit for bit in poses, frames and every key of the extras; world, reproj,
    quality and the fused skeletons - of the final poses and of every look - are the restatements on the device's own poses."""
    t0 = time.time()
    scn = lc.clip_scene(CENTRED, with_conf)
    ticks = scn["ticks"]
    _, rows = _clip_rows()
    table = lc.member_table(lc.GROUPS)
    eager = _all_on_run(with_conf, repair)
    cap, row_fed = _all_on(with_conf, repair), _all_on(with_conf, repair, encoding=None)
    px = np.stack([f for f, _, _ in ticks])                                         # (T, S, J, 2)
    dev_rows = np.stack([lc.device_rows(px[:, s], rows["cam_rows"][s], "ray", DEV) for s in range(lc.S_CLIPS)], 1)
    try:
        captured = _play(cap, ticks, capture_after=CAPTURE_AFTER)
        assert cap._graph is not None and len(ticks) > CAPTURE_AFTER + 10
        fed = _play(row_fed, ticks, frames=dev_rows)
        _done(CENTRED)
    finally:
        cap.release()
    dropped = two = gated = 0
    K = len(lc.looks_of(CENTRED))
    for t, (e, c, r) in enumerate(zip(eager, captured, fed)):
        assert set(e) == {"poses", "frames", "ray", "pray", "synthetic", "previews"} | set(FINISH) | set(FUSED), sorted(e)
        _agree(e, c, ("captured", t), set(e) - {"ray", "pray"})
        _agree(e, r, ("row-fed", t), set(e) - {"ray", "pray"}, any_nan=True)
        want = _check_finish(e, rows, e["ray"], ("final", t), table)
        n, cut = _candidates(e, table, want)
        dropped, two, gated = dropped + n - int((want["count"] == 2).sum()), two + int((want["count"] == 2).sum()), gated + cut
        for k in range(K):
            pv = e["previews"][k]
            assert set(pv) == {"look", "poses", "frames"} | set(FINISH)
            _check_finish(pv, rows, e["pray"][k], ("look", pv["look"], t))
    assert sum(int((e["synthetic"] != 0).sum()) for e in eager) > 0
    assert dropped > 0 and gated > 0, (dropped, gated, two)      # joints both cameras delivered that fuse_max_px / fuse_max_dist cut
    assert with_conf or two > 0, (dropped, two)  # (frame 0: the shared-camera pair saw the same window and is fused from both)
    print("every option on, step(), conf=%s repair=%d: %d ticks; joints fused from both cameras %d, left to one or none %d (%d of them by "
          "a gate); %.2f s" % (with_conf, repair, len(ticks), two, dropped, gated, time.time() - t0))


# ------------------------------------------------------------------ 3. options do not disturb each other

def _poses_agree(a, b, what):
    """The kernel finish (r3d_streams_poses) against the torch flip finish: the same float32 arithmetic, so the same bits wherever
    the pose is a number; a pose that is not a number is not one in both (the two finishes need not agree on a NaN's payload)."""
    assert np.array_equal(a["frames"], b["frames"]), what
    live = a["frames"] >= 0
    pa, pb = a["poses"][live], b["poses"][live]
    nan = np.isnan(pa)
    assert np.array_equal(nan, np.isnan(pb)) and np.array_equal(pc.bits(pa)[~nan], pc.bits(pb)[~nan]), what


def test_options_do_not_disturb_each_other():
    """With the same pixels: final poses and frames of the all-on lifter are those of a lifter with only encoding + flip + repair;
    world / reproj / quality are bit-equal to one without groups and previews; synthetic is bit-equal to one without world."""
    with_conf, repair = lc.CLIP_CASES[0]
    ticks = lc.clip_scene(CENTRED, with_conf)["ticks"]
    full = _all_on_run(with_conf, repair)
    few = _play(_all_on(with_conf, repair, world=False, quality=False, previews=None, groups=None), ticks)
    mid = _play(_all_on(with_conf, repair, previews=None, groups=None), ticks)
    _done(CENTRED)
    posed = 0
    for t, (a, b, m) in enumerate(zip(full, few, mid)):
        assert set(b) == {"poses", "frames", "ray", "synthetic"} and set(m) == set(b) | set(FINISH), (sorted(b), sorted(m))
        _poses_agree(a, b, ("encoding + flip + repair", t))
        assert pc.same_bits(a["synthetic"], b["synthetic"]), ("synthetic without world", t)
        _agree(a, m, ("without groups and previews", t), {"poses", "frames", "synthetic"} | set(FINISH))
        posed += int((a["frames"] >= 0).sum())
    assert posed == lc.finite_share(lc.clip_history(with_conf, repair)[2])[0]


# ------------------------------------------------------------------ 5. previews from the repaired ring (and the finals) against the oracle

@pytest.mark.parametrize("with_conf,repair", lc.CLIP_CASES, ids=["conf-repair2", "repair0"])
def test_finals_and_previews_from_the_repaired_ring_agree_with_the_oracle(with_conf, repair):
    """The all-on run against the oracle chain on the restated, repaired, host-encoded history: every final pose and every preview
    within 1e-4 - among them the look-0 preview of a frame at the tick its gap was closed by interpolation: the prefix window the
    peek reads from the ring the repair has just rewritten."""
    scn, cams, hist = lc.clip_history(with_conf, repair)
    recs = _all_on_run(with_conf, repair)
    print(_against_the_oracle(CENTRED, recs, hist, cams, "all-on clip scene conf=%s repair=%d" % (with_conf, repair)))
    for t, (rec, h) in enumerate(zip(recs, hist)):
        assert rec["synthetic"].view(np.uint32).tolist() == h["synthetic"].tolist(), t
    if repair:
        oracle = lc.oracle_poses(CENTRED, hist, cams, flip=True)
        closed = [(t, s) for t, s, _, _ in lc.gap_census(hist, repair)["closures"] if s in oracle[t]["previews"][0]]
        assert closed
        got = np.stack([recs[t]["previews"][0]["poses"][s] for t, s in closed])
        check_parity(got, np.stack([oracle[t]["previews"][0][s] for t, s in closed]), "look-0 previews at the tick a gap closed")
    _done(CENTRED)


# ------------------------------------------------------------------ 4. every option on, track() from pixel detections

def _trackers(name, fill, repair, with_conf):
    """-> (a pixel-fed lifter without cameras=, the tracking lifter, the one that is captured), every other option on."""
    cams = lc.stream_cameras(lc.TRACK_CAMERAS)
    rows = lc.camera_rows(name, cams)
    kw = dict(flip=True, world=True, quality=True, repair=repair, min_conf=MIN_CONF if with_conf else 0.0, groups=lc.TRACK_GROUPS, **FUSE)
    if lc.looks_of(name):
        kw["previews"] = lc.looks_of(name)
    track_kw = dict(cameras=lc.C_LIVE, max_detections=lc.D_LIVE, assign_max_cost=0.5, assign_max_missed=lc.MAX_MISSED, assign_fill=fill)
    ols = [_online(name, lc.S_LIVE, "ray", **kw), _online(name, lc.S_LIVE, "ray", **kw, **track_kw), _online(name, lc.S_LIVE, "ray", **kw, **track_kw)]
    for ol in ols:
        ol.set_cameras(**rows)
    return cams, rows, ols


@pytest.mark.parametrize("name,fill,repair,with_conf", lc.TRACK_CASES, ids=lc.TRACK_IDS)
def test_every_option_on_track_from_pixel_detections(name, fill, repair, with_conf):
    """40 ticks of pixel detections - a birth, a two-tick miss, an end, a drain (causal: IDLE) and a slot reuse, five people on a
    camera of four rows and three slots, shuffled rows, missing joints, a joint delivered late: track() eager and captured (after
    tick 3) equal, bit for bit, a pixel-fed lifter without cameras= stepped with the frame / action / conf of
    tests/streams_assign_cases.restate; track_id, match and assign_stats are the restatement's; the finish and the fused skeletons
    are the restatements on the device's own poses; the poses are within 1e-4 of the oracle chain.  Afterwards one eager step() on
    the tracking lifter behaves as a plain step."""
    t0 = time.time()
    scene, cams, wants, hist = lc.track_history(name, fill, repair, with_conf)
    _, rows, (plain, eager, cap) = _trackers(name, fill, repair, with_conf)
    table = lc.member_table(lc.TRACK_GROUPS)
    stepped = lc.assigned_ticks(wants, repair)
    lag, K = plain.lag, len(lc.looks_of(name) or ())
    assert (lag == 0) == (name == CAUSAL) and plain.width == 2 and tuple(eager._assign["det"].shape) == (lc.C_LIVE, lc.D_LIVE, plain.J, 2)
    recs, c = [], plain.rf - 1 - plain.lag
    try:
        for t, ((det, counts, conf), want, (frame, act, cf)) in enumerate(zip(scene, wants, stepped)):
            p = _cpu(plain.step(frame, act, conf=cf) if cf is not None else plain.step(frame, act))
            p["ray"] = plain.x[:, c].cpu().numpy()
            if K:
                p["pray"] = plain.px[:, :, c].cpu().numpy()
            for what, ol in (("eager", eager), ("captured", cap)):
                g = _cpu(ol.track(det, counts, conf=conf))
                assert set(g) == (set(p) - {"ray", "pray"}) | {"track_id", "match", "assign_stats"}, (what, t, sorted(g))
                _agree(p, g, (what, t), set(p) - {"ray", "pray"})
                assert g["track_id"].dtype == np.int64 and g["match"].dtype == np.int32 and g["assign_stats"].shape == (lc.C_LIVE, 4)
                assert np.array_equal(g["track_id"], want["id"]) and np.array_equal(g["match"], want["match"]), (what, t)
                assert np.array_equal(g["assign_stats"], want["stats"]), (what, t)
                assert np.array_equal(ol.action.cpu().numpy(), want["action"]), (what, t)
                assert pc.same_bits(ol.frame.cpu().numpy(), want["frame_out"].view(np.float32)), (what, t, "the assign state holds pixels")
            _check_finish(p, rows, p["ray"], ("final", t), table, repair is not None)
            for k in range(K):
                _check_finish(p["previews"][k], rows, p["pray"][k], ("look", k, t))
            recs.append(p)
            if t == 3:
                cap.capture()
        assert cap._graph is not None
        line = _against_the_oracle(name, recs, hist, cams, "track() %s" % lc.TRACK_IDS[lc.TRACK_CASES.index((name, fill, repair, with_conf))])
        if lag == 0:                        # a causal track ends with IDLE, not DRAIN
            assert not any((w["action"] == lc.DRAIN).any() for w in wants) and any(((w["action"] == lc.IDLE) & (w["id"] >= 0)).any() for w in wants)
        # one eager step() on the tracking lifter behaves as a plain step: _tracking falls back to False
        frame, act = np.full((lc.S_LIVE, plain.J, 2), np.nan, np.float32), np.full(lc.S_LIVE, lc.IDLE, np.int32)
        live = np.flatnonzero(wants[-1]["action"] == lc.PUSH)
        frame[live], act[live] = wants[-1]["frame_out"].view(np.float32)[live] + np.float32(1.5), lc.PUSH
        a, b = _cpu(plain.step(frame, act)), _cpu(eager.step(frame, act))
        assert eager._tracking is False and set(a) == set(b) and "track_id" not in b and (a["frames"] >= 0).any()
        _agree(a, b, "a plain step after the tracking run")
        with pytest.raises(ValueError, match="use track"):
            cap.step(frame, act)
        _done(name)
    finally:
        cap.release()
    print("%s; %.2f s" % (line, time.time() - t0))
