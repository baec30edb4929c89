"""What tests/test_streams_repair_host.py and tests/test_gpu_streams_repair.py share: a rig that keeps every buffer of
r3d_streams_repair and of the r3d_streams_step behind it inside guard bands (tests/buffers_util.py) and runs a tick on the host
hooks or on the device; a NumPy RESTATEMENT of the call's rules, written from the contract block of include/ray3d_hip.h (float64
scalar arithmetic rounded to float32; it does not call the library - the one exception is the encoding of a pixel, which the
contract DEFINES as the bits the step pushes: the pixel scenarios hand the restatement r3d_debug_clips_encode_host for it); the
reference's window builder (edge padding + slicing) and offline repair of a clip; the gapped inputs made from the clips of
tests/golden/windows.npz; the scenarios both suites play."""
import copy
import functools

import numpy as np
import torch

import buffers_util as bu
import streams_cases as sc
from conftest import hooks_library
from ray3d_amd import _capi, evaluate
from streams_cases import DRAIN, IDLE, NONE, PUSH, RESTART

QNAN = 0x7FC00000
INT32_MAX, COUNT_MAX = 2 ** 31 - 1, 1 << 62
FILL_BITS = 0xC0E00000            # -7.0f: what frame_out, x and x_mirror hold before every tick
FILL_SYN = 0x5EEDBEEF             # ... and synthetic
POISON = 0xA5                     # every byte of a state / track nobody zeroed (heads: count < 0; ages < 0)
MAX_GAP = {"rf27": 5, "rf9": 3}  # the interpolation scenarios' max_gap


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------ the rig

class RepairRig:
    """The buffers of one caller of r3d_streams_repair + r3d_streams_step, carved exact-sized out of one pattern-filled arena on
    `device` ("cpu": the host hooks run on them; a cuda device: the kernels).  State and track persist from tick to tick;
    frame_out, synthetic, x, x_mirror, emit and status are pattern-filled before every tick; the guards are checked after each of
    the two calls of every tick."""

    def __init__(self, device, S, rf, lag, J, F, encoding=NONE, perm=None, cam_rows=None, max_gap=0, min_conf=0.0,
                 zero_state=False, zero_track=False, pattern=bu.NANS):
        self.device = torch.device(device)
        self.S, self.rf, self.lag, self.J, self.F, self.encoding, self.perm = S, rf, lag, J, F, encoding, perm
        self.max_gap, self.min_conf = max_gap, min_conf
        self.width = W = F if encoding == NONE else 2
        self.state_bytes = S * 16 + S * rf * J * F * 4
        self.track_bytes = (4 * S * (J + J * W + rf) + 7) // 8 * 8
        arrays = [("state", np.full(self.state_bytes, 0 if zero_state else POISON, np.uint8)),
                  ("track", np.full(self.track_bytes, 0 if zero_track else POISON, np.uint8)),
                  ("frame", sc.garbage_frame(S, J, W)), ("conf", np.zeros((S, J), np.float32)),
                  ("cam", np.zeros((S, 16), np.float64) if cam_rows is None else np.ascontiguousarray(cam_rows, dtype=np.float64)),
                  ("action", np.zeros(S, np.int32)), ("frame_out", np.zeros((S, J, W), np.float32)), ("synthetic", np.zeros(S, np.int32)),
                  ("x", np.zeros((S, rf, J, F), np.float32)), ("x_mirror", np.zeros((S, rf, J, F), np.float32)),
                  ("emit", np.zeros(S, np.int64)), ("status", np.zeros(S, np.int32))]
        self.has_cam = cam_rows is not None
        self.arena = bu.Arena(self.device, pattern, bu.Arena.capacity_for([a.nbytes for _, a in arrays]))
        self.t = {n: self.arena.put(a, 256, 4 if n in ("frame", "frame_out", "x", "x_mirror", "conf") else 0, n)() for n, a in arrays}

    def _np(self, name):
        return self.t[name].cpu().numpy().copy()

    def state(self):
        """-> (heads: structured array of S, rings (S, RF, J, F) uint32)."""
        raw = self._np("state")
        return raw[:self.S * 16].view(_capi.stream_head_dtype()), raw[self.S * 16:].view(np.uint32).reshape(self.S, self.rf, self.J, self.F)

    def track(self):
        """-> (age (S, J) int32, last (S, J, width) uint32, missing (S, RF) uint32): the layout of the header."""
        S, J, W, rf = self.S, self.J, self.width, self.rf
        w = self._np("track").view(np.uint32)
        return (w[:S * J].view(np.int32).reshape(S, J), w[S * J:S * J * (1 + W)].reshape(S, J, W),
                w[S * J * (1 + W):S * J * (1 + W) + S * rf].reshape(S, rf))

    def set_head(self, s, count, drained):
        heads = np.zeros(1, _capi.stream_head_dtype())
        heads["count"], heads["drained"] = count, drained
        self.t["state"][s * 16:(s + 1) * 16].copy_(torch.from_numpy(heads.view(np.uint8)))

    def _fill(self, name, word):
        self.t[name].view(torch.int32).fill_(int(np.array([word], np.uint32).view(np.int32)[0]))

    def repair_args(self, conf):
        t = self.t
        return (t["state"].data_ptr(), t["track"].data_ptr(), self.S, self.rf, self.lag, self.J, self.F, self.encoding, t["frame"].data_ptr(),
                t["conf"].data_ptr() if conf is not None else None, self.min_conf, t["cam"].data_ptr() if self.has_cam else None,
                t["action"].data_ptr(), self.max_gap, t["frame_out"].data_ptr(), t["synthetic"].data_ptr())

    def tick(self, frame, action, conf=None, step=True):
        """r3d_streams_repair, then (step) r3d_streams_step on frame_out -> a dict of NumPy copies: what the repair call left
        (frame_out, synthetic, ring_r, age, last, missing), then what the step left (x, x_mirror, emit, status, ring, heads)."""
        t = self.t
        t["frame"].copy_(torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32)))
        t["action"].copy_(torch.from_numpy(np.ascontiguousarray(action, dtype=np.int32)))
        if conf is not None:
            t["conf"].copy_(torch.from_numpy(np.ascontiguousarray(conf, dtype=np.float32)))
        for name in ("frame_out", "x", "x_mirror"):
            self._fill(name, FILL_BITS)
        self._fill("synthetic", FILL_SYN)
        t["emit"].fill_(sc.FILL_EMIT), t["status"].fill_(sc.FILL_STATUS)
        host = self.device.type == "cpu"
        stream = None if host else torch.cuda.current_stream(self.device).cuda_stream
        if host:
            hooks_library()
            rc = _capi.debug_streams_repair_host(*self.repair_args(conf))
        else:
            _capi.streams_repair(*self.repair_args(conf), stream)
            rc = 0
        self.arena.check()
        age, last, missing = self.track()
        out = dict(rc=rc, frame_out=bits(self._np("frame_out")), synthetic=bits(self._np("synthetic")), ring_r=self.state()[1], age=age,
                   last=last, missing=missing, heads_r=self.state()[0])
        if not step:
            return out
        args = (t["state"].data_ptr(), self.S, self.rf, self.lag, self.J, self.F, self.encoding, t["frame_out"].data_ptr(),
                t["cam"].data_ptr() if self.has_cam else None, t["action"].data_ptr(), t["x"].data_ptr(),
                t["x_mirror"].data_ptr() if self.perm is not None else None, self.perm, t["emit"].data_ptr(), t["status"].data_ptr())
        if host:
            out["rc_step"] = _capi.debug_streams_step_host(*args)
        else:
            _capi.streams_step(*args, stream)
            out["rc_step"] = 0
        self.arena.check()
        heads, ring = self.state()
        out.update(x=bits(self._np("x")), x_mirror=bits(self._np("x_mirror")), emit=self._np("emit"), status=self._np("status"), ring=ring,
                   heads=heads)
        return out


# ------------------------------------------------------------------------------------ the restatement

def finite_bits(b):
    return (int(b) & 0x7F800000) != 0x7F800000


def interp_bits(a_bits, e_bits, m, g):
    """fl32((double)a + ((double)e - (double)a) * ((double)m / (double)(g + 1))), every operation rounded once (Python floats are
    float64 and Python does not contract); a NaN leaves as the canonical quiet NaN."""
    a, e = float(np.uint32(a_bits).view(np.float32)), float(np.uint32(e_bits).view(np.float32))
    with np.errstate(all="ignore"):
        t = float(m) / float(g + 1)
        d = np.float64(e) - np.float64(a)
        r = np.float64(a) + d * np.float64(t)
        f = np.float32(r)
    return QNAN if f != f else int(f.view(np.uint32))


def verdict(count, drained, action, lag):
    """The step's ARITHMETIC PER STREAM AND TICK and REFUSED STREAMS of the header -> dict(refused, push, count, drained, emit)."""
    c, d = int(count), int(drained)
    r = dict(refused=False, push=False, write=False, count=c, drained=d, emit=-1)
    if action == IDLE:
        return r
    if action == RESTART:
        c = d = 0
    elif action not in (PUSH, DRAIN):
        return dict(r, refused=True)
    if not (0 <= c <= COUNT_MAX and 0 <= d <= lag):
        return dict(r, refused=True)
    if action == DRAIN:
        if c == 0 or d == lag:
            return r
        d += 1
        k = d
    else:
        if d > 0 or c == COUNT_MAX:
            return dict(r, refused=True)
        r["push"] = True
        c += 1
        k = 0
    n = c - 1 - lag + k
    return dict(r, write=True, count=c, drained=d, emit=n if n >= 0 else -1)


class Restatement:
    """The rules of r3d_streams_repair and of the r3d_streams_step behind it on NumPy arrays of 32-bit patterns.  It starts from
    the rig's state and track as they are (initial conditions, poisoned or not).  `encode(s, row)`: (width,) input bits of stream
    s -> (F,) bits of what the step pushes for them; the identity for R3D_ENCODE_NONE."""

    def __init__(self, rig, encode=None):
        self.S, self.rf, self.lag, self.J, self.F, self.W, self.perm = rig.S, rig.rf, rig.lag, rig.J, rig.F, rig.width, rig.perm
        self.max_gap, self.min_conf = rig.max_gap, np.float32(rig.min_conf)
        heads, ring = rig.state()
        self.count, self.drained, self.ring = [int(v) for v in heads["count"]], [int(v) for v in heads["drained"]], ring.copy()
        age, last, missing = rig.track()
        self.age, self.last, self.missing = age.astype(np.int64), last.copy(), missing.copy()
        self.encode = encode or (lambda s, row: row)

    def repair(self, frame, action, conf=None):
        """-> (frame_out: {s: (J, width) bits} of the rows that are written, synthetic (S,) uint32, pushed: [bool])."""
        fb, rf = bits(np.asarray(frame, np.float32)), self.rf
        out, syn, pushed = {}, np.zeros(self.S, np.uint32), []
        for s in range(self.S):
            v = verdict(self.count[s], self.drained[s], int(action[s]), self.lag)
            pushed.append(v["push"])
            if not v["push"]:
                if not v["refused"] and v["emit"] >= 0:
                    syn[s] = self.missing[s, v["emit"] % rf]
                continue
            if int(action[s]) == RESTART:
                self.age[s], self.last[s], self.missing[s] = 0, 0, 0
            c, mask, row = v["count"] - 1, 0, np.zeros((self.J, self.W), np.uint32)
            for j in range(self.J):
                k = max(int(self.age[s, j]), 0)
                observed = all(finite_bits(b) for b in fb[s, j])
                if conf is not None:
                    observed = observed and bool(np.float32(conf[s][j]) >= self.min_conf)
                if not observed:
                    mask |= 1 << j
                    if k == 0:
                        row[j], self.age[s, j] = QNAN, 0
                    else:
                        row[j], self.age[s, j] = self.last[s, j], (k if k == INT32_MAX else k + 1)
                    continue
                row[j] = self.last[s, j] = fb[s, j]
                self.age[s, j] = 1
                e = np.asarray(self.encode(s, fb[s, j].copy()), np.uint32)
                if k == 0 and c >= 1:
                    for f in range(max(0, c - (rf - 1)), c):
                        self.ring[s, f % rf, j] = e
                elif k >= 2:
                    g = k - 1
                    if 1 <= g <= self.max_gap and g + 1 <= c:
                        a = self.ring[s, (c - 1) % rf, j].copy()
                        for m in range(1, g + 1):
                            self.ring[s, (c - 1 - g + m) % rf, j] = [interp_bits(a[i], e[i], m, g) for i in range(self.F)]
            self.missing[s, c % rf] = mask
            n = c - self.lag
            syn[s] = self.missing[s, n % rf] if n >= 0 else 0
            out[s] = row
        return out, syn, pushed

    def step(self, frame_out, action):
        """r3d_streams_step on the repaired rows -> (x {s: (RF, J, F)}, x_mirror {s: ...}, emit (S,), status (S,))."""
        rf, lag = self.rf, self.lag
        x, xm, emit, status = {}, {}, np.full(self.S, -1, np.int64), np.zeros(self.S, np.int32)
        for s in range(self.S):
            v = verdict(self.count[s], self.drained[s], int(action[s]), lag)
            status[s] = 1 if v["refused"] else 0
            if v["push"]:
                for j in range(self.J):
                    self.ring[s, (v["count"] - 1) % rf, j] = self.encode(s, frame_out[s][j].copy())
            if v["write"]:
                self.count[s], self.drained[s] = v["count"], v["drained"]
            emit[s] = v["emit"]
            if v["emit"] >= 0:
                x[s] = window_of(self.ring[s], v["emit"], self.count[s], rf, lag)
                if self.perm is not None:
                    xm[s] = mirrored(x[s], self.perm)
        return x, xm, emit, status


def window_of(ring, n, c, rf, lag):
    """Row i of the window of frame n is the ring's copy of frame clamp(n - (RF - 1 - lag) + i, 0, c - 1), at slot frame % RF."""
    frames = np.clip(n - (rf - 1 - lag) + np.arange(rf), 0, c - 1)
    return ring[frames % rf].copy()


def mirrored(w, perm):
    """x_mirror[.., j] = x[.., perm[j]] with the sign bit of component 0 turned."""
    m = bits(w)[..., list(perm), :].copy()
    m[..., 0] ^= np.uint32(0x80000000)
    return m


# ------------------------------------------------------------------------------------ the reference's windows; offline repair

def reference_windows(clip, rf, lag):
    """UnchunkedGenerator's np.pad(..., 'edge') (pad - shift in front ... the reference's split is RF - 1 - lag frames in front,
    lag behind) + eval_data_prepare's slicing: window n of an N-frame clip is padded[n : n + RF].  -> (N, RF, J, F)."""
    clip = np.ascontiguousarray(clip)
    padded = np.concatenate([np.repeat(clip[:1], rf - 1 - lag, axis=0), clip, np.repeat(clip[-1:], lag, axis=0)], axis=0)
    return np.stack([padded[n:n + rf] for n in range(clip.shape[0])])


def offline_repair(enc, observed, max_gap):
    """A clip repaired offline, in ENCODED space: `enc` (N, J, F) bits of the encoded frames (anything where not observed),
    `observed` (N, J) bool.  Per joint: a leading gap is back-filled with the first observation, every other gap holds the last
    one - and a gap of at most max_gap frames that closes is interpolated by the header's formula; a joint never observed is the
    canonical quiet NaN.  -> (N, J, F) bits."""
    N, J, F = enc.shape
    out = np.full((N, J, F), QNAN, np.uint32)
    for j in range(J):
        seen = np.nonzero(observed[:, j])[0]
        if seen.size == 0:
            continue
        out[:seen[0] + 1, j] = enc[seen[0], j]
        for a, b in zip(seen, list(seen[1:]) + [N]):      # a observed, a + 1 .. b - 1 missing, b observed (or the clip's end)
            out[a:b, j] = enc[a, j]
            g = b - a - 1
            if b < N and 1 <= g <= max_gap:
                for m in range(1, g + 1):
                    out[a + m, j] = [interp_bits(enc[a, j, i], enc[b, j, i], m, g) for i in range(F)]
    return out


def leading_gaps(observed):
    """Per joint the number of frames in front of its first observation (N: never observed)."""
    N = observed.shape[0]
    return [int(np.argmax(observed[:, j])) if observed[:, j].any() else N for j in range(observed.shape[1])]


# ------------------------------------------------------------------------------------ gapped inputs

def punch(clips, holes):
    """The golden clips with the entries of `holes` - (stream, joint or None = every joint, first frame, last frame) - made
    non-finite: a NaN in ONE component (which one varies), except one +Inf and one NaN with a payload (the first two holes).
    -> (clips, observed: per clip (N, J) bool)."""
    clips = [c.copy() for c in clips]
    observed = [np.ones(c.shape[:2], bool) for c in clips]
    for h, (s, j, f0, f1) in enumerate(holes):
        b = bits(clips[s])
        for f in range(f0, min(f1, clips[s].shape[0] - 1) + 1):
            for jj in (range(clips[s].shape[1]) if j is None else [j]):
                b[f, jj, (f + jj) % b.shape[2]] = 0x7F800000 if h == 0 else (0x7FC12345 if h == 1 else QNAN)
                observed[s][f, jj] = False
    return clips, observed


def hold_holes(rf, lag):
    """Every gap shape of the hold test on the clips of 1, 2, 5, 13, 14 and 40 frames (streams 0 .. 5)."""
    return [(5, 3, 10, 10),                  # a single frame
            (5, 1, 0, 2),                    # at the start, shorter than a centred lag
            (4, 2, 0, lag + 2),              # at the start, longer than lag
            (5, 7, 36, 39),                  # still open when the drain begins
            (3, 5, 0, 12),                   # a joint never observed
            (5, None, 20, 20),               # a frame with every joint missing
            (5, 9, 8, 8 + rf + 2),           # longer than RF
            (0, 4, 0, 0),                    # the one-frame clip: never observed
            (1, 6, 0, 0), (1, 2, 1, 1),      # the two-frame clip: a leading gap, a gap open at its end
            (2, 0, 1, 3)]


def interp_holes(K):
    """Gaps of 1, K and K + 1 frames; a gap whose frames straddle ring slot RF - 1 -> 0 (frames 26 .. 28: slots 26, 0, 1 of 27 and
    8, 0, 1 of 9); a closure while c < RF.  Streams 4 and 5 (14 and 40 frames) are clips whose gaps all close: every joint observed
    in the last frame, every gap <= K."""
    return [(5, 1, 10, 10), (5, 2, 14, 14 + K - 1), (5, 3, 26, 28), (5, 4, 2, 3), (5, 6, 0, 1), (5, None, 33, 34),
            (4, 0, 3, 5), (4, 8, 0, 1), (4, 10, 12, 12), (4, 12, 8, 9),
            (3, 5, 3, 3 + K),                # K + 1 frames: held, not interpolated
            (2, 1, 1, 2), (2, 3, 4, 4)]


# ------------------------------------------------------------------------------------ scenarios

def clip_ticks(clips, lag, S=None, extra_idle=1):
    """The schedule of `clips` (one stream each: RESTART, PUSH ..., DRAIN x lag, IDLE) -> [(frame, action, None)]."""
    lengths = [c.shape[0] for c in clips]
    actions, frame_of = sc.schedule(lengths, lag)
    S = S or len(clips)
    J, W = clips[0].shape[1:]
    ticks = []
    for t in range(actions.shape[0] + extra_idle):
        act = actions[t] if t < actions.shape[0] else np.full(S, IDLE, np.int32)
        frame = sc.garbage_frame(S, J, W)
        for s, c in enumerate(clips):
            if t < actions.shape[0] and frame_of[t, s] >= 0:
                frame[s] = c[frame_of[t, s]]
        ticks.append((frame, act, None))
    return ticks


def golden_scenario(case, shift, kind):
    """kind: "nogap<K>" (K: max_gap), "hold", "interp" -> dict(rig=kwargs of RepairRig, ticks, clips, observed, golden...)."""
    clips, rf, lag, perm, want, want_mirror = sc.golden_case(case, shift)
    J, F = clips[0].shape[1:]
    observed = [np.ones(c.shape[:2], bool) for c in clips]
    if kind == "hold":
        max_gap = 0
        clips, observed = punch(clips, hold_holes(rf, lag))
    elif kind == "interp":
        max_gap = MAX_GAP[case]
        clips, observed = punch(clips, interp_holes(max_gap))
    else:
        max_gap = {"nogap0": 0, "nogapK": MAX_GAP[case], "nogapmax": rf - 1}[kind]
    return dict(rig=dict(S=len(clips), rf=rf, lag=lag, J=J, F=F, encoding=NONE, perm=perm, max_gap=max_gap), ticks=clip_ticks(clips, lag),
                clips=clips, observed=observed, want=want, want_mirror=want_mirror)


PIXEL_CASES = [("ray", 27, 13, 5), ("intrinsic", 9, 0, 3), ("screen", 9, 4, 2)]      # (encoding, RF, lag, max_gap)


def pixel_scenario(encoding, rf, lag, max_gap):
    """Pixels through two distorted H36M camera rows (the fixtures tests/test_streams_host.py uses), 14 frames per stream, with a
    leading gap, a gap that is interpolated, one that is only held and one still open at the end."""
    from test_clips_encode_host import cameras, pixels
    J, S, N = 17, 2, 14
    enc = evaluate.ENCODINGS[encoding]
    rows = np.stack([c.cam_row(distortion=True) for c in (cameras()[1], cameras()[2])])
    px = pixels("streams.repair.%s" % encoding, (S, N, J, 2))
    clips, observed = punch([px[0], px[1]], [(0, 3, 4, 5), (1, 2, 7, 7), (0, 1, 0, 1), (0, 5, 2, 2 + max_gap), (1, 8, 11, 13), (1, None, 5, 5),
                                             (0, 9, 8, 8 + max_gap - 1)])
    return dict(rig=dict(S=S, rf=rf, lag=lag, J=J, F=_capi.ENCODE_FLOATS[enc], encoding=enc, perm=None, cam_rows=rows, max_gap=max_gap),
                ticks=clip_ticks(clips, lag), clips=clips, observed=observed, encoding=encoding, rows=rows)


def pixel_encoder(scn):
    """`encode` of the restatement for a pixel scenario: r3d_debug_clips_encode_host on one pixel through the stream's row - the
    routine the contract names ("the routine and bits the step will push")."""
    from test_clips_encode_host import run_hook
    cache = {}

    def encode(s, row):
        key = (s, int(row[0]), int(row[1]))
        if key not in cache:
            table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
            table[0]["n_frames"], table[0]["cam"] = 1, scn["rows"][s]
            rc, x, _, status = run_hook(1, scn["encoding"], table, np.asarray(row, np.uint32).view(np.float32).reshape(1, 1, 2), 1, 1, mirror=False)
            assert rc == 0 and status.tolist() == [0]
            cache[key] = bits(x)[0, 0].copy()
        return cache[key]
    return encode


def conf_scenario():
    """Finite keypoints throughout (the golden RF-9 clips, centred); the detector's confidences decide: at min_conf (observed), one
    float below it (not), above it, and NaN (not).  -> (scenario with confidences, the same ticks with the rejected keypoints made
    NaN and no confidences)."""
    scn = golden_scenario("rf9", "centred", "nogapK")
    min_conf = np.float32(0.3)
    below = np.nextafter(min_conf, np.float32(0))
    rng = np.random.RandomState(11)
    with_conf, with_nan = [], []
    for t, (frame, act, _) in enumerate(scn["ticks"]):
        conf = rng.uniform(0.5, 1.0, frame.shape[:2]).astype(np.float32)
        conf[:, t % 14] = min_conf                              # exactly at the threshold: observed
        conf[:, (t + 3) % 14] = np.float32(10.0)
        rejected = np.zeros(conf.shape, bool)
        rejected[rng.uniform(size=conf.shape) < 0.15] = True
        conf[rejected] = np.where(rng.uniform(size=int(rejected.sum())) < 0.5, below, np.float32(np.nan))
        conf[(rng.uniform(size=conf.shape) < 0.05) & rejected] = np.float32(-1.0)
        bad = frame.copy()
        bad[rejected, t % 2] = np.nan
        with_conf.append((frame, act, conf))
        with_nan.append((bad, act, None))
    rig = dict(scn["rig"], min_conf=float(min_conf))
    return dict(scn, rig=rig, ticks=with_conf), dict(scn, rig=rig, ticks=with_nan)


def actions_scenario():
    """Every action case on a state AND a track nobody zeroed (every byte 0xA5: heads with count < 0, negative ages), RF 9 / lag 4,
    the golden RF-9 clips as the source of frames.  Streams: 0 - 2 RESTART and run; 3 is PUSHed on its poisoned head first; 4 a valid head (3 frames) set by hand over a
    poisoned ring and track, PUSHed without a RESTART; 5 a zeroed head: DRAIN with nothing to drain, IDLE."""
    clips, rf, lag, perm, _, _ = sc.golden_case("rf9", "centred")
    src = clips[5]
    S, J, F = 6, src.shape[1], src.shape[2]

    def frame(t, holes=()):
        f = np.stack([src[(t + 3 * s) % 40] for s in range(S)]).copy()
        for s, j in holes:
            f[s, j, (s + j) % F] = np.nan
        return f
    X = 17                                # an unknown action word
    ticks = [(frame(0, [(0, 2), (4, 1)]), [RESTART, RESTART, RESTART, PUSH, PUSH, DRAIN], None),      # stream 3: a poisoned head, refused
             (frame(1, [(0, 2), (1, 3), (4, 1)]), [PUSH, PUSH, PUSH, RESTART, PUSH, IDLE], None),
             (frame(2, [(1, 3), (2, 0)]), [PUSH, PUSH, X, IDLE, PUSH, DRAIN], None),
             (frame(3, [(3, 5)]), [PUSH, PUSH, PUSH, PUSH, IDLE, X], None),
             (frame(4, [(0, 6)]), [PUSH, PUSH, PUSH, PUSH, PUSH, IDLE], None),
             (frame(5, [(1, 7)]), [PUSH, PUSH, PUSH, PUSH, PUSH, IDLE], None),
             (frame(6), [DRAIN, PUSH, IDLE, PUSH, DRAIN, IDLE], None),                 # stream 0 and 4 begin to drain: they emit
             (frame(7, [(0, 1)]), [PUSH, PUSH, DRAIN, X, DRAIN, IDLE], None),          # PUSH after a drain began: refused
             (frame(8, [(0, 4), (0, 5)]), [RESTART, DRAIN, DRAIN, PUSH, DRAIN, IDLE], None),   # RESTART clears the track, whatever it held
             (frame(9), [PUSH, DRAIN, DRAIN, PUSH, DRAIN, RESTART], None),
             (frame(10), [IDLE, DRAIN, DRAIN, DRAIN, DRAIN, PUSH], None),
             (frame(11), [IDLE] * S, None)]
    ticks = [(f, np.array(a, np.int32), c) for f, a, c in ticks]
    return dict(rig=dict(S=S, rf=rf, lag=lag, J=J, F=F, encoding=NONE, perm=perm, max_gap=3), ticks=ticks, heads={4: (3, 0), 5: (0, 0)})


def play(device, scn, **rig_kw):
    """The scenario's ticks on a fresh rig on `device` -> (the rig, a restatement that holds the rig's state and track as they
    were BEFORE the first tick - its initial conditions -, the per-tick results)."""
    rig = RepairRig(device, **dict(scn["rig"], **rig_kw))
    for s, (count, drained) in scn.get("heads", {}).items():
        rig.set_head(s, count, drained)
    model = Restatement(rig, scn.get("encode"))
    return rig, model, [rig.tick(f, a, c) for f, a, c in scn["ticks"]]


def host_run(kind, *key):
    """A scenario played on the host hooks, once per session: the GPU suite compares the device against it, the host suite
    compares it against the restatement.  -> (scenario, a restatement at the run's initial conditions, results)."""
    scn, model, results = _host_run(kind, *key)
    return scn, copy.deepcopy(model), results


@functools.lru_cache(maxsize=None)
def _host_run(kind, *key):
    scn = {"golden": golden_scenario, "pixels": lambda *k: pixel_scenario(*[c for c in PIXEL_CASES if c[0] == k[0]][0]),
           "actions": actions_scenario, "conf": lambda i: conf_scenario()[i]}[kind](*key)
    if kind == "pixels":
        scn["encode"] = pixel_encoder(scn)
    _, model, results = play("cpu", scn)
    _capi.use_hooks(False)
    return scn, model, results


RESULT_KEYS = ("frame_out", "synthetic", "ring_r", "age", "last", "missing", "x", "x_mirror", "emit", "status", "ring")


def agree(got, want, what):
    """Two runs of a scenario (device against hook) are the same bits, tick by tick, in everything the two calls write."""
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert g["rc"] == w["rc"] == 0 and g["rc_step"] == w["rc_step"] == 0, (what, t)
        for k in RESULT_KEYS:
            assert np.array_equal(g[k], w[k]), (what, t, k)
        assert g["heads"].tolist() == w["heads"].tolist(), (what, t)
