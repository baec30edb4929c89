"""What tests/test_streams_peek_host.py and tests/test_gpu_streams_peek.py share: the rule of r3d_streams_peek restated in NumPy, a
rig that adds the call's buffers - inside guard bands of their own (tests/buffers_util.py) - to the r3d_streams_step rig of
tests/streams_cases.py and runs the peek on the host hook or on the device, the tick schedules both run, and the pairs of
tests/golden/peek.npz."""
import functools
import os

import numpy as np
import torch

import buffers_util as bu
import streams_cases as sc
from conftest import GOLDEN, hooks_library
from ray3d_amd import _capi
from streams_cases import DRAIN, FILL, IDLE, NONE, PUSH, RESTART

FILL_EMIT, FILL_STATUS = -77, -3
COUNT_MAX = 2 ** 62


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "peek.npz"))


def looks_of(lag):
    """The looks of the fixture: the newest frame, a middle look, the last admissible one."""
    return (0, lag // 2, lag - 1)


# ------------------------------------------------------------------------------------ the rule, restated

def head_valid(count, drained, lag):
    return 0 <= count <= COUNT_MAX and 0 <= drained <= lag


def verdict(count, drained, action, status, look, lag):
    """-> (emit, peek_status) of one (look, stream): include/ray3d_hip.h, "PER LOOK k AND STREAM s".  `action` None: no action words."""
    if status != 0 or not head_valid(count, drained, lag):
        return -1, 1
    pushed = action is None or action in (PUSH, RESTART)
    p = count - 1 - look
    return (p if pushed and drained == 0 and count >= 1 and p >= 0 else -1), 0


def window_frames(p, c, rf, lag):
    """The stream frames rows 0 .. RF - 1 of the window of frame p repeat, c frames pushed: clamp(p - (RF - 1 - lag) + i, 0, c - 1)."""
    return np.clip(p - (rf - 1 - lag) + np.arange(rf), 0, c - 1)


def mirrored(w, perm):
    m = np.ascontiguousarray(w[:, list(perm), :]).copy()
    m.view(np.uint32)[:, :, 0] ^= np.uint32(0x80000000)
    return m


def window_of_history(hist, p, rf, lag):
    """From the frames a stream was given since its last RESTART (a list of (J, F) arrays)."""
    return np.stack([hist[f] for f in window_frames(p, len(hist), rf, lag)])


def window_of_ring(ring, p, c, rf, lag):
    """From the ring of one stream (RF, J, F) as it stands: frame f lives in slot f % RF."""
    return ring[window_frames(p, c, rf, lag) % rf]


def expected(heads, action, status, looks, lag):
    """-> (emit (K, S) int64, peek_status (K, S) int32) from the heads (structured array) and the step's words."""
    K, S = len(looks), len(heads)
    emit, pst = np.empty((K, S), np.int64), np.empty((K, S), np.int32)
    for k, look in enumerate(looks):
        for s in range(S):
            emit[k, s], pst[k, s] = verdict(int(heads["count"][s]), int(heads["drained"][s]), None if action is None else int(action[s]),
                                            int(status[s]), look, lag)
    return emit, pst


# ------------------------------------------------------------------------------------ the rig

class PeekRig(sc.Rig):
    """sc.Rig plus the buffers of r3d_streams_peek - (K, S, RF, J, F) windows and mirrored windows, (K, S) emit and status words -
    carved exact-sized out of a second pattern-filled arena; they are filled with FILL* before every peek, and the guards of both
    arenas are checked after it."""

    def __init__(self, device, S, rf, lag, J, F, looks, encoding=NONE, perm=None, cam_rows=None, pattern=bu.NANS, zero_state=False):
        super().__init__(device, S, rf, lag, J, F, encoding, perm, cam_rows, pattern, zero_state)
        self.looks = tuple(looks)
        K = self.K = len(self.looks)
        arrays = [("px", np.full((K, S, rf, J, F), FILL, np.float32)), ("px_mirror", np.full((K, S, rf, J, F), FILL, np.float32)),
                  ("pemit", np.full((K, S), FILL_EMIT, np.int64)), ("pstatus", np.full((K, S), FILL_STATUS, np.int32))]
        self.peek_arena = bu.Arena(self.device, pattern, bu.Arena.capacity_for([a.nbytes for _, a in arrays]))
        self.t.update({n: self.peek_arena.put(a, 256, 4 if n in ("px", "px_mirror") else 0, n)() for n, a in arrays})

    def peek(self, use_action=True, mirror=True, looks=None):
        """One call behind the last tick.  -> dict(rc, x, x_mirror, emit, status, state) as NumPy copies (rc: the hook's; 0 on a
        device, where a failure raises); `state` the state's bytes after the call."""
        t = self.t
        looks = self.looks if looks is None else tuple(looks)
        assert len(looks) <= self.K
        t["px"].fill_(float(FILL)), t["px_mirror"].fill_(float(FILL)), t["pemit"].fill_(FILL_EMIT), t["pstatus"].fill_(FILL_STATUS)
        with_mirror = mirror and self.perm is not None
        args = (t["state"].data_ptr(), self.S, self.rf, self.lag, self.J, self.F, looks, t["action"].data_ptr() if use_action else None,
                t["status"].data_ptr(), t["px"].data_ptr(), t["px_mirror"].data_ptr() if with_mirror else None,
                self.perm if with_mirror else None, t["pemit"].data_ptr(), t["pstatus"].data_ptr())
        if self.device.type == "cpu":
            hooks_library()
            rc = _capi.debug_streams_peek_host(*args)
        else:
            _capi.streams_peek(*args, torch.cuda.current_stream(self.device).cuda_stream)
            rc = 0
        self.arena.check(), self.peek_arena.check()
        n = len(looks)          # (fewer looks than the buffers hold: the front row blocks, with the shorter (n, S) word arrays)
        words = lambda name: self._np(name).reshape(-1)                                     # noqa: E731
        return dict(rc=rc, x=self._np("px"), x_mirror=self._np("px_mirror"), emit=words("pemit")[:n * self.S].reshape(n, self.S),
                    status=words("pstatus")[:n * self.S].reshape(n, self.S), emit_rest=words("pemit")[n * self.S:],
                    status_rest=words("pstatus")[n * self.S:], state=self._np("state"))


def check_peek(rig, out, looks, action, hists=None, what=""):
    """One peek's result against the restatement: emit / peek_status of every (k, s), the previewing row blocks against the ring as
    it stands (and, with `hists`, against the frames the stream was given), every other row block - and, without a mirror,
    x_mirror - at its fill value."""
    heads, rings, _ = rig.state()
    status = rig._np("status")
    emit, pst = expected(heads, action, status, looks, rig.lag)
    assert out["rc"] == 0, what
    assert np.array_equal(out["emit"], emit) and np.array_equal(out["status"], pst), (what, out["emit"], emit, out["status"], pst)
    assert (out["emit_rest"] == FILL_EMIT).all() and (out["status_rest"] == FILL_STATUS).all(), what
    flat = lambda a: a.reshape((-1,) + a.shape[2:])                                        # noqa: E731
    x, xm = flat(out["x"]), flat(out["x_mirror"])
    for b in range(x.shape[0]):
        k, s = divmod(b, rig.S)
        p = int(emit[k, s]) if k < len(looks) else -1
        if p < 0:
            assert (x[b] == FILL).all() and (xm[b] == FILL).all(), (what, k, s)
            continue
        c = int(heads["count"][s])
        want = window_of_ring(rings[s], p, c, rig.rf, rig.lag)
        assert sc.same_bits(x[b], want), (what, k, s, p)
        if hists is not None:
            assert len(hists[s]) == c and sc.same_bits(want, window_of_history(hists[s], p, rig.rf, rig.lag)), (what, k, s, p)
        if out.get("mirror", True) and rig.perm is not None:
            assert sc.same_bits(xm[b], mirrored(want, rig.perm)), (what, k, s, p)
        else:
            assert (xm[b] == FILL).all(), (what, k, s)


def track(hists, frame, action, status):
    """The frames every stream holds since its last RESTART, after a tick with these words (a refused stream keeps what it had)."""
    for s in range(len(hists)):
        if status[s] != 0:
            continue
        if action[s] == RESTART:
            hists[s] = [frame[s].copy()]
        elif action[s] == PUSH:
            hists[s] = hists[s] + [frame[s].copy()]
    return hists


def run(rig, frames, actions, use_action=True, mirror=True, checker=check_peek):
    """Ticks of (frames[t], actions[t]) through `rig`, a peek behind each -> the list of peek results (each with `tick`, the step's
    result, added).  The state is compared byte for byte around every peek."""
    hists = [[] for _ in range(rig.S)]
    outs = []
    for t in range(len(actions)):
        tick = rig.tick(frames[t], actions[t])
        assert tick["rc"] == 0
        hists = track(hists, frames[t], actions[t], tick["status"])
        before = rig.state()[2]
        out = rig.peek(use_action, mirror)
        out["mirror"] = mirror
        assert np.array_equal(out["state"], before), t
        if checker is not None:         # (a stream that previews took every frame of its history: RESTART or a zeroed state began it)
            checker(rig, out, rig.looks, actions[t] if use_action else None, hists, (t,))
        out["tick"] = tick
        outs.append(out)
    return outs


def clip_schedule(clips, lag, extra_idle=1):
    """sc.schedule as (frames (T, S, J, F), actions (T, S)): the clips side by side, garbage rows where nothing is delivered."""
    lengths = [c.shape[0] for c in clips]
    actions, frame_of = sc.schedule(lengths, lag)
    actions = np.concatenate([actions, np.full((extra_idle, len(clips)), IDLE, np.int32)])
    J, F = clips[0].shape[1:]
    frames = np.stack([sc.garbage_frame(len(clips), J, F) for _ in range(actions.shape[0])])
    for s, c in enumerate(clips):
        frames[:c.shape[0], s] = c
    return frames, actions


def mixed_schedule(S, J, F, lag, rf, ticks, seed=5):
    """Six streams with everything mixed in (on a state of 0xA5 bytes): 0 pushes throughout; 1 skips ticks (IDLE); 2 drains in the
    middle and RESTARTs; 3 meets an unknown action once (refused, then goes on); 4 stays IDLE - its head is never written: invalid;
    5 PUSHes without a RESTART on the poisoned head (refused every tick)."""
    assert S == 6 and ticks > rf + 6
    rng = np.random.RandomState(seed)
    frames = rng.standard_normal((ticks, S, J, F)).astype(np.float32)
    actions = np.full((ticks, S), PUSH, np.int32)
    actions[0, :4] = RESTART
    actions[[2, 3, 7, rf + 1], 1] = IDLE
    mid = min(lag + 3, ticks - lag - 3)
    actions[mid:mid + lag + 1, 2] = DRAIN               # (one more DRAIN than there is to drain: a valid no-op)
    actions[mid + lag + 1, 2] = RESTART
    actions[5, 3] = 9
    actions[:, 4] = IDLE
    return frames, actions
