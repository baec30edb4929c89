"""What tests/test_streams_assign_host.py and tests/test_gpu_streams_assign.py share: a NumPy RESTATEMENT of r3d_streams_assign's
rule, written from the contract block of include/ray3d_hip.h with explicit Python loops over np.float64 scalars - one IEEE rounding
per operation, joints in ascending order, sums from zero; it does not call the library -, a rig that keeps every buffer of one call
inside guard bands (tests/buffers_util.py) with poisoned outputs and runs it on the host hook or on the device, and the seeded
multi-tick cases both suites play."""
import functools

import numpy as np
import torch

import buffers_util as bu
from conftest import hooks_library
from ray3d_amd import _capi

QNAN32 = 0x7FC00000
ONE32 = 0x3F800000
FILL32 = 0xA5A5A5A5               # what every output holds before a call
IDLE, PUSH, RESTART, DRAIN = 0, 1, 2, 3
FILL_NAN, FILL_HOLD = 0, 1
OUT_KEYS = ("action", "frame_out", "conf_out", "match", "id", "stats")


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------ the state's layout

def state_bytes(C, P, J, width):
    """The documented layout: int64 next_id[C], int64 id[S], int32 phase / missed / left [S], uint32 seen[S], float32
    ref[S][J][width], rounded up to 8."""
    S = C * P
    return (8 * C + 8 * S + 4 * 4 * S + 4 * S * J * width + 7) // 8 * 8


def unpack_state(raw, C, P, J, width):
    """The state's bytes -> dict of arrays (copies), ref as 32-bit patterns."""
    raw = np.ascontiguousarray(raw, np.uint8)
    assert raw.size == state_bytes(C, P, J, width)
    S, at, out = C * P, 0, {}
    for name, dtype, count in (("next_id", np.int64, C), ("id", np.int64, S), ("phase", np.int32, S), ("missed", np.int32, S),
                               ("left", np.int32, S), ("seen", np.uint32, S), ("ref", np.uint32, S * J * width)):
        n = count * np.dtype(dtype).itemsize
        out[name] = raw[at:at + n].view(dtype).copy()
        at += n
    out["ref"] = out["ref"].reshape(S, J, width)
    return out


def pack_state(st, C, P, J, width):
    raw = np.zeros(state_bytes(C, P, J, width), np.uint8)
    at = 0
    for name in ("next_id", "id", "phase", "missed", "left", "seen", "ref"):
        b = np.ascontiguousarray(st[name]).reshape(-1).view(np.uint8)
        raw[at:at + b.size] = b
        at += b.size
    return raw


# ------------------------------------------------------------------------------------ the restatement

def finite32(word):
    return (int(word) & 0x7F800000) != 0x7F800000


def f64(word):
    """A 32-bit pattern widened to float64."""
    return np.float64(np.array([word], np.uint32).view(np.float32)[0])


def restate(st, prm, det, conf, count):
    """One call on the state dict `st` (replaced in place) -> dict of the six outputs, frame_out and conf_out as bit patterns."""
    C, P, D, J, W = prm["C"], prm["P"], prm["D"], prm["J"], prm["width"]
    lag, max_missed = prm["lag"], prm["max_missed"]
    S = C * P
    det = bits32(np.asarray(det, np.float32)).reshape(C, D, J, W)
    cbits = bits32(np.asarray(conf, np.float32)).reshape(C, D, J) if conf is not None else None
    cval = np.asarray(conf, np.float32).reshape(C, D, J) if conf is not None else None
    min_conf, max_cost = np.float32(prm["min_conf"]), np.float64(prm["max_cost"])
    action = np.zeros(S, np.int32)
    frame_out = np.full((S, J, W), QNAN32, np.uint32)
    conf_out = np.zeros((S, J), np.uint32)
    match = np.full(S, -1, np.int32)
    ids = np.full(S, -1, np.int64)
    stats = np.zeros((C, 4), np.int32)

    def phase_of(s):
        w = int(st["phase"][s])
        return 1 if w == 1 else 2 if (w == 2 and lag > 0) else 0

    def take(s, c, d, obs):
        """Slot s pushes detection d: the rows, and ref / seen per observed joint."""
        frame_out[s] = det[c, d]
        conf_out[s] = cbits[c, d] if cbits is not None else ONE32
        for j in obs:
            st["ref"][s, j] = det[c, d, j]
            st["seen"][s] |= np.uint32(1 << j)
        match[s] = d

    with np.errstate(all="ignore"):
        for c in range(C):
            n = min(max(int(count[c]), 0), D)
            # 1. detections
            obs, size, valid = [], [], []
            for d in range(n):
                o = [j for j in range(J) if all(finite32(det[c, d, j, k]) for k in range(W))
                     and (cval is None or bool(cval[c, d, j] >= min_conf))]
                xs, ys = [f64(det[c, d, j, 0]) for j in o], [f64(det[c, d, j, 1]) for j in o]
                sz = np.float64(0.0)
                if o:
                    dx, dy = max(xs) - min(xs), max(ys) - min(ys)
                    sz = dy if dy > dx else dx
                obs.append(o), size.append(sz), valid.append(len(o) >= prm["min_joints"] and bool(sz > 0))
            # 2. costs of the admissible pairs
            entry = [phase_of(c * P + p) for p in range(P)]
            cost = {}
            for p in range(P):
                s = c * P + p
                if entry[p] != 1:
                    continue
                seen = int(st["seen"][s])
                for d in range(n):
                    if not valid[d]:
                        continue
                    common = [j for j in obs[d] if (seen >> j) & 1]
                    if len(common) < prm["min_common"]:
                        continue
                    total = np.float64(0.0)
                    for j in common:
                        dx = f64(det[c, d, j, 0]) - f64(st["ref"][s, j, 0])
                        dy = f64(det[c, d, j, 1]) - f64(st["ref"][s, j, 1])
                        total = total + np.sqrt((dx * dx) + (dy * dy))
                    v = (total / np.float64(len(common))) / size[d]
                    if v <= max_cost:
                        cost[(p, d)] = v
            # 3. greedy matching
            pairs, taken_p, taken_d = {}, set(), set()
            while True:
                left = [(v, p, d) for (p, d), v in cost.items() if p not in taken_p and d not in taken_d]
                if not left:
                    break
                v, p, d = min(left)
                pairs[p] = d
                taken_p.add(p), taken_d.add(d)
            # 4. / 5. live and draining slots
            for p in range(P):
                s = c * P + p
                if entry[p] == 1:
                    ids[s] = st["id"][s]
                    missed = max(int(st["missed"][s]), 0)
                    if p in pairs:
                        action[s] = PUSH
                        st["missed"][s] = 0
                        take(s, c, pairs[p], obs[pairs[p]])
                    elif missed + 1 <= max_missed:
                        action[s] = PUSH
                        st["missed"][s] = missed + 1
                        if prm["fill"] == FILL_HOLD:
                            for j in range(J):
                                if (int(st["seen"][s]) >> j) & 1:
                                    frame_out[s, j] = st["ref"][s, j]
                    elif lag > 0:
                        action[s] = DRAIN
                        st["left"][s] = lag - 1
                        st["phase"][s] = 2 if lag - 1 > 0 else 0
                    else:
                        action[s] = IDLE
                        st["phase"][s] = 0
                elif entry[p] == 2:
                    ids[s] = st["id"][s]
                    action[s] = DRAIN
                    left = min(max(int(st["left"][s]), 1), lag) - 1
                    st["left"][s] = left
                    st["phase"][s] = 2 if left > 0 else 0
            # 6. births
            orphans = [d for d in range(n) if valid[d] and d not in taken_d]
            free = [p for p in range(P) if entry[p] == 0]
            born = 0
            for d, p in zip(orphans, free):
                s = c * P + p
                action[s] = RESTART
                ids[s] = st["id"][s] = st["next_id"][c]
                st["next_id"][c] += 1
                st["phase"][s], st["missed"][s], st["seen"][s] = 1, 0, 0
                take(s, c, d, obs[d])
                born += 1
            stats[c] = [sum(valid), len(taken_d), born, len(orphans) - born]
    return dict(action=action, frame_out=frame_out, conf_out=conf_out, match=match, id=ids, stats=stats)


# ------------------------------------------------------------------------------------ the rig

class AssignRig:
    """The buffers of r3d_streams_assign calls, carved exact-sized out of one pattern-filled arena on `device` ("cpu": the host hook
    runs on them; a cuda device: the kernel), the state and id 8-byte aligned, the others 4 bytes off a 256-byte line.  The state
    persists over the ticks; the outputs are poisoned before every call and the guards checked after it."""

    def __init__(self, device, case, pattern=bu.NANS):
        self.device, self.case = torch.device(device), case
        C, P, D, J, W = case["C"], case["P"], case["D"], case["J"], case["width"]
        S = C * P
        assert case["state0"].size == state_bytes(C, P, J, W)
        arrays = [("state", case["state0"].view(np.int64)), ("det", np.zeros((C, D, J, W), np.int32)), ("conf", np.zeros((C, D, J), np.int32)),
                  ("count", np.zeros(C, np.int32)), ("action", np.zeros(S, np.int32)), ("frame_out", np.zeros((S, J, W), np.int32)),
                  ("conf_out", np.zeros((S, J), np.int32)), ("match", np.zeros(S, np.int32)), ("id", np.zeros(S, np.int64)),
                  ("stats", np.zeros((C, 4), np.int32))]
        self.arena = bu.Arena(self.device, pattern, bu.Arena.capacity_for([a.nbytes for _, a in arrays]))
        self.t = {n: self.arena.put(a, 256, 4 if a.dtype.itemsize == 4 else 0, n)() for n, a in arrays}
        self.prm = _capi.assign_params(C, P, D, J, W, case["lag"], case["min_joints"], case["min_common"], case["max_missed"],
                                       case["fill"], case["min_conf"], case["max_cost"])
        self.with_conf = case["with_conf"]

    def ptrs(self, **over):
        p = {n: v.data_ptr() for n, v in self.t.items()}
        if not self.with_conf:
            p["conf"] = None
        p["prm"] = self.prm
        p.update(over)
        return (p["state"], p["prm"], p["det"], p["conf"], p["count"], p["action"], p["frame_out"], p["conf_out"], p["match"], p["id"], p["stats"])

    def load(self, tick):
        t = self.t
        t["det"].copy_(torch.from_numpy(bits32(tick["det"]).view(np.int32).reshape(t["det"].shape)))
        if tick["conf"] is not None:
            t["conf"].copy_(torch.from_numpy(bits32(tick["conf"]).view(np.int32).reshape(t["conf"].shape)))
        t["count"].copy_(torch.from_numpy(np.asarray(tick["count"], np.int32)))

    def poison(self):
        for k in OUT_KEYS:
            self.t[k].view(torch.int32).fill_(int(np.uint32(FILL32).view(np.int32)))

    def run(self, tick=None, **over):
        """One call (on `tick`'s inputs when given) -> (rc, dict of NumPy copies of the outputs and the state's bytes)."""
        if tick is not None:
            self.load(tick)
        self.poison()
        if self.device.type == "cpu":
            hooks_library()
            rc = _capi.debug_streams_assign_host(*self.ptrs(**over))
        else:
            _capi.use_hooks(False)
            _capi.streams_assign(*self.ptrs(**over), torch.cuda.current_stream(self.device).cuda_stream)
            rc = 0
        self.arena.check()
        return rc, self.read()

    def read(self):
        t = self.t
        out = {k: t[k].cpu().numpy().copy() for k in ("action", "match", "id", "stats")}
        out["frame_out"], out["conf_out"] = bits32(t["frame_out"].cpu().numpy().copy()), bits32(t["conf_out"].cpu().numpy().copy())
        out["state"] = t["state"].cpu().numpy().copy().view(np.uint8)
        return out


def agree(got, want, what=None, keys=OUT_KEYS + ("state",)):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4].tolist())


def restate_case(case):
    """The restatement over the case's ticks -> per tick the outputs and the state's bytes after it."""
    C, P, J, W = case["C"], case["P"], case["J"], case["width"]
    st = unpack_state(case["state0"], C, P, J, W)
    outs = []
    for tick in case["ticks"]:
        out = restate(st, case, tick["det"], tick["conf"], tick["count"])
        out["state"] = pack_state(st, C, P, J, W)
        outs.append(out)
    return outs


# ------------------------------------------------------------------------------------ the seeded cases

SHAPES = [(1, 1, 1), (2, 3, 5), (3, 5, 3), (2, 32, 1), (2, 1, 32), (1, 32, 32)]
LAGS = (0, 1, 4)
MAX_MISSED = 2
BONES = np.random.RandomState(7).uniform(-0.5, 0.5, (17, 2))      # a skeleton in units of its size
BONES[0], BONES[1] = [-0.5, -0.5], [0.5, 0.5]                      # (the size is exactly the scale while both are observed)


def case_ids():
    """(C, P, D, J, width, lag, fill, with_conf, poisoned state): every shape with both J and both widths; the lags, fills,
    confidences and the 0xA5 state rotate over them so that each occurs with small and large shapes."""
    out, k = [], 0
    for (C, P, D) in SHAPES:
        for J in (14, 17):
            for W in (2, 3):
                out.append((C, P, D, J, W, LAGS[k % 3], (FILL_NAN, FILL_HOLD)[(k // 2) % 2], k % 2 == 1, k % 4 == 2))
                k += 1
    return out


def make_case(C, P, D, J, W, lag, fill, with_conf, poisoned, seed=0):
    """A scene per camera: people 260 px apart (size 200 px) who enter and leave at seeded ticks, walk 6 - 10 px per tick, are
    detected with 2 px noise, lose a quarter of their joints and a fifth of their detections, in shuffled order - more people than
    slots and than detections at times.  lag + MAX_MISSED + 3 ticks and more, so that tracks are born, missed, end, drain and their
    slots are reused.  On top of that the edge cases, at fixed ticks on camera t % C: det_count at -3, 0, D and D + 7, NaN / Inf
    keypoints, NaN confidences, two bit-identical detections, a detection of zero size."""
    rng = np.random.RandomState(100003 * seed + 1009 * C + 101 * P + 11 * D + J + 3 * W + lag)
    ticks_n = max(lag + MAX_MISSED + 3, 12) + 4
    people = min(max(P, D) + 2, 12)
    home = np.stack([[260.0 * (k % 4) + 150, 260.0 * (k // 4) + 150] for k in range(people)])
    vel = rng.uniform(6, 10, (C, people, 1)) * np.stack([np.cos(a := rng.uniform(0, 6.28, (C, people))), np.sin(a)], -1)
    start = rng.randint(0, 4, (C, people))
    stop = start + rng.randint(2, ticks_n, (C, people))
    start[:, 0], stop[:, 0] = 0, 3                       # somebody leaves early: the slot drains and is reused
    ticks = []
    for t in range(ticks_n):
        det = np.full((C, D, J, W), np.nan, np.float32)
        conf = rng.uniform(0.4, 1.0, (C, D, J)).astype(np.float32) if with_conf else None
        count = np.zeros(C, np.int32)
        for c in range(C):
            rows = []
            for k in range(people):
                if not start[c, k] <= t < stop[c, k] or rng.uniform() < 0.2:
                    continue
                pts = home[k] + vel[c, k] * t + 200.0 * BONES[:J] + rng.normal(0, 2.0, (J, 2))
                row = np.concatenate([pts, np.ones((J, W - 2))], -1).astype(np.float32)
                row[rng.uniform(size=J) < 0.25] = np.nan
                rows.append(row)
            rng.shuffle(rows)
            rows = rows[:D]
            for d, row in enumerate(rows):
                det[c, d] = row
            count[c] = len(rows)
        c = t % C
        if t == 2:
            count[c] = -3
        elif t == 3:                                     # every row a far-away stranger: more births than free slots
            for d in range(D):
                pts = np.array([3000.0 + 300 * d, 2000.0]) + 200.0 * BONES[:J]
                det[c, d] = np.concatenate([pts, np.ones((J, W - 2))], -1)
            count[c] = D + 7
        elif t == 5:
            count[c] = 0
        elif t == 6 and count[c] >= 1:                   # two bit-identical detections (D >= 2): the tie rule
            if D >= 2:
                det[c, 1] = det[c, 0]
                if conf is not None:
                    conf[c, 1] = conf[c, 0]
                count[c] = max(count[c], 2)
        elif t == 7:                                     # non-finite keypoints and confidences
            det[c, 0, 0, 0], det[c, 0, 1 % J, 1] = np.inf, -np.inf
            if W == 3:
                det[c, 0, 2 % J, 2] = np.inf
            if conf is not None:
                conf[c, 0, 3 % J], conf[c, 0, 4 % J] = np.nan, 0.05
            count[c] = max(count[c], 1)
        elif t == 8:                                     # a detection of zero size in front
            det[c, 0] = np.concatenate([np.full((J, 2), 321.5), np.ones((J, W - 2))], -1)
            count[c] = max(count[c], 1)
        elif t == 9:
            count[c] = D
        ticks.append(dict(det=det, conf=conf, count=count))
    nbytes = state_bytes(C, P, J, W)
    state0 = np.full(nbytes, 0xA5, np.uint8) if poisoned else np.zeros(nbytes, np.uint8)
    return dict(C=C, P=P, D=D, J=J, width=W, lag=lag, min_joints=min(4, J), min_common=min(3, J), max_missed=MAX_MISSED, fill=fill,
                min_conf=0.3, max_cost=0.5, with_conf=with_conf, state0=state0, ticks=ticks)


@functools.lru_cache(maxsize=None)
def host_run(*key):
    """A seeded case played on the host hook, once per session -> (case, per-tick outputs with the state after the tick).  The GPU
    suite compares the device against it, the host suite compares it against the restatement."""
    case = make_case(*key)
    rig = AssignRig("cpu", case)
    outs = []
    for tick in case["ticks"]:
        rc, out = rig.run(tick)
        assert rc == 0
        outs.append(out)
    _capi.use_hooks(False)
    return case, outs
