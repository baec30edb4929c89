"""What tests/test_streams_fuse_host.py and tests/test_gpu_streams_fuse.py share: a NumPy RESTATEMENT of r3d_streams_fuse's rule,
written from the contract block of include/ray3d_hip.h with explicit Python loops over np.float64 scalars - one IEEE rounding per
operation, slots in ascending order, sums from zero; it does not call the library -, a rig that keeps every buffer of one call
inside guard bands (tests/buffers_util.py) with poisoned outputs and runs it on the host hook or on the device, and the seeded
cases both suites play."""
import functools

import numpy as np
import torch

import buffers_util as bu
from conftest import hooks_library
from ray3d_amd import _capi

QNAN64 = 0x7FF8000000000000
INT32_MAX = 2 ** 31 - 1
FILL64 = 0xA5A5A5A5A5A5A5A5       # what fused and spread hold before the call (a negative finite double) ...
FILL32 = 0xA5A5A5A5               # ... and count and used
POISON64 = 0x7FF4DEADBEEF0001     # a signalling-NaN pattern: the stale world / reproj rows of streams that did not finish


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------ the restatement

def finite(v):
    return (int(np.float64(v).view(np.uint64)) & 0x7FF0000000000000) != 0x7FF0000000000000


def canon(v, force=False):
    """The canonical quiet NaN for a NaN (decided on the bits), the value's own bits otherwise -> uint64."""
    b = int(np.float64(v).view(np.uint64))
    return QNAN64 if force or (b & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000 else b


def sqdist(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def restate(world, reproj, emit, status, synthetic, member, soft_px, max_px, max_dist):
    """-> dict(fused (G, J, 3) uint64 bits, spread (G, J) uint64 bits, count (G, J) int32, used (G, M) uint32)."""
    world = np.asarray(world, np.float64)
    S, J, _ = world.shape
    G, M = member.shape
    one, zero = np.float64(1.0), np.float64(0.0)
    soft, max_px, max_dist = np.float64(soft_px), np.float64(max_px), np.float64(max_dist)
    fused, spread = np.zeros((G, J, 3), np.uint64), np.zeros((G, J), np.uint64)
    count, used = np.zeros((G, J), np.int32), np.zeros((G, M), np.uint32)
    with np.errstate(all="ignore"):
        for g in range(G):
            for j in range(J):
                cands = []                       # (slot, x, w, synthetic)
                for m in range(M):
                    s = int(member[g, m])
                    if s < 0 or s >= S:
                        continue                 # not followed
                    if not (int(status[s]) == 0 and int(emit[s]) >= 0):
                        continue
                    x = [world[s, j, 0], world[s, j, 1], world[s, j, 2]]
                    if not all(finite(v) for v in x):
                        continue
                    w = one
                    if reproj is not None:
                        r = np.float64(reproj[s, j])
                        if not finite(r) or (max_px > 0 and not r <= max_px):
                            continue
                        ss, rr = soft * soft, r * r
                        w = one / (ss + rr)
                    syn = synthetic is not None and bool((int(np.uint32(synthetic[s])) >> j) & 1)
                    cands.append((m, x, w, syn))
                if any(not c[3] for c in cands):
                    cands = [c for c in cands if not c[3]]
                inl = cands
                if max_dist > 0 and len(cands) >= 2:
                    best, c_best = None, None
                    for c in cands:
                        cost = zero
                        for t in cands:
                            if t is c:
                                continue
                            cost = cost + t[2] * np.sqrt(sqdist(c[1], t[1]))
                        if best is None or cost < c_best:
                            best, c_best = c, cost
                    inl = [c for c in cands if np.sqrt(sqdist(best[1], c[1])) <= max_dist]
                den, num = zero, [zero, zero, zero]
                for _, x, w, _ in inl:
                    den = den + w
                    for r in range(3):
                        num[r] = num[r] + w * x[r]
                f = [num[r] / den for r in range(3)]
                acc = zero
                for _, x, w, _ in inl:
                    acc = acc + w * sqdist(f, x)
                none = len(inl) == 0
                fused[g, j] = [canon(v, none) for v in f]
                spread[g, j] = canon(np.sqrt(acc / den), none)
                count[g, j] = len(inl)
                for m, _, _, _ in inl:
                    used[g, m] |= np.uint32(1 << j)
    return dict(fused=fused, spread=spread, count=count, used=used)


# ------------------------------------------------------------------------------------ the rig

class FuseRig:
    """The buffers of one r3d_streams_fuse call, carved exact-sized out of one pattern-filled arena on `device` ("cpu": the host hook
    runs on them; a cuda device: the kernel), the float64 / int64 ones 8-byte aligned, the others 4 bytes off a 256-byte line.  The
    outputs are poisoned before every call and the guards checked after it."""

    def __init__(self, device, case, pattern=bu.NANS):
        self.device, self.case = torch.device(device), case
        S, J, G, M = case["S"], case["J"], case["G"], case["M"]
        arrays = [("world", case["world"]), ("reproj", case["reproj"] if case["reproj"] is not None else np.zeros((S, J))),
                  ("emit", case["emit"]), ("status", case["status"]),
                  ("synthetic", case["synthetic"] if case["synthetic"] is not None else np.zeros(S, np.uint32)),
                  ("member", case["member"]), ("fused", np.zeros((G, J, 3), np.uint64)), ("spread", np.zeros((G, J), np.uint64)),
                  ("count", np.zeros((G, J), np.uint32)), ("used", np.zeros((G, M), np.uint32))]
        arrays = [(n, np.ascontiguousarray(a).view({8: np.int64, 4: np.int32}[a.dtype.itemsize])) for n, a in arrays]
        self.arena = bu.Arena(self.device, pattern, bu.Arena.capacity_for([a.nbytes for _, a in arrays]))
        self.t = {n: self.arena.put(a, 256, 4 if a.dtype.itemsize == 4 else 0, n)() for n, a in arrays}

    def args(self, **over):
        c, t = self.case, self.t
        p = {n: v.data_ptr() for n, v in t.items()}
        if c["reproj"] is None:
            p["reproj"] = None
        if c["synthetic"] is None:
            p["synthetic"] = None
        v = dict(p, S=c["S"], J=c["J"], G=c["G"], M=c["M"], soft_px=c["soft_px"], max_px=c["max_px"], max_dist=c["max_dist"])
        v.update(over)
        return (v["world"], v["reproj"], v["emit"], v["status"], v["synthetic"], v["S"], v["J"], v["member"], v["G"], v["M"], v["soft_px"],
                v["max_px"], v["max_dist"], v["fused"], v["spread"], v["count"], v["used"])

    def run(self, **over):
        """One call -> (rc, dict of NumPy copies of the four outputs as bit patterns)."""
        t = self.t
        t["fused"].fill_(int(np.uint64(FILL64).view(np.int64))), t["spread"].fill_(int(np.uint64(FILL64).view(np.int64)))
        t["count"].fill_(int(np.uint32(FILL32).view(np.int32))), t["used"].fill_(int(np.uint32(FILL32).view(np.int32)))
        if self.device.type == "cpu":
            hooks_library()
            rc = _capi.debug_streams_fuse_host(*self.args(**over))
        else:
            _capi.use_hooks(False)
            _capi.streams_fuse(*self.args(**over), torch.cuda.current_stream(self.device).cuda_stream)
            rc = 0
        self.arena.check()
        return rc, self.read()

    def read(self):
        t = self.t
        return dict(fused=bits64(t["fused"].cpu().numpy()), spread=bits64(t["spread"].cpu().numpy()), count=t["count"].cpu().numpy().copy(),
                    used=bits32(t["used"].cpu().numpy()))


def agree(got, want, what=None):
    for k in ("fused", "spread", "count", "used"):
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


def restate_case(case):
    return restate(case["world"], case["reproj"], case["emit"], case["status"], case["synthetic"], case["member"], case["soft_px"],
                   case["max_px"], case["max_dist"])


# ------------------------------------------------------------------------------------ the seeded cases

S_CASE, G_CASE = 7, 3
SHAPES = [(M, J) for M in (1, 4, 16) for J in (14, 17)]
VARIANTS = [(rp, sy, gate) for rp in (False, True) for sy in (False, True) for gate in (False, True)]


def make_case(M, J, with_reproj, with_synthetic, gate, seed=0, all_empty_group=None):
    """S = 7 streams, G = 3 groups.  Streams 0 - 4 finished a frame this tick, 5 did not (emit -1) and 6 was refused (status 1); the
    rows of 5 and 6 hold a poison pattern.  Every person stands at a place of their own and the streams see them within a few
    centimetres, with one stream a metre off; single elements are NaN / Inf.  The member table holds empty slots (-1, -2), words
    that name no stream (S, INT32_MAX), the unfinished and the refused stream, and - from M = 4 - one stream twice."""
    S, G = S_CASE, G_CASE
    rng = np.random.RandomState(1000 * M + 10 * J + 4 * with_reproj + 2 * with_synthetic + gate + 97 * seed)
    person = rng.uniform(-2.0, 2.0, (G, J, 3))
    member = np.full((G, M), -1, np.int32)
    for g in range(G):
        for m in range(M):
            member[g, m] = rng.randint(0, S)
    world = np.zeros((S, J, 3))
    home = rng.randint(0, G, S)                 # the person a stream mostly watches
    for s in range(S):
        world[s] = person[home[s]] + 0.02 * rng.standard_normal((J, 3))
    world[3] += np.array([1.0, 0.0, 0.0])       # a camera that is a metre off
    if M >= 4:
        member[0, :4] = [0, 1, 0, 3]            # stream 0 twice; the displaced stream
        member[1, :4] = [2, -1, 5, 4]           # an empty slot, the unfinished stream
        member[2, :4] = [6, S, -2, INT32_MAX]   # the refused stream and three words that name nothing: no candidate at all ...
        if M == 16:
            member[2, 9], member[0, 15], member[1, 7] = 1, S, -2     # ... unless a later slot holds one
        for g in range(2):                      # groups 0 and 1 see their own person
            for s in set(member[g][(member[g] >= 0) & (member[g] < S)].tolist()) - {3}:
                world[s] = person[g] + 0.02 * rng.standard_normal((J, 3))
        world[3] = person[0] + 0.02 * rng.standard_normal((J, 3)) + np.array([1.0, 0.0, 0.0])
    else:
        member[:, 0] = [0, 5, -1] if seed == 0 else [2, S, 6]
    if all_empty_group is not None:
        member[all_empty_group] = -1
    world[1, 2, 1], world[2, 3, 0], world[0, 1, 2] = np.nan, np.inf, -np.inf
    world[4, 0] = np.nan
    reproj = rng.uniform(0.3, 10.0, (S, J)) if with_reproj else None
    if with_reproj:
        reproj[3, 4], reproj[0, 5], reproj[4, 6] = np.nan, np.inf, 50.0
    for s in (5, 6):                            # stale rows of streams without a pose this tick
        world[s] = np.full((J, 3), POISON64, np.uint64).view(np.float64)
        if with_reproj:
            reproj[s] = np.full(J, POISON64, np.uint64).view(np.float64)
    emit = np.array([4, 0, 17, 2, 9, -1, 3], np.int64)
    status = np.array([0, 0, 0, 0, 0, 0, 1], np.int32)
    synthetic = rng.randint(0, 1 << 17, S).astype(np.uint32) if with_synthetic else None
    if with_synthetic:
        synthetic[0], synthetic[1] = 0, (1 << 17) - 1          # nothing made up; everything made up
    return dict(S=S, J=J, G=G, M=M, world=world, reproj=reproj, emit=emit, status=status, synthetic=synthetic, member=member,
                soft_px=2.0, max_px=12.0 if (with_reproj and gate) else 0.0, max_dist=0.2 if gate else 0.0)


@functools.lru_cache(maxsize=None)
def host_run(M, J, with_reproj, with_synthetic, gate, all_empty_group=None):
    """A seeded case played on the host hook, once per session -> (case, outputs).  The GPU suite compares the device against it,
    the host suite compares it against the restatement."""
    case = make_case(M, J, with_reproj, with_synthetic, gate, all_empty_group=all_empty_group)
    rc, out = FuseRig("cpu", case).run()
    _capi.use_hooks(False)
    assert rc == 0
    return case, out


def simple_case(world, member, reproj=None, synthetic=None, emit=None, status=None, soft_px=2.0, max_px=0.0, max_dist=0.0):
    """A case from explicit arrays: every stream finished unless emit / status say otherwise."""
    world = np.ascontiguousarray(world, np.float64)
    S, J, _ = world.shape
    member = np.ascontiguousarray(member, np.int32)
    return dict(S=S, J=J, G=member.shape[0], M=member.shape[1], world=world,
                reproj=None if reproj is None else np.ascontiguousarray(reproj, np.float64),
                emit=np.zeros(S, np.int64) if emit is None else np.ascontiguousarray(emit, np.int64),
                status=np.zeros(S, np.int32) if status is None else np.ascontiguousarray(status, np.int32),
                synthetic=None if synthetic is None else np.ascontiguousarray(synthetic, np.uint32), member=member, soft_px=soft_px,
                max_px=max_px, max_dist=max_dist)
