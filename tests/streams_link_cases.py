"""What tests/test_streams_link_host.py and tests/test_gpu_streams_link.py share: a NumPy RESTATEMENT of r3d_streams_link's rule,
written sequentially from the contract block of include/ray3d_hip.h with explicit Python loops over np.float64 scalars - one IEEE
rounding per operation, joints and cameras in ascending order, sums from zero; it does not call the library -, the state's pack
and unpack helpers, a rig that keeps every buffer of one call inside guard bands (tests/buffers_util.py) with poisoned outputs and
runs it on the host hook or on the device, and the seeded multi-tick cases both suites play."""
import functools

import numpy as np
import torch

import buffers_util as bu
from conftest import hooks_library
from ray3d_amd import _capi

FILL32 = 0xA5A5A5A5               # what every output holds before a call
OUT_KEYS = ("member", "person", "group", "stats")
STATE_FIELDS = ("next_id", "pid", "link_id", "ref", "phase", "missed", "link", "seen")


# ------------------------------------------------------------------------------------ the state's layout

def state_bytes(N, C, G, J):
    """The documented layout: int64 next_id[N], int64 pid[NG], int64 link_id[NG][C], double ref[NG][J][3], int32 phase[NG], int32
    missed[NG], int32 link[NG][C], uint32 seen[NG], rounded up to 8."""
    NG = N * G
    return (8 * N + NG * (8 + 8 * C + 24 * J + 4 + 4 + 4 * C + 4) + 7) // 8 * 8


def _fields(N, C, G, J):
    NG = N * G
    return (("next_id", np.int64, (N,)), ("pid", np.int64, (NG,)), ("link_id", np.int64, (NG, C)), ("ref", np.float64, (NG, J, 3)),
            ("phase", np.int32, (NG,)), ("missed", np.int32, (NG,)), ("link", np.int32, (NG, C)), ("seen", np.uint32, (NG,)))


def unpack_state(raw, N, C, G, J):
    """The state's bytes -> dict of arrays (copies), and "tail": the bytes of the rounding."""
    raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    assert raw.size == state_bytes(N, C, G, J)
    at, out = 0, {}
    for name, dtype, shape in _fields(N, C, G, J):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out[name] = raw[at:at + n].view(dtype).reshape(shape).copy()
        at += n
    out["tail"] = raw[at:].copy()
    return out


def pack_state(st, N, C, G, J):
    raw = np.zeros(state_bytes(N, C, G, J), np.uint8)
    at = 0
    for name in STATE_FIELDS + ("tail",):
        b = np.ascontiguousarray(st[name]).reshape(-1).view(np.uint8)
        raw[at:at + b.size] = b
        at += b.size
    assert at == raw.size
    return raw


# ------------------------------------------------------------------------------------ the restatement

def finite64(v):
    return (int(np.array([v], np.float64).view(np.uint64)[0]) & 0x7FF0000000000000) != 0x7FF0000000000000


def restate(st, prm, world, emit, status, ids):
    """One call on the state dict `st` (changed in place) -> dict of the four outputs."""
    N, C, P, G, M, J = prm["N"], prm["C"], prm["P"], prm["G"], prm["M"], prm["J"]
    S, NG = N * C * P, N * G
    world = np.asarray(world, np.float64).reshape(S, J, 3)
    emit, status, ids = np.asarray(emit, np.int64), np.asarray(status, np.int32), np.asarray(ids, np.int64)
    max_dist, break_dist = np.float64(prm["max_dist"]), np.float64(prm["break_dist"])
    member = np.full((NG, M), -1, np.int32)
    person = np.full(NG, -1, np.int64)
    group = np.full(S, -1, np.int32)
    stats = np.zeros((N, 4), np.int32)

    def finished(s):
        return int(status[s]) == 0 and int(emit[s]) >= 0

    def present(s):
        return [j for j in range(J) if all(finite64(world[s, j, k]) for k in range(3))]

    def seen(gi):
        return [j for j in range(J) if (int(st["seen"][gi]) >> j) & 1]

    def cost(gi, s, common):
        total = np.float64(0.0)
        for j in common:
            dx, dy, dz = (world[s, j, k] - st["ref"][gi, j, k] for k in range(3))
            total = total + np.sqrt(((dx * dx) + (dy * dy)) + (dz * dz))
        return total / np.float64(len(common))

    with np.errstate(all="ignore"):
        for n in range(N):
            def stream(c, p):
                return (n * C + c) * P + p
            live = [int(st["phase"][n * G + g]) == 1 for g in range(G)]
            link = [[0] * C for _ in range(G)]                      # slot plus one, as the rule reads the words
            for g in range(G):
                for c in range(C):
                    w = int(st["link"][n * G + g, c])
                    link[g][c] = w if live[g] and 1 <= w <= P else 0
            # A. validate
            for g in range(G):
                if not live[g]:
                    continue
                gi = n * G + g
                for c in range(C):
                    if not link[g][c]:
                        continue
                    s = stream(c, link[g][c] - 1)
                    drop = int(ids[s]) < 0 or int(ids[s]) != int(st["link_id"][gi, c])
                    drop = drop or any(link[h][c] == link[g][c] for h in range(g))
                    if not drop and break_dist > 0 and finished(s):
                        common = [j for j in present(s) if j in seen(gi)]
                        drop = bool(common) and bool(cost(gi, s, common) > break_dist)
                    if drop:
                        link[g][c] = 0
            # B. per camera
            made = [[False] * C for _ in range(G)]
            links = births = dropped = 0
            for c in range(C):
                held = {link[g][c] - 1 for g in range(G) if link[g][c]}
                cands = [p for p in range(P) if int(ids[stream(c, p)]) >= 0 and finished(stream(c, p)) and p not in held
                         and len(present(stream(c, p))) >= prm["min_joints"]]
                elig = [g for g in range(G) if live[g] and not link[g][c] and seen(n * G + g)]
                costs = {}
                for g in elig:
                    for p in cands:
                        common = [j for j in present(stream(c, p)) if j in seen(n * G + g)]
                        if len(common) < max(prm["min_common"], 1):
                            continue
                        v = cost(n * G + g, stream(c, p), common)
                        if v <= max_dist:
                            costs[(g, p)] = v
                taken_g, taken_p = set(), set()
                while True:
                    left = [(v, g, p) for (g, p), v in costs.items() if g not in taken_g and p not in taken_p]
                    if not left:
                        break
                    v, g, p = min(left)
                    taken_g.add(g), taken_p.add(p)
                    link[g][c], made[g][c] = p + 1, True
                    st["link_id"][n * G + g, c] = ids[stream(c, p)]
                    links += 1
                orphans = [p for p in cands if p not in taken_p]
                free = [g for g in range(G) if not live[g]]
                for p, g in zip(orphans, free):
                    gi, s = n * G + g, stream(c, p)
                    st["pid"][gi] = st["next_id"][n]
                    st["next_id"][n] += 1
                    st["phase"][gi], st["missed"][gi], st["seen"][gi] = 1, 0, 0
                    for j in present(s):
                        st["ref"][gi, j] = world[s, j]
                        st["seen"][gi] |= np.uint32(1 << j)
                    live[g] = True
                    link[g] = [0] * C
                    link[g][c] = p + 1
                    st["link_id"][gi, c] = ids[s]
                    births += 1
                dropped += max(len(orphans) - len(free), 0)
            # C. per live person
            lives = 0
            for g in range(G):
                gi = n * G + g
                st["link"][gi] = link[g]
                for c in range(C):
                    if link[g][c]:
                        member[gi, c] = stream(c, link[g][c] - 1)
                        group[stream(c, link[g][c] - 1)] = gi
                if not live[g]:
                    continue
                for j in range(J):
                    pts = [world[stream(c, link[g][c] - 1), j] for c in range(C)
                           if link[g][c] and finished(stream(c, link[g][c] - 1)) and j in present(stream(c, link[g][c] - 1))]
                    if not pts:
                        continue
                    for k in range(3):
                        total = np.float64(0.0)
                        for pt in pts:
                            total = total + pt[k]
                        st["ref"][gi, j, k] = total / np.float64(len(pts))
                    st["seen"][gi] |= np.uint32(1 << j)
                if any(link[g]):
                    st["missed"][gi] = 0
                else:
                    missed = max(int(st["missed"][gi]), 0)
                    if missed + 1 > prm["max_missed"]:
                        st["phase"][gi] = 0
                        continue
                    st["missed"][gi] = missed + 1
                person[gi] = st["pid"][gi]
                lives += 1
            stats[n] = [lives, links, births, dropped]
    return dict(member=member, person=person, group=group, stats=stats)


# ------------------------------------------------------------------------------------ the rig

class LinkRig:
    """The buffers of r3d_streams_link calls, carved exact-sized out of one pattern-filled arena on `device` ("cpu": the host hook
    runs on them; a cuda device: the kernel), the 8-byte ones aligned, the others 4 bytes off a 256-byte line.  The state persists
    over the ticks; the outputs are poisoned before every call and the guards checked after it."""

    def __init__(self, device, case, pattern=bu.NANS):
        self.device, self.case = torch.device(device), case
        N, C, P, G, M, J = (case[k] for k in "NCPGMJ")
        S, NG = N * C * P, N * G
        assert case["state0"].size == state_bytes(N, C, G, J)
        arrays = [("state", case["state0"].view(np.int64)), ("world", np.zeros((S, J, 3), np.float64)), ("emit", np.zeros(S, np.int64)),
                  ("status", np.zeros(S, np.int32)), ("id", np.zeros(S, np.int64)), ("member", np.zeros((NG, M), np.int32)),
                  ("person", np.zeros(NG, np.int64)), ("group", np.zeros(S, np.int32)), ("stats", np.zeros((N, 4), np.int32))]
        self.arena = bu.Arena(self.device, pattern, bu.Arena.capacity_for([a.nbytes for _, a in arrays]))
        self.t = {n: self.arena.put(a, 256, 4 if a.dtype.itemsize == 4 else 0, n)() for n, a in arrays}
        self.prm = _capi.link_params(N, C, P, G, M, J, case["min_joints"], case["min_common"], case["max_missed"], case["max_dist"],
                                     case["break_dist"])

    def ptrs(self, **over):
        p = {n: v.data_ptr() for n, v in self.t.items()}
        p["prm"] = self.prm
        p.update(over)
        return (p["state"], p["prm"], p["world"], p["emit"], p["status"], p["id"], p["member"], p["person"], p["group"], p["stats"])

    def load(self, tick):
        t = self.t
        t["world"].copy_(torch.from_numpy(np.asarray(tick["world"], np.float64).reshape(t["world"].shape)))
        t["emit"].copy_(torch.from_numpy(np.asarray(tick["emit"], np.int64)))
        t["status"].copy_(torch.from_numpy(np.asarray(tick["status"], np.int32)))
        t["id"].copy_(torch.from_numpy(np.asarray(tick["id"], np.int64)))

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
            rc = _capi.debug_streams_link_host(*self.ptrs(**over))
        else:
            _capi.use_hooks(False)
            _capi.streams_link(*self.ptrs(**over), torch.cuda.current_stream(self.device).cuda_stream)
            rc = 0
        self.arena.check()
        return rc, self.read()

    def read(self):
        out = {k: self.t[k].cpu().numpy().copy() for k in OUT_KEYS}
        out["state"] = self.t["state"].cpu().numpy().copy().view(np.uint8)
        return out


def poisoned(a):
    return (np.ascontiguousarray(a).reshape(-1).view(np.uint32) == FILL32).all()


def agree(got, want, what=None, keys=OUT_KEYS + ("state",)):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4].tolist())


def restate_case(case):
    """The restatement over the case's ticks -> per tick the outputs and the state's bytes after it."""
    N, C, G, J = case["N"], case["C"], case["G"], case["J"]
    st = unpack_state(case["state0"], N, C, G, J)
    outs = []
    for tick in case["ticks"]:
        out = restate(st, case, tick["world"], tick["emit"], tick["status"], tick["id"])
        out["state"] = pack_state(st, N, C, G, J)
        outs.append(out)
    return outs


# ------------------------------------------------------------------------------------ the seeded cases

SHAPES = [(1, 1, 1, 1), (1, 2, 3, 4), (2, 3, 5, 3), (1, 16, 2, 32), (1, 2, 32, 32), (1, 4, 32, 2)]
MAX_MISSED = 2
TICKS = 12


def case_ids():
    """(N, C, P, G, J, M, break_dist on, kind of the first state): every shape twice; J in {1, 14, 17}, M = C and M = 16, the break
    test off and on and the three first states (zero, 0xA5 bytes, the same stream linked twice) rotate over them."""
    out, k = [], 0
    for (N, C, P, G) in SHAPES:
        for rep in range(2):
            out.append((N, C, P, G, (17, 14, 1)[k % 3], C if k % 2 else 16, k % 4 in (1, 2), ("zero", "a5", "twice")[(k // 2) % 3]))
            k += 1
    return out


def make_case(N, C, P, G, J, M, breaking, first, seed=0):
    """A scene per n: people 2 m apart who enter and leave at seeded ticks and walk 5 cm per tick; every camera sees each of them
    with 4 cm of its own offset and 1 cm of noise, in a slot that is the camera's own track table: a person keeps its slot and
    track identity while it is seen, loses them at seeded ticks (a new identity in the same or another slot follows) - more people
    than G and than P at times.  A quarter of the joints are non-finite, a fifth of the streams did not finish.  On top of that
    the edge cases, at fixed ticks: every stream a far-away stranger (more births than free people), two bit-identical candidates
    in one camera (the ties), identities that go to -1 and change in place, a member that jumps 3 m (the break test), NaN and Inf
    rows."""
    rng = np.random.RandomState(100003 * seed + 7919 * N + 1009 * C + 101 * P + 11 * G + J + 3 * M)
    S = N * C * P
    people = min(max(P, G) + 2, 10)
    home = np.stack([[2.0 * (k % 4), 2.0 * (k // 4), 3.0] for k in range(people)])
    shape = np.random.RandomState(5).uniform(-0.4, 0.4, (17, 3))[:J]
    vel = 0.05 * rng.standard_normal((N, people, 3))
    start = rng.randint(0, 3, (N, people))
    stop = start + rng.randint(3, TICKS + 2, (N, people))
    offset = 0.04 * rng.uniform(-1, 1, (N, C, 3))
    slot_of = -np.ones((N, C, people), np.int64)           # the camera's track table: person -> slot
    ident = -np.ones((N, C, P), np.int64)                  # slot -> track identity
    next_track = np.zeros((N, C), np.int64)
    ticks = []
    for t in range(TICKS):
        world = rng.uniform(-50, 50, (S, J, 3))             # (a free slot's row is whatever it is)
        emit = np.full(S, -1, np.int64)
        status = np.zeros(S, np.int32)
        for n in range(N):
            for c in range(C):
                for k in range(people):
                    seen_now = start[n, k] <= t < stop[n, k] and rng.uniform() > 0.15
                    p = slot_of[n, c, k]
                    if p >= 0 and (not seen_now or rng.uniform() < 0.1):        # the track ends
                        ident[n, c, p], slot_of[n, c, k], p = -1, -1, -1
                    if seen_now and p < 0:                                       # a new track on a free slot
                        free = [q for q in range(P) if ident[n, c, q] < 0]
                        if free:
                            p = free[rng.randint(len(free))]
                            ident[n, c, p], slot_of[n, c, k] = next_track[n, c], p
                            next_track[n, c] += 1
                    if p >= 0:
                        s = (n * C + c) * P + p
                        world[s] = home[k] + vel[n, k] * t + shape + offset[n, c] + 0.01 * rng.standard_normal((J, 3))
                        emit[s] = t
                        world[s][rng.uniform(size=J) < 0.25] = np.nan
                        if rng.uniform() < 0.2:
                            emit[s] = -1 if rng.uniform() < 0.5 else emit[s]
                            status[s] = 0 if emit[s] < 0 else 3
        ids = ident.reshape(S).copy()
        jumped = -1
        n, c = t % N, t % C
        base = (n * C + c) * P
        if t == 3:                                           # strangers everywhere: more births than free people
            for p in range(P):
                world[base + p] = np.array([30.0 + 3 * p, -20.0, 5.0]) + shape
                emit[base + p], status[base + p] = t, 0
                if ids[base + p] < 0:
                    ids[base + p] = 1000 + p
        elif t == 4:                                         # (the strangers' tracks are gone again) ... and Inf rows
            world[base, 0, 0], world[base, (1 % J), 2] = np.inf, -np.inf
        elif t == 5 and P >= 2:                              # two bit-identical candidates: the tie rule
            world[base + 1] = world[base]
            emit[base + 1], status[base + 1] = emit[base], status[base]
            if ids[base] >= 0 and ids[base + 1] < 0:
                ids[base + 1] = 2000
        elif t == 6:                                         # identities go to -1 / change in place
            ids[base] = -1
            ids[base + P - 1] = 3000 if ids[base + P - 1] >= 0 else ids[base + P - 1]
        elif t == 7:                                         # a member jumps 3 m: the break test (and a plain mismatch without it)
            tracked = [p for p in range(P) if ids[base + p] >= 0]
            if tracked:
                jumped = base + tracked[0]
                world[jumped] = world[jumped] + 3.0
                emit[jumped], status[jumped] = t, 0
        elif t == 8:                                         # everything NaN in one camera
            world[base:base + P] = np.nan
        ticks.append(dict(world=world, emit=emit, status=status, id=ids, jumped=jumped))
    nbytes = state_bytes(N, C, G, J)
    if first == "a5":
        state0 = np.full(nbytes, 0xA5, np.uint8)
    else:
        state0 = np.zeros(nbytes, np.uint8)
        if first == "twice":                                 # every person live on slot 1 (and, where there is one, 2) of every camera
            st = unpack_state(state0, N, C, G, J)
            st["phase"][:] = 1
            st["seen"][:] = 0xFFFFFFFF
            st["pid"][:] = np.arange(N * G)
            st["next_id"][:] = G
            st["link"][:] = np.where(np.arange(N * G)[:, None] % 3 == 2, min(2, P), 1)
            st["link"][0, 0] = P + 1                         # (out of range: reads as none)
            st["link_id"][:] = 0                             # the identity the first track of every camera gets
            st["ref"][:] = home[0] + shape
            state0 = pack_state(st, N, C, G, J)
    return dict(N=N, C=C, P=P, G=G, M=M, J=J, min_joints=min(4, J), min_common=min(3, J), max_missed=MAX_MISSED, max_dist=0.5,
                break_dist=1.0 if breaking else 0.0, state0=state0, ticks=ticks)


@functools.lru_cache(maxsize=None)
def host_run(*key):
    """A seeded case played on the host hook, once per session -> (case, per-tick outputs with the state after the tick).  The GPU
    suite compares the device against it, the host suite compares it against the restatement."""
    case = make_case(*key)
    rig = LinkRig("cpu", case)
    outs = []
    for tick in case["ticks"]:
        rc, out = rig.run(tick)
        assert rc == 0
        outs.append(out)
    _capi.use_hooks(False)
    return case, outs
