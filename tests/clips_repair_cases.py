"""What tests/test_clips_repair_host.py and tests/test_gpu_clips_repair.py share (a helper, not a test): a NumPy RESTATEMENT of
r3d_clips_repair, written from the rule table of include/ray3d_hip.h - a plain double loop per (clip, joint), the interpolation in
float64 with one cast; it does not call the library -, the case generator, and a rig that keeps every buffer of one call inside
guard bands (tests/buffers_util.py) and runs it on the host hook ("cpu") or on the device."""
import functools

import numpy as np
import torch

import buffers_util as bu
from conftest import hooks_library
from ray3d_amd import _capi, evaluate

QNAN = 0x7FC00000
SNAN = 0x7F800001                 # a signalling-NaN payload
PINF, NINF = 0x7F800000, 0xFF800000
FILL_BITS = 0xC0E00000            # -7.0f: what the rows of x / x_mirror no clip covers hold
FILL_STATE, FILL_STATS, FILL_STATUS = 0x5A, 0x5EED5EED, -77
SIGN = 0x80000000
KPS = {17: ([4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]), 3: ([1], [2])}
R_VALUES = (1, 2, 63, 64, 65, 255, 256, 257, 600)
PADS = ((0, 0), (13, 13), (26, 7))          # (pad_front, pad_back): none, a centred RF 27, a causal RF 27 with a surplus of 7 rows


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mirror_perm(J):
    return evaluate.mirror_permutation(J, *KPS[J])


# ------------------------------------------------------------------------------------ the restatement

def finite_bits(b):
    return (int(b) & 0x7F800000) != 0x7F800000


def interp_bits(a_bits, e_bits, m, g):
    """fl32(a + (e - a) * (m / (g + 1))) in float64, every operation rounded once, one cast; a NaN is the canonical quiet NaN."""
    a, e = np.float64(np.uint32(a_bits).view(np.float32)), np.float64(np.uint32(e_bits).view(np.float32))
    with np.errstate(all="ignore"):
        f = np.float32(a + (e - a) * (np.float64(m) / np.float64(g + 1)))
    return QNAN if f != f else int(f.view(np.uint32))


def descriptor_valid(d, out_rows, max_rows, total_frames):
    """INVALID DESCRIPTORS of the header; total_frames None: no confidences, the source range is not judged."""
    n, pf, pb, at, first = (int(d[k]) for k in ("n_frames", "pad_front", "pad_back", "out_first", "first_frame"))
    if n < 1 or pf < 0 or pb < 0:
        return False
    R = pf + n + pb
    if R > max_rows or R > _capi.REPAIR_MAX_ROWS or at < 0 or at + R > out_rows:
        return False
    return total_frames is None or (first >= 0 and first + n <= total_frames)


def restate(x, xm, perm, table, out_rows, max_rows, conf, min_conf, max_gap, state=None, stats=None, status=None):
    """The rule on uint32 copies of x (out_rows, J, F) / xm (or None): -> (x, xm, state, stats, status); `state` / `stats` /
    `status`: what the buffers held before (None: not asked for / all zero)."""
    x, xm = x.copy(), (xm.copy() if xm is not None else None)
    entry = x.copy()                                      # decided on the contents at entry
    J, F = x.shape[1:]
    state = state.copy() if state is not None else None
    stats = stats.copy() if stats is not None else None
    status = status.copy() if status is not None else np.zeros(len(table), np.int32)
    total = None if conf is None else conf.shape[0]
    for c, d in enumerate(table):
        ok = descriptor_valid(d, out_rows, max_rows, total)
        status[c] = 0 if ok else 1
        if not ok:
            continue
        n, pf, pb, at, first = (int(d[k]) for k in ("n_frames", "pad_front", "pad_back", "out_first", "first_frame"))
        R = pf + n + pb
        for j in range(J):
            def observed(r):
                if not all(finite_bits(entry[at + r, j, k]) for k in range(F)):
                    return False
                return conf is None or bool(conf[first + min(max(r - pf, 0), n - 1), j] >= np.float32(min_conf))
            obs = [observed(r) for r in range(R)]
            O = [r for r in range(R) if obs[r]]
            below, above, last = [None] * R, [None] * R, None      # the largest o in O below r, the smallest above
            for r in range(R):
                below[r] = last
                last = r if obs[r] else last
            last = None
            for r in range(R - 1, -1, -1):
                above[r] = last
                last = r if obs[r] else last
            counts = [0, 0, 0, 0, 0]
            for r in range(R):
                if obs[r]:
                    st = 0
                else:
                    if not O:
                        st, v = 4, [QNAN] * F
                    elif below[r] is None:
                        st, v = 3, [int(entry[at + O[0], j, k]) for k in range(F)]
                    else:
                        p, q = below[r], above[r]
                        if q is not None and q - p - 1 <= max_gap:
                            st, v = 1, [interp_bits(entry[at + p, j, k], entry[at + q, j, k], r - p, q - p - 1) for k in range(F)]
                        else:
                            st, v = 2, [int(entry[at + p, j, k]) for k in range(F)]
                    x[at + r, j] = v
                    if xm is not None:
                        dest = list(perm).index(j)        # x_mirror[row, dest] is x[row, perm[dest]]
                        xm[at + r, dest] = [v[0] ^ SIGN] + v[1:]
                if state is not None:
                    state[at + r, j] = st
                if pf <= r < pf + n:
                    counts[st] += 1
            if stats is not None:
                stats[c, j] = counts[1:]
    return x, xm, state, stats, status


# ------------------------------------------------------------------------------------ the cases

def _holes(kind, R, max_gap, rng):
    """Missing LOCAL rows of one (clip, joint) of R rows."""
    miss = np.zeros(R, bool)
    if kind == 1:                                         # never observed
        miss[:] = True
    elif kind == 2:                                       # random drop-out
        miss = rng.random(R) < 0.3
    elif kind == 3:                                       # a gap that straddles a 64-row word boundary
        miss[60:69] = True
    elif kind == 4:                                       # ... and one that straddles a 256-row step boundary
        miss[250:263] = True
        miss[3:3 + max_gap] = True                        # exactly max_gap (row 2 and the row behind are observed)
        miss[70:70 + max_gap + 1] = True                  # max_gap + 1
    elif kind == 5:                                       # a first observation at local row >= 64
        miss[:70] = True
    elif kind == 6:                                       # ... at >= 256, and a last observation more than 256 rows before the end
        miss[:300] = True
        miss[320:] = True
    elif kind == 7:                                       # one observation, then missing to the end
        miss[1:] = True
    elif kind == 8:                                       # gaps of max_gap and max_gap + 1 across the word / step boundaries
        miss[max(64 - max_gap // 2, 1):max(64 - max_gap // 2, 1) + max_gap] = True
        miss[256 - 1:256 + max_gap] = True
    return miss


def _missing_value(kind, F, finite):
    """A missing point's bits: NaN, +Inf, -Inf in every component, or a signalling NaN in one component only."""
    if kind == 3:
        v = [int(b) for b in finite]
        v[F - 1] = SNAN
        return v
    return [(QNAN, PINF, NINF)[kind]] * F


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> dict(J, F, perm, table, x, xm (uint32, or None), conf, min_conf, max_gap, out_rows, max_rows, total)."""
    spec = CASES[name]
    J, F, max_gap = spec["J"], spec["F"], spec["max_gap"]
    rng = np.random.default_rng(spec["seed"])
    clips = [(R, pf, pb) for (pf, pb) in spec.get("pads", PADS) for R in spec.get("R", R_VALUES) if R - pf - pb >= 1]
    order = rng.permutation(len(clips))                   # stored shuffled, with gaps
    table = np.zeros(len(clips) + len(spec.get("invalid", ())), dtype=_capi.clip_input_desc_dtype())
    src_at, out_at = 2, 3
    for c in order:
        R, pf, pb = clips[c]
        table[c]["first_frame"], table[c]["n_frames"], table[c]["out_first"] = src_at, R - pf - pb, out_at
        table[c]["pad_front"], table[c]["pad_back"] = pf, pb
        src_at += R - pf - pb + int(rng.integers(0, 4))
        out_at += R + int(rng.integers(0, 6))
    total, out_rows = src_at + 1, out_at + 2
    max_rows = spec.get("max_rows", max(R for R, _, _ in clips))
    src = rng.normal(0, 1, (total, J, F)).astype(np.float32)
    conf = None
    if spec["conf"]:
        conf = rng.uniform(0.5, 1.0, (total, J)).astype(np.float32)
    srcb = bits(src).copy()
    for c, (R, pf, pb) in enumerate(clips):
        first, n = int(table[c]["first_frame"]), R - pf - pb
        for j in range(J):
            kind = 0 if spec.get("complete") == c else (j + 3 * c + spec["seed"]) % 9
            miss = _holes(kind, R, max_gap, rng)[pf:pf + n]       # the own frames' rows
            for f in np.nonzero(miss)[0]:
                how = (f + j) % (6 if conf is not None else 4)
                if how < 4:
                    srcb[first + f, j] = _missing_value(how, F, srcb[first + f, j])
                else:                                     # finite, but not confident: a NaN confidence, or one below min_conf
                    conf[first + f, j] = np.nan if how == 4 else np.float32(spec["min_conf"]) - np.float32(0.25)
            if conf is not None and n > 2 and not miss[1]:
                conf[first + 1, j] = np.float32(spec["min_conf"])          # exactly min_conf: observed
    perm = mirror_perm(J) if spec["mirror"] else None
    x = np.full((out_rows, J, F), FILL_BITS, np.uint32)
    for c, (R, pf, pb) in enumerate(clips):
        first, n, at = int(table[c]["first_frame"]), R - pf - pb, int(table[c]["out_first"])
        x[at:at + R] = srcb[first + np.clip(np.arange(R) - pf, 0, n - 1)]
    for k, over in enumerate(spec.get("invalid", ())):   # a copy of clip k's descriptor, made invalid: nothing of it may change
        c = len(clips) + k
        table[c] = table[k]
        for key, v in over.items():
            table[c][key] = v(table[k], out_rows) if callable(v) else v
    xm = None
    if perm is not None:
        xm = x[:, perm].copy()
        xm[..., 0] ^= SIGN
        xm[(x == FILL_BITS).all(axis=(1, 2))] = FILL_BITS
    return dict(J=J, F=F, perm=perm, table=table, x=x, xm=xm, conf=conf, min_conf=spec["min_conf"], max_gap=max_gap, out_rows=out_rows,
                max_rows=max_rows, total=total, clips=clips)


CASES = {
    "j17_f3_gap5": dict(J=17, F=3, max_gap=5, mirror=True, conf=False, min_conf=0.0, seed=1),
    "j3_f2_gap0_conf": dict(J=3, F=2, max_gap=0, mirror=False, conf=True, min_conf=0.75, seed=2),
    "j17_f2_gap1_conf": dict(J=17, F=2, max_gap=1, mirror=True, conf=True, min_conf=0.625, seed=3, R=(2, 65, 256, 600)),
    "j3_f3_gap300": dict(J=3, F=3, max_gap=300, mirror=True, conf=False, min_conf=0.0, seed=4),
    "j17_f3_gapR": dict(J=17, F=3, max_gap=600, mirror=False, conf=False, min_conf=0.0, seed=5, R=(1, 257, 600), complete=1),
    # a table of five: three pad-free clips, then copies of the first two made invalid - one whose output rows leave the buffer, one
    # with R > max_rows (max_rows is the third clip's 65 rows; the copy of the 64-row clip claims three pad rows more)
    "five_two_invalid": dict(J=17, F=3, max_gap=5, mirror=True, conf=True, min_conf=0.75, seed=6, R=(63, 64, 65), pads=((0, 0),), max_rows=65,
                             invalid=(dict(out_first=lambda d, out_rows: out_rows - int(d["n_frames"]) + 1), dict(pad_back=3))),
}
CASE_NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement of case `name` with every optional output, over buffers pre-filled as the rig fills them."""
    c = make_case(name)
    nclips = len(c["table"])
    return restate(c["x"], c["xm"], c["perm"], c["table"], c["out_rows"], c["max_rows"], c["conf"], c["min_conf"], c["max_gap"],
                   np.full((c["out_rows"], c["J"]), FILL_STATE, np.uint8), np.full((nclips, c["J"], 4), FILL_STATS, np.uint32).view(np.int32),
                   np.full(nclips, FILL_STATUS, np.int32))


# ------------------------------------------------------------------------------------ the rig

def run(device, x, xm, perm, table, out_rows, max_rows, conf, min_conf, max_gap, want_state=True, want_stats=True,
        pattern=bu.NANS):
    """One call on exact-size regions of one pattern-filled arena on `device` ("cpu": the host hook; a cuda device: the kernel); x
    and x_mirror 4 bytes off their alignment; state / stats / status pre-poisoned; the guards are checked.
    -> dict(rc, x, xm, state, stats, status) of NumPy copies (state / stats as poisoned when not asked for)."""
    device = torch.device(device)
    J, F = x.shape[1:]
    nclips = len(table)
    x, xm = bits(x).view(np.int32), (bits(xm).view(np.int32) if xm is not None else None)
    arrays = [("x", x), ("table", np.ascontiguousarray(table).view(np.uint8)), ("state", np.full((out_rows, J), FILL_STATE, np.uint8)),
              ("stats", np.full((nclips, J, 4), FILL_STATS, np.uint32).view(np.int32)), ("status", np.full(nclips, FILL_STATUS, np.int32))]
    if xm is not None:
        arrays.append(("xm", xm))
    if conf is not None:
        arrays.append(("conf", conf))
    arena = bu.Arena(device, pattern, bu.Arena.capacity_for([a.nbytes for _, a in arrays]))
    t = {n: arena.put(a, 256, 4 if n in ("x", "xm", "conf") else 0, n)() for n, a in arrays}
    ptr = lambda n: t[n].data_ptr() if n in t else None
    args = (ptr("x"), out_rows, J, F, ptr("xm"), perm, ptr("table"), nclips, max_rows, ptr("conf"), conf.shape[0] if conf is not None else 0,
            min_conf, max_gap, ptr("state") if want_state else None, ptr("stats") if want_stats else None, ptr("status"))
    if device.type == "cpu":
        hooks_library()
        rc = _capi.debug_clips_repair_host(*args)
    else:
        with torch.cuda.device(device):
            _capi.clips_repair(*args, torch.cuda.current_stream(device).cuda_stream)
        rc = 0
    arena.check()
    out = {n: t[n].cpu().numpy().copy() for n in ("state", "stats", "status")}
    out["x"] = t["x"].cpu().numpy().view(np.uint32).copy()
    out["xm"] = t["xm"].cpu().numpy().view(np.uint32).copy() if xm is not None else None
    out["rc"] = rc
    return out


def run_case(device, name, **kw):
    c = make_case(name)
    return run(device, c["x"], c["xm"], c["perm"], c["table"], c["out_rows"], c["max_rows"], c["conf"], c["min_conf"], c["max_gap"], **kw)


@functools.lru_cache(maxsize=None)
def host_case(name):
    """The host hook on case `name`, once per session: what the device is held to."""
    return run_case("cpu", name)


def agree(got, want, what):
    """The five outputs of two runs, bit for bit."""
    for k in ("x", "xm", "state", "stats", "status"):
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5])
