"""r3d_clips_repair without a GPU: the exports, the header and the ABI version; every argument rule through the host hook and through
the product entry point (on pointers that are never followed); the host hook against the NumPy restatement of
tests/clips_repair_cases.py over every case, bit for bit in all five outputs; repair(pad(clip)) == pad(repair(clip)); and the live
rule's bits: a stream of at most RF frames pushed through r3d_streams_repair + r3d_streams_step leaves in its ring what the offline
rule makes of the same rows."""
import os
import re

import numpy as np
import pytest

import clips_repair_cases as cc
import streams_repair_cases as rc
from clips_repair_cases import FILL_BITS, FILL_STATE, FILL_STATS, FILL_STATUS, QNAN, bits
from conftest import ROOT, hooks_library
from ray3d_amd import _capi
from streams_cases import NONE, PUSH, RESTART

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed


def _define(name):
    return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, HDR).group(1))


# ------------------------------------------------------------------------------------ header, binding, exports

def test_exports_header_and_abi():
    assert "r3d_clips_repair" in _capi.EXPORTS and "r3d_debug_clips_repair_host" in _capi.HOOK_EXPORTS
    assert "r3d_debug_clips_repair_host" not in _capi.EXPORTS and "r3d_clips_repair" not in _capi.HOOK_EXPORTS
    assert re.search(r"\bint r3d_clips_repair\(", HDR) and re.search(r"\bint r3d_debug_clips_repair_host\(", HDR)
    assert hasattr(_capi.load(), "r3d_clips_repair") and not hasattr(_capi.load(), "r3d_debug_clips_repair_host")
    assert hasattr(hooks_library(), "r3d_debug_clips_repair_host") and hasattr(hooks_library(), "r3d_clips_repair")
    assert _define("R3D_ABI_VERSION") == _capi.ABI_VERSION == 6          # no struct changed
    assert _define("R3D_REPAIR_MAX_ROWS") == _capi.REPAIR_MAX_ROWS == 65536
    assert "near FLT_MAX" in HDR                                         # the one exception to "finite afterwards" is stated


# ------------------------------------------------------------------------------------ the argument rules

def _host_buffers(rows, J, F, nclips, total):
    def aligned(nbytes):
        raw = np.zeros(nbytes + 8, np.uint8)
        return raw[(-raw.ctypes.data) % 8:][:nbytes]
    table = aligned(nclips * _capi.CLIP_INPUT_DESC_BYTES)
    t = table.view(_capi.clip_input_desc_dtype())
    for c in range(nclips):
        t[c]["first_frame"], t[c]["n_frames"], t[c]["out_first"] = 2 * c, 2, 2 * c
    # x and x_mirror are the two halves of one array, so that "adjacent" and "overlapping" are exact statements
    both = np.full((2 * rows, J, F), np.nan, np.float32)
    return dict(both=both, table=table, conf=np.ones((total, J), np.float32), state=np.full((rows, J), 9, np.uint8),
                stats=np.full((nclips, J, 4), 9, np.int32), status=np.full(nclips, 9, np.int32))


def test_argument_rules():
    """Every R3D_ERR_ARG rule of the header through the host hook, each with its word in the message; nothing is written."""
    hooks = hooks_library()
    rows, J, F, nclips, total = 8, 17, 3, 3, 6
    b = _host_buffers(rows, J, F, nclips, total)
    p = {k: v.ctypes.data for k, v in b.items()}
    xb = rows * J * F * 4
    perm = cc.mirror_perm(J)
    base = dict(x=p["both"], rows=rows, J=J, F=F, xm=p["both"] + xb, perm=perm, table=p["table"], n=nclips, max_rows=4, conf=p["conf"], total=total,
                min_conf=0.5, max_gap=2, state=p["state"], stats=p["stats"], status=p["status"])

    def call(**kw):
        a = dict(base, **kw)
        return _capi.debug_clips_repair_host(a["x"], a["rows"], a["J"], a["F"], a["xm"], a["perm"], a["table"], a["n"], a["max_rows"], a["conf"],
                                             a["total"], a["min_conf"], a["max_gap"], a["state"], a["stats"], a["status"])

    big = _capi.ENCODE_MAX_POINTS
    bad = [(dict(x=0), "null"), (dict(table=0), "null"), (dict(status=0), "null"), (dict(F=1), "in_features"), (dict(F=4), "in_features"),
           (dict(J=0), "num_joints"), (dict(J=18), "num_joints"), (dict(n=0), "num_clips"), (dict(n=_capi.CLIPS_MAX + 1), "num_clips"),
           (dict(max_rows=0), "max_rows"), (dict(max_rows=_capi.REPAIR_MAX_ROWS + 1), "max_rows"), (dict(rows=0), "out_rows"),
           (dict(rows=big + 1), "out_rows"), (dict(max_gap=-1), "max_gap"), (dict(max_gap=_capi.REPAIR_MAX_ROWS + 1), "max_gap"),
           (dict(min_conf=float("nan")), "min_conf"), (dict(min_conf=float("inf")), "min_conf"), (dict(min_conf=float("-inf")), "min_conf"),
           (dict(total=0), "total_frames"), (dict(total=-3), "total_frames"), (dict(xm=0), "go together"), (dict(perm=None), "go together"),
           (dict(perm=[0] * J), "permutation"), (dict(perm=list(range(1, J + 1))), "permutation"), (dict(table=p["table"] + 4), "aligned"),
           (dict(xm=p["both"]), "x_dev overlaps x_mirror_dev"), (dict(xm=p["both"] + xb - 4), "x_dev overlaps x_mirror_dev"),
           (dict(x=p["both"] + 4), "x_dev overlaps x_mirror_dev"),
           (dict(state=p["both"]), "state_dev overlaps x_dev"), (dict(state=p["both"] + xb - 1), "state_dev overlaps x_dev"),
           (dict(state=p["both"] + 2 * xb - 1), "state_dev overlaps x_mirror_dev"), (dict(stats=p["both"] + xb - 4), "stats_dev overlaps x_dev"),
           (dict(stats=p["both"] + xb), "stats_dev overlaps x_mirror_dev"), (dict(status=p["both"] + 8), "status_dev overlaps x_dev"),
           (dict(status=p["both"] + xb + 8), "status_dev overlaps x_mirror_dev"), (dict(conf=p["both"] + xb - 4), "conf_dev overlaps x_dev"),
           (dict(conf=p["both"] + 2 * xb - 4), "conf_dev overlaps x_mirror_dev"), (dict(table=p["both"] + 16), "clip table overlaps x_dev"),
           (dict(table=p["both"] + xb + 16), "clip table overlaps x_mirror_dev"),
           (dict(x=p["state"], xm=0, perm=None), "state_dev overlaps x_dev")]
    before = {k: v.copy() for k, v in b.items()}
    for kw, word in bad:
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
        assert word in hooks.r3d_last_error().decode(), (kw, hooks.r3d_last_error())
    assert all(np.array_equal(b[k].view(np.uint8), before[k].view(np.uint8)) for k in b)       # nothing was written
    assert call() == 0 and b["status"].tolist() == [0, 0, 0]
    assert call(conf=0, total=0) == 0 and call(conf=0, total=-5) == 0 and call(xm=0, perm=None) == 0 and call(state=0, stats=0) == 0
    assert call(F=2) == 0 and call(max_gap=0) == 0 and call(max_gap=_capi.REPAIR_MAX_ROWS) == 0 and call(min_conf=-3.0) == 0
    assert call(max_rows=_capi.REPAIR_MAX_ROWS) == 0 and call(J=1, perm=[0]) == 0


def test_device_entry_point_refuses_before_any_device_call():
    """The same rules through r3d_clips_repair itself, on pointers that are never followed: R3D_ERR_ARG without a GPU."""
    import ctypes as C
    lib = _capi.load()
    J = 17
    good = (C.c_int32 * J)(*cc.mirror_perm(J))
    xb = 1000 * J * 3 * 4

    def call(x=BOGUS, rows=1000, J=J, F=3, xm=64 * BOGUS, perm=good, table=2 * BOGUS, n=5, max_rows=300, conf=3 * BOGUS, total=900,
             min_conf=0.0, max_gap=5, state=4 * BOGUS, stats=5 * BOGUS, status=6 * BOGUS):
        return lib.r3d_clips_repair(x, rows, J, F, xm, perm, table, n, max_rows, conf, total, min_conf, max_gap, state, stats, status, None)

    twice = (C.c_int32 * J)(*([0] * J))
    for kw in (dict(x=None), dict(table=None), dict(status=None), dict(F=1), dict(F=4), dict(J=0), dict(J=18), dict(n=0), dict(n=65536),
               dict(max_rows=0), dict(max_rows=65537), dict(rows=0), dict(rows=2 ** 31), dict(max_gap=-1), dict(max_gap=65537),
               dict(min_conf=float("nan")), dict(min_conf=float("inf")), dict(total=0), dict(xm=None), dict(perm=None), dict(perm=twice),
               dict(table=2 * BOGUS + 4), dict(xm=BOGUS + xb - 4), dict(state=BOGUS + 8), dict(state=64 * BOGUS + xb - 1),
               dict(stats=BOGUS + xb - 4), dict(status=64 * BOGUS), dict(conf=BOGUS + 4), dict(table=BOGUS + 160),
               dict(x=4 * BOGUS - xb + 8, xm=None, perm=None)):
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
        assert lib.r3d_last_error()


# ------------------------------------------------------------------------------------ the hook against the restatement

@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_host_hook_equals_the_restatement(name):
    """x, x_mirror, state, stats and status of the host hook, inside guard bands, are the restatement's - bit for bit.  With it:
    rows no valid clip covers keep their fill, nothing of an invalid clip changes (its poisoned stats row included), and a clip
    without a missing point keeps its exact bits."""
    c, got = cc.make_case(name), cc.host_case(name)
    x, xm, state, stats, status = cc.restated(name)
    assert got["rc"] == 0
    cc.agree(got, dict(x=x, xm=xm, state=state, stats=stats, status=status), name)
    covered = np.zeros(c["out_rows"], bool)
    for d, st in zip(c["table"], status):
        if st == 0:
            covered[int(d["out_first"]):int(d["out_first"] + d["pad_front"] + d["n_frames"] + d["pad_back"])] = True
    assert (got["x"][~covered] == FILL_BITS).all() and (got["state"][~covered] == FILL_STATE).all() and (~covered).any()
    if xm is not None:
        assert (got["xm"][~covered] == FILL_BITS).all()
    assert (got["stats"][status == 1].view(np.uint32) == FILL_STATS).all()
    touched = got["state"] != FILL_STATE
    assert np.array_equal(got["x"][touched & (got["state"] == 0)], c["x"][touched & (got["state"] == 0)])       # observed: never written


def test_the_cases_hold_what_they_promise():
    """The ingredients the issue lists are in the cases: every state, gaps of exactly max_gap and max_gap + 1, first observations at
    rows >= 64 and >= 256, a joint never observed, a gap-free clip, two invalid descriptors in a table of five."""
    seen = set()
    for name in cc.CASE_NAMES:
        c = cc.make_case(name)
        _, _, state, stats, status = cc.restated(name)
        seen |= set(np.unique(state[state != FILL_STATE]).tolist())
        if name == "five_two_invalid":
            assert len(c["table"]) == 5 and status.tolist() == [0, 0, 0, 1, 1]
        if name == "j17_f3_gapR":
            assert not stats[1].any() and stats[0].any()                 # the gap-free clip
        if name == "j17_f3_gap5":
            big = [k for k, (R, pf, pb) in enumerate(c["clips"]) if R == 600 and pf == 0][0]
            at = int(c["table"][big]["out_first"])
            s = state[at:at + 600]
            first = [int(np.argmax(s[:, j] != 3)) for j in range(17) if s[0, j] == 3]
            assert any(64 <= f < 256 for f in first) and any(f >= 256 for f in first)
            assert any((s[:, j] == 4).all() for j in range(17))
            runs = {(st, n) for j in range(17) for st, n in _runs(s[:, j])}
            assert (1, 5) in runs and (2, 6) in runs                     # a gap of max_gap is interpolated, one of max_gap + 1 held
    assert seen == {0, 1, 2, 3, 4}


def _runs(col):
    out, start = [], 0
    for r in range(1, len(col) + 1):
        if r == len(col) or col[r] != col[start]:
            out.append((int(col[start]), r - start))
            start = r
    return out


def test_optional_outputs_left_out_and_gap_free_clips():
    """Without state and stats the same x; and a buffer without a missing point is not written: pre-filled with a recognisable pattern
    of finite values, it keeps its exact bits, every state is 0 and every count 0."""
    name = "j17_f2_gap1_conf"
    got = cc.run_case("cpu", name, want_state=False, want_stats=False)
    want = cc.host_case(name)
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["xm"], want["xm"]) and np.array_equal(got["status"], want["status"])
    assert (got["state"] == FILL_STATE).all() and (got["stats"].view(np.uint32) == FILL_STATS).all()
    c = cc.make_case(name)
    x = (0x3F800000 + np.arange(c["x"].size, dtype=np.uint32) * 7).reshape(c["x"].shape)     # 1.0 upwards: finite, every word different
    xm = x[::-1].copy()
    out = cc.run("cpu", x, xm, c["perm"], c["table"], c["out_rows"], c["max_rows"], None, 0.0, c["max_gap"])
    assert np.array_equal(out["x"], x) and np.array_equal(out["xm"], xm) and not out["stats"].any()
    assert set(np.unique(out["state"]).tolist()) == {0, FILL_STATE}


# ------------------------------------------------------------------------------------ repair(pad(clip)) == pad(repair(clip))

def _one_clip(n, pf, pb):
    table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
    table[0]["n_frames"], table[0]["pad_front"], table[0]["pad_back"] = n, pf, pb
    return table


@pytest.mark.parametrize("pads", cc.PADS + ((0, 31),))
@pytest.mark.parametrize("J,F", [(17, 3), (3, 2)])
def test_repair_of_the_padded_clip_is_the_padding_of_the_repaired_clip(J, F, pads):
    """The unpadded clip repaired by the hook and then padded with np.pad(..., 'edge') equals the hook on the padded layout: x,
    x_mirror and state, for the pad shapes of the cases and for a surplus alone.  (First and last frames missing in some joints: the
    padding rows then repeat a missing frame and are repaired with it.)"""
    pf, pb = pads
    rng = np.random.default_rng(11 + J)
    n, max_gap = 300, 5
    perm = cc.mirror_perm(J)
    raw = bits(rng.normal(0, 1, (n, J, F)).astype(np.float32)).copy()
    for j in range(J):
        miss = cc._holes((j + 1) % 9, n, max_gap, rng)
        if j % 3 == 0:
            miss[:2 + j] = True
        if j % 3 == 1:
            miss[n - 1 - j:] = True
        raw[miss, j] = QNAN
    mir = raw[:, perm].copy()
    mir[..., 0] ^= cc.SIGN
    flat = cc.run("cpu", raw, mir, perm, _one_clip(n, 0, 0), n, n, None, 0.0, max_gap)
    edge = lambda a: np.pad(a, ((pf, pb),) + ((0, 0),) * (a.ndim - 1), "edge")
    padded = cc.run("cpu", edge(raw), edge(mir), perm, _one_clip(n, pf, pb), n + pf + pb, n + pf + pb, None, 0.0, max_gap)
    assert flat["rc"] == padded["rc"] == 0 and flat["state"].any()
    assert np.array_equal(padded["x"], edge(flat["x"])) and np.array_equal(padded["xm"], edge(flat["xm"]))
    assert np.array_equal(padded["state"], edge(flat["state"])) and np.array_equal(padded["stats"], flat["stats"])


# ------------------------------------------------------------------------------------ the live rule's bits

@pytest.mark.parametrize("with_conf", [False, True])
@pytest.mark.parametrize("F,N,max_gap", [(3, 27, 5), (2, 27, 26), (3, 20, 0), (3, 1, 3), (2, 9, 1)])
def test_the_live_ring_holds_the_offline_rule_s_bits(F, N, max_gap, with_conf):
    """Streams of N <= RF = 27 frames (R3D_ENCODE_NONE, random drop patterns) pushed tick by tick through r3d_debug_streams_repair_host
    + r3d_debug_streams_step_host: with N <= RF the ring holds every frame and the live back-fill reaches frame 0, so both rules are
    defined on the same frames - the ring's frames 0 .. N-1 (slot frame % RF) equal the offline hook on the same N rows, pads 0."""
    S, J, rf, lag, min_conf = 6, 17, 27, 13, 0.5
    rng = np.random.default_rng(100 * N + 10 * F + max_gap + int(with_conf))
    frames = rng.normal(0, 1, (S, N, J, F)).astype(np.float32)
    conf = rng.uniform(0.5, 1.0, (S, N, J)).astype(np.float32) if with_conf else None
    for s in range(S):
        drop = rng.random((N, J)) < (0.15, 0.4, 0.7, 0.3, 0.5, 0.9)[s]
        drop[:, s] = True                                                 # a joint never observed
        drop[: min(N, 3 + s), (s + 1) % J] = True                         # a late first observation
        for f, j in np.argwhere(drop):
            how = (f + j + s) % (6 if with_conf else 4)
            if how == 0:
                frames[s, f, j] = np.nan
            elif how == 1:
                frames[s, f, j, F - 1] = np.inf
            elif how == 2:
                frames[s, f, j, 0] = -np.inf
            elif how == 3:
                bits(frames)[s, f, j, 1] = cc.SNAN
            else:
                conf[s, f, j] = np.nan if how == 4 else 0.25
    rig = rc.RepairRig("cpu", S, rf, lag, J, F, NONE, max_gap=max_gap, min_conf=min_conf, zero_state=True, zero_track=True)
    for t in range(N):
        out = rig.tick(frames[:, t], np.full(S, RESTART if t == 0 else PUSH, np.int32), conf[:, t] if with_conf else None)
        assert out["rc"] == 0 and out["rc_step"] == 0 and not out["status"].any()
    ring = rig.state()[1]                                                 # (S, RF, J, F) uint32
    live = np.stack([np.stack([ring[s, f % rf] for f in range(N)]) for s in range(S)])
    table = np.zeros(S, dtype=_capi.clip_input_desc_dtype())
    for s in range(S):
        table[s]["first_frame"], table[s]["n_frames"], table[s]["out_first"] = s * N, N, s * N
    off = cc.run("cpu", bits(frames).reshape(S * N, J, F), None, None, table, S * N, N, conf.reshape(S * N, J) if with_conf else None,
                 min_conf, max_gap)
    assert off["rc"] == 0 and not off["status"].any()
    assert np.array_equal(off["x"].reshape(S, N, J, F), live)
    st = off["state"].reshape(S, N, J)
    assert (st == 4).any() and (st == 3).any() == (N > 1) and ((st == 1).any() or max_gap == 0 or N < 3)
