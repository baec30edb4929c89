"""CPU suite: the host side of r3d_clips_windows (a batch of materialised windows gathered from a pool of windows drawn from many
clips) - the layout of r3d_window_run_desc against the header, the exports, the argument rules (all checked before any device
call: they run without a GPU), and the host hook r3d_debug_clips_windows_host (the call's bisection, descriptor rule and per-point
routine on the CPU) against the REFERENCE's own windows (tests/golden/windows.npz, made by tests/golden/make_golden_windows.py:
UnchunkedGenerator + Trainer.eval_data_prepare, ChunkedGenerator) and against a NumPy restatement, inside guard bands
(tests/buffers_util.py).  tests/test_gpu_clips_windows.py runs the kernel on the layouts built here."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, hooks_library

import buffers_util as bu
import windows_cases as wc
from ray3d_amd import _capi, evaluate

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "windows.npz"))


def host_call(src, table, run_param, window0, batch, rf, perm, pattern=bu.NANS, skew=0):
    """r3d_debug_clips_windows_host with every buffer carved exact-sized out of one pattern-filled arena; x / param start as FILL,
    status as FILL_STATUS.  -> (rc, x, param, status); the guards are checked."""
    hooks_library()
    total, J, F = src.shape
    E = 0 if run_param is None else run_param.shape[1]
    x0 = np.full((batch, rf, J, F), wc.FILL, np.float32)
    p0 = np.full((batch, max(E, 1)), wc.FILL, np.float32)
    s0 = np.full(len(table), wc.FILL_STATUS, np.int32)
    arrays = [src, table.view(np.uint8), run_param if E else np.zeros(1, np.float32), x0, p0, s0]
    arena = bu.Arena("cpu", pattern, bu.Arena.capacity_for([a.nbytes for a in arrays]))
    names = ("src", "table", "run_param", "x", "param", "status")
    views = [arena.put(a, 256, skew if n in ("src", "x", "param") else 0, n)() for a, n in zip(arrays, names)]
    rc = _capi.debug_clips_windows_host(views[0].data_ptr(), total, J, F, rf, views[1].data_ptr(), len(table),
                                        views[2].data_ptr() if E else None, E, window0, batch, views[3].data_ptr(),
                                        views[4].data_ptr() if E else None, perm, views[5].data_ptr())
    arena.check()
    return rc, views[3].numpy().copy(), (views[4].numpy().copy() if E else None), views[5].numpy().copy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------ header, binding, exports

def test_struct_matches_header():
    body = re.search(r"typedef struct \{([^}]*)\} r3d_window_run_desc;\s*/\* 48 bytes", HDR).group(1)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", body)
    dt = _capi.window_run_dtype()
    assert [n for _, n in fields] == list(dt.names)
    at = 0
    for ctype, name in fields:
        size = 8 if ctype == "int64_t" else 4
        assert dt.fields[name][1] == at and dt.fields[name][0].itemsize == size and dt.fields[name][0].kind == "i"
        at += size
    assert at == dt.itemsize == _capi.WINDOW_RUN_DESC_BYTES == 48
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24, 32, 40, 44]


def test_exports_and_abi():
    assert "r3d_clips_windows" in _capi.EXPORTS and "r3d_debug_clips_windows_host" in _capi.HOOK_EXPORTS
    assert re.search(r"\bint r3d_clips_windows\(", HDR) and re.search(r"\bint r3d_debug_clips_windows_host\(", HDR)
    assert HDR.index("int r3d_debug_clips_windows_host(") > HDR.index("#ifdef R3D_TEST_HOOKS")
    product = C.CDLL(_capi.LIB_PATH)
    assert hasattr(product, "r3d_clips_windows") and not hasattr(product, "r3d_debug_clips_windows_host")
    hooks = hooks_library()
    assert hasattr(hooks, "r3d_clips_windows") and hasattr(hooks, "r3d_debug_clips_windows_host")
    assert hooks.r3d_abi_version() == 6 == _capi.ABI_VERSION and int(re.search(r"#define R3D_ABI_VERSION (\d+)", HDR).group(1)) == 6


def test_clip_window_table():
    table, win_first, total = evaluate.clip_window_table([3, 1, 7], 27, causal=False, flip=False, surplus=5)
    assert total == 11 and win_first == [0, 3, 4]
    assert table["first_frame"].tolist() == [0, 3, 4] and table["n_frames"].tolist() == [3, 1, 7]
    assert table["n_windows"].tolist() == [3, 1, 12] and table["win_first"].tolist() == win_first
    assert set(table["start"].tolist()) == {-13} and set(table["step"].tolist()) == {1} and set(table["flip"].tolist()) == {0}
    causal, _, _ = evaluate.clip_window_table([3, 1, 7], 27, causal=True, flip=True, first_frames=[10, 0, 20])
    assert set(causal["start"].tolist()) == {-26} and set(causal["flip"].tolist()) == {1} and causal["first_frame"].tolist() == [10, 0, 20]
    assert causal["n_windows"].tolist() == [3, 1, 7]
    with pytest.raises(ValueError):
        evaluate.clip_window_table([3], 27, surplus=-1)


# ------------------------------------------------------------------------------------ the reference's windows

@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("shift", ["centred", "causal"])
@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_evaluation_windows_equal_the_reference(case, shift, flip):
    """clip_window_table + the host twin == UnchunkedGenerator's edge padding + eval_data_prepare's windows (flip: the mirrored
    sequence), bit for bit - in one batch, and in batches of 16 that start and end inside clips and end in surplus windows."""
    z = golden()
    src, lengths = z[case + "_src"], z["lengths"].tolist()
    rf = {"rf27": 27, "rf9": 9}[case]
    want = z["%s_eval_s%d_f%d" % (case, (rf - 1) // 2 if shift == "causal" else 0, flip)]
    perm = evaluate.mirror_permutation(src.shape[1], z[case + "_kps_left"].tolist(), z[case + "_kps_right"].tolist())
    n = sum(lengths)
    assert want.shape == (n, rf) + src.shape[1:]
    table, _, total = evaluate.clip_window_table(lengths, rf, shift == "causal", bool(flip))
    rc, x, _, status = host_call(src, table, None, 0, n, rf, perm if flip else None)
    assert rc == 0 and total == n and same_bits(x, want) and (status == 0).all()
    surplus = -n % 16
    table, _, _ = evaluate.clip_window_table(lengths, rf, shift == "causal", bool(flip), surplus)
    for w0 in range(0, n + surplus, 16):
        rc, x, _, status = host_call(src, table, None, w0, 16, rf, perm if flip else None)
        assert rc == 0
        real = min(16, n - w0)
        assert same_bits(x[:real], want[w0:w0 + real])
        if real < 16:
            ref = wc.ref_windows(src, table, None, w0, 16, rf, perm if flip else None)[0]
            assert same_bits(x, ref)
        touched = np.nonzero(status != wc.FILL_STATUS)[0].tolist()
        first = np.searchsorted(np.cumsum(lengths), w0, side="right")
        assert touched and touched[0] == first and (status[touched] == 0).all()


@pytest.mark.parametrize("shift", ["centred", "causal"])
@pytest.mark.parametrize("case", ["rf27", "rf9"])
def test_training_chunks_equal_the_reference(case, shift):
    """ChunkedGenerator's (sequence, start, flip) chunks as hand-made one-window runs."""
    z = golden()
    src, lengths = z[case + "_src"], z["lengths"].tolist()
    rf = {"rf27": 27, "rf9": 9}[case]
    pad = (rf - 1) // 2
    s = pad if shift == "causal" else 0
    want, pairs = z["%s_chunk_s%d" % (case, s)], z["%s_chunk_s%d_pairs" % (case, s)]
    firsts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    table = np.zeros(len(pairs), dtype=_capi.window_run_dtype())
    for i, (seq, start, flip) in enumerate(pairs.tolist()):
        table[i] = (firsts[seq], lengths[seq], i, 1, start - pad - s, 1, flip)
    assert pairs[:, 2].min() == 0 and pairs[:, 2].max() == 1
    perm = evaluate.mirror_permutation(src.shape[1], z[case + "_kps_left"].tolist(), z[case + "_kps_right"].tolist())
    rc, x, _, status = host_call(src, table, None, 0, len(pairs), rf, perm)
    assert rc == 0 and same_bits(x, want) and (status == 0).all()


# ------------------------------------------------------------------------------------ the restatement: steps, order, gaps, payloads

@pytest.mark.parametrize("J,F,rf", [(17, 3, 27), (14, 2, 9)])
def test_steps_order_gaps_and_nan_payloads(J, F, rf):
    src, table, run_param, total = wc.scattered_layout(J, F, rf)
    perm = wc.mirror_perm(J)
    assert (np.diff(table["first_frame"]) < 0).any() and table["step"].max() > 1
    for w0, b in ((0, total), (3, 7), (total - 4, 9), (total, 3)):
        rc, x, param, status = host_call(src, table, run_param, w0, b, rf, perm, skew=4)
        rx, rp, rs = wc.ref_windows(src, table, run_param, w0, b, rf, perm)
        assert rc == 0 and same_bits(x, rx) and same_bits(param, rp) and np.array_equal(status, rs)
    rc, x, _, _ = host_call(src, table, run_param, 0, total, rf, perm)
    xb = x.view(np.uint32)
    for bits in (0x7FC12345, 0xFFC00001, 0x7F800001):
        assert (xb == bits).any() or (xb == bits ^ 0x80000000).any()
    assert not (xb == 0x7FC00BAD).any() and not (xb == 0x7FC00BAD ^ 0x80000000).any()      # nothing came out of the gaps


def test_invalid_runs_are_not_followed():
    """Every kind of invalid descriptor: status 1, its windows' rows keep what they held, every other run's rows are what they are
    without it, nothing outside the buffers is written (the guard bands).  The kinds that break the order of win_first stand at
    the table's start, where the bisection still ends on them."""
    J, F, rf = 17, 3, 9
    src, table, run_param, total = wc.eval_layout(J, F, rf, lengths=(4, 1, 6, 3, 9))
    perm = wc.mirror_perm(J)
    good = wc.ref_windows(src, table, run_param, 0, total, rf, perm)
    r = 2
    w0, w1 = int(table[r]["win_first"]), int(table[r]["win_first"] + table[r]["n_windows"])
    kinds = dict(wc.invalid_cases(table[r], src.shape[0]))
    for name, bad in kinds.items():
        t = table.copy()
        t[r] = bad
        rc, x, param, status = host_call(src, t, run_param, 0, total, rf, perm)
        assert rc == 0, name
        assert status[r] == 1 and (np.delete(status, r) == 0).all(), name
        assert (x[w0:w1] == wc.FILL).all() and (param[w0:w1] == wc.FILL).all(), name
        keep = np.r_[0:w0, w1:total]
        assert same_bits(x[keep], good[0][keep]) and same_bits(param[keep], good[1][keep]), name
    # a flip run without mirror_perm
    t = table.copy()
    t[r]["flip"] = 1
    rc, x, param, status = host_call(src, t, run_param, 0, total, rf, None)
    assert rc == 0 and status[r] == 1 and (x[w0:w1] == wc.FILL).all() and same_bits(x[:w0], good[0][:w0])
    rc, x, _, status = host_call(src, t, run_param, 0, total, rf, perm)
    assert rc == 0 and status[r] == 0 and not (x[w0:w1] == wc.FILL).any()
    # a negative win_first (run 0: every window in front of run 1 is looked up in it)
    t = table.copy()
    t[0]["win_first"] = -1
    rc, x, _, status = host_call(src, t, run_param, 0, total, rf, perm)
    n0 = int(table[0]["n_windows"])
    assert rc == 0 and status[0] == 1 and (x[:n0] == wc.FILL).all() and same_bits(x[n0:], good[0][n0:])


def test_garbage_tables_stay_inside_the_buffers():
    """Unsorted, overlapping and random tables: whatever the bisection ends on is validated; the guard bands stay clean and every
    row is either untouched or a window of some valid run."""
    J, F, rf = 14, 2, 9
    src, table, run_param, total = wc.eval_layout(J, F, rf, lengths=(4, 1, 6, 3, 9))
    perm = wc.mirror_perm(J)
    rng = np.random.RandomState(3)
    for trial in range(6):
        t = table.copy()
        if trial < 3:
            t = t[rng.permutation(len(t))]
            if trial == 2:
                t["win_first"] = 0                                  # all runs overlap
        else:
            raw = rng.randint(0, 256, size=t.nbytes).astype(np.uint8)
            t = raw.view(t.dtype).copy()
            t["first_frame"] %= 40
            t["n_frames"] %= 40
        rc, x, param, status = host_call(src, t, run_param, 0, total, rf, perm)
        assert rc == 0 and set(np.unique(status).tolist()) <= {wc.FILL_STATUS, 0, 1}


# ------------------------------------------------------------------------------------ the argument rules

def test_argument_rules():
    hooks = hooks_library()
    J, F, rf = 17, 3, 9
    src, table, run_param, total = wc.eval_layout(J, F, rf, lengths=(4, 6))
    x = np.full((total, rf, J, F), wc.FILL, np.float32)
    param = np.full((total, 2), wc.FILL, np.float32)
    status = np.full(len(table), wc.FILL_STATUS, np.int32)
    perm = wc.mirror_perm(J)
    base = dict(src=src.ctypes.data, total=src.shape[0], J=J, F=F, rf=rf, runs=table.ctypes.data, n=len(table), rp=run_param.ctypes.data,
                E=2, w0=0, batch=total, x=x.ctypes.data, param=param.ctypes.data, perm=perm, status=status.ctypes.data)

    def call(**kw):
        a = dict(base, **kw)
        return _capi.debug_clips_windows_host(a["src"], a["total"], a["J"], a["F"], a["rf"], a["runs"], a["n"], a["rp"], a["E"], a["w0"],
                                              a["batch"], a["x"], a["param"], a["perm"], a["status"])

    twice = [0] * J
    big = _capi.ENCODE_MAX_POINTS
    bad = [dict(src=0), dict(runs=0), dict(x=0), dict(status=0), dict(n=0), dict(n=_capi.CLIPS_MAX + 1), dict(J=0, perm=None), dict(J=18, perm=None),
           dict(F=1), dict(F=4), dict(rf=0), dict(total=0), dict(batch=0), dict(batch=65536), dict(w0=-1), dict(w0=2 ** 62 + 1),
           dict(rf=big // J + 1), dict(total=big + 1), dict(rf=2 ** 20, batch=200), dict(rp=0), dict(param=0), dict(E=0), dict(E=-1),
           dict(perm=twice), dict(perm=[J] + perm[1:]), dict(runs=table.ctypes.data + 4)]
    for kw in bad:
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
        assert hooks.r3d_last_error()
    assert (x == wc.FILL).all() and (param == wc.FILL).all() and (status == wc.FILL_STATUS).all()      # nothing was written
    assert call() == 0 and call(rp=0, param=0, E=0) == 0 and call(perm=None) == 0
    with pytest.raises(_capi.Ray3DHipError):
        call(perm=perm[:-1])


def test_device_entry_point_refuses_before_any_device_call():
    """The same rules through r3d_clips_windows itself, on pointers that are never followed: R3D_ERR_ARG without a GPU."""
    lib = _capi.load()
    perm = (C.c_int32 * 17)(*range(17))

    def call(src=BOGUS, total=100, J=17, F=3, rf=27, runs=BOGUS, n=4, rp=BOGUS, E=2, w0=0, batch=64, x=BOGUS, param=BOGUS, status=BOGUS):
        return lib.r3d_clips_windows(src, total, J, F, rf, runs, n, rp, E, w0, batch, x, param, perm, status, None)

    for kw in (dict(src=None), dict(runs=None), dict(x=None), dict(status=None), dict(n=0), dict(n=65536), dict(J=18), dict(F=4), dict(rf=0),
               dict(total=0), dict(batch=0), dict(batch=65536), dict(w0=-1), dict(rp=None), dict(param=None), dict(E=0), dict(runs=BOGUS + 4),
               dict(rf=2 ** 20, batch=200)):
        assert call(**kw) == _capi.R3D_ERR_ARG, kw
    with pytest.raises(_capi.Ray3DHipError, match="mirror_perm"):
        _capi.clips_windows(BOGUS, 100, 17, 3, 27, BOGUS, 4, BOGUS, 2, 0, 64, BOGUS, BOGUS, [0] * 17, BOGUS, 0)
