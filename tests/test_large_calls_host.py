"""Calls whose buffers cross 2^31 and 2^32 bytes, on the host (hooks library, no GPU): the workspace table the crossing helper reads
(r3d_debug_plan_buffers) against r3d_workspace_bytes, the edges of the size rules (r3d_debug_call_check: the functions the forward
driver asks) against the documented rule evaluated with Python integers, and the tile lists at one batch above each crossing."""
import ctypes
import time

import pytest

import large_call_cases as lc

SHIPPED = {"rf9": "3,3", "rf27": "3,3,3", "rf243": "3,3,3,3,3"}


@pytest.mark.parametrize("name", list(SHIPPED))
def test_buffer_table_is_the_documented_workspace(name):
    """Below 2^31 bytes, between 2^31 and 2^32 and above 2^32 (of the widest buffer): the rows' sizes add up to r3d_workspace_bytes,
    every row starts where the previous one ends (no overlap, no gap), buffers start on 64-byte multiples - on 256-byte ones when
    the batch is a multiple of four, since a buffer's offset is B * 16 k floats - and the control region on a 256-byte multiple."""
    with lc.HostPair(lc.model_config(SHIPPED[name])) as pr:
        b31, b32 = lc.first_crossing(pr, "2^31 bytes")[0], lc.first_crossing(pr, "2^32 bytes")[0]
        assert 1024 < b31 < b32
        for batch in (b31 // 2 + 1, (b31 + b32) // 2 + 1, b32 + 3):
            for B in (batch, (batch + 3) // 4 * 4):
                rows, total = pr.buffers(B)
                widest = max(r[3] for r in rows if not r[4])      # (the per-frame buffer: a clip call's, test_gpu_large_calls case e)
                assert (widest < 2 ** 31) == (B < b31) and (widest >= 2 ** 32) == (B >= b32), (B, widest)
                assert sum(r[3] for r in rows) == total == pr.workspace_bytes(B), (B, total)
                at = 0
                for rname, fpw, off, nbytes, per_frame in rows:
                    assert off == at, (B, rname, off, at)
                    assert off % (256 if B % 4 == 0 or rname == "(control)" else 64) == 0, (B, rname, off)
                    if not rname.startswith("("):
                        assert nbytes == B * fpw * 4 and fpw % 16 == 0, (B, rname)
                    at += nbytes
                assert [r[0] for r in rows[-2:]] == ["(tail)", "(control)"] and sum(1 for r in rows if r[4]) == 1 and rows[-3][4]
                # the per-frame buffer's rows beyond B lie in the tail
                assert (pr.rf - 1) * rows[-3][1] * 4 <= rows[-2][3]


def test_crossing_helper_names_the_widest_buffer_first():
    with lc.HostPair(lc.model_config("3,3")) as pr:
        rows = pr.buffers(1 << 20)[0]
        widest = max(r[1] for r in rows if not r[0].startswith("(") and not r[4])
        for lname, lim in lc.LIMITS:
            b, i, name = lc.first_crossing(pr, lname)
            assert rows[i][1] == widest and b == -(-lim // (widest * 4)), (lname, b, name)
            assert lc.crossed(pr, b - 1) == [c for c in lc.crossed(pr, b) if not (c[0] == i and c[2] == lname)]


# ---- guard edges: the expected edge from the documented rule in exact integers, the verdict from the driver's own functions

RAYS, UV, UV_DIST = 0, 1, 2
EDGES = {
    # name: (architecture, mode, window_stride (None: RF), cam_stride, materialised, which rule refuses first)
    "rays-windows-rf9": ("3,3", RAYS, None, 0, False, "raw"),
    "rays-windows-rf243": ("3,3,3,3,3", RAYS, None, 0, False, "raw"),
    "uv-stride-1-camera-per-window": ("3,3", UV, 1, 8, False, "raw"),
    "uv-stride-3-rf27": ("3,3,3", UV, 3, 0, False, "raw"),
    "distorted-materialised": ("3,3,3", UV_DIST, 1, 16, True, "materialised"),
    "rows-rf729-clip": ("3,3,3,3,3,3", RAYS, 1, 0, False, "rows"),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_last_accepted_and_first_refused_batch(name):
    arch, mode, stride, cam_stride, materialised, rule = EDGES[name]
    with lc.HostPair(lc.model_config(arch)) as pr:
        rf, J = pr.rf, pr.joints
        ws = rf if stride is None else stride
        last = lc.last_accepted_batch(ws, rf, J, materialised)
        # which of the documented rules it is that gives way at last + 1 (the case is named after it)
        raw = lc.frames_of(last + 1, ws, rf) * J * 12 >= lc.GUARD
        rows = (last + 1) * (rf // 3) >= lc.GUARD
        mat = materialised and (last + 1) * rf * J * 12 >= lc.GUARD
        assert {"raw": raw and not rows, "rows": rows and not raw, "materialised": mat and not raw and not rows}[rule], (raw, rows, mat)
        rc, msg, _ = pr.call_check(last, ws, mode, cam_stride)
        assert (rc, msg) == (0, ""), (name, last, rc, msg)
        rc, msg, _ = pr.call_check(last + 1, ws, mode, cam_stride)
        assert rc == -1 and "B too large for one call" in msg and ("materialised" in msg) == (rule == "materialised"), (name, last + 1, rc, msg)
        # far beyond the edge nothing wraps back into "accepted"
        for B in (2 * last, 2 ** 31, 2 ** 32 + 5, 2 ** 40):
            assert pr.call_check(B, ws, mode, cam_stride)[0] == -1, (name, B)


def test_bad_shapes_are_refused_before_the_size_rules():
    with lc.HostPair(lc.model_config("3,3")) as pr:
        assert pr.call_check(0, 9)[0] == -1 and pr.call_check(-5, 9)[0] == -1
        assert pr.call_check(16, 0)[:2] == (-1, "window_stride must be positive")
        assert pr.call_check(16, 9, mode=7)[0] == -1


def test_per_frame_first_layers_give_up_where_their_buffer_reaches_4_gib():
    """call_shares_first_layers: a clip call of the RF-27 pair keeps the per-frame path up to the last frame count whose buffer stays
    below 2^32 - 1 bytes (include/ray3d_hip.h) and takes the gathered one from the next; RF 9 never takes it (3 rows per window: the
    per-frame launch would not have "four times fewer rows")."""
    with lc.HostPair(lc.model_config("3,3,3")) as pr:
        ld = [r[1] for r in pr.buffers(1 << 20)[0] if r[4]]
        assert len(ld) == 1
        frames = lc.first_gathered_frames(ld[0])
        assert (frames - 1) * ld[0] * 4 < lc.PER_FRAME_GUARD <= frames * ld[0] * 4
        first = frames - (pr.rf - 1)                               # window_stride 1: frames = B + RF - 1
        assert pr.call_check(first - 1, 1) == (0, "", True)
        assert pr.call_check(first, 1) == (0, "", False)
        assert pr.call_check(first + 100000, 1) == (0, "", False)
        assert pr.call_check(4096, 1) == (0, "", True) and pr.call_check(4096, pr.rf) == (0, "", False)
        assert pr.call_check(4096, 1, UV, 8) == (0, "", False)      # a camera row per window: frames have no single camera
    with lc.HostPair(lc.model_config("3,3")) as pr:
        assert pr.call_check(4096, 1) == (0, "", False) and pr.call_check(400000, 1) == (0, "", False)


# ---- the tile lists at one batch above each crossing (RF-9 pair)

@pytest.mark.parametrize("limit_name", [l for l, _ in lc.LIMITS])
def test_tile_lists_are_sound_above_each_crossing(limit_name):
    """r3d_debug_plan_check (launch by launch: every cell once, producers first) and r3d_debug_forward_check (the single-launch
    lists executed as a dependency machine) at 37 windows above the first buffer to reach the limit: 419 468, 838 898 and
    1 677 759 windows.  On one core the two take 1.6 s, 3.1 s and 6.9 s."""
    with lc.HostPair(lc.model_config("3,3")) as pr:
        from ray3d_amd import _capi
        lib = _capi.load()
        sig = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        n0, n1 = ctypes.c_int(), ctypes.c_int()
        B = lc.first_crossing(pr, limit_name)[0] + 37
        assert any(c[2] == limit_name for c in lc.crossed(pr, B))
        t0 = time.time()
        for fn, ok in ((lib.r3d_debug_plan_check, (0,)), (lib.r3d_debug_forward_check, (0,))):
            fn.argtypes, fn.restype = sig, ctypes.c_int
            rc = fn(pr.hp.ptr, pr.ht.ptr, B, 256, ctypes.byref(n0), ctypes.byref(n1))
            assert rc in ok, (fn.__name__, B, rc)
        # the dependency machine really ran: at least one ready counter per 32-row unit of the widest problem
        assert n1.value >= B // 32, (B, n0.value, n1.value)
        print("\n%s: %d windows, %d tiles, %d counters, %.1f s" % (limit_name, B, n0.value, n1.value, time.time() - t0))
