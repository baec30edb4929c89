"""Where a forward's buffers cross 2^31 bytes, 2^32 bytes and 2^31 floats - read from the library (r3d_debug_plan_buffers, hooks build,
no GPU), not typed by hand: tests/test_large_calls_host.py and tests/test_gpu_large_calls.py choose their batch sizes here, so a
change of the plan moves them with it.

A workspace buffer of a call of B windows holds B * floats_per_window floats at byte offset B * offset_per_window * 4; the
per-frame buffer of a clip call (window stride one frame) holds (B + RF - 1) * floats_per_frame floats.  The CROSSING BATCH of a
buffer and a limit is the smallest B at which the buffer's extent reaches the limit.  The raw input has the same kind of edge
against the library's own guard (include/ray3d_hip.h, "Size limits of one forward"); those expectations are computed here from
the documented rule with Python integers, never by asking the library."""
import numpy as np

LIMITS = (("2^31 bytes", 2 ** 31), ("2^32 bytes", 2 ** 32), ("2^31 floats", 2 ** 33))      # (name, bytes)
GUARD = 2 ** 31 - 1            # the documented rules refuse a quantity that reaches this
PER_FRAME_GUARD = 2 ** 32 - 1  # ... and the per-frame first layers give up where their buffer reaches this many bytes
CHUNK = 4096                   # windows per call of the chunked comparison (Ray3DLifter.CLIP_CHUNK)


def model_config(arch="3,3", **over):
    import ray3d_amd
    return {str(k): v for k, v in ray3d_amd.default_model_config(ARCHITECTURE=arch, **over).items()}


class HostPair:
    """A pos + trj pair of handles of the hooks library, created from the configuration alone (nothing is uploaded)."""

    def __init__(self, mc):
        from conftest import hooks_library
        from ray3d_amd import _capi
        from ray3d_amd.spec import config_from_dicts
        hooks_library()
        self.cp, self.ct = config_from_dicts(mc, "pos"), config_from_dicts(mc, "trj")
        self.hp, self.ht = _capi.Handle(self.cp), _capi.Handle(self.ct)
        self.rf, self.joints = self.cp.receptive_field, self.cp.num_joints

    def buffers(self, batch):
        """(rows, workspace_bytes) of r3d_debug_plan_buffers: rows (name, floats_per_window, offset_bytes, bytes, per_frame)."""
        from ray3d_amd import _capi
        return _capi.debug_plan_buffers(self.hp, self.ht, batch)

    def workspace_bytes(self, batch):
        from ray3d_amd import _capi
        return _capi.workspace_bytes(self.hp, self.ht, batch)

    def call_check(self, batch, window_stride, mode=0, cam_stride=0):
        from ray3d_amd import _capi
        return _capi.debug_call_check(self.hp, self.ht, batch, window_stride, mode, cam_stride)

    def close(self):
        self.hp.close()
        self.ht.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def extent_bytes(row, batch, rf, clip):
    """Bytes of one buffer a call of `batch` windows touches (a clip call's per-frame buffer: a row per input frame)."""
    _, fpw, _, _, per_frame = row
    return ((batch + rf - 1) if (per_frame and clip) else batch) * fpw * 4


def _ceil_div(a, b):
    return -(-a // b)


def crossing_batches(pair, clip=False, probe_batch=1 << 20):
    """{(buffer index, buffer name, limit name): crossing batch} of the plan large calls run.  The floats per window are read at
    `probe_batch` (every call of >= 1024 windows runs the same plan: r3d_debug_plan_kind_edges); each crossing is then checked
    against the hook AT the crossing: the buffer reaches the limit there and not one window earlier."""
    rows, _ = pair.buffers(probe_batch)
    out = {}
    for i, row in enumerate(rows):
        name, fpw, _, _, per_frame = row
        if name.startswith("(") or fpw == 0 or (per_frame and not clip):
            continue
        for lname, lim in LIMITS:
            b = _ceil_div(lim, fpw * 4) - ((pair.rf - 1) if per_frame else 0)
            for bb, reached in ((b, True), (b - 1, False)):
                r2 = pair.buffers(bb)[0][i]
                assert r2[0] == name and r2[1] == fpw, (name, bb, r2)
                assert (extent_bytes(r2, bb, pair.rf, clip) >= lim) == reached, (name, lname, bb)
            out[(i, name, lname)] = b
    return out


def first_crossing(pair, limit_name, clip=False, per_frame_only=False):
    """(batch, buffer index, buffer name): the first buffer to reach `limit_name` as the batch grows, and where."""
    best = None
    rows = pair.buffers(1 << 20)[0]
    for (i, name, lname), b in crossing_batches(pair, clip).items():
        if lname != limit_name or (per_frame_only and not rows[i][4]):
            continue
        if best is None or b < best[0]:
            best = (b, i, name)
    assert best is not None, limit_name
    return best


def crossed(pair, batch, clip=False):
    """[(buffer index, name, limit name, limit bytes, floats per window, per_frame)] of every limit some buffer has reached at `batch`."""
    rows, _ = pair.buffers(batch)
    out = []
    for i, row in enumerate(rows):
        if row[0].startswith("(") or row[1] == 0 or (row[4] and not clip):
            continue
        for lname, lim in LIMITS:
            if extent_bytes(row, batch, pair.rf, clip) >= lim:
                out.append((i, row[0], lname, lim, row[1], row[4]))
    return out


# ---- the documented size rules, in exact integers (include/ray3d_hip.h, "Size limits of one forward")

def frames_of(batch, window_stride, rf):
    return (batch - 1) * window_stride + rf


def rule_accepts(batch, window_stride, rf, joints, materialised=False):
    ok = frames_of(batch, window_stride, rf) * joints * 3 * 4 < GUARD and batch * (rf // 3) < GUARD
    if materialised:
        ok = ok and batch * rf * joints * 3 * 4 < GUARD
    return ok


def last_accepted_batch(window_stride, rf, joints, materialised=False):
    """The largest B the documented rules accept (they are monotonic in B): bisection over exact integers."""
    lo, hi = 1, 2 ** 40
    assert rule_accepts(lo, window_stride, rf, joints, materialised) and not rule_accepts(hi, window_stride, rf, joints, materialised)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rule_accepts(mid, window_stride, rf, joints, materialised):
            lo = mid
        else:
            hi = mid
    return lo


def first_gathered_frames(floats_per_frame):
    """The first frame count of a clip call whose per-frame buffer reaches the documented 2^32 - 1 bytes."""
    return _ceil_div(PER_FRAME_GUARD, floats_per_frame * 4)


# ---- inputs any window of which can be re-created on the host: a hash of the element's global index

_MUL = np.int64(-7046029254386353131)      # 0x9E3779B97F4A7C15 as a two's-complement int64 (products wrap alike on host and device)
_OFFSETS = (0.0, 0.18, 0.98)               # rays: (x/z, c*y + s, -s*y + c) around a camera pitched by ~0.18 rad


def _unit(h, xp):
    """int64 indices -> float32 in [-0.5, 0.5): 24 hashed bits, every step exact in float32 on both sides."""
    h = h * _MUL if xp is np else h * int(_MUL)
    h = h ^ (h >> 29)
    h = h * _MUL if xp is np else h * int(_MUL)
    h = h ^ (h >> 32)
    return h & 0xFFFFFF


def hashed_rows_host(first, count, width, kind):
    """Rows [first, first + count) of `width` floats of the hashed input, float32 numpy: `kind` "rays" (width = J * 3), "pixels"
    (J * 2, in [200, 1800)) or "param" (2: height, pitch)."""
    idx = (np.arange(first, first + count, dtype=np.int64)[:, None] * np.int64(width) + np.arange(width, dtype=np.int64)[None, :])
    with np.errstate(over="ignore"):
        u = (_unit(idx, np).astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5))
    return _shape_values(u, idx % (3 if kind == "rays" else 2), kind, np)


def hashed_rows_device(first, count, width, kind, device):
    import torch
    idx = (torch.arange(first, first + count, dtype=torch.int64, device=device)[:, None] * width +
           torch.arange(width, dtype=torch.int64, device=device)[None, :])
    u = _unit(idx, torch).to(torch.float32) * (2.0 ** -24) - 0.5
    return _shape_values(u, idx % (3 if kind == "rays" else 2), kind, torch)


def _shape_values(u, comp, kind, xp):
    f32 = np.float32
    if kind == "rays":
        off = xp.where(comp == 0, f32(_OFFSETS[0]), xp.where(comp == 1, f32(_OFFSETS[1]), f32(_OFFSETS[2]))) if xp is np else \
            xp.where(comp == 0, _OFFSETS[0], xp.where(comp == 1, _OFFSETS[1], _OFFSETS[2])).to(u.dtype)
        scale = xp.where(comp == 2, f32(0.1), f32(0.8)) if xp is np else xp.where(comp == 2, 0.1, 0.8).to(u.dtype)
        return (u * scale + off).astype(f32) if xp is np else u * scale + off
    if kind == "pixels":
        return (u * f32(1600.0) + f32(1000.0)).astype(f32) if xp is np else u * 1600.0 + 1000.0
    assert kind == "param"
    off = xp.where(comp == 0, f32(1.6), f32(0.15)) if xp is np else xp.where(comp == 0, 1.6, 0.15).to(u.dtype)
    scale = xp.where(comp == 0, f32(0.8), f32(0.5)) if xp is np else xp.where(comp == 0, 0.8, 0.5).to(u.dtype)
    return (u * scale + off).astype(f32) if xp is np else u * scale + off


def fill_hashed(out2d, kind, rows_per_step=1 << 16):
    """Fill a (rows, width) float32 device tensor with the hashed input, a slab at a time (the int64 indices of a whole 2 GiB input
    would be another 4 GiB)."""
    rows, width = out2d.shape
    for r0 in range(0, rows, rows_per_step):
        n = min(rows_per_step, rows - r0)
        out2d[r0:r0 + n] = hashed_rows_device(r0, n, width, kind, out2d.device)


# ---- which windows of a large call the oracle sees

def sample_windows(batch, crossings, spread=32, cap=128):
    """Window indices for the oracle: the first and the last window; around every crossing - the window that holds the limit's byte,
    its neighbours, and the windows one 32-row tile below and above (a buffer of `fpw` floats per window is cut into tiles of 32
    rows; with r rows per window a tile spans ceil(32 / r) windows - 32 at most); then `spread` windows evenly.  At most `cap`."""
    picks = [0, batch - 1]
    for _, _, _, lim, fpw, per_frame in crossings:
        w = lim // (fpw * 4)                                   # the window (the frame) whose row holds byte `lim` of the buffer
        for d in (0, -1, 1, -32, 32, -33, 33):
            picks.append(w + d)
    picks += [int(v) for v in np.linspace(0, batch - 1, spread).round()]
    seen, out = set(), []
    for w in picks:
        if 0 <= w < batch and w not in seen:
            seen.add(w)
            out.append(w)
    return sorted(out[:cap])
