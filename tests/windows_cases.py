"""What tests/test_clips_windows_host.py and tests/test_gpu_clips_windows.py share: a NumPy restatement of r3d_clips_windows (the
rule of include/ray3d_hip.h, written independently of r3d_windows.hpp), the layouts both run, the invalid descriptors."""
import numpy as np

from ray3d_amd import _capi, evaluate

LIM = _capi.ENCODE_MAX_POINTS
FILL = np.float32(-7.0)       # what x / param hold before a call: rows no valid run holds must keep it
FILL_STATUS = -1              # ... and the status words of runs without a window in the range
CLIP_FRAMES = (1, 2, 5, 13, 14, 40, 100)
KPS = {17: ([4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]), 14: ([4, 5, 6, 10, 11], [1, 2, 3, 12, 13])}


def mirror_perm(J):
    return evaluate.mirror_permutation(J, *KPS[J])


def run_valid(d, total_frames, has_perm):
    first, n, wf, nw, start, step, flip = (int(d[k]) for k in ("first_frame", "n_frames", "win_first", "n_windows", "start", "step", "flip"))
    if n < 1 or nw < 1 or step < 1 or flip not in (0, 1) or (flip and not has_perm):
        return False
    if first < 0 or first + n > total_frames or wf < 0 or nw > LIM or abs(start) > LIM:
        return False
    return start + (nw - 1) * step <= LIM          # (Python integers: no overflow to think about)


def ref_windows(src, table, run_param, window0, batch, rf, perm, x0=None, param0=None, status0=None):
    """The call on a table SORTED by win_first -> (x, param or None, status), from the buffers' previous contents (default: FILL)."""
    total, J, F = src.shape
    wf = table["win_first"].astype(np.int64)
    assert (np.diff(wf) >= 0).all()
    x = np.full((batch, rf, J, F), FILL, np.float32) if x0 is None else x0.copy()
    E = 0 if run_param is None else run_param.shape[1]
    param = None if run_param is None else (np.full((batch, E), FILL, np.float32) if param0 is None else param0.copy())
    status = np.full(len(table), FILL_STATUS, np.int32) if status0 is None else status0.copy()
    bits, xb = src.view(np.uint32), x.view(np.uint32)
    for w in range(batch):
        g = window0 + w
        at = np.nonzero(wf <= g)[0]
        r = int(at[-1]) if len(at) else 0
        d = table[r]
        if not run_valid(d, total, perm is not None):
            status[r] = 1
            continue
        k = g - int(d["win_first"])
        if not 0 <= k < int(d["n_windows"]):
            continue
        status[r] = 0
        t = np.clip(int(d["start"]) + k * int(d["step"]) + np.arange(rf), 0, int(d["n_frames"]) - 1) + int(d["first_frame"])
        rows = bits[t]
        if int(d["flip"]):
            rows = rows[:, perm, :].copy()
            rows[:, :, 0] ^= np.uint32(0x80000000)
        xb[w] = rows
        if param is not None:
            param[w] = run_param[r]
    return x, param, status


def noise(seed, shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def eval_layout(J, F, rf, causal=False, flip=False, surplus=0, lengths=CLIP_FRAMES, seed=5, E=2):
    """Evaluation clips of `lengths` frames back to back -> (src, table, run_param, total_windows)."""
    src = noise(seed + J + F, (sum(lengths), J, F))
    table, _, total = evaluate.clip_window_table(list(lengths), rf, causal, flip, surplus)
    run_param = noise(seed + 1, (len(lengths), E)) if E else None
    return src, table, run_param, total


def scattered_layout(J, F, rf):
    """Runs with step 1, 2 and 3, with and without flip, whose clips lie in the source OUT OF ORDER with gaps of NaNs that carry
    payloads (nothing may read them - and inside the clips a few NaN payloads that must arrive bit for bit) -> (src, table,
    run_param, total_windows)."""
    lengths, steps, flips, nwin = (7, 30, 1, 12, 19), (2, 3, 1, 1, 2), (0, 1, 0, 1, 0), (5, 11, 3, 12, 9)
    order, gap = (3, 0, 4, 1, 2), 3
    first, at = {}, gap
    for c in order:
        first[c] = at
        at += lengths[c] + gap
    src = np.full((at, J, F), np.nan, np.float32)
    src.view(np.uint32)[:] = 0x7FC00BAD
    for c, n in enumerate(lengths):
        src[first[c]:first[c] + n] = noise(40 + c, (n, J, F))
    sb = src.view(np.uint32)
    sb[first[1] + 3, 2, 0], sb[first[1] + 4, J - 1, 1], sb[first[3], 0, 0] = 0x7FC12345, 0xFFC00001, 0x7F800001
    table = np.zeros(len(lengths), dtype=_capi.window_run_dtype())
    at = 0
    for c, n in enumerate(lengths):
        table[c]["first_frame"], table[c]["n_frames"], table[c]["win_first"], table[c]["n_windows"] = first[c], n, at, nwin[c]
        table[c]["start"], table[c]["step"], table[c]["flip"] = -(rf // 2) - c, steps[c], flips[c]
        at += nwin[c]
    return src, table, noise(9, (len(lengths), 2)), at


def invalid_cases(d, total_frames):
    """One run of each invalid kind made from the valid run `d` (its window slots kept): name -> (descriptor, needs mirror_perm
    to be given for the kind to be the reason)."""
    def edit(**kw):
        e = np.array([d])[0].copy()
        for k, v in kw.items():
            e[k] = v
        return e
    n = int(d["n_frames"])
    return {"n_frames 0": edit(n_frames=0), "n_frames < 0": edit(n_frames=-3), "n_windows 0": edit(n_windows=0), "step 0": edit(step=0),
            "step < 0": edit(step=-1), "flip 2": edit(flip=2), "flip -1": edit(flip=-1), "first < 0": edit(first_frame=-1),
            "source past the end": edit(first_frame=total_frames - n + 1), "huge n_frames": edit(n_frames=2 ** 62),
            "huge first": edit(first_frame=2 ** 63 - 1), "start over the limit": edit(start=LIM + 1), "start under the limit": edit(start=-LIM - 1),
            "start INT64_MIN": edit(start=-2 ** 63), "last window over the limit": edit(n_windows=LIM, step=2, start=0),
            "huge n_windows": edit(n_windows=2 ** 62), "n_windows * step overflows": edit(n_windows=LIM, step=2 ** 31 - 1, start=LIM)}
