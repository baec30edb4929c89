"""CPU suite: the host side of r3d_clips_valid_losses (a shard's validation losses in one call over the device-side clip table) -
the exports, the scratch formula, the argument checks (all made before any device call: they run without a GPU), the host hook
r3d_debug_clips_valid_losses_host (the call's validation and descriptor rule on the CPU, per valid clip exactly
r3d_debug_valid_losses_host) on shuffled clips with gaps and on invalid descriptors, forward_clip(trj_out=) on a stand-in, and
validate_clips_batched's refusal of CPU tensors.  tests/test_gpu_clips_valid.py runs the kernels on the clips built here."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, hooks_library
import valid_oracle as vo

from ray3d_amd import _capi, evaluate

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed
FILL = -7.0              # what the output buffers hold before a call
# one frame, two, the sizes around a wavefront and around a workgroup, more than two workgroups
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
GAP = 37                 # frames between stored clips that belong to no clip (NaN: nothing may read them)
VARIANTS = ("trj", "sum", "abs", "rel")       # trj; trj + POS_IS_SUM; no trj; no trj + GT_ROOT_RELATIVE
DOUBLES, COUNT = vo.DOUBLES, vo.COUNT


def _define(name):
    return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, HDR).group(1))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def same(a, b):
    """Bit for bit: NaN matches NaN, everything else by its uint64 view."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


@functools.lru_cache(maxsize=None)
def clip_inputs(n, J, variant):
    """(pos, trj or None, gt, flags) of one clip (tests/valid_oracle.py's seeded poses).  The 65-frame clip has a frame whose
    ground-truth root is exactly 0 deep (1 / z: Inf), the 257-frame clip a frame whose joint 2 lies on its parent in the
    prediction (a zero-length bone: 0 / 0 in the direction term) - the reference's Inf / NaN, which both calls must reproduce."""
    pos, trj, gt, flags = vo.variant_inputs(n, J, variant)
    pos, gt = np.array(pos), np.array(gt)
    if n == 65:
        gt[3, 0, 2] = 0.0
    if n == 257 and J > 2:
        pos[200, 2] = pos[200, vo.tree_for(J)[2]]
    for v in (pos, gt):
        v.setflags(write=False)
    return pos, trj, gt, flags


@functools.lru_cache(maxsize=None)
def layout(J, variant, lengths=LENGTHS):
    """The clips stored in a shuffled order, a gap of NaN frames behind each; the table names them in the order of `lengths`,
    its transforms are garbage (they are not read).  -> (table, pos_all, trj_all or None, gt_all, total, flags)."""
    store = np.random.default_rng(3 + J).permutation(len(lengths))
    first, at = {}, GAP
    for c in store:
        first[int(c)] = at
        at += lengths[c] + GAP
    total = at
    pos_all = np.full((total, J, 3), np.nan, np.float32)
    gt_all = np.full((total, J, 3), np.nan, np.float32)
    trj_all = np.full((total, 3), np.nan, np.float32) if variant in ("trj", "sum") else None
    table = np.zeros(len(lengths), dtype=_capi.clip_desc_dtype())
    flags = 0
    for c, n in enumerate(lengths):
        pos, trj, gt, flags = clip_inputs(n, J, variant)
        pos_all[first[c]:first[c] + n], gt_all[first[c]:first[c] + n] = pos, gt
        if trj_all is not None:
            trj_all[first[c]:first[c] + n] = trj
        table[c]["first_frame"], table[c]["n_frames"] = first[c], n
        table[c]["rn2w"], table[c]["tn2w"] = np.nan, np.inf
    if len(lengths) > 2:
        assert sorted(first.values()) != [first[c] for c in range(len(lengths))]          # really shuffled
    for v in (pos_all, gt_all, table) + ((trj_all,) if trj_all is not None else ()):
        v.setflags(write=False)
    return table, pos_all, trj_all, gt_all, total, flags


def invalid_descriptors(total, max_frames):
    """(first_frame, n_frames) of the four kinds - n_frames < 1, n_frames > max_frames, a range that ends past total_frames, a
    range that starts before 0 - and of ranges far outside."""
    return [(5, 0), (10, -5), (0, max_frames + 1), (total - 99, 100), (total, 1), (-1, 50), (2 ** 63 - 1, 3), (-2 ** 62, 2)]


def with_invalid(table, total, max_frames, keep):
    """The valid clips `keep` of `table` with an invalid descriptor in front of, between and behind them.
    -> (mixed table, [index into `table` or None for every row])."""
    bad = invalid_descriptors(total, max_frames)
    rows, src = [], []
    for k, c in enumerate(keep):
        rows += [bad[2 * k], None, bad[2 * k + 1]] if 2 * k + 1 < len(bad) else [None]
        src += [None, c, None] if 2 * k + 1 < len(bad) else [c]
    assert sum(r is not None for r in rows) == len(bad)
    mixed = np.zeros(len(rows), dtype=table.dtype)
    for i, (r, c) in enumerate(zip(rows, src)):
        if c is not None:
            mixed[i] = table[c]
        else:
            mixed[i]["first_frame"], mixed[i]["n_frames"] = r
    return mixed, src


def run_hook(J, table, pos_all, trj_all, gt_all, parents, flags, max_frames, row_stride=DOUBLES, frames=True, total=None):
    """r3d_debug_clips_valid_losses_host on host arrays pre-filled with FILL -> (rc, rows (k, row_stride), frame table or None)."""
    lib = hooks_library()
    total = pos_all.shape[0] if total is None else total
    table = np.ascontiguousarray(table)
    rows = np.full((table.shape[0], row_stride), FILL)
    fr = np.full((total, COUNT), FILL) if frames else None
    par = (C.c_int32 * len(parents))(*parents) if parents is not None else None
    pos_all, gt_all = np.ascontiguousarray(pos_all), np.ascontiguousarray(gt_all)
    trj_all = np.ascontiguousarray(trj_all) if trj_all is not None else None
    first = rows[:, row_stride - DOUBLES:]
    rc = lib.r3d_debug_clips_valid_losses_host(ptr(pos_all), ptr(trj_all), ptr(gt_all), total, J, par, flags, ptr(table), table.shape[0],
                                               max_frames, C.c_void_p(first.ctypes.data), row_stride, ptr(fr))
    return rc, rows, fr


# ------------------------------------------------------------------ exports, scratch, argument rules

def test_entry_points_are_declared_and_bound():
    product, hooks = _capi.load(), hooks_library()
    assert product._name == _capi.LIB_PATH and hooks._name == _capi.HOOKS_LIB_PATH
    for name in ("r3d_clips_valid_losses", "r3d_clips_valid_scratch_bytes"):
        assert name in _capi.EXPORTS and name not in _capi.HOOK_EXPORTS
        assert hasattr(product, name) and hasattr(hooks, name)
        assert re.search(r"\b%s\(" % name, HDR)
    hook = "r3d_debug_clips_valid_losses_host"
    assert hook in _capi.HOOK_EXPORTS and hook not in _capi.EXPORTS
    assert hasattr(hooks, hook) and not hasattr(product, hook)
    block = re.search(r"#ifdef R3D_TEST_HOOKS(.*?)#endif /\* R3D_TEST_HOOKS \*/", HDR, flags=re.S).group(1)
    assert hook + "(" in block and "r3d_clips_valid_losses(" not in block
    assert _define("R3D_ABI_VERSION") == _capi.ABI_VERSION == 6 == product.r3d_abi_version() == hooks.r3d_abi_version()      # no existing struct changed
    assert _capi.clip_desc_dtype().itemsize == 112 == C.sizeof(_capi.ClipDesc)
    assert evaluate.VALID_COLS == 3 + DOUBLES == 3 + _capi.VALID_DOUBLES


@pytest.mark.parametrize("max_frames", [1, 256, 257, 32768, 32769, 10 ** 6])
def test_scratch_bytes_is_the_documented_formula(max_frames):
    blocks = min(-(-max_frames // _capi.METRIC_THREADS), _capi.METRIC_MAX_BLOCKS)
    assert blocks == {1: 1, 256: 1, 257: 2, 32768: 128, 32769: 128, 10 ** 6: 128}[max_frames]
    for k in (1, 7, _capi.CLIPS_MAX):
        assert _capi.clips_valid_scratch_bytes(k, max_frames) == k * blocks * DOUBLES * 8
    for lib in (_capi.load(), hooks_library()):
        assert lib.r3d_clips_valid_scratch_bytes(3, max_frames) == 3 * blocks * DOUBLES * 8


def test_scratch_bytes_is_zero_for_bad_arguments():
    for k, m in ((0, 100), (-1, 100), (3, 0), (3, -7), (0, 0)):
        assert _capi.clips_valid_scratch_bytes(k, m) == 0


def _call(**over):
    """r3d_clips_valid_losses with bogus non-null pointers and otherwise valid arguments; -> the return code."""
    a = dict(pos=BOGUS, trj=BOGUS, gt=BOGUS, total=1000, J=17, parents=vo.H36M, flags=vo.POS_IS_SUM, table=BOGUS, num_clips=3, max_frames=600,
             rows=BOGUS, row_stride=DOUBLES, frame=BOGUS, scratch=BOGUS, scratch_bytes=None, stream=0)
    a.update(over)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = max(_capi.clips_valid_scratch_bytes(a["num_clips"], a["max_frames"]), 8)
    par = (C.c_int32 * len(a["parents"]))(*a["parents"]) if a["parents"] is not None else None
    return _capi.load().r3d_clips_valid_losses(a["pos"], a["trj"], a["gt"], a["total"], a["J"], par, a["flags"], a["table"], a["num_clips"],
                                               a["max_frames"], a["rows"], a["row_stride"], a["frame"], a["scratch"], a["scratch_bytes"],
                                               a["stream"])


ARG_CASES = [
    (dict(pos=None), "null pointer"), (dict(gt=None), "null pointer"), (dict(rows=None), "null pointer"), (dict(table=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(J=0), "num_joints"), (dict(J=18), "num_joints"),
    (dict(parents=(0,) + vo.H36M[1:]), "parent table"), (dict(parents=vo.H36M[:5] + (5,) + vo.H36M[6:]), "parent table"),
    (dict(parents=vo.H36M[:9] + (-1,) + vo.H36M[10:]), "parent table"),
    (dict(flags=4), "unknown flags"), (dict(flags=-1), "unknown flags"),
    (dict(trj=None, flags=vo.POS_IS_SUM), "POS_IS_SUM"), (dict(flags=vo.GT_ROOT_RELATIVE), "GT_ROOT_RELATIVE"),
    (dict(num_clips=0), "num_clips"), (dict(num_clips=-3), "num_clips"), (dict(num_clips=65536), "num_clips"),
    (dict(max_frames=0), "max_frames"), (dict(max_frames=-5), "max_frames"), (dict(total=0), "total_frames"), (dict(total=-1), "total_frames"),
    (dict(table=BOGUS + 4), "8-byte aligned"), (dict(scratch=BOGUS + 4), "8-byte aligned"),
    (dict(row_stride=DOUBLES - 1), "row_stride"), (dict(row_stride=0), "row_stride"), (dict(row_stride=-DOUBLES), "row_stride"),
]


@pytest.mark.parametrize("over,word", ARG_CASES, ids=["%d:%s" % (i, next(iter(o))) for i, (o, _) in enumerate(ARG_CASES)])
def test_bad_arguments_return_err_arg_before_any_device_call(over, word):
    """Bogus pointers: the call must decide on the host.  (Without a GPU a launch would fail with R3D_ERR_HIP, with one it
    would fault: R3D_ERR_ARG shows that neither was tried.)"""
    assert _call(**over) == _capi.R3D_ERR_ARG == -1
    assert word in _capi.load().r3d_last_error().decode()


@pytest.mark.parametrize("max_frames", [1, 257, 40000])
def test_a_short_scratch_returns_err_workspace_before_any_launch(max_frames):
    need = _capi.clips_valid_scratch_bytes(3, max_frames)
    for short in (need - 1, need // 2, 0):
        assert _call(max_frames=max_frames, scratch_bytes=short) == _capi.R3D_ERR_WORKSPACE == -6
        assert "r3d_clips_valid_scratch_bytes" in _capi.load().r3d_last_error().decode()
    with pytest.raises(_capi.Ray3DHipError, match="scratch"):
        _capi.clips_valid_losses(BOGUS, BOGUS, BOGUS, 1000, 17, vo.H36M, 0, BOGUS, 3, max_frames, BOGUS, DOUBLES, None, BOGUS, need - 8, 0)


def test_the_hook_applies_the_same_argument_rules():
    table, pos_all, trj_all, gt_all, total, flags = layout(17, "trj", (2, 5))
    assert run_hook(17, table, pos_all, trj_all, gt_all, vo.H36M, flags, 5)[0] == 0
    assert run_hook(17, table, pos_all, trj_all, gt_all, vo.H36M, 4, 5)[0] == _capi.R3D_ERR_ARG
    assert run_hook(17, table, pos_all, trj_all, gt_all, vo.H36M, flags, 0)[0] == _capi.R3D_ERR_ARG
    assert run_hook(17, table, pos_all, None, gt_all, vo.H36M, vo.POS_IS_SUM, 5)[0] == _capi.R3D_ERR_ARG
    assert run_hook(17, table, pos_all, trj_all, gt_all, (0,) + vo.H36M[1:], flags, 5)[0] == _capi.R3D_ERR_ARG
    assert run_hook(17, table, pos_all, trj_all, gt_all, vo.H36M, flags, 5, total=0)[0] == _capi.R3D_ERR_ARG
    assert "total_frames" in hooks_library().r3d_last_error().decode()


# ------------------------------------------------------------------ the hook against the per-clip hook

@pytest.mark.parametrize("bones", [True, False], ids=["parents", "noparents"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("J", [1, 14, 17])
def test_hook_equals_the_per_clip_hook_on_shuffled_clips_with_gaps(J, variant, bones):
    """Rows and frame rows bit for bit those of r3d_debug_valid_losses_host on every clip alone; frame rows no clip covers and
    the columns between the strided rows keep their fill."""
    table, pos_all, trj_all, gt_all, total, flags = layout(J, variant)
    parents = vo.tree_for(J) if bones else None
    stride = DOUBLES + 3
    rc, rows, fr = run_hook(J, table, pos_all, trj_all, gt_all, parents, flags, max(LENGTHS), row_stride=stride)
    assert rc == 0
    assert (rows[:, :3] == FILL).all()
    covered = np.zeros(total, bool)
    for c, n in enumerate(LENGTHS):
        pos, trj, gt, _ = clip_inputs(n, J, variant)
        rc1, want, want_fr = vo.host_call(hooks_library(), pos, trj, gt, parents, flags)
        at = int(table[c]["first_frame"])
        assert rc1 == 0 and same(rows[c, 3:], want) and same(fr[at:at + n], want_fr), (J, variant, n)
        covered[at:at + n] = True
    assert (~covered).sum() == GAP * (len(LENGTHS) + 1) and (fr[~covered] == FILL).all()
    if variant == "trj":
        n65 = LENGTHS.index(65)
        assert np.isinf(rows[n65, 3 + 3])                              # TRJ_WSUM of the clip with the zero root depth
    if bones and J > 2:
        assert np.isnan(rows[LENGTHS.index(257), 3 + 6]) and np.isfinite(rows[LENGTHS.index(256), 3:]).all()
    if bones and J == 1:
        assert np.isnan(rows[:, 3 + 5]).all()                          # the empty bone mean of a one-joint tree
    rc, rows2, none = run_hook(J, table, pos_all, trj_all, gt_all, parents, flags, max(LENGTHS), frames=False)
    assert rc == 0 and none is None and same(rows2, rows[:, 3:])
    rc, rows3, fr3 = run_hook(J, table, pos_all, trj_all, gt_all, parents, flags, 10 ** 6)       # a looser bound moves nothing
    assert rc == 0 and same(rows3, rows[:, 3:]) and same(fr3, fr)


def test_hook_invalid_descriptors_give_nan_rows_and_touch_nothing():
    table, pos_all, trj_all, gt_all, total, flags = layout(17, "sum")
    keep = [LENGTHS.index(n) for n in (1, 65, 257, 513)]
    mixed, src = with_invalid(table, total, 513, keep)
    assert len(mixed) == 12 and sum(c is None for c in src) == 8
    stride = DOUBLES + 2
    rc, rows, fr = run_hook(17, mixed, pos_all, trj_all, gt_all, vo.H36M, flags, 513, row_stride=stride)
    _, ref, ref_fr = run_hook(17, table, pos_all, trj_all, gt_all, vo.H36M, flags, 513)
    assert rc == 0 and (rows[:, :2] == FILL).all()
    touched = np.zeros(total, bool)
    for i, c in enumerate(src):
        if c is None:
            assert np.isnan(rows[i, 2:]).all(), (i, mixed[i])
        else:
            at, n = int(table[c]["first_frame"]), LENGTHS[c]
            assert same(rows[i, 2:], ref[c]) and same(fr[at:at + n], ref_fr[at:at + n])
            touched[at:at + n] = True
    assert (fr[~touched] == FILL).all()
    # the bounds are the stated extents exactly: a clip that ends on the last frame is followed, one frame less of buffer and it is not
    c = int(np.argmax(table["first_frame"]))
    last, n = np.array(table[c:c + 1]), LENGTHS[c]
    end = int(table[c]["first_frame"]) + n
    rc, r1, _ = run_hook(17, last, pos_all, trj_all, gt_all, vo.H36M, flags, n, total=end)
    assert rc == 0 and same(r1[0], ref[c])
    assert np.isnan(run_hook(17, last, pos_all, trj_all, gt_all, vo.H36M, flags, n, total=end - 1)[1]).all()
    assert np.isnan(run_hook(17, last, pos_all, trj_all, gt_all, vo.H36M, flags, n - 1, total=end)[1]).all()


# ------------------------------------------------------------------ forward_clip(trj_out=) and validate_clips_batched

class _Recorder:
    """Ray3DLifter.forward_clip on a stand-in: _run records its batch sizes; window i's pose is the frame in its middle, its
    trajectory that frame's joint 0."""

    def __init__(self):
        import ray3d_amd
        self.calls = []
        self.pos = types.SimpleNamespace(num_joints_in=17, in_features=3, camera_embedding=False)
        for name in ("clip_batch_sizes", "forward_clip", "_forward_clip_into"):
            setattr(self, name, types.MethodType(getattr(ray3d_amd.Ray3DLifter, name), self))
        self.CLIP_CHUNK, self.CLIP_ROUND, self.CLIP_BALANCED = 256, 128, True

    def receptive_field(self):
        return 9

    def join_lanes(self):
        pass

    def _lane_of_current_stream(self, dev):
        return None

    def _run(self, mode, x, stride, B, p, pstride, return_trj=False, out=None, out_trj=None):
        assert stride == 1 and x.shape[0] >= B + 8
        self.calls.append(B)
        if out is None:
            out = torch.empty((B, 1, 17, 3))
        out[:] = x[4:4 + B].reshape(B, 1, 17, 3)
        if not return_trj:
            assert out_trj is None
            return out
        if out_trj is None:
            out_trj = torch.empty((B, 1, 1, 3))
        out_trj[:] = x[4:4 + B, :1].reshape(B, 1, 1, 3)
        return out, out_trj


@pytest.mark.parametrize("n", [1, 33, 128, 300, 420])
def test_forward_clip_trj_out_runs_the_same_forwards_and_concatenates_nothing(n, monkeypatch):
    """1 (exact), 33 (one call of 64, all of it through the scratch tensors), 128 (exact), 300 (256, then 44 lifted as 64: the
    tail overhangs) and 420 (256 + 256: the tail overhangs) with CLIP_CHUNK 256."""
    lifter = _Recorder()
    sizes = lifter.clip_batch_sizes(n)
    rng = np.random.default_rng(n)
    padded = torch.from_numpy(rng.normal(size=(n + 8, 17, 3)).astype(np.float32))
    want, want_trj = lifter.forward_clip(padded, return_trj=True)
    assert lifter.calls == sizes and want_trj.shape == (n, 1, 1, 3)
    lifter.calls = []
    monkeypatch.setattr(torch, "cat", lambda *a, **k: pytest.fail("forward_clip(out=, trj_out=) must not concatenate"))
    surplus = sum(sizes) - n
    full = torch.empty((n + 8 + surplus, 17, 3))
    full[:n + 8], full[n + 8:] = padded, padded[-1]
    buf = torch.full((n + 6, 1, 17, 3), FILL)
    tbuf = torch.full((n + 6, 1, 1, 3), FILL)
    got, got_trj = lifter.forward_clip(full, return_trj=True, out=buf[2:2 + n], trj_out=tbuf[4:4 + n], n_windows=n)
    assert lifter.calls == sizes
    assert got.data_ptr() == buf[2:].data_ptr() and got_trj.data_ptr() == tbuf[4:].data_ptr()
    assert torch.equal(got, want) and torch.equal(got_trj, want_trj)
    assert (buf[:2] == FILL).all() and (buf[2 + n:] == FILL).all() and (tbuf[:4] == FILL).all() and (tbuf[4 + n:] == FILL).all()
    # without `out`: the poses in a new tensor, the trajectory still in place
    tbuf2 = torch.full((n, 1, 1, 3), FILL)
    got2, got_trj2 = lifter.forward_clip(full, return_trj=True, trj_out=tbuf2, n_windows=n)
    assert torch.equal(got2, want) and got_trj2 is tbuf2 and torch.equal(tbuf2, want_trj)
    with pytest.raises(ValueError, match="return_trj"):
        lifter.forward_clip(full, out=buf[2:2 + n], trj_out=tbuf[4:4 + n], n_windows=n)
    with pytest.raises(ValueError, match="trj_out"):
        lifter.forward_clip(full, return_trj=True, out=buf[2:2 + n], trj_out=tbuf[:n + 1], n_windows=n)
    with pytest.raises(ValueError, match="trj_out"):
        lifter.forward_clip(full, return_trj=True, trj_out=torch.empty((n, 1, 1, 3), dtype=torch.float64), n_windows=n)


def test_clip_frame_table():
    table, first, total, longest = evaluate.clip_frame_table([5, 1, 300])
    assert table.dtype == _capi.clip_desc_dtype() and table.view(np.uint8).shape == (3 * 112,)
    assert table["first_frame"].tolist() == first == [0, 5, 6] and table["n_frames"].tolist() == [5, 1, 300]
    assert (total, longest) == (306, 300)
    assert evaluate.clip_frame_table([])[1:] == ([], 0, 0)


def test_validate_clips_batched_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="validate_clips"):
        evaluate.validate_clips_batched(vo.standin_lift, vo.valid_clips(), vo.RF, "cpu")
    with pytest.raises(RuntimeError, match="validate_clips"):
        evaluate.validate_clips_batched(vo.standin_lift, [], vo.RF, torch.device("cpu"))
