"""CPU suite: the host side of r3d_clips_metrics (a whole shard of clips in one call) - the layout of r3d_clip_desc against
the header, the argument and scratch checks (all made before any device call: they run without a GPU), the scratch formula
and evaluate.clip_table.  tests/test_gpu_clips_metrics.py runs the kernels."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT

from ray3d_amd import _capi, evaluate

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed


def _define(name):
    return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, HDR).group(1))


def test_entry_points_are_declared_and_bound():
    assert {"r3d_clips_metrics", "r3d_clips_metrics_scratch_bytes"} <= set(_capi.EXPORTS)
    lib = _capi.load()
    assert hasattr(lib, "r3d_clips_metrics") and hasattr(lib, "r3d_clips_metrics_scratch_bytes")
    assert re.search(r"int r3d_clips_metrics\(", HDR) and re.search(r"size_t r3d_clips_metrics_scratch_bytes\(", HDR)
    assert _define("R3D_ABI_VERSION") == _capi.ABI_VERSION == 6          # no existing struct changed
    assert _define("R3D_CLIPS_MAX") == _capi.CLIPS_MAX


def test_clip_desc_layout_against_the_header():
    m = re.search(r"typedef struct \{([^}]*)\} r3d_clip_desc;", HDR)
    assert m, "the header declares r3d_clip_desc"
    fields = re.findall(r"^\s*(int64_t|double)\s+(\w+)(?:\[(\d+)\])?;", m.group(1), flags=re.M)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [("int64_t", "first_frame", 1), ("int64_t", "n_frames", 1),
                                                           ("double", "rn2w", 9), ("double", "tn2w", 3)]
    offsets, at = {}, 0
    for _, name, k in fields:
        offsets[name] = at
        at += 8 * int(k or 1)
    assert at == 112
    assert C.sizeof(_capi.ClipDesc) == 112 and C.alignment(_capi.ClipDesc) == 8
    dt = _capi.clip_desc_dtype()
    assert dt.itemsize == 112 and dt.names == tuple(n for _, n, _ in fields)
    for name, off in offsets.items():
        assert getattr(_capi.ClipDesc, name).offset == off == dt.fields[name][1], name
    assert dt.fields["rn2w"][0].shape == (9,) and dt.fields["tn2w"][0].shape == (3,)
    assert dt.fields["first_frame"][0].base == np.int64 and dt.fields["rn2w"][0].base == np.float64
    # the same bytes through both views
    row = np.zeros(1, dtype=dt)
    row[0]["first_frame"], row[0]["n_frames"] = 7, 9
    row[0]["rn2w"], row[0]["tn2w"] = np.arange(9.0), np.arange(3.0) + 20
    d = _capi.ClipDesc.from_buffer_copy(row.tobytes())
    assert (d.first_frame, d.n_frames, list(d.rn2w), list(d.tn2w)) == (7, 9, list(np.arange(9.0)), [20.0, 21.0, 22.0])


def _blocks(max_frames):
    return min(-(-max_frames // 256), 128)


@pytest.mark.parametrize("num_clips,max_frames", [(1, 1), (1, 256), (1, 257), (3, 513), (240, 6000), (7, 32768), (7, 32769), (2, 10 ** 9)])
@pytest.mark.parametrize("detail", [False, True])
def test_scratch_bytes_equal_the_formula(num_clips, max_frames, detail):
    want = num_clips * _blocks(max_frames) * (5 + (_define("R3D_DETAIL_THRESHOLDS") + 3 * 17 if detail else 0)) * 8
    assert _capi.clips_metrics_scratch_bytes(num_clips, max_frames, detail) == want
    assert _capi.DETAIL_DOUBLES == _define("R3D_DETAIL_THRESHOLDS") + 3 * 17


def test_scratch_bytes_of_bad_arguments_are_zero():
    assert _capi.clips_metrics_scratch_bytes(0, 100, False) == 0
    assert _capi.clips_metrics_scratch_bytes(-1, 100, True) == 0
    assert _capi.clips_metrics_scratch_bytes(4, 0, False) == 0


def _call(**over):
    """r3d_clips_metrics with bogus non-null pointers and otherwise valid arguments; -> the return code."""
    a = dict(pred=BOGUS, gt=BOGUS, total=1000, J=17, table=BOGUS, num_clips=3, max_frames=600, rows=BOGUS, row_stride=8,
             detail=BOGUS, detail_stride=_capi.DETAIL_DOUBLES, frame=BOGUS, scratch=BOGUS, scratch_bytes=None, stream=0)
    a.update(over)
    if a["scratch_bytes"] is None:
        a["scratch_bytes"] = _capi.clips_metrics_scratch_bytes(max(a["num_clips"], 1), max(a["max_frames"], 1), a["detail"] is not None)
    return _capi.load().r3d_clips_metrics(a["pred"], a["gt"], a["total"], a["J"], a["table"], a["num_clips"], a["max_frames"], a["rows"],
                                          a["row_stride"], a["detail"], a["detail_stride"], a["frame"], a["scratch"], a["scratch_bytes"],
                                          a["stream"])


ARG_CASES = [
    (dict(pred=None), "null pointer"), (dict(gt=None), "null pointer"), (dict(table=None), "null pointer"),
    (dict(rows=None), "null pointer"), (dict(scratch=None), "null pointer"),
    (dict(num_clips=0), "num_clips"), (dict(num_clips=-3), "num_clips"), (dict(num_clips=65536), "num_clips"),
    (dict(J=0), "num_joints"), (dict(J=18), "num_joints"),
    (dict(max_frames=0), "max_frames"), (dict(max_frames=-5), "max_frames"),
    (dict(total=0), "total_frames"), (dict(total=-1), "total_frames"),
    (dict(row_stride=4), "row_stride"), (dict(row_stride=0), "row_stride"), (dict(row_stride=-8), "row_stride"),
    (dict(detail_stride=_capi.DETAIL_DOUBLES - 1), "detail_stride"), (dict(detail_stride=0), "detail_stride"),
    (dict(table=BOGUS + 4), "8-byte aligned"), (dict(scratch=BOGUS + 4), "8-byte aligned"),
]


@pytest.mark.parametrize("over,word", ARG_CASES, ids=["%s=%s" % next(iter(o.items())) for o, _ in ARG_CASES])
def test_bad_arguments_return_err_arg_before_any_device_call(over, word):
    """Bogus pointers, as test_forward_before_finalize_fails passes them: the call must decide on the host.  (Without a GPU a
    launch would fail with R3D_ERR_HIP, with one it would fault: R3D_ERR_ARG shows that neither was tried.)"""
    assert _call(**over) == _capi.R3D_ERR_ARG
    assert word in _capi.load().r3d_last_error().decode()


def test_optional_pointers_are_optional_for_the_argument_checks():
    # without detail_dev its stride is not looked at; a too-small scratch is then the first complaint
    assert _call(detail=None, detail_stride=0, frame=None, scratch_bytes=0) == _capi.R3D_ERR_WORKSPACE


@pytest.mark.parametrize("detail", [False, True])
def test_scratch_too_small_returns_err_workspace(detail):
    need = _capi.clips_metrics_scratch_bytes(3, 600, detail)
    for short in (0, 8, need - 1):
        assert _call(detail=BOGUS if detail else None, scratch_bytes=short) == _capi.R3D_ERR_WORKSPACE
        assert "scratch" in _capi.load().r3d_last_error().decode()
    # the scratch of the five sums alone does not do for a detail call
    if detail:
        assert _call(scratch_bytes=_capi.clips_metrics_scratch_bytes(3, 600, False)) == _capi.R3D_ERR_WORKSPACE
    with pytest.raises(_capi.Ray3DHipError, match="scratch"):
        _capi.clips_metrics(BOGUS, BOGUS, 1000, 17, BOGUS, 3, 600, BOGUS, 8, BOGUS if detail else None, _capi.DETAIL_DOUBLES, None,
                            BOGUS, need - 8, 0)


def _stub_clip(n, seed, frame="normalized"):
    rng = np.random.default_rng(seed)
    cam = types.SimpleNamespace(Rn2w=rng.normal(size=(3, 3)), Tn2w=rng.normal(size=(3, 1)),
                                Rc2w=rng.normal(size=(3, 3)), Tc2w=rng.normal(size=(3, 1)))
    return evaluate.Clip(cam, np.zeros((n, 17, 3), np.float32), np.zeros((n, 17, 3), np.float32), "A", seed, frame)


def test_clip_table_offsets_transforms_and_bound():
    lengths = [5, 1, 300, 77]
    clips = [_stub_clip(n, k, "camera" if k == 2 else "normalized") for k, n in enumerate(lengths)]
    table, first, total, longest = evaluate.clip_table(clips)
    assert table.dtype == _capi.clip_desc_dtype() and table.shape == (4,) and table.flags["C_CONTIGUOUS"]
    assert first == [0, 5, 6, 306] and total == 383 and longest == 300
    assert table["first_frame"].tolist() == first and table["n_frames"].tolist() == lengths
    for k, c in enumerate(clips):
        R, T = (c.camera.Rc2w, c.camera.Tc2w) if k == 2 else (c.camera.Rn2w, c.camera.Tn2w)
        assert np.array_equal(table[k]["rn2w"].reshape(3, 3), R) and np.array_equal(table[k]["tn2w"], T.reshape(3))   # row-major, exact
    # root-relative evaluation: the identity, whatever the clip's frame
    table_r, first_r, total_r, longest_r = evaluate.clip_table(clips, root_relative=True)
    assert (first_r, total_r, longest_r) == (first, total, longest)
    for k in range(4):
        assert np.array_equal(table_r[k]["rn2w"], np.eye(3).reshape(9)) and np.array_equal(table_r[k]["tn2w"], np.zeros(3))
    # the bytes that travel: 112 per clip, in clip order
    raw = table.view(np.uint8)
    assert raw.shape == (4 * 112,)
    assert _capi.ClipDesc.from_buffer_copy(raw[112 * 3:].tobytes()).first_frame == 306
    with pytest.raises(ValueError, match="frame"):
        evaluate.clip_table([_stub_clip(3, 0, "world")])
    empty = evaluate.clip_table([])
    assert empty[0].shape == (0,) and empty[1:] == ([], 0, 0)
