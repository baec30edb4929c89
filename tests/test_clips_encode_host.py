"""CPU suite: the host side of r3d_clips_encode (a shard's padded, encoded model inputs from its raw pixel archive in one call) -
the layout of r3d_clip_input_desc against the header, the argument checks (all made before any device call: they run without a
GPU), the host hook r3d_debug_clips_encode_host (the call's validation, row mapping and per-keypoint routines on the CPU)
against a NumPy restatement (pad_clip + ray3d_amd/camera.py's encoders + mirror_input) and tests/golden/px2d.npz, invalid
descriptors, forward_clip(n_windows=) and evaluate.clip_input_table.  tests/test_gpu_clips_encode.py runs the kernel on the
clips built here."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, hooks_library

from ray3d_amd import _capi, evaluate

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed
FILL = np.float32(-7.0)  # what the output buffers hold before a call: rows outside every clip must keep it
ENCODINGS = ("ray", "intrinsic", "screen")
KPS = {17: ([4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]), 14: ([2, 3, 4, 8, 9], [5, 6, 7, 11, 12])}   # (left, right) keypoints
# (frames, pad, causal shift, extra rows behind, camera): pad_front = pad + shift, pad_back = pad - shift + extra.  Lengths 1,
# 2, 15, 16 (255 / 256 / 272 points at J 17: both sides of a workgroup edge) and 40; pads 0, 4, 13; a causal shift; an extra
# pad_back (the surplus of a rounded-up batch size).  Cameras 0..3: distorted H36M rows, 4..7: the same with zero coefficients.
SPECS = ((1, 0, 0, 0, 0), (2, 4, 0, 0, 5), (15, 0, 0, 0, 1), (16, 0, 0, 0, 2), (40, 13, 0, 7, 3), (16, 4, 4, 0, 6),
         (15, 13, 13, 0, 0), (40, 0, 0, 0, 4), (1, 13, 0, 24, 7), (2, 13, 0, 62, 2), (16, 13, 0, 0, 1), (40, 4, 4, 3, 5))
GAP_SRC, GAP_OUT = 5, 3  # frames / rows between stored clips that belong to no clip


def _define(name):
    return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, HDR).group(1))


@functools.lru_cache(maxsize=None)
def cameras():
    """The four H36M cameras of cameras.npz (S9; 1000 x 1002 pixels) with the coefficient sets of undistort.npz
    (undistort=True), then the same four without (zero-coefficient rows)."""
    import ray3d_amd
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    u = np.load(os.path.join(GOLDEN, "undistort.npz"))
    return tuple(ray3d_amd.Camera(u["cam%d/K" % i], z["h36m_S9_%d/R" % i], z["h36m_S9_%d/t" % i], res_w=1000, res_h=1002,
                                  dist_coeff=u["cam%d/dist" % i] if d else None, undistort=d) for d in (True, False) for i in range(4))


def pixels(tag, shape):
    """Keypoints over the whole 1000 x 1002 H36M image."""
    from ray3d_amd import synth
    return (1000.0 * synth.hash_uniform(tag, shape, 7)).astype(np.float32)


def host_encode(cam, uv, encoding):
    """The host chain of ray3d_amd/camera.py: float32 pixels promoted to float64, the encoding in float64, one cast."""
    uv = np.asarray(uv, dtype=np.float32).astype(np.float64)
    fn = {"ray": cam.rays_from_uv, "intrinsic": cam.intrinsic_from_uv, "screen": cam.screen_from_uv}[encoding]
    return fn(uv).astype(np.float32)


@functools.lru_cache(maxsize=None)
def layout(J, specs=SPECS):
    """The clips of `specs`: their pixels stored in a shuffled order with NaN gaps (nothing may read them), their output rows
    laid out in another shuffled order with gaps; the table names them in spec order.
    -> (table, px (total, J, 2), total_frames, out_rows, max_rows, clip pixel arrays)."""
    rng = np.random.default_rng(11 + J)
    src_order, out_order = rng.permutation(len(specs)), rng.permutation(len(specs))
    rows_of = [2 * pad + n + extra for n, pad, _, extra, _ in specs]
    first, at = {}, GAP_SRC
    for c in src_order:
        first[int(c)] = at
        at += specs[c][0] + GAP_SRC
    total = at
    ofirst, at = {}, GAP_OUT
    for c in out_order:
        ofirst[int(c)] = at
        at += rows_of[c] + GAP_OUT
    out_rows = at
    px = np.full((total, J, 2), np.nan, np.float32)
    table = np.zeros(len(specs), dtype=_capi.clip_input_desc_dtype())
    clips = []
    for c, (n, pad, shift, extra, cam) in enumerate(specs):
        clips.append(pixels("clips_encode.%d.%d" % (J, c), (n, J, 2)))
        px[first[c]:first[c] + n] = clips[-1]
        table[c]["first_frame"], table[c]["n_frames"], table[c]["out_first"] = first[c], n, ofirst[c]
        table[c]["pad_front"], table[c]["pad_back"] = pad + shift, pad - shift + extra
        table[c]["cam"] = cameras()[cam].cam_row(distortion=True)
    assert [first[c] for c in range(len(specs))] != sorted(first.values())            # really out of order
    assert [ofirst[c] for c in range(len(specs))] != sorted(ofirst.values())
    for v in (px, table):
        v.setflags(write=False)
    return table, px, total, out_rows, max(rows_of), tuple(clips)


def mirror_perm(J):
    return evaluate.mirror_permutation(J, *KPS[J])


@functools.lru_cache(maxsize=None)
def restatement(J, encoding, specs=SPECS):
    """(x, x_mirror) of `layout`: every clip through evaluate.pad_clip (+ the extra rows behind, as forward_clip repeats the last
    one), the Camera's encoder and evaluate.mirror_input; FILL everywhere else."""
    table, _, _, out_rows, _, clips = layout(J, specs)
    F = 3 if encoding == "ray" else 2
    x = np.full((out_rows, J, F), FILL, np.float32)
    xm = np.full((out_rows, J, F), FILL, np.float32)
    for c, (n, pad, shift, extra, cam) in enumerate(specs):
        padded = evaluate.pad_clip(clips[c], pad, shift)
        padded = np.concatenate([padded, np.repeat(padded[-1:], extra, axis=0)], axis=0)
        enc = host_encode(cameras()[cam], padded, encoding)
        at = int(table[c]["out_first"])
        x[at:at + enc.shape[0]] = enc
        xm[at:at + enc.shape[0]] = evaluate.mirror_input(torch.from_numpy(enc), *KPS[J]).numpy()
    return x, xm


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_hook(J, encoding, table, px, out_rows, max_rows, mirror=True, total=None):
    """r3d_debug_clips_encode_host on host arrays pre-filled with FILL -> (rc, x, x_mirror or None, status)."""
    lib = hooks_library()
    enc = evaluate.ENCODINGS[encoding]
    F = _capi.ENCODE_FLOATS[enc]
    px, table = np.ascontiguousarray(px), np.ascontiguousarray(table)
    x = np.full((out_rows, J, F), FILL, np.float32)
    xm = np.full((out_rows, J, F), FILL, np.float32) if mirror else None
    status = np.full(table.shape[0], -1, np.int32)
    perm = (C.c_int32 * J)(*mirror_perm(J)) if mirror else None
    rc = lib.r3d_debug_clips_encode_host(ptr(px), px.shape[0] if total is None else total, J, enc, ptr(table), table.shape[0], max_rows,
                                         ptr(x), out_rows, ptr(xm) if mirror else None, perm, ptr(status))
    return rc, x, xm, status


def ulps(got, want):
    """Largest distance in float32 representation steps (same-sign finite values)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.isfinite(got).all() and np.isfinite(want).all()
    return int(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max(initial=0))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------ the descriptor and the host-checked errors

def test_entry_points_are_declared_and_bound():
    assert "r3d_clips_encode" in _capi.EXPORTS and "r3d_debug_clips_encode_host" in _capi.HOOK_EXPORTS
    assert hasattr(_capi.load(), "r3d_clips_encode") and not hasattr(_capi.load(), "r3d_debug_clips_encode_host")
    assert hasattr(hooks_library(), "r3d_debug_clips_encode_host") and hasattr(hooks_library(), "r3d_clips_encode")
    assert re.search(r"int r3d_clips_encode\(", HDR)
    assert _define("R3D_ABI_VERSION") == _capi.ABI_VERSION == 6          # no existing struct changed
    assert (_define("R3D_ENCODE_RAY"), _define("R3D_ENCODE_INTRINSIC"), _define("R3D_ENCODE_SCREEN")) == \
        (_capi.R3D_ENCODE_RAY, _capi.R3D_ENCODE_INTRINSIC, _capi.R3D_ENCODE_SCREEN) == (0, 1, 2)
    assert _define("R3D_ENCODE_MAX_POINTS") == _capi.ENCODE_MAX_POINTS
    assert evaluate.ENCODINGS == {"ray": 0, "intrinsic": 1, "screen": 2}


def test_clip_input_desc_layout_against_the_header():
    m = re.search(r"typedef struct \{([^}]*)\} r3d_clip_input_desc;", HDR)
    assert m, "the header declares r3d_clip_input_desc"
    fields = re.findall(r"^\s*(int64_t|int32_t|double)\s+(\w+)(?:\[(\d+)\])?;", m.group(1), flags=re.M)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [("int64_t", "first_frame", 1), ("int64_t", "n_frames", 1), ("int64_t", "out_first", 1),
                                                           ("int32_t", "pad_front", 1), ("int32_t", "pad_back", 1), ("double", "cam", 16)]
    dt = _capi.clip_input_desc_dtype()
    assert dt.itemsize == 160 == _capi.CLIP_INPUT_DESC_BYTES and dt.names == tuple(n for _, n, _ in fields)
    at = 0
    for t, name, k in fields:
        size = 4 if t == "int32_t" else 8
        assert dt.fields[name][1] == at and at % size == 0, name
        assert dt.fields[name][0].base == {"int64_t": np.int64, "int32_t": np.int32, "double": np.float64}[t], name
        at += size * int(k or 1)
    assert at == 160 and dt.fields["cam"][0].shape == (16,)


def _call(**over):
    """r3d_clips_encode with bogus non-null pointers and otherwise valid arguments; -> the return code."""
    a = dict(px=BOGUS, total=1000, J=17, enc=0, table=BOGUS, num_clips=3, max_rows=600, x=BOGUS, out_rows=2000, xm=BOGUS,
             perm=list(range(17)), status=BOGUS, stream=0)
    a.update(over)
    perm = (C.c_int32 * len(a["perm"]))(*a["perm"]) if a["perm"] is not None else None
    return _capi.load().r3d_clips_encode(a["px"], a["total"], a["J"], a["enc"], a["table"], a["num_clips"], a["max_rows"], a["x"],
                                         a["out_rows"], a["xm"], perm, a["status"], a["stream"])


ARG_CASES = [
    (dict(px=None), "null pointer"), (dict(table=None), "null pointer"), (dict(x=None), "null pointer"), (dict(status=None), "null pointer"),
    (dict(num_clips=0), "num_clips"), (dict(num_clips=-3), "num_clips"), (dict(num_clips=65536), "num_clips"),
    (dict(J=0), "num_joints"), (dict(J=18), "num_joints"),
    (dict(enc=3), "encoding"), (dict(enc=-1), "encoding"),
    (dict(max_rows=0), "max_rows"), (dict(max_rows=-5), "max_rows"), (dict(total=0), "total_frames"), (dict(total=-1), "total_frames"),
    (dict(out_rows=0), "out_rows"), (dict(out_rows=-2), "out_rows"),
    (dict(max_rows=2 ** 31 // 17), "must not exceed"), (dict(total=2 ** 31), "must not exceed"), (dict(out_rows=2 ** 40), "must not exceed"),
    (dict(xm=None), "go together"), (dict(perm=None), "go together"),
    (dict(perm=[0] * 17), "permutation"), (dict(perm=list(range(1, 18))), "permutation"), (dict(perm=[-1] + list(range(1, 17))), "permutation"),
    (dict(table=BOGUS + 4), "8-byte aligned"),
]


@pytest.mark.parametrize("over,word", ARG_CASES, ids=["%s=%s" % next(iter(o.items())) for o, _ in ARG_CASES])
def test_bad_arguments_return_err_arg_before_any_device_call(over, word):
    """Bogus pointers: the call must decide on the host.  (Without a GPU a launch would fail with R3D_ERR_HIP, with one it
    would fault: R3D_ERR_ARG shows that neither was tried.)"""
    assert _call(**over) == _capi.R3D_ERR_ARG
    assert word in _capi.load().r3d_last_error().decode()


def test_the_binding_refuses_a_short_permutation():
    with pytest.raises(_capi.Ray3DHipError, match="mirror_perm"):
        _capi.clips_encode(BOGUS, 10, 17, 0, BOGUS, 1, 10, BOGUS, 10, BOGUS, list(range(14)), BOGUS, 0)
    with pytest.raises(_capi.Ray3DHipError, match="go together"):
        _capi.clips_encode(BOGUS, 10, 17, 0, BOGUS, 1, 10, BOGUS, 10, None, list(range(17)), BOGUS, 0)


# ------------------------------------------------------------------ the hook against the NumPy restatement

@pytest.mark.parametrize("J", [17, 14])
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_hook_equals_the_numpy_restatement(encoding, J):
    """Every element within one float32 ulp of pad_clip + the Camera's encoder (the bound tests/test_gpu_undistort.py puts on
    elements that differ); the mirrored buffer is the negated, permuted plain one bit for bit; rows outside every clip keep
    their fill."""
    table, px, total, out_rows, max_rows, _ = layout(J)
    want, want_m = restatement(J, encoding)
    rc, x, xm, status = run_hook(J, encoding, table, px, out_rows, max_rows)
    assert rc == 0 and not status.any()
    covered = np.zeros(out_rows, bool)
    for d in table:
        covered[d["out_first"]:d["out_first"] + d["pad_front"] + d["n_frames"] + d["pad_back"]] = True
    assert 0 < (~covered).sum() and (x[~covered] == FILL).all() and (xm[~covered] == FILL).all()
    assert (want[~covered] == FILL).all()
    worst = ulps(x[covered], want[covered])
    print("%s J %d: %.6f of %d elements equal, max %d ulp" % (encoding, J, float((x == want).mean()), x.size, worst))
    assert worst <= 1
    assert ulps(xm[covered], want_m[covered]) <= 1
    # the mirrored copy: x_mirror[row, j] = x[row, perm[j]], component 0 negated - exactly
    perm = mirror_perm(J)
    exp = x[:, perm].copy()
    exp[..., 0] = -exp[..., 0]
    assert same_bits(xm[covered], exp[covered])
    assert same_bits(exp[covered], evaluate.mirror_input(torch.from_numpy(x), *KPS[J]).numpy()[covered])
    # a padding row has the bits of the frame it repeats
    for d in table:
        at, pf, n, pb = int(d["out_first"]), int(d["pad_front"]), int(d["n_frames"]), int(d["pad_back"])
        assert all(same_bits(x[at + r], x[at + pf]) for r in range(pf))
        assert all(same_bits(x[at + pf + n + r], x[at + pf + n - 1]) for r in range(pb))
    # without the mirrored copy: the same plain buffer
    rc, x2, none, status = run_hook(J, encoding, table, px, out_rows, max_rows, mirror=False)
    assert rc == 0 and none is None and not status.any() and same_bits(x2, x)


@pytest.mark.parametrize("encoding", ["intrinsic", "screen"])
def test_hook_two_float_encodings_equal_the_reference_fixture(encoding):
    """tests/golden/px2d.npz: normalize_screen_coordinates / encode_uv_with_intrinsic of the reference's own cameras (zero
    coefficients) and pixel pairs.  The call takes float32 pixels: for the pairs a float32 holds exactly the result is the
    fixture's value cast once; for all of them it is within one ulp of the host chain on the rounded pixels."""
    import ray3d_amd
    z = np.load(os.path.join(GOLDEN, "px2d.npz"))
    for tag in z["enc/tags"]:
        p = "enc/%s" % tag
        w, h = z[p + "/res"]
        cam = ray3d_amd.Camera(z[p + "/K"], z[p + "/R"], z[p + "/t"], res_w=w, res_h=h)
        X = z[p + "/X"]
        X32 = X.astype(np.float32)
        exact = (X32.astype(np.float64) == X).all(axis=1)
        assert exact.sum() >= 4, "the fixture's corners are float32 numbers"
        n = X.shape[0] // 4
        table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
        table[0]["n_frames"], table[0]["cam"] = n, cam.cam_row(distortion=True)
        rc, x, _, status = run_hook(4, encoding, table, X32.reshape(n, 4, 2), n, n, mirror=False)
        assert rc == 0 and not status.any()
        got = x.reshape(-1, 2)
        assert same_bits(got[exact], z[p + "/" + encoding][exact].astype(np.float32))
        assert ulps(got, host_encode(cam, X32, encoding)) <= 1


# ------------------------------------------------------------------ invalid descriptors

def invalid_cases(total, out_rows, max_rows):
    """(what, fields to overwrite in a valid descriptor): each of the five conditions, and ranges that point far outside."""
    big = 2 ** 62
    return [("n_frames < 1", dict(n_frames=0)), ("n_frames < 1", dict(n_frames=-4)),
            ("pad < 0", dict(pad_front=-1)), ("pad < 0", dict(pad_back=-2 ** 31)),
            ("rows > max_rows", dict(pad_back=max_rows)), ("rows > max_rows", dict(n_frames=max_rows + 1, first_frame=0)),
            ("rows > max_rows", dict(pad_front=2 ** 31 - 1, pad_back=2 ** 31 - 1)),
            ("source outside", dict(first_frame=-1)), ("source outside", dict(first_frame=total - 1, n_frames=2, pad_front=0, pad_back=0)),
            ("source outside", dict(first_frame=big)), ("source outside", dict(first_frame=-big)), ("source outside", dict(n_frames=big)),
            ("output outside", dict(out_first=-1)), ("output outside", dict(out_first=out_rows - 1, n_frames=2, pad_front=0, pad_back=0)),
            ("output outside", dict(out_first=big)), ("output outside", dict(out_first=-big))]


def with_invalid(J):
    """`layout`'s table with every second clip's descriptor replaced by an invalid one (each case in turn, cycling)."""
    table, px, total, out_rows, max_rows, _ = layout(J)
    cases = invalid_cases(total, out_rows, max_rows)
    tables = []
    for start in range(0, len(cases), len(table) // 2):
        t = np.array(table)
        bad = {}
        for k, (what, over) in enumerate(cases[start:start + len(table) // 2]):
            c = 2 * k + 1
            for name, v in over.items():
                t[c][name] = v
            bad[c] = what
        tables.append((t, bad))
    return tables


@pytest.mark.parametrize("J", [17, 14])
def test_hook_invalid_descriptors_are_not_followed(J):
    """Each of the five conditions in a table that also has valid clips: status 1, nothing of that clip written, the other
    clips as in the all-valid run."""
    table, px, total, out_rows, max_rows, _ = layout(J)
    _, ref, ref_m, _ = run_hook(J, "ray", table, px, out_rows, max_rows)
    seen = set()
    for t, bad in with_invalid(J):
        rc, x, xm, status = run_hook(J, "ray", t, px, out_rows, max_rows)
        assert rc == 0
        assert status.tolist() == [1 if c in bad else 0 for c in range(len(t))], bad
        want, want_m = ref.copy(), ref_m.copy()
        for c in bad:
            d = table[c]
            rows = slice(int(d["out_first"]), int(d["out_first"] + d["pad_front"] + d["n_frames"] + d["pad_back"]))
            want[rows], want_m[rows] = FILL, FILL
        assert same_bits(x, want) and same_bits(xm, want_m), bad
        seen |= set(bad.values())
    assert seen == {"n_frames < 1", "pad < 0", "rows > max_rows", "source outside", "output outside"}


def test_hook_bounds_are_the_stated_extents_exactly():
    """A clip that fills the pixel archive and the output buffer to their last rows is followed; one row more is not."""
    J = 3
    px = pixels("clips_encode.exact", (6, J, 2))
    table = np.zeros(2, dtype=_capi.clip_input_desc_dtype())
    for c in range(2):
        table[c]["cam"] = cameras()[c].cam_row(distortion=True)
    table[0]["first_frame"], table[0]["n_frames"], table[0]["out_first"], table[0]["pad_front"], table[0]["pad_back"] = 0, 6, 0, 2, 1
    table[1]["first_frame"], table[1]["n_frames"], table[1]["out_first"], table[1]["pad_front"], table[1]["pad_back"] = 5, 1, 9, 0, 0
    rc, x, _, status = run_hook(J, "ray", table, px, 10, 9, mirror=False)
    assert rc == 0 and status.tolist() == [0, 0] and (x != FILL).all()
    rc, x, _, status = run_hook(J, "ray", table, px, 10, 8, mirror=False)              # max_rows one short of clip 0
    assert status.tolist() == [1, 0] and (x[:9] == FILL).all() and (x[9] != FILL).all()
    rc, x, _, status = run_hook(J, "ray", table, px, 9, 9, mirror=False)               # out_rows one short of clip 1
    assert status.tolist() == [0, 1]
    rc, x, _, status = run_hook(J, "ray", table, px, 10, 9, mirror=False, total=5)     # total_frames one short of both
    assert status.tolist() == [1, 1] and (x == FILL).all()


# ------------------------------------------------------------------ forward_clip(n_windows=) and clip_input_table

class _Recorder:
    """Ray3DLifter.forward_clip on a stand-in: _run records (rows of the clip it was handed, batch size) and fills `out`."""

    def __init__(self):
        import ray3d_amd
        self.calls = []
        self.pos = types.SimpleNamespace(num_joints_in=17, in_features=3, camera_embedding=False)
        for name in ("clip_batch_sizes", "forward_clip", "_forward_clip_into"):
            setattr(self, name, types.MethodType(getattr(ray3d_amd.Ray3DLifter, name), self))
        self.CLIP_CHUNK, self.CLIP_ROUND, self.CLIP_BALANCED = 4096, 128, True

    def receptive_field(self):
        return 27

    def join_lanes(self):
        pass

    def _lane_of_current_stream(self, dev):
        return None

    def _run(self, mode, x, stride, B, p, pstride, return_trj=False, out=None):
        assert stride == 1 and x.shape[0] >= B + 26
        self.calls.append((x[:B + 26].clone(), B))
        if out is None:
            out = torch.empty((B, 1, 17, 3))
        out[:] = x[13:13 + B, :, :].reshape(B, 1, 17, 3)          # "the pose of window i is the frame in its middle"
        return out


@pytest.mark.parametrize("n", [1, 40, 65, 100, 128, 300])
def test_forward_clip_n_windows_runs_the_same_forwards_without_concatenating(n):
    lifter = _Recorder()
    sizes = lifter.clip_batch_sizes(n)
    total = sum(sizes)
    padded = torch.from_numpy(pixels("clips_encode.fc.%d" % n, (n + 26, 17, 3)))
    full = torch.cat([padded, padded[-1:].expand(total - n, -1, -1)], dim=0)
    want = lifter.forward_clip(padded)
    calls = lifter.calls
    lifter.calls = []
    got = lifter.forward_clip(full, n_windows=n)
    assert torch.equal(got, want) and got.shape == (n, 1, 17, 3)
    assert [b for _, b in lifter.calls] == [b for _, b in calls] == sizes
    assert all(torch.equal(a, b) for (a, _), (b, _) in zip(lifter.calls, calls))
    out = torch.zeros((n, 1, 17, 3))
    assert lifter.forward_clip(full, out=out, n_windows=n) is out and torch.equal(out, want)
    # any other row count is refused - the unpadded clip, one row more, one less
    for bad in ([padded] if total > n else []) + [torch.cat([full, full[-1:]]), full[:-1]]:
        with pytest.raises(ValueError, match="n_windows"):
            lifter.forward_clip(bad, n_windows=n)
    with pytest.raises(ValueError, match="n_windows"):
        lifter.forward_clip(full, n_windows=0)


def _stub_clip(n, cam, seed, J=17):
    return evaluate.Clip(cam, pixels("clips_encode.table.%d" % seed, (n, J, 2)), np.zeros((n, J, 3), np.float32), "A", seed)


@pytest.mark.parametrize("causal", [False, True])
def test_clip_input_table_reproduces_pad_clip_and_the_surplus(causal):
    lifter = _Recorder()
    lengths, rf = [5, 1, 300, 77, 128], 27
    clips = [_stub_clip(n, cameras()[k % 8], k) for k, n in enumerate(lengths)]
    surplus = lambda n: sum(lifter.clip_batch_sizes(n)) - n
    table, out_first, out_rows, max_rows = evaluate.clip_input_table(clips, rf, causal, surplus)
    assert table.dtype == _capi.clip_input_desc_dtype() and table.shape == (5,) and table.flags["C_CONTIGUOUS"]
    assert table["first_frame"].tolist() == [0, 5, 6, 306, 383] and table["n_frames"].tolist() == lengths
    rows = [n + 26 + surplus(n) for n in lengths]
    assert [surplus(n) for n in lengths] == [3, 0, 84, 51, 0]
    assert out_first == table["out_first"].tolist() == [sum(rows[:k]) for k in range(5)] and out_rows == sum(rows) and max_rows == max(rows)
    assert table["pad_front"].tolist() == [26 if causal else 13] * 5
    assert table["pad_back"].tolist() == [(0 if causal else 13) + surplus(n) for n in lengths]
    for k, c in enumerate(clips):
        assert np.array_equal(table[k]["cam"], c.camera.cam_row(distortion=True))
    # through the hook: a clip's slice is pad_clip's padding plus the repeated last row - what forward_clip(n_windows=) takes
    px = np.concatenate([c.rays for c in clips], axis=0)
    rc, x, _, status = run_hook(17, "screen", table, px, out_rows, max_rows, mirror=False)
    assert rc == 0 and not status.any() and (x != FILL).all()
    for k, c in enumerate(clips):
        padded = evaluate.pad_clip(c.rays, 13, 13 if causal else 0)
        padded = np.concatenate([padded, np.repeat(padded[-1:], surplus(lengths[k]), axis=0)], axis=0)
        assert padded.shape[0] == sum(lifter.clip_batch_sizes(lengths[k])) + rf - 1
        assert ulps(x[out_first[k]:out_first[k] + rows[k]], host_encode(c.camera, padded, "screen")) <= 1
    # without a surplus function: pad_clip's rows alone; the bytes that travel: 160 per clip
    t0, f0, r0, m0 = evaluate.clip_input_table(clips, rf, causal)
    assert r0 == sum(n + 26 for n in lengths) and m0 == 326 and t0["pad_back"].tolist() == [0 if causal else 13] * 5
    assert table.view(np.uint8).shape == (5 * 160,)
    assert evaluate.clip_input_table([], rf)[1:] == ([], 0, 0)


def test_mirror_permutation():
    assert evaluate.mirror_permutation(5, [1], [3]) == [0, 3, 2, 1, 4]
    x = torch.arange(2 * 17 * 3, dtype=torch.float32).reshape(2, 17, 3) + 1
    m = x[:, mirror_perm(17)].clone()
    m[..., 0] *= -1
    assert torch.equal(m, evaluate.mirror_input(x, *KPS[17]))
    with pytest.raises(ValueError, match="permutation"):
        evaluate.mirror_permutation(5, [1, 2], [2, 3])
