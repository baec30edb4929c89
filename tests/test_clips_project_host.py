"""CPU suite: the host side of r3d_clips_project (a camera sweep's model inputs, ground truth, pixels and in-frame counts from world
poses in one call) - the layout of r3d_clip_project_desc against the header, the argument rules (all checked before any device
call: they run without a GPU), the host hook r3d_debug_clips_project_host (the call's validation, row mapping and per-point
routines on the CPU) against the REFERENCE's own values (tests/golden/project.npz, made by tests/golden/make_golden_project.py)
and against a NumPy restatement on the shapes of the device test, invalid descriptors, non-finite points, Camera.proj_row and
evaluate.clip_project_table.  tests/test_gpu_clips_project.py runs the kernel on the layouts built here."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, hooks_library

from ray3d_amd import _capi, evaluate

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
BOGUS = 1 << 20          # a non-null, 8-byte aligned "device pointer" that is never followed
FILL = np.float32(-7.0)  # what the output buffers hold before a call: rows outside every descriptor must keep it
FILL_COUNT = 1000        # what `outside` holds before a call: the call ADDS to it
ENCODINGS = ("ray", "intrinsic", "screen")
KPS = {17: ([4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]), 14: ([2, 3, 4, 8, 9], [5, 6, 7, 11, 12]), 1: ([], [])}
RF = 9
PAD = (RF - 1) // 2
# (source clip, camera, pad_front, pad_back): clips of 1, 15, 16 and 31 frames (16 x 17 = 272 points: past one workgroup) under
# RF 9 - centred padding, causal padding (8, 0), a surplus in pad_back - and two cameras on the SAME source frames
CLIP_FRAMES = (1, 15, 16, 31)
SPECS = ((0, 0, PAD, PAD), (1, 1, PAD, PAD), (2, 0, PAD, PAD), (3, 2, PAD, PAD), (2, 1, 2 * PAD, 0), (1, 2, PAD, PAD + 1),
         (3, 0, PAD, PAD + 1), (0, 2, 2 * PAD, 0), (2, 2, PAD, PAD + 16))
GAP_SRC, GAP_OUT, GAP_GT = 5, 3, 2   # frames / rows between stored clips that belong to no descriptor


def _define(name):
    return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, HDR).group(1))


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "project.npz"))


@functools.lru_cache(maxsize=None)
def cameras():
    """The three virtual cameras of project.npz (1000 x 1000 frame): two keep the figure in frame, the third does not."""
    import ray3d_amd
    z = golden()
    res = z["res"]
    return tuple(ray3d_amd.Camera(z["cam/%d/K" % i], z["cam/%d/R" % i], z["cam/%d/t" % i], name=str(z["cam/names"][i]),
                                  res_w=res[0], res_h=res[1]) for i in range(3))


def world_points(tag, shape):
    """A figure's points in a 0.7 x 0.7 x 1.7 m box around (0, 0, 0.9): in front of every camera of the fixture."""
    from ray3d_amd import synth
    return ((synth.hash_uniform(tag, shape, 3) - 0.5) * np.array([0.7, 0.7, 1.7]) + np.array([0.0, 0.0, 0.9])).astype(np.float32)


def transform(cam, frame):
    return (cam.Rw2n, cam.Tw2n) if frame == "normalized" else (cam.Rw2c, cam.Tw2c)


def fill_desc(d, cam, frame, first, n, out_first, gt_first, pad_front, pad_back):
    R, T = transform(cam, frame)
    d["first_frame"], d["n_frames"], d["out_first"], d["gt_first"] = first, n, out_first, gt_first
    d["pad_front"], d["pad_back"] = pad_front, pad_back
    d["proj"], d["cam"] = cam.proj_row(), cam.cam_row(distortion=True)
    d["rw2g"], d["tw2g"] = np.asarray(R).reshape(9), np.asarray(T).reshape(3)


@functools.lru_cache(maxsize=None)
def layout(J, frame="normalized", specs=SPECS):
    """The descriptors of `specs`: the source clips stored ONCE each, in a shuffled order with NaN gaps (nothing may read them);
    output rows and ground-truth rows laid out in two other shuffled orders with gaps; the table names them in spec order.
    -> (table, world (total, J, 3), out_rows, max_rows, gt_rows, source clips)."""
    rng = np.random.default_rng(23 + J)
    src_order = rng.permutation(len(CLIP_FRAMES))
    out_order, gt_order = rng.permutation(len(specs)), rng.permutation(len(specs))
    first, at = {}, GAP_SRC
    for c in src_order:
        first[int(c)] = at
        at += CLIP_FRAMES[c] + GAP_SRC
    total = at
    rows_of = [pf + CLIP_FRAMES[c] + pb for c, _, pf, pb in specs]
    ofirst, at = {}, GAP_OUT
    for k in out_order:
        ofirst[int(k)] = at
        at += rows_of[k] + GAP_OUT
    out_rows = at
    gfirst, at = {}, GAP_GT
    for k in gt_order:
        gfirst[int(k)] = at
        at += CLIP_FRAMES[specs[k][0]] + GAP_GT
    gt_rows = at
    world = np.full((total, J, 3), np.nan, np.float32)
    clips = []
    for c, n in enumerate(CLIP_FRAMES):
        clips.append(world_points("clips_project.%d.%d" % (J, c), (n, J, 3)))
        world[first[c]:first[c] + n] = clips[-1]
    table = np.zeros(len(specs), dtype=_capi.clip_project_desc_dtype())
    for k, (c, cam, pf, pb) in enumerate(specs):
        fill_desc(table[k], cameras()[cam], frame, first[c], CLIP_FRAMES[c], ofirst[k], gfirst[k], pf, pb)
    assert [ofirst[k] for k in range(len(specs))] != sorted(ofirst.values())            # really out of order
    for v in (world, table):
        v.setflags(write=False)
    return table, world, out_rows, max(rows_of), gt_rows, tuple(clips)


def invalid_cases(table, total, out_rows, max_rows, gt_rows):
    """One descriptor of each invalid kind, made from descriptor 1 of `table`: name -> descriptor."""
    def edit(**kw):
        d = table[1:2].copy()
        for k, v in kw.items():
            d[0][k] = v
        return d[0]
    n = int(table[1]["n_frames"])
    return {"n<1": edit(n_frames=0), "negative pad": edit(pad_front=-1), "rows over max_rows": edit(pad_back=max_rows),
            "source out of range": edit(first_frame=total - n + 1), "output out of range": edit(out_first=out_rows - n),
            "gt out of range": edit(gt_first=gt_rows - n + 1), "negative gt_first": edit(gt_first=-1),
            "huge n": edit(n_frames=2 ** 62), "huge first": edit(first_frame=2 ** 63 - 1)}


def with_invalid(table, total, out_rows, max_rows, gt_rows):
    """`table` with one invalid descriptor of each kind between its valid ones -> (table, indices of the invalid ones)."""
    bad = list(invalid_cases(table, total, out_rows, max_rows, gt_rows).values())
    rows, where = [], []
    for k in range(len(table)):
        rows.append(table[k])
        if k < len(bad):
            where.append(len(rows))
            rows.append(bad[k])
    assert len(bad) <= len(table)
    return np.array(rows, dtype=table.dtype), where


def mirror_perm(J):
    return evaluate.mirror_permutation(J, *KPS[J])


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def host_buffers(J, encoding, num, out_rows, gt_rows, mirror=True, gt=True, px=True, count=True):
    F = _capi.ENCODE_FLOATS[evaluate.ENCODINGS[encoding]]
    return dict(x=np.full((out_rows, J, F), FILL, np.float32), xm=np.full((out_rows, J, F), FILL, np.float32) if mirror else None,
                gt=np.full((gt_rows, J, 3), FILL, np.float32) if gt else None,
                px=np.full((gt_rows, J, 2), float(FILL), np.float64) if px else None,
                outside=np.full(num, FILL_COUNT, np.int32) if count else None, status=np.full(num, -1, np.int32))


def run_hook(J, encoding, table, world, out_rows, max_rows, gt_rows, mirror=True, gt=True, px=True, count=True, total=None):
    """r3d_debug_clips_project_host on host arrays pre-filled with FILL -> (rc, dict of the buffers)."""
    lib = hooks_library()
    world, table = np.ascontiguousarray(world), np.ascontiguousarray(table)
    b = host_buffers(J, encoding, table.shape[0], out_rows, gt_rows, mirror, gt, px, count)
    perm = (C.c_int32 * J)(*mirror_perm(J)) if mirror else None
    rc = lib.r3d_debug_clips_project_host(ptr(world), world.shape[0] if total is None else total, J, evaluate.ENCODINGS[encoding],
                                          ptr(table), table.shape[0], max_rows, ptr(b["x"]), out_rows, ptr(b["xm"]), perm,
                                          ptr(b["gt"]), ptr(b["px"]), gt_rows, ptr(b["outside"]), ptr(b["status"]))
    return rc, b


def same_bits(a, b):
    w = np.int32 if a.dtype.itemsize == 4 else np.int64
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(w), b.view(w))


def within_one_f32_ulp(got, want, what):
    """|a - b| <= 2^-23 max(|a|, |b|) + 1e-12 for every element, at most 1e-3 of them other than bit-equal: two float64 chains of
    fewer than 10 operations that differ in the order of a four-term dot product, after ONE cast - at most one float32 ulp, and
    only at a rounding boundary."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    a, b = got.astype(np.float64), want.astype(np.float64)
    off = float((got.view(np.int32) != want.view(np.int32)).mean())
    worst = float((np.abs(a - b) - (2.0 ** -23 * np.maximum(np.abs(a), np.abs(b)) + 1e-12)).max())
    print("%s: %d elements, share not bit-equal %.2e, worst |a-b| - bound %.3e" % (what, got.size, off, worst))
    assert worst <= 0.0, what
    assert off <= 1e-3, what


# ------------------------------------------------------------------ the descriptor, the bindings, the host-side pieces

def test_entry_points_are_declared_and_bound():
    assert "r3d_clips_project" in _capi.EXPORTS and "r3d_debug_clips_project_host" in _capi.HOOK_EXPORTS
    assert hasattr(_capi.load(), "r3d_clips_project") and not hasattr(_capi.load(), "r3d_debug_clips_project_host")
    assert hasattr(hooks_library(), "r3d_debug_clips_project_host") and hasattr(hooks_library(), "r3d_clips_project")
    assert re.search(r"int r3d_clips_project\(", HDR) and re.search(r"int r3d_debug_clips_project_host\(", HDR)
    assert _define("R3D_ABI_VERSION") == _capi.ABI_VERSION == 6          # no existing struct changed


def test_clip_project_desc_layout_against_the_header():
    m = re.search(r"typedef struct \{([^}]*)\} r3d_clip_project_desc;", HDR)
    assert m, "the header declares r3d_clip_project_desc"
    fields = re.findall(r"^\s*(int64_t|int32_t|double)\s+(\w+)(?:\[(\d+)\])?;", m.group(1), flags=re.M)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [
        ("int64_t", "first_frame", 1), ("int64_t", "n_frames", 1), ("int64_t", "out_first", 1), ("int64_t", "gt_first", 1),
        ("int32_t", "pad_front", 1), ("int32_t", "pad_back", 1), ("double", "proj", 12), ("double", "cam", 16), ("double", "rw2g", 9),
        ("double", "tw2g", 3)]
    dt = _capi.clip_project_desc_dtype()
    assert dt.itemsize == 360 == _capi.CLIP_PROJECT_DESC_BYTES and dt.names == tuple(n for _, n, _ in fields)
    at = 0
    for t, name, k in fields:
        size = 4 if t == "int32_t" else 8
        assert dt.fields[name][1] == at and at % size == 0, name
        assert dt.fields[name][0].base == {"int64_t": np.int64, "int32_t": np.int32, "double": np.float64}[t], name
        at += size * int(k or 1)
    assert at == 360


def test_proj_row_is_the_reference_projection_matrix():
    """Camera.proj_row(): K @ hstack([R, t]) as CameraInfoPacket builds P (a 3x4 product of float64 numbers: a few ulps at most
    between two BLAS builds)."""
    z = golden()
    for i, cam in enumerate(cameras()):
        row = cam.proj_row()
        assert row.dtype == np.float64 and row.shape == (12,) and row.flags["C_CONTIGUOUS"]
        np.testing.assert_allclose(row.reshape(3, 4), z["cam/%d/P" % i], rtol=1e-14, atol=1e-12)
        np.testing.assert_allclose(cam.Rw2n, z["cam/%d/Rw2n" % i], rtol=0, atol=1e-14)
        np.testing.assert_allclose(cam.Tw2n, z["cam/%d/Tw2n" % i], rtol=0, atol=1e-14)


def _world_clips():
    z = golden()
    return [evaluate.WorldClip(z["world/" + str(t)], action="A" if k == 0 else "B", clip_id=k) for k, t in enumerate(z["clips"])]


def test_clip_project_table_layout():
    """Camera-major pairs over the two fixture clips: every camera's descriptors name the SAME source frames, outputs and ground
    truth are back to back in pair order, pads and surplus as clip_input_table's."""
    wc = _world_clips()
    pairs = [(k, ci) for ci in range(3) for k in range(2)]
    surplus = lambda n: (-n) % 8
    for causal in (False, True):
        t, out_first, out_rows, max_rows, gt_first, gt_rows = evaluate.clip_project_table(wc, pairs, cameras(), RF, causal, surplus, "camera")
        assert t.dtype == _capi.clip_project_desc_dtype() and len(t) == 6
        assert t["first_frame"].tolist() == [0, 1] * 3 and t["n_frames"].tolist() == [1, 19] * 3
        rows = [2 * PAD + n + surplus(n) for n in (1, 19)] * 3
        assert out_first == np.concatenate([[0], np.cumsum(rows)[:-1]]).tolist() == t["out_first"].tolist()
        assert out_rows == sum(rows) and max_rows == max(rows) and gt_rows == 60
        assert gt_first == [0, 1, 20, 21, 40, 41] == t["gt_first"].tolist()
        assert t["pad_front"].tolist() == [2 * PAD if causal else PAD] * 6
        assert (t["pad_front"] + t["n_frames"] + t["pad_back"]).tolist() == rows
        for k, (_, ci) in enumerate(pairs):
            cam = cameras()[ci]
            assert np.array_equal(t[k]["proj"], cam.proj_row()) and np.array_equal(t[k]["cam"], cam.cam_row(distortion=True))
            assert t[k]["cam"][6] == t[k]["cam"][7] == 1000.0
            assert np.array_equal(t[k]["rw2g"].reshape(3, 3), cam.Rw2c) and np.array_equal(t[k]["tw2g"], cam.Tw2c.reshape(3))
    t = evaluate.clip_project_table(wc, pairs, cameras(), RF)[0]
    assert np.array_equal(t[3]["rw2g"].reshape(3, 3), cameras()[1].Rw2n) and (t["pad_back"] == PAD).all()
    with pytest.raises(ValueError, match="frame"):
        evaluate.clip_project_table(wc, pairs, cameras(), RF, frame="world")
    import ray3d_amd
    blind = ray3d_amd.Camera(cameras()[0].K, cameras()[0].Rw2c, cameras()[0].Tw2c)
    with pytest.raises(ValueError, match="res_w"):
        evaluate.clip_project_table(wc, [(0, 0)], [blind], RF)


# ------------------------------------------------------------------ 1. reference parity: the hook against project.npz

@pytest.mark.parametrize("frame", ["normalized", "camera"])
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_hook_equals_the_reference(encoding, frame):
    """Every (clip, camera) pair of project.npz through r3d_debug_clips_project_host with a table of evaluate.clip_project_table:
    the model input against get_cam_ray_given_uv / encode_uv_with_intrinsic / normalize_screen_coordinates of the reference's
    float64 pixels, the ground truth against world2normalized / world2camera - float32 values within one ulp of the reference's
    cast to float32 and at most 1e-3 of them not bit-equal -, the float64 pixels within 1e-10 px of CameraInfoPacket.project, and
    the outside counts equal to the reference's."""
    z = golden()
    wc = _world_clips()
    world = np.concatenate([c.world for c in wc], axis=0)
    pairs = [(k, ci) for ci in range(3) for k in range(2)]
    table, out_first, out_rows, max_rows, gt_first, gt_rows = evaluate.clip_project_table(wc, pairs, cameras(), RF, frame=frame)
    rc, b = run_hook(17, encoding, table, world, out_rows, max_rows, gt_rows)
    assert rc == 0 and not b["status"].any()
    got_x, want_x, got_gt, want_gt, got_px, want_px = [], [], [], [], [], []
    for k, (ci_clip, ci) in enumerate(pairs):
        tag = str(z["clips"][ci_clip])
        n = wc[ci_clip].world.shape[0]
        key = "ref/%s/%d/" % (tag, ci)
        x = b["x"][out_first[k]:out_first[k] + 2 * PAD + n]
        got_x.append(x[PAD:PAD + n])
        want_x.append(z[key + encoding].astype(np.float32))
        assert all(same_bits(x[r], x[PAD]) for r in range(PAD)) and all(same_bits(x[PAD + n + r], x[PAD + n - 1]) for r in range(PAD))
        got_gt.append(b["gt"][gt_first[k]:gt_first[k] + n])
        want_gt.append(z[key + ("gt_norm" if frame == "normalized" else "gt_cam")].astype(np.float32))
        got_px.append(b["px"][gt_first[k]:gt_first[k] + n])
        want_px.append(z[key + "px"])
        assert int(b["outside"][k]) - FILL_COUNT == int(z[key + "outside"]), (tag, ci)
        assert bool(z[key + "in_frame"]) == (int(z[key + "outside"]) == 0)
    within_one_f32_ulp(np.concatenate(got_x), np.concatenate(want_x), "input %s" % encoding)
    within_one_f32_ulp(np.concatenate(got_gt), np.concatenate(want_gt), "ground truth %s" % frame)
    err = float(np.abs(np.concatenate(got_px) - np.concatenate(want_px)).max())
    print("pixels: max |diff| %.3e px" % err)
    assert err <= 1e-10
    assert [int(v) - FILL_COUNT for v in b["outside"]] == [0, 0, 0, 0] + [int(z["ref/one/2/outside"]), int(z["ref/walk/2/outside"])]
    assert int(z["ref/walk/2/outside"]) > 0
    mir = evaluate.mirror_input(__import__("torch").from_numpy(b["x"].copy()), *KPS[17]).numpy()
    assert same_bits(b["xm"], mir)


# ------------------------------------------------------------------ the hook on the device test's layouts

def restatement(J, encoding, frame, table, clips_of, out_rows, gt_rows):
    """(x, gt, px, outside) of the descriptors `table` (spec order) in float64 NumPy through ray3d_amd/camera.py; FILL elsewhere."""
    F = 3 if encoding == "ray" else 2
    x = np.full((out_rows, J, F), np.nan)
    gt, px = np.full((gt_rows, J, 3), np.nan), np.full((gt_rows, J, 2), np.nan)
    outside = []
    for d, (c, ci, pf, pb) in zip(table, SPECS):
        cam, w = cameras()[ci], clips_of[c].astype(np.float64)
        uv = cam.project(w)
        enc = {"ray": cam.rays_from_uv, "intrinsic": cam.intrinsic_from_uv, "screen": cam.screen_from_uv}[encoding](uv)
        padded = np.concatenate([np.repeat(enc[:1], pf, axis=0), enc, np.repeat(enc[-1:], pb, axis=0)], axis=0)
        x[int(d["out_first"]):int(d["out_first"]) + padded.shape[0]] = padded
        g = int(d["gt_first"])
        gt[g:g + w.shape[0]] = cam.world2normalized(w) if frame == "normalized" else cam.world2camera(w)
        px[g:g + w.shape[0]] = uv
        outside.append(int((~((uv[..., 0] >= 0) & (uv[..., 0] <= 1000) & (uv[..., 1] >= 0) & (uv[..., 1] <= 1000))).sum()))
    return x, gt, px, outside


@pytest.mark.parametrize("J", [1, 14, 17])
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_hook_on_shuffled_layouts(encoding, J):
    """Clips of 1 / 15 / 16 / 31 frames, centred, causal and surplus padding, three cameras on shared source frames, out of order
    with gaps: the hook against the NumPy chain of ray3d_amd/camera.py (a different operation order: 4 float32 ulps / 1e-9 px),
    FILL in every row no descriptor covers, the mirrored copy the exact mirror_input of the plain one."""
    import torch
    frame = "camera" if J == 14 else "normalized"
    table, world, out_rows, max_rows, gt_rows, clips = layout(J, frame)
    rc, b = run_hook(J, encoding, table, world, out_rows, max_rows, gt_rows)
    assert rc == 0 and not b["status"].any()
    x, gt, px, outside = restatement(J, encoding, frame, table, clips, out_rows, gt_rows)
    for got, want, rel in ((b["x"], x, 4 * 2.0 ** -23), (b["gt"], gt, 4 * 2.0 ** -23), (b["px"], px, 1e-12)):
        covered = ~np.isnan(want)
        assert (got[~covered] == FILL).all() and np.isfinite(got[covered]).all()
        assert (np.abs(got[covered] - want[covered]) <= rel * np.maximum(1.0, np.abs(want[covered]))).all()
    assert [int(v) - FILL_COUNT for v in b["outside"]] == outside and sum(outside) > 0
    xm = b["x"].copy()
    rows = ~(b["x"] == FILL).all(axis=(1, 2))
    xm[rows] = evaluate.mirror_input(torch.from_numpy(b["x"][rows].copy()), *KPS[J]).numpy()
    assert same_bits(b["xm"], xm)


@pytest.mark.parametrize("outputs", ["all", "none", "gt", "px", "count"])
def test_hook_optional_outputs_keep_the_other_bits(outputs):
    """Every optional output alone and none at all: what is written has the bits of the call that writes everything."""
    table, world, out_rows, max_rows, gt_rows, _ = layout(17)
    _, full = run_hook(17, "ray", table, world, out_rows, max_rows, gt_rows)
    kw = dict(mirror=outputs == "all", gt=outputs in ("all", "gt"), px=outputs in ("all", "px"), count=outputs in ("all", "count"))
    rc, b = run_hook(17, "ray", table, world, out_rows, max_rows, gt_rows, **kw)
    assert rc == 0 and not b["status"].any()
    for name, v in b.items():
        assert v is None or same_bits(v, full[name]), name
    # without gt and px, gt_first / gt_rows are not read: the same descriptors with a gt range of nonsense are followed
    if not (kw["gt"] or kw["px"]):
        t2 = table.copy()
        t2["gt_first"] = -5
        rc, b2 = run_hook(17, "ray", t2, world, out_rows, max_rows, 0, **kw)
        assert rc == 0 and not b2["status"].any() and same_bits(b2["x"], full["x"])


def test_hook_invalid_descriptors():
    """One invalid descriptor of each kind between the valid ones: status 1, nothing of it written - the valid ones' outputs have
    the bits of the table without the invalid ones, `outside` of an invalid descriptor stays what the caller put there."""
    table, world, out_rows, max_rows, gt_rows, _ = layout(17)
    _, clean = run_hook(17, "ray", table, world, out_rows, max_rows, gt_rows)
    t, bad = with_invalid(table, world.shape[0], out_rows, max_rows, gt_rows)
    assert len(bad) == len(invalid_cases(table, world.shape[0], out_rows, max_rows, gt_rows)) >= 6
    rc, b = run_hook(17, "ray", t, world, out_rows, max_rows, gt_rows)
    assert rc == 0 and b["status"].tolist() == [1 if k in bad else 0 for k in range(len(t))]
    for name in ("x", "xm", "gt", "px"):
        assert same_bits(b[name], clean[name]), name
    good = [k for k in range(len(t)) if k not in bad]
    assert b["outside"][good].tolist() == clean["outside"].tolist() and (b["outside"][bad] == FILL_COUNT).all()


def nonfinite_world(world, table):
    """`world` with NaN, +-Inf and a point in camera 0's plane (h2 == 0 up to rounding is not reachable by a float32 point in
    general: a zero third row of `proj` makes it exact) planted in the frames of descriptor 3 -> (world, table, touched (frame, joint))."""
    w = world.copy()
    f0 = int(table[3]["first_frame"])
    J = w.shape[1]
    touched = [(f0 + 1, 0 % J, 0, np.nan), (f0 + 2, 5 % J, 1, np.inf), (f0 + 3, 7 % J, 2, -np.inf)]
    for f, j, k, v in touched:
        w[f, j, k] = v
    return w, [(f, j) for f, j, _, _ in touched]


def test_hook_nonfinite_points_poison_only_their_own_outputs():
    """NaN / Inf world elements and a camera whose plane holds every point (h2 == 0): exactly the outputs that read them are
    non-finite, NaNs are the canonical quiet NaN, every other element keeps its bits; each such point counts as outside."""
    table, world, out_rows, max_rows, gt_rows, _ = layout(17)
    _, clean = run_hook(17, "ray", table, world, out_rows, max_rows, gt_rows)
    w, touched = nonfinite_world(world, table)
    t = table.copy()
    t[0]["proj"][8:12] = 0.0                               # descriptor 0 (one frame): h2 == 0 for every point, u = v = +-Inf
    rc, b = run_hook(17, "ray", t, w, out_rows, max_rows, gt_rows)
    assert rc == 0 and not b["status"].any()
    d3, d0 = table[3], table[0]
    users = [k for k in range(len(table)) if table[k]["first_frame"] == d3["first_frame"]]
    assert users == [3, 6]                                 # two cameras read the poisoned frames
    expect_bad = {name: np.zeros(clean[name].shape[:2], bool) for name in ("x", "gt", "px")}
    for k in users:
        d = table[k]
        for f, j in touched:
            rel = f - int(d["first_frame"])
            expect_bad["x"][int(d["out_first"]) + int(d["pad_front"]) + rel, j] = True
            expect_bad["gt"][int(d["gt_first"]) + rel, j] = True
            expect_bad["px"][int(d["gt_first"]) + rel, j] = True
    rows0 = int(d0["pad_front"] + d0["n_frames"] + d0["pad_back"])
    expect_bad["x"][int(d0["out_first"]):int(d0["out_first"]) + rows0] = True
    expect_bad["px"][int(d0["gt_first"])] = True
    for name in ("x", "gt", "px"):
        got, bad = b[name], expect_bad[name]
        assert (~np.isfinite(got)).any(axis=2)[bad].all(), name
        assert same_bits(got[~bad], clean[name][~bad]), name
        nan_bits = got[np.isnan(got)].view(np.int32 if got.dtype == np.float32 else np.int64)
        assert (nan_bits == (0x7fc00000 if got.dtype == np.float32 else 0x7ff8000000000000)).all(), name
    # the mirrored copy: the same points, at their mirrored joints
    perm = np.array(mirror_perm(17))
    assert np.array_equal(np.isfinite(b["xm"]), np.isfinite(b["x"][:, perm]))
    delta = (b["outside"] - clean["outside"]).tolist()
    res = 1000.0
    for k in users:                                        # (a touched point that was outside already adds nothing)
        g = int(table[k]["gt_first"]) - int(table[k]["first_frame"])
        was_inside = sum(bool((clean["px"][g + f, j] >= 0).all() and (clean["px"][g + f, j] <= res).all()) for f, j in touched)
        assert delta[k] == was_inside > 0, k
    assert delta[0] == 17 - (int(clean["outside"][0]) - FILL_COUNT)
    assert all(v == 0 for k, v in enumerate(delta) if k not in (0, 3, 6))


# ------------------------------------------------------------------ 4. the R3D_ERR_ARG table

def _hook_call(b, world_arr, table_arr, **over):
    lib = hooks_library()
    a = dict(world=ptr(world_arr), total=world_arr.shape[0], J=17, enc=0, table=ptr(table_arr), num_clips=table_arr.shape[0], max_rows=60, x=ptr(b["x"]),
             out_rows=b["x"].shape[0], xm=ptr(b["xm"]), perm=list(range(17)), gt=ptr(b["gt"]), px=ptr(b["px"]), gt_rows=b["gt"].shape[0],
             outside=ptr(b["outside"]), status=ptr(b["status"]))
    a.update(over)
    perm = (C.c_int32 * len(a["perm"]))(*a["perm"]) if a["perm"] is not None else None
    return lib.r3d_debug_clips_project_host(a["world"], a["total"], a["J"], a["enc"], a["table"], a["num_clips"], a["max_rows"], a["x"],
                                            a["out_rows"], a["xm"], perm, a["gt"], a["px"], a["gt_rows"], a["outside"], a["status"])


ARG_CASES = [
    (dict(world=None), "null pointer"), (dict(table=None), "null pointer"), (dict(x=None), "null pointer"), (dict(status=None), "null pointer"),
    (dict(num_clips=0), "num_clips"), (dict(num_clips=65536), "num_clips"),
    (dict(J=0), "num_joints"), (dict(J=18), "num_joints"),
    (dict(enc=3), "encoding"), (dict(enc=-1), "encoding"),
    (dict(max_rows=0), "max_rows"), (dict(total=0), "total_frames"), (dict(out_rows=-2), "out_rows"),
    (dict(max_rows=2 ** 31 // 17), "must not exceed"), (dict(total=2 ** 31), "must not exceed"), (dict(out_rows=2 ** 40), "must not exceed"),
    (dict(xm=None), "go together"), (dict(perm=None), "go together"),
    (dict(perm=[0] * 17), "permutation"), (dict(perm=list(range(1, 18))), "permutation"),
    (dict(table="+4"), "8-byte aligned"),
    (dict(gt_rows=0), "gt_rows"), (dict(gt_rows=-1, gt=None), "gt_rows"), (dict(gt_rows=0, px=None), "gt_rows"), (dict(gt_rows=2 ** 31), "gt_rows"),
    (dict(px="+4"), "px_dev must be 8-byte aligned"),
]


@pytest.mark.parametrize("over,message", ARG_CASES, ids=["%s-%d" % (m.split()[0], i) for i, (_, m) in enumerate(ARG_CASES)])
def test_err_arg_rules_and_nothing_written(over, message):
    """Every rule of clips_project_check_args once (those shared with r3d_clips_encode and the call's own): R3D_ERR_ARG, the
    message names the rule, and no output buffer - status and outside included - has a byte changed."""
    table, world, out_rows, max_rows, gt_rows, _ = layout(17)
    table, world = np.ascontiguousarray(table), np.ascontiguousarray(world)
    ok = host_buffers(17, "ray", table.shape[0], out_rows, gt_rows)
    assert _hook_call(ok, world, table, max_rows=max_rows) == 0                  # the unedited call is valid ...
    b = host_buffers(17, "ray", table.shape[0], out_rows, gt_rows)
    before = {k: v.copy() for k, v in b.items()}
    over = dict(dict(max_rows=max_rows), **over)
    for name, arr in (("table", table), ("px", b["px"])):
        if over.get(name) == "+4":
            over[name] = C.c_void_p(arr.ctypes.data + 4)
    assert _hook_call(b, world, table, **over) == _capi.R3D_ERR_ARG             # ... and the edited one is refused
    assert message in hooks_library().r3d_last_error().decode()
    for k, v in b.items():
        assert same_bits(v, before[k]), k


def test_err_arg_of_the_device_entry_point_without_a_device():
    """The product library's r3d_clips_project runs the same rules before any HIP call: bogus non-null pointers are never followed."""
    lib = _capi.load()
    perm = (C.c_int32 * 17)(*range(17))

    def call(**over):
        a = dict(world=BOGUS, total=100, J=17, enc=0, table=BOGUS, n=3, max_rows=60, x=BOGUS, out_rows=500, xm=BOGUS, perm=perm, gt=BOGUS,
                 px=BOGUS, gt_rows=100, outside=BOGUS, status=BOGUS)
        a.update(over)
        return lib.r3d_clips_project(a["world"], a["total"], a["J"], a["enc"], a["table"], a["n"], a["max_rows"], a["x"], a["out_rows"], a["xm"],
                                     a["perm"], a["gt"], a["px"], a["gt_rows"], a["outside"], a["status"], None)
    for over, message in ((dict(world=None), "null pointer"), (dict(n=0), "num_clips"), (dict(enc=7), "encoding"), (dict(perm=None), "go together"),
                          (dict(gt_rows=0), "gt_rows"), (dict(px=BOGUS + 4), "px_dev"), (dict(table=BOGUS + 4), "8-byte aligned")):
        assert call(**over) == _capi.R3D_ERR_ARG, over
        assert message in lib.r3d_last_error().decode(), over
    with pytest.raises(_capi.Ray3DHipError, match="mirror_perm has 3 entries"):
        _capi.clips_project(BOGUS, 100, 17, 0, BOGUS, 3, 60, BOGUS, 500, BOGUS, [0, 1, 2], BOGUS, BOGUS, 100, BOGUS, BOGUS, 0)
