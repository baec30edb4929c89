"""CPU suite: the host side of r3d_clips_poses (a shard's finished poses - flip average and world coordinates - in one call) - the
argument checks (all made before any device call: they run without a GPU), the host hook r3d_debug_clips_poses_host (the call's
validation, descriptor rule and per-point routines on the CPU) against a NumPy restatement written here, invalid descriptors,
the stated extents, forward_clip(raw_out=) on a stand-in and evaluate.clip_raw_table.  tests/test_gpu_clips_poses.py runs the
kernel on the shards built here."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, hooks_library

from ray3d_amd import _capi, evaluate
from test_clips_encode_host import KPS, cameras

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
FILL = np.float32(-7.0)      # what the output buffers hold before a call: rows outside every clip must keep it
JOINTS = (1, 14, 17)
# Clip lengths 1, 2, 15, 16 (with J = 17: 255 and 272 points, either side of a workgroup edge) and 40; the raw rows each clip owns
# behind its frames (the surplus of rounded-up call sizes, never read); max_frames larger than every clip.
LENGTHS = (1, 2, 15, 16, 40)
SURPLUS = (0, 2, 1, 0, 24)
MAX_FRAMES = 41
GAP_RAW, GAP_OUT = 3, 2      # raw rows / output rows between stored clips that belong to no clip
EPS64 = 2.0 ** -53


def _define(name):
    return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, HDR).group(1))


def mirror_perm(J):
    return [0] if J == 1 else evaluate.mirror_permutation(J, *KPS[J])


def transforms():
    """(R (3,3), T (3,)) per clip, from the cameras of tests/golden/cameras.npz: normalised-frame clips (Rn2w / Tn2w), one
    camera-frame clip (Rc2w / Tc2w) and one root-relative clip (the identity)."""
    cams = cameras()
    pairs = [(cams[0].Rn2w, cams[0].Tn2w), (cams[1].Rc2w, cams[1].Tc2w), (np.eye(3), np.zeros(3)), (cams[2].Rn2w, cams[2].Tn2w),
             (cams[3].Rn2w, cams[3].Tn2w)]
    return [(np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3)) for R, T in pairs]


# (raw, mirrored-pass value) planted into all three components of one point each: signed zeros, subnormals, sums that overflow
# (component 0 adds the NEGATED mirrored value), then NaN and +-Inf on either side
FINITE_SPECIALS = ((0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (1e-45, 1e-45), (5e-39, -3e-39), (-1e-45, 3e-45), (3e38, 3e38), (3e38, -3e38),
                   (-3.4e38, -3.4e38), (1.17549435e-38, 1e-45))
NONFINITE_SPECIALS = ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (-np.inf, np.inf), (1.0, -np.inf), (np.nan, np.inf))


@functools.lru_cache(maxsize=None)
def layout(J, nonfinite=True):
    """A shard of the clips above: their raw rows stored in a shuffled order, NaN in the gaps and in the surplus rows (nothing may
    read them); their output rows in another shuffled order with gaps; the table names them in LENGTHS order.  The longest clip
    carries the special values.  -> (table, raw_first (int64), raw, raw_mirror, raw_rows, total_frames)."""
    rng = np.random.default_rng(23 + J)
    k = len(LENGTHS)
    src_order, out_order = rng.permutation(k), rng.permutation(k)
    raw_first, at = np.zeros(k, np.int64), GAP_RAW
    for c in src_order:
        raw_first[c] = at
        at += LENGTHS[c] + SURPLUS[c] + GAP_RAW
    raw_rows = at
    first, at = np.zeros(k, np.int64), GAP_OUT
    for c in out_order:
        first[c] = at
        at += LENGTHS[c] + GAP_OUT
    total = at
    assert list(raw_first) != sorted(raw_first) and list(first) != sorted(first)          # really out of order
    raw = np.full((raw_rows, J, 3), np.nan, np.float32)
    raw_m = np.full((raw_rows, J, 3), np.nan, np.float32)
    table = np.zeros(k, dtype=_capi.clip_desc_dtype())
    perm = mirror_perm(J)
    for c, n in enumerate(LENGTHS):
        rows = slice(raw_first[c], raw_first[c] + n)
        raw[rows] = (2.0 * rng.standard_normal((n, J, 3))).astype(np.float32)
        raw_m[rows] = (2.0 * rng.standard_normal((n, J, 3))).astype(np.float32)
        R, T = transforms()[c]
        table[c]["first_frame"], table[c]["n_frames"], table[c]["rn2w"], table[c]["tn2w"] = first[c], n, R.reshape(9), T
    with np.errstate(over="ignore"):
        for f, (a, b) in enumerate(FINITE_SPECIALS + (NONFINITE_SPECIALS if nonfinite else ())):
            j = f % J
            raw[raw_first[4] + f, j] = np.float32(a)
            raw_m[raw_first[4] + f, perm[j]] = np.float32(b)
    for v in (raw, raw_m, table, raw_first):
        v.setflags(write=False)
    return table, raw_first, raw, raw_m, raw_rows, total


def restatement(J, mirror, nonfinite=True):
    """NumPy, float32 arithmetic in the stated order: p = fl32(fl32(raw + m) * 0.5f) with m the mirrored pass's point of joint
    perm[j], component 0 negated - or the raw value; world = p.astype(float64) @ R.T + T.T (the reference's normalized2world) with
    its bound per component, 8 * 2^-53 * (sum_k |R_rk||p_k| + |T_r|): at most four roundings on each side.
    -> (pred, world, bound, covered rows)."""
    table, raw_first, raw, raw_m, _, total = layout(J, nonfinite)
    pred = np.full((total, J, 3), FILL, np.float32)
    world = np.full((total, J, 3), float(FILL), np.float64)
    bound = np.zeros((total, J, 3), np.float64)
    covered = np.zeros(total, bool)
    perm = mirror_perm(J)
    with np.errstate(over="ignore", invalid="ignore"):
        for c, d in enumerate(table):
            n, rf = int(d["n_frames"]), int(raw_first[c])
            p = raw[rf:rf + n].copy()
            if mirror:
                m = raw_m[rf:rf + n][:, perm].copy()
                m[..., 0] = -m[..., 0]
                p = (p + m).astype(np.float32) * np.float32(0.5)
                assert p.dtype == np.float32
            R, T = d["rn2w"].reshape(3, 3), d["tn2w"]
            p64 = p.astype(np.float64)
            rows = slice(int(d["first_frame"]), int(d["first_frame"]) + n)
            pred[rows] = p
            world[rows] = p64 @ R.T + T.reshape(1, 1, 3)
            bound[rows] = 8 * EPS64 * (np.abs(p64) @ np.abs(R).T + np.abs(T).reshape(1, 1, 3))
            covered[rows] = True
    return pred, world, bound, covered


def ptr(a):
    return a.ctypes.data_as(C.c_void_p).value if a is not None else None


def run_hook(J, table, raw_first, raw, raw_m, total, mirror=True, want_pred=True, want_world=True, max_frames=MAX_FRAMES, raw_rows=None):
    """r3d_debug_clips_poses_host on host arrays pre-filled with FILL -> (rc, pred or None, world or None, status)."""
    hooks_library()
    table, raw_first, raw = np.ascontiguousarray(table), np.ascontiguousarray(raw_first, dtype=np.int64), np.ascontiguousarray(raw)
    raw_m = np.ascontiguousarray(raw_m) if mirror else None
    pred = np.full((total, J, 3), FILL, np.float32) if want_pred else None
    world = np.full((total, J, 3), float(FILL), np.float64) if want_world else None
    status = np.full(table.shape[0], -1, np.int32)
    rc = _capi.debug_clips_poses_host(ptr(raw), ptr(raw_m), raw.shape[0] if raw_rows is None else raw_rows, J,
                                      mirror_perm(J) if mirror else None, ptr(table), ptr(raw_first), table.shape[0], max_frames,
                                      ptr(pred), ptr(world), total, ptr(status))
    return rc, pred, world, status


def same_bits(a, b):
    w = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(w), b.view(w))


def same_positions_and_bits(got, want):
    """Non-finite values at the same positions, the same bits everywhere else."""
    bad = ~np.isfinite(want)
    return np.array_equal(~np.isfinite(got), bad) and same_bits(np.where(bad, 0, got).astype(got.dtype), np.where(bad, 0, want).astype(want.dtype))


# ------------------------------------------------------------------ 1. binding and the host-checked errors

def test_entry_points_are_declared_and_bound():
    assert "r3d_clips_poses" in _capi.EXPORTS and "r3d_debug_clips_poses_host" in _capi.HOOK_EXPORTS
    assert hasattr(_capi.load(), "r3d_clips_poses") and not hasattr(_capi.load(), "r3d_debug_clips_poses_host")
    assert hasattr(hooks_library(), "r3d_debug_clips_poses_host") and hasattr(hooks_library(), "r3d_clips_poses")
    assert re.search(r"int r3d_clips_poses\(", HDR) and re.search(r"int r3d_debug_clips_poses_host\(", HDR)
    assert _define("R3D_ABI_VERSION") == _capi.ABI_VERSION == 6          # no struct changed
    assert callable(_capi.clips_poses) and callable(evaluate.shard_poses_hip) and callable(evaluate.predict_clips_batched)


B = 1 << 30     # bogus, 8-byte aligned "device pointers", never followed; a gigabyte apart: no extent of the call below overlaps


def _call(**over):
    """r3d_clips_poses with bogus non-null pointers and otherwise valid arguments; -> the return code."""
    a = dict(raw=B, rawm=2 * B, raw_rows=2000, J=17, perm=list(range(17)), table=3 * B, raw_first=4 * B, num_clips=3, max_frames=600,
             pred=5 * B, world=6 * B, total=1000, status=7 * B, stream=0)
    a.update(over)
    perm = (C.c_int32 * len(a["perm"]))(*a["perm"]) if a["perm"] is not None else None
    return _capi.load().r3d_clips_poses(a["raw"], a["rawm"], a["raw_rows"], a["J"], perm, a["table"], a["raw_first"], a["num_clips"],
                                        a["max_frames"], a["pred"], a["world"], a["total"], a["status"], a["stream"])


IN_BYTES, PRED_BYTES, WORLD_BYTES = 2000 * 17 * 12, 1000 * 17 * 12, 1000 * 17 * 24
ARG_CASES = [
    (dict(raw=None), "null pointer"), (dict(table=None), "null pointer"), (dict(raw_first=None), "null pointer"), (dict(status=None), "null pointer"),
    (dict(pred=None, world=None), "both null"),
    (dict(rawm=None), "go together"), (dict(perm=None), "go together"),
    (dict(perm=[0] * 17), "permutation"), (dict(perm=list(range(1, 18))), "permutation"), (dict(perm=[-1] + list(range(1, 17))), "permutation"),
    (dict(num_clips=0), "num_clips"), (dict(num_clips=-3), "num_clips"), (dict(num_clips=65536), "num_clips"),
    (dict(J=0), "num_joints"), (dict(J=18), "num_joints"),
    (dict(max_frames=0), "max_frames"), (dict(total=0), "total_frames"), (dict(total=-1), "total_frames"), (dict(raw_rows=0), "raw_rows"),
    (dict(raw_rows=-2), "raw_rows"),
    (dict(max_frames=2 ** 31 // 17), "must not exceed"), (dict(total=2 ** 31), "must not exceed"), (dict(raw_rows=2 ** 40), "must not exceed"),
    (dict(table=3 * B + 4), "8-byte aligned"), (dict(raw_first=4 * B + 4), "8-byte aligned"), (dict(world=6 * B + 4), "8-byte aligned"),
    (dict(pred=B), "overlaps"), (dict(pred=B + IN_BYTES - 4), "overlaps"), (dict(pred=B - PRED_BYTES + 4), "overlaps"),
    (dict(pred=2 * B + 12), "overlaps"), (dict(world=B + 8), "overlaps"), (dict(world=2 * B - WORLD_BYTES + 8), "overlaps"),
    (dict(world=2 * B, pred=None), "overlaps"),
]


@pytest.mark.parametrize("over,word", ARG_CASES, ids=["-".join("%s=%s" % kv for kv in o.items()) for o, _ in ARG_CASES])
def test_bad_arguments_return_err_arg_before_any_device_call(over, word):
    """Bogus pointers: the call must decide on the host.  (Without a GPU a launch would fail with R3D_ERR_HIP, with one it
    would fault: R3D_ERR_ARG shows that neither was tried.)"""
    assert _call(**over) == _capi.R3D_ERR_ARG
    assert word in _capi.load().r3d_last_error().decode()


def test_the_binding_refuses_a_short_permutation():
    with pytest.raises(_capi.Ray3DHipError, match="mirror_perm"):
        _capi.clips_poses(B, 2 * B, 10, 17, list(range(14)), 3 * B, 4 * B, 1, 10, 5 * B, None, 10, 7 * B, 0)
    with pytest.raises(_capi.Ray3DHipError, match="go together"):
        _capi.clips_poses(B, None, 10, 17, list(range(17)), 3 * B, 4 * B, 1, 10, 5 * B, None, 10, 7 * B, 0)


# ------------------------------------------------------------------ 2. the hook against the NumPy restatement

@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("J", JOINTS)
def test_hook_equals_the_numpy_restatement(J, mirror):
    """pred bit for bit (non-finite values: at the same positions); world within 8 * 2^-53 * (sum |R||p| + |T|) of
    pred.astype(float64) @ R.T + T.T; rows outside every clip keep their fill; +-0, subnormals, overflowing sums, NaN, +-Inf."""
    table, raw_first, raw, raw_m, raw_rows, total = layout(J)
    want, want_w, bound, covered = restatement(J, mirror)
    rc, pred, world, status = run_hook(J, table, raw_first, raw, raw_m, total, mirror)
    assert rc == 0 and not status.any()
    assert 0 < (~covered).sum() and (pred[~covered] == FILL).all() and (world[~covered] == float(FILL)).all()
    assert same_positions_and_bits(pred, want)
    if not mirror:
        assert same_bits(pred[covered], want[covered])                  # a copy: NaN payloads included
    assert np.isinf(want).any() and np.isnan(want).any() and (np.abs(want[np.isfinite(want) & (want != 0)]) < 1e-38).any()
    assert (np.signbit(want) & (want == 0)).any(), "a negative zero among the results"
    # world: the points with a non-finite component are non-finite in all three, the others inside the bound
    bad = ~np.isfinite(want).all(axis=-1)
    assert not np.isfinite(world[bad]).any() and np.isfinite(world[~bad]).all()
    err = np.abs(world[~bad] - want_w[~bad])
    print("J %d mirror %d: worst world error / bound %.3f" % (J, mirror, float((err / np.maximum(bound[~bad], 1e-300)).max())))
    assert (err <= bound[~bad]).all()
    # world alone, pred alone: the same bits as together
    rc, none, world2, _ = run_hook(J, table, raw_first, raw, raw_m, total, mirror, want_pred=False)
    assert rc == 0 and none is None and same_bits(world2, world)
    rc, pred2, none, _ = run_hook(J, table, raw_first, raw, raw_m, total, mirror, want_world=False)
    assert rc == 0 and none is None and same_bits(pred2, pred)


def test_hook_nan_results_are_canonical():
    """What the arithmetic makes NaN leaves as the canonical quiet NaN, so that the kernel and the hook can be held to the same bits."""
    table, raw_first, raw, raw_m, _, total = layout(17)
    _, pred, world, _ = run_hook(17, table, raw_first, raw, raw_m, total, True)
    assert set(pred.view(np.uint32)[np.isnan(pred)].tolist()) == {0x7fc00000}
    assert set(world.view(np.uint64)[np.isnan(world)].tolist()) == {0x7ff8000000000000}


# ------------------------------------------------------------------ 3. invalid descriptors

def invalid_cases(total, raw_rows):
    """(what, fields of a valid descriptor to overwrite, raw_first or None): each of the five conditions, and ranges far outside."""
    big = 2 ** 62
    return [("n_frames < 1", dict(n_frames=0), None), ("n_frames < 1", dict(n_frames=-4), None),
            ("n_frames > max_frames", dict(n_frames=MAX_FRAMES + 1, first_frame=0), 0), ("n_frames > max_frames", dict(n_frames=big), None),
            ("output outside", dict(first_frame=-1), None), ("output outside", dict(first_frame=total - 15), None),
            ("output outside", dict(first_frame=big), None), ("output outside", dict(first_frame=-big), None),
            ("raw_first < 0", {}, -1), ("raw_first < 0", {}, -big),
            ("raw outside", {}, raw_rows - 15), ("raw outside", {}, raw_rows), ("raw outside", {}, big)]


@pytest.mark.parametrize("J", [17, 1])
def test_hook_invalid_descriptors_are_not_followed(J):
    """Each condition in turn in clip 3 (16 frames) of a table that also has valid clips: status 1, nothing of the clip written,
    the other clips bit-identical to a table without it."""
    table, raw_first, raw, raw_m, raw_rows, total = layout(J)
    keep = [0, 1, 2, 4]
    rc, ref, ref_w, status = run_hook(J, table[keep], raw_first[keep], raw, raw_m, total)
    assert rc == 0 and not status.any()
    rows = slice(int(table[3]["first_frame"]), int(table[3]["first_frame"]) + 16)
    assert (ref[rows] == FILL).all() and (ref_w[rows] == float(FILL)).all()
    seen = set()
    for what, over, rf in invalid_cases(total, raw_rows):
        t, r = np.array(table), np.array(raw_first)
        for name, v in over.items():
            t[3][name] = v
        if rf is not None:
            r[3] = rf
        rc, pred, world, status = run_hook(J, t, r, raw, raw_m, total)
        assert rc == 0 and status.tolist() == [0, 0, 0, 1, 0], what
        assert same_bits(pred, ref) and same_bits(world, ref_w), what
        seen.add(what)
    assert seen == {"n_frames < 1", "n_frames > max_frames", "output outside", "raw_first < 0", "raw outside"}


# ------------------------------------------------------------------ 4. extents

def test_hook_bounds_are_the_stated_extents_exactly():
    """Clips that end on the last raw row and on the last output row are followed - from allocations that end there, between
    guard bands the call must neither read (NaN: a read would show in the outputs) nor write - and one row more is not."""
    J, G = 3, 64
    rng = np.random.default_rng(5)
    raw_rows, total = 9, 7
    store = np.full((2, G + raw_rows * J * 3 + G), np.nan, np.float32)
    raws = [s[G:G + raw_rows * J * 3].reshape(raw_rows, J, 3) for s in store]
    for r in raws:
        r[:] = rng.standard_normal(r.shape).astype(np.float32)
    out32 = np.full(G + total * J * 3 + G, FILL, np.float32)
    out64 = np.full(G + total * J * 3 + G, float(FILL), np.float64)
    pred, world = out32[G:G + total * J * 3].reshape(total, J, 3), out64[G:G + total * J * 3].reshape(total, J, 3)
    table = np.zeros(2, dtype=_capi.clip_desc_dtype())
    table[0]["first_frame"], table[0]["n_frames"] = 0, 6
    table[1]["first_frame"], table[1]["n_frames"] = 6, 1
    for c in range(2):
        table[c]["rn2w"], table[c]["tn2w"] = transforms()[c][0].reshape(9), transforms()[c][1]
    raw_first = np.array([3, 0], np.int64)          # clip 0 ends on raw row 8, the last one; clip 1 on output row 6, the last one
    status = np.full(2, -1, np.int32)
    perm = [2, 1, 0]
    hooks_library()

    def call(max_frames=6, rr=raw_rows, tot=total):
        out32[:], out64[:], status[:] = FILL, float(FILL), -1
        return _capi.debug_clips_poses_host(ptr(raws[0]), ptr(raws[1]), rr, J, perm, ptr(table), ptr(raw_first), 2, max_frames,
                                            ptr(pred), ptr(world), tot, ptr(status))
    assert call() == 0 and status.tolist() == [0, 0]
    assert np.isfinite(pred).all() and np.isfinite(world).all() and (pred != FILL).all()
    for o, fill in ((out32, FILL), (out64, float(FILL))):
        assert (o[:G] == fill).all() and (o[-G:] == fill).all()
    assert call(max_frames=5) == 0 and status.tolist() == [1, 0] and (pred[:6] == FILL).all() and (pred[6] != FILL).all()
    assert call(rr=8) == 0 and status.tolist() == [1, 0] and (world[:6] == float(FILL)).all()        # raw_rows one short of clip 0
    assert call(tot=6) == 0 and status.tolist() == [0, 1] and (pred[6] == FILL).all()                 # total_frames one short of clip 1
    # outputs that END where an input begins, and begin where one ends, do not overlap it: no R3D_ERR_ARG
    flat = np.zeros(4 * J * 3 * 3, np.float32)
    a, b, c = (flat[i * 4 * J * 3:(i + 1) * 4 * J * 3].reshape(4, J, 3) for i in range(3))
    b[:] = 1.5
    t1 = np.zeros(1, dtype=_capi.clip_desc_dtype())
    t1[0]["n_frames"], t1[0]["rn2w"] = 4, np.eye(3).reshape(9)
    for dst in (a, c):
        assert _capi.debug_clips_poses_host(ptr(b), None, 4, J, None, ptr(t1), ptr(np.zeros(1, np.int64)), 1, 4, ptr(dst), None, 4,
                                            ptr(status)) == 0
        assert (dst == 1.5).all()
    assert _capi.debug_clips_poses_host(ptr(b), None, 4, J, None, ptr(t1), ptr(np.zeros(1, np.int64)), 1, 4, ptr(b[1:]), None, 3,
                                        ptr(status)) == _capi.R3D_ERR_ARG


# ------------------------------------------------------------------ 5. forward_clip(raw_out=) and clip_raw_table

class _Recorder:
    """Ray3DLifter.forward_clip on a stand-in: _run records (rows of the clip it was handed, batch size, where it wrote)."""

    def __init__(self):
        import ray3d_amd
        self.calls = []
        self.pos = types.SimpleNamespace(num_joints_in=17, in_features=3, camera_embedding=False)
        for name in ("clip_batch_sizes", "forward_clip", "_forward_clip_into", "_forward_clip_raw"):
            setattr(self, name, types.MethodType(getattr(ray3d_amd.Ray3DLifter, name), self))
        self.CLIP_CHUNK, self.CLIP_ROUND, self.CLIP_BALANCED = 4096, 128, True

    def receptive_field(self):
        return 27

    def join_lanes(self):
        raise AssertionError("forward_clip(raw_out=) never joins")

    def _lane_of_current_stream(self, dev):
        return None

    def _run(self, mode, x, stride, B, p, pstride, return_trj=False, out=None, out_trj=None):
        assert stride == 1 and x.shape[0] >= B + 26
        self.calls.append((x[:B + 26].clone(), B, None if out is None else out.data_ptr(), None if out_trj is None else out_trj.data_ptr()))
        if out is None:
            out = torch.zeros((B, 1, 17, 3))
        out[:] = x[13:13 + B, :, :].reshape(B, 1, 17, 3)          # "the pose of window i is the frame in its middle"
        if return_trj:
            if out_trj is None:
                out_trj = torch.zeros((B, 1, 1, 3))
            out_trj[:] = x[13:13 + B, :1, :].reshape(B, 1, 1, 3)
            return out, out_trj
        return out


@pytest.mark.parametrize("n", [1, 40, 65, 100, 128, 300, 5000])
def test_forward_clip_raw_out_runs_the_same_forwards_straight_into_its_rows(n, monkeypatch):
    lifter = _Recorder()
    lifter.join_lanes = lambda: None
    sizes = lifter.clip_batch_sizes(n)
    total = sum(sizes)
    padded = torch.from_numpy(np.random.default_rng(n).standard_normal((n + 26, 17, 3)).astype(np.float32))
    full = torch.cat([padded, padded[-1:].expand(total - n, -1, -1)], dim=0)
    want, want_trj = lifter.forward_clip(padded, return_trj=True, out=torch.zeros((n, 1, 17, 3)))
    calls, lifter.calls = lifter.calls, []
    lifter.join_lanes = _Recorder.join_lanes.__get__(lifter)
    raw, raw_trj = torch.full((total, 1, 17, 3), -7.0), torch.full((total, 1, 1, 3), -7.0)
    # no scratch tensor, no concatenation: neither torch.empty nor torch.cat may be called
    for name in ("empty", "cat", "zeros"):
        monkeypatch.setattr(torch, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("forward_clip(raw_out=) allocated")))
    got = lifter.forward_clip(full, return_trj=True, raw_out=raw, raw_trj_out=raw_trj, n_windows=n)
    monkeypatch.undo()
    assert got[0] is raw and got[1] is raw_trj
    assert [c[1] for c in lifter.calls] == [c[1] for c in calls] == sizes                       # the same call sizes
    assert all(torch.equal(a[0], b[0]) for a, b in zip(lifter.calls, calls))                    # on the same values
    starts = [sum(sizes[:i]) for i in range(len(sizes))]
    assert [c[2] for c in lifter.calls] == [raw.data_ptr() + s * 17 * 3 * 4 for s in starts]    # the same destinations: its rows
    assert [c[3] for c in lifter.calls] == [raw_trj.data_ptr() + s * 3 * 4 for s in starts]
    assert torch.equal(raw[:n], want) and torch.equal(raw_trj[:n], want_trj) and (raw != -7.0).all()
    # without n_windows the clip is padded as out= pads it; without return_trj the poses alone
    lifter.calls = []
    raw2 = torch.zeros((total, 1, 17, 3))
    assert lifter.forward_clip(padded, raw_out=raw2) is raw2 and torch.equal(raw2, raw)
    assert all(c[3] is None for c in lifter.calls)


def test_forward_clip_raw_out_refuses_other_shapes_and_combinations():
    lifter = _Recorder()
    n = 100
    total = sum(lifter.clip_batch_sizes(n))
    assert total == 128
    padded = torch.zeros((n + 26, 17, 3))
    for bad in (torch.zeros((n, 1, 17, 3)), torch.zeros((total, 17, 3)), torch.zeros((total, 1, 17, 3), dtype=torch.float64),
                torch.zeros((total + 1, 1, 17, 3)), torch.zeros((total, 1, 17, 6))[..., ::2], torch.zeros((total, 1, 17, 3), device="meta")):
        with pytest.raises(ValueError, match="raw_out"):
            lifter.forward_clip(padded, raw_out=bad)
    with pytest.raises(ValueError, match="raw_trj_out"):
        lifter.forward_clip(padded, return_trj=True, raw_out=torch.zeros((total, 1, 17, 3)), raw_trj_out=torch.zeros((n, 1, 1, 3)))
    with pytest.raises(ValueError, match="return_trj"):
        lifter.forward_clip(padded, raw_out=torch.zeros((total, 1, 17, 3)), raw_trj_out=torch.zeros((total, 1, 1, 3)))
    with pytest.raises(ValueError, match="one kind"):
        lifter.forward_clip(padded, out=torch.zeros((n, 1, 17, 3)), raw_out=torch.zeros((total, 1, 17, 3)))
    with pytest.raises(ValueError, match="one kind"):
        lifter.forward_clip(padded, return_trj=True, trj_out=torch.zeros((n, 1, 1, 3)), raw_out=torch.zeros((total, 1, 17, 3)))
    assert lifter.calls == []


def test_clip_raw_table_reproduces_the_sums_of_clip_batch_sizes():
    lifter = _Recorder()
    lengths = [5, 1, 300, 77, 128, 5000]
    raw_first, raw_rows = evaluate.clip_raw_table(lengths, lifter.clip_batch_sizes)
    sums = [sum(lifter.clip_batch_sizes(n)) for n in lengths]
    assert sums == [8, 1, 384, 128, 128, 5120]
    assert raw_first == [sum(sums[:k]) for k in range(len(lengths))] and raw_rows == sum(sums)
    assert evaluate.clip_raw_table([], lifter.clip_batch_sizes) == ([], 0)


def test_finish_and_predict_refuse_a_lift_clip_that_is_no_lifters_forward_clip():
    """Decided before any shard is cut or the device is touched beyond its name: every rank raises alike."""
    with pytest.raises(ValueError, match="bound forward_clip"):
        evaluate.evaluate_clips_batched(lambda *a, **k: None, [], 27, "cuda", finish=True)
    with pytest.raises(ValueError, match="bound forward_clip"):
        evaluate.predict_clips_batched(lambda *a, **k: None, [], 27, "cuda")
