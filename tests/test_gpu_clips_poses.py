"""GPU suite: r3d_clips_poses (a shard's finished poses - flip average and world coordinates - in one launch) on the shards of
tests/test_clips_poses_host.py: the kernel against the host hook and against the torch sequence it replaces, bit for bit; guard
bands, surplus rows, gaps and non-finite inputs; evaluate_clips_batched(finish=True), predict_clips_batched and hipGraph capture.
Shapes of a few hundred frames at most."""
import functools

import numpy as np
import pytest
import torch

from buffers_util import NANS, Arena
from ray3d_amd import _capi, evaluate
from test_clips_encode_host import KPS
from test_clips_poses_host import (EPS64, FILL, JOINTS, MAX_FRAMES, invalid_cases, layout, mirror_perm, run_hook, same_bits)

pytestmark = pytest.mark.gpu

H36M_LEFT, H36M_RIGHT = KPS[17]


@functools.lru_cache(maxsize=None)
def hook(J, mirror, nonfinite=True):
    """(pred, world, status) of the host hook on `layout` (the product library is selected again afterwards)."""
    table, raw_first, raw, raw_m, _, total = layout(J, nonfinite)
    rc, pred, world, status = run_hook(J, table, raw_first, raw, raw_m, total, mirror)
    _capi.use_hooks(False)
    assert rc == 0
    return pred, world, status


def run_device(J, table, raw_first, raw, raw_m, total, mirror=True, want_pred=True, want_world=True, max_frames=MAX_FRAMES):
    """evaluate.shard_poses_hip on device buffers pre-filled with FILL -> (pred or None, world or None, status) as NumPy arrays."""
    dev = torch.device("cuda:0")
    tab = torch.from_numpy(np.array(table).view(np.uint8)).to(dev)            # (copies: the cached layout is read-only)
    rf = torch.from_numpy(np.array(raw_first, dtype=np.int64)).to(dev)
    pred = torch.full((total, J, 3), float(FILL), dtype=torch.float32, device=dev) if want_pred else None
    world = torch.full((total, J, 3), float(FILL), dtype=torch.float64, device=dev) if want_world else None
    status = torch.full((len(table),), -1, dtype=torch.int32, device=dev)
    p, w, s = evaluate.shard_poses_hip(torch.from_numpy(np.array(raw)).to(dev), tab, rf, len(table), total, max_frames,
                                       torch.from_numpy(np.array(raw_m)).to(dev) if mirror else None,
                                       mirror_perm(J) if mirror else None, pred=want_pred, world=want_world, pred_all=pred,
                                       world_all=world, status=status)
    torch.cuda.synchronize()
    assert (p is None) == (not want_pred) and (w is None) == (not want_world) and s is status
    return (p.cpu().numpy() if p is not None else None), (w.cpu().numpy() if w is not None else None), s.cpu().numpy()


# ------------------------------------------------------------------ 6. the device against the host hook

@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("J", JOINTS)
def test_device_equals_the_host_hook_bit_for_bit(J, mirror):
    """Clips of 1, 2, 15, 16 and 40 frames out of order with gaps in both layouts, NaN in the surplus rows; +-0, subnormals,
    overflowing sums, NaN and +-Inf among the values; pred only, world only and both."""
    table, raw_first, raw, raw_m, _, total = layout(J)
    want, want_w, _ = hook(J, mirror)
    pred, world, status = run_device(J, table, raw_first, raw, raw_m, total, mirror)
    assert not status.any()
    assert same_bits(pred, want) and same_bits(world, want_w)
    pred2, none, status = run_device(J, table, raw_first, raw, raw_m, total, mirror, want_world=False)
    assert none is None and not status.any() and same_bits(pred2, want)
    none, world2, status = run_device(J, table, raw_first, raw, raw_m, total, mirror, want_pred=False)
    assert none is None and not status.any() and same_bits(world2, want_w)


def test_device_invalid_descriptors_equal_the_host_hook():
    """Every kind of invalid descriptor in clip 3: status 1, the outputs those of the hook - the clip's rows keep their fill."""
    J = 17
    table, raw_first, raw, raw_m, raw_rows, total = layout(J)
    for what, over, rf in invalid_cases(total, raw_rows):
        t, r = np.array(table), np.array(raw_first)
        for name, v in over.items():
            t[3][name] = v
        if rf is not None:
            r[3] = rf
        rc, want, want_w, want_s = run_hook(J, t, r, raw, raw_m, total)
        _capi.use_hooks(False)
        pred, world, status = run_device(J, t, r, raw, raw_m, total)
        assert rc == 0 and status.tolist() == want_s.tolist() == [0, 0, 0, 1, 0], what
        assert same_bits(pred, want) and same_bits(world, want_w), what
        rows = slice(int(table[3]["first_frame"]), int(table[3]["first_frame"]) + 16)
        assert (pred[rows] == FILL).all() and (world[rows] == float(FILL)).all(), what


# ------------------------------------------------------------------ 7. the device against the torch sequence it replaces

@pytest.mark.parametrize("J", JOINTS)
def test_device_equals_the_torch_sequence_bit_for_bit(J):
    """torch.add(dst, mirror_output(pred_m, jl, jr), out=dst); dst.mul_(0.5) per clip, as evaluate_clips_batched runs it: finite
    inputs with signed zeros, subnormals and sums that overflow."""
    table, raw_first, raw, raw_m, _, total = layout(J, nonfinite=False)
    pred, _, status = run_device(J, table, raw_first, raw, raw_m, total, True, want_world=False)
    assert not status.any()
    jl, jr = KPS[J] if J in KPS else ([], [])
    saw = set()
    for c, d in enumerate(table):
        n, rf, first = int(d["n_frames"]), int(raw_first[c]), int(d["first_frame"])
        dst = torch.from_numpy(raw[rf:rf + n].copy()).cuda().view(n, 1, J, 3)
        pred_m = torch.from_numpy(raw_m[rf:rf + n].copy()).cuda().view(n, 1, J, 3)
        torch.add(dst, evaluate.mirror_output(pred_m, jl, jr), out=dst)
        dst.mul_(0.5)
        want = dst.view(n, J, 3).cpu().numpy()
        assert same_bits(pred[first:first + n], want), c
        saw |= {"inf"} if np.isinf(want).any() else set()
        saw |= {"subnormal"} if ((want != 0) & (np.abs(want) < 1.1e-38)).any() else set()
    assert saw == {"inf", "subnormal"}


# ------------------------------------------------------------------ 8. guard bands, surplus rows, gaps, one NaN

@pytest.mark.parametrize("J", [17, 1])
def test_guard_bands_and_untouched_rows(J):
    """Every buffer of the call carved exact-sized out of one NaN-filled allocation: nothing outside them is written, nothing
    outside them is read (the outputs equal the hook's), the inputs - surplus rows and gaps included - are unchanged, the output
    rows no clip covers keep their fill."""
    table, raw_first, raw, raw_m, raw_rows, total = layout(J)
    want, want_w, _ = hook(J, True)
    fill32, fill64 = np.full((total, J, 3), FILL, np.float32), np.full((total, J, 3), float(FILL), np.float64)
    arrays = [("raw", raw), ("raw_mirror", raw_m), ("table", table.view(np.uint8)), ("raw_first", raw_first), ("pred", fill32),
              ("world", fill64), ("status", np.full(len(table), -1, np.int32))]
    arena = Arena("cuda:0", NANS, Arena.capacity_for([a.nbytes for _, a in arrays]))
    t = {name: arena.put(a, name=name)() for name, a in arrays}
    _capi.clips_poses(t["raw"].data_ptr(), t["raw_mirror"].data_ptr(), raw_rows, J, mirror_perm(J), t["table"].data_ptr(),
                      t["raw_first"].data_ptr(), len(table), MAX_FRAMES, t["pred"].data_ptr(), t["world"].data_ptr(), total,
                      t["status"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    arena.check()
    assert not t["status"].cpu().numpy().any()
    assert same_bits(t["pred"].cpu().numpy(), want) and same_bits(t["world"].cpu().numpy(), want_w)
    assert same_bits(t["raw"].cpu().numpy(), raw) and same_bits(t["raw_mirror"].cpu().numpy(), raw_m)
    covered = np.zeros(total, bool)
    for d in table:
        covered[int(d["first_frame"]):int(d["first_frame"] + d["n_frames"])] = True
    assert 0 < (~covered).sum() and (want[~covered] == FILL).all() and (want_w[~covered] == float(FILL)).all()


@pytest.mark.parametrize("side", ["raw", "raw_mirror"])
def test_one_nan_changes_exactly_the_point_that_reads_it(side):
    """A NaN planted in one raw element: the output point (frame, joint) that reads it is non-finite - that component of pred,
    all three of world - and every other output keeps its bits."""
    J, c, f, k = 17, 2, 7, 1
    table, raw_first, raw, raw_m, _, total = layout(J, nonfinite=False)
    base, base_w, _ = run_device(J, table, raw_first, raw, raw_m, total)
    assert np.isfinite(base_w[int(table[c]["first_frame"]):int(table[c]["first_frame"]) + 15]).all()
    perm = mirror_perm(J)
    j_src = 5
    j_out = j_src if side == "raw" else perm.index(j_src)
    assert j_out != j_src or side == "raw"
    a, b = np.array(raw), np.array(raw_m)
    (a if side == "raw" else b)[int(raw_first[c]) + f, j_src, k] = np.nan
    pred, world, status = run_device(J, table, raw_first, a, b, total)
    assert not status.any()
    row = int(table[c]["first_frame"]) + f
    hit = np.zeros((total, J, 3), bool)
    hit[row, j_out, k] = True
    assert np.isnan(pred[hit]).all() and same_bits(np.where(hit, 0, pred), np.where(hit, 0, base))
    hit[row, j_out, :] = True
    assert not np.isfinite(world[hit]).any() and same_bits(np.where(hit, 0, world), np.where(hit, 0, base_w))


# ------------------------------------------------------------------ 9. evaluate_clips_batched(finish=True)

def _lifter(own=False):
    from test_gpu_clips_metrics import _lifter as make
    return make.__wrapped__() if own else make()


def _near_clips(lifter):
    from test_metrics_detail_host import evalcore_clips, near_clips
    return near_clips(lifter.forward_clip, evalcore_clips(), torch.device("cuda:0"))


def _rows_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_finish_rows_equal_the_per_clip_finish_bit_for_bit(flip):
    """The lifter and clips of test_evaluate_clips_batched_equals_evaluate_clips: rows and detail rows of finish=True are those of
    finish=False; with flip the figures on the recorded clips reproduce tests/golden/evalcore.npz to the bounds of
    test_evaluate_clips_reproduces_reference_metrics (0.05 mm, MPJPE 0.02 mm)."""
    import os
    from conftest import GOLDEN
    from test_metrics_detail_host import evalcore_clips
    lifter, dev = _lifter(), torch.device("cuda:0")
    clips = _near_clips(lifter)
    kw = dict(flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    with torch.no_grad():
        named, avg, rows = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, **kw)
        named_f, avg_f, rows_f = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, finish=True, **kw)
        _, _, rows_d, detail = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, detail=True, **kw)
        _, _, rows_df, detail_f = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, detail=True, finish=True, **kw)
        _, _, rows_r = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, root_relative=True, **kw)
        _, _, rows_rf = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, root_relative=True, finish=True, **kw)
    assert rows_f.shape == (3, 8) and torch.isfinite(rows_f).all() and _rows_equal(rows_f, rows)
    assert named_f == named and avg_f == avg
    assert _rows_equal(rows_df, rows_d) and _rows_equal(detail_f["rows"], detail["rows"]) and detail_f["rows"].shape == (3, 82)
    assert _rows_equal(rows_rf, rows_r) and not _rows_equal(rows_r, rows)
    if flip:
        z = np.load(os.path.join(GOLDEN, "evalcore.npz"))
        recorded = [evaluate.Clip(c.camera, c.rays, c.gt_norm, "A", c.clip_id) for c in evalcore_clips()]
        with torch.no_grad():
            named_z, _, _ = evaluate.evaluate_clips_batched(lifter.forward_clip, recorded, 27, dev, finish=True, flip=True,
                                                            kps_left=list(z["kps_left"]), kps_right=list(z["kps_right"]))
        got, ref = np.array(named_z["A"]), z["metrics_flip1"]
        print("finish=True flip vs evalcore.npz: got", got, "ref", ref)
        assert np.abs(got - ref).max() < 5e-2 and abs(got[0] - ref[0]) < 2e-2, (got, ref)
    with pytest.raises(ValueError, match="bound forward_clip"):
        evaluate.evaluate_clips_batched(lambda *a, **k: lifter.forward_clip(*a, **k), clips, 27, dev, finish=True)
    with pytest.raises(ValueError, match="bound forward_clip"):     # a rank with an empty shard refuses alike
        evaluate.evaluate_clips_batched(lambda *a, **k: None, clips, 27, dev, finish=True, rank=3, world_size=4)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_finish_from_raw_pixels_equals_the_per_clip_finish(flip):
    """encode="ray": clips of 1, 40 (lifted as 64) and 100 (as 128) frames - tails in the per-clip path, none here."""
    from test_gpu_clips_encode import _pixel_clips
    lifter, dev = _lifter(), torch.device("cuda:0")
    clips = _pixel_clips()
    kw = dict(flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, encode="ray", detail=True)
    with torch.no_grad():
        _, _, rows, detail = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, **kw)
        _, _, rows_f, detail_f = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, finish=True, **kw)
    assert torch.isfinite(rows[:, 3:6]).all() and _rows_equal(rows_f, rows) and _rows_equal(detail_f["rows"], detail["rows"])


def test_finish_on_two_lanes_equals_the_per_clip_finish_on_two_lanes():
    """set_lanes(2), flip, clips with tails, with and without encode=: the per-clip path joins in the middle of the pass, the
    finished one once - the same forwards on the same lanes, the same bits."""
    from test_clips_encode_host import host_encode
    from test_gpu_clips_encode import _pixel_clips
    lifter, dev = _lifter(own=True), torch.device("cuda:0")           # (a pair of its own: the lanes are an option of its handles)
    px_clips = _pixel_clips()
    ray_clips = [evaluate.Clip(c.camera, host_encode(c.camera, c.rays, "ray"), c.gt_norm, c.action, c.clip_id) for c in px_clips]
    got = {}
    try:
        for finish in (False, True):
            for name, clips, enc in (("rays", ray_clips, None), ("pixels", px_clips, "ray")):
                lifter.set_lanes(0)
                lifter.set_lanes(2)                                   # (the round-robin starts at lane 0 in every pass)
                with torch.no_grad():
                    _, _, rows = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, flip=True, kps_left=H36M_LEFT,
                                                                 kps_right=H36M_RIGHT, encode=enc, finish=finish)
                torch.cuda.synchronize()
                lifter.check_status()
                got[name, finish] = rows
    finally:
        lifter.set_lanes(0)
    for name in ("rays", "pixels"):
        assert torch.isfinite(got[name, True][:, 3:6]).all() and _rows_equal(got[name, True], got[name, False]), name


# ------------------------------------------------------------------ 10. predict_clips_batched

@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_predict_clips_batched_equals_predict_clip_and_the_numpy_transform(flip):
    """Normalised-frame clips, a camera-frame clip (Rc2w / Tc2w) and root_relative (the identity); no ground truth anywhere."""
    from test_metrics_detail_host import evalcore_clips
    lifter, dev = _lifter(), torch.device("cuda:0")
    none = np.zeros((0,), np.float32)
    clips = [evaluate.Clip(c.camera, c.rays, none, c.action, c.clip_id, frame="camera" if k == 1 else "normalized")
             for k, c in enumerate(evalcore_clips())]
    kw = dict(flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    for root_relative in (False, True):
        with torch.no_grad():
            res = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, root_relative=root_relative, **kw)
            want = [evaluate.predict_clip(lifter.forward_clip, c, 27, dev, **kw) for c in clips]
        torch.cuda.synchronize()
        assert len(res) == 3
        for c, (poses, world), w in zip(clips, res, want):
            n = c.rays.shape[0]
            assert poses.shape == (n, 17, 3) and poses.dtype == torch.float32 and world.shape == (n, 17, 3) and world.dtype == torch.float64
            assert torch.isfinite(w).all() and torch.equal(poses.view(torch.int32), w.view(n, 17, 3).view(torch.int32))
            R, T = evaluate.clip_world_transform(c, root_relative)
            R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(1, 1, 3)
            p64 = poses.cpu().numpy().astype(np.float64)
            ref = p64 @ R.T + T
            bound = 8 * EPS64 * (np.abs(p64) @ np.abs(R).T + np.abs(T))
            err = np.abs(world.cpu().numpy() - ref)
            print("flip %d root_relative %d frame %s: worst world error / bound %.3f" % (flip, root_relative, c.frame, float((err / bound).max())))
            assert (err <= bound).all()
            if root_relative:
                assert np.array_equal(world.cpu().numpy(), p64)
        assert res[0][0].untyped_storage().data_ptr() == res[2][0].untyped_storage().data_ptr()          # views of one shard buffer
    with torch.no_grad():
        only = evaluate.predict_clips_batched(lifter.forward_clip, clips, 27, dev, world=False, **kw)
    assert all(w is None for _, w in only) and all(torch.equal(a, b[0]) for (a, _), b in zip(only, res))
    assert evaluate.predict_clips_batched(lifter.forward_clip, [], 27, dev) == []


# ------------------------------------------------------------------ 11. hipGraph

def test_the_call_captured_in_a_hip_graph_replays_on_new_contents():
    """One r3d_clips_poses call captured (a single-node graph), replayed after new raw values were written into the captured
    buffers: the outputs equal an eager call on those values."""
    J = 17
    table, raw_first, raw, raw_m, _, total = layout(J, nonfinite=False)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    new, new_m = (rng.standard_normal(raw.shape).astype(np.float32) for _ in range(2))
    tab = torch.from_numpy(np.array(table).view(np.uint8)).to(dev)
    rf = torch.from_numpy(np.array(raw_first)).to(dev)
    a, b = torch.from_numpy(np.array(raw)).to(dev), torch.from_numpy(np.array(raw_m)).to(dev)
    pred = torch.full((total, J, 3), float(FILL), dtype=torch.float32, device=dev)
    world = torch.full((total, J, 3), float(FILL), dtype=torch.float64, device=dev)
    status = torch.full((len(table),), -1, dtype=torch.int32, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            evaluate.shard_poses_hip(a, tab, rf, len(table), total, MAX_FRAMES, b, mirror_perm(J), pred_all=pred, world_all=world, status=status)
    a.copy_(torch.from_numpy(new))
    b.copy_(torch.from_numpy(new_m))
    g.replay()
    torch.cuda.synchronize()
    want, want_w, want_s = run_device(J, table, raw_first, new, new_m, total)
    assert not want_s.any() and not status.cpu().numpy().any()
    assert same_bits(pred.cpu().numpy(), want) and same_bits(world.cpu().numpy(), want_w)
    del g
    torch.cuda.synchronize()
