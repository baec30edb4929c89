"""-m gpu: r3d_clips_project - a camera sweep's padded, encoded (and mirrored) model inputs, its ground truth, its float64 pixels
and its in-frame counts from world poses in one launch over a device-side table - against its host hook on the layouts of
tests/test_clips_project_host.py BIT FOR BIT (the projection and the ground truth are compiled with contraction off on both
sides; the encoding is the routine r3d_clips_encode writes with), inside guard bands with descriptors that point far outside,
with non-finite points, captured in a hipGraph, and end to end through evaluate_camera_sweep against the host path."""
import functools

import numpy as np
import pytest
import torch

from buffers_util import NANS, Arena
from test_clips_project_host import (ENCODINGS, FILL, FILL_COUNT, KPS, RF, _world_clips, cameras, golden, layout,
                                     mirror_perm, nonfinite_world, run_hook, same_bits, with_invalid)

pytestmark = pytest.mark.gpu

H36M_LEFT, H36M_RIGHT = KPS[17]
NAMES = ("x", "xm", "gt", "px", "outside", "status")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_device(J, encoding, table, world, out_rows, max_rows, gt_rows, mirror=True, gt=True, px=True, count=True):
    """One r3d_clips_project call (product library) on device tensors pre-filled as run_hook's host arrays -> dict of NumPy arrays."""
    from ray3d_amd import _capi, evaluate
    _capi.use_hooks(False)
    enc = evaluate.ENCODINGS[encoding]
    F = _capi.ENCODE_FLOATS[enc]
    num = table.shape[0]
    wd = torch.from_numpy(np.array(world)).cuda()
    tab = torch.from_numpy(np.array(table).view(np.uint8)).cuda()
    b = dict(x=torch.full((out_rows, J, F), float(FILL), device="cuda"),
             xm=torch.full((out_rows, J, F), float(FILL), device="cuda") if mirror else None,
             gt=torch.full((gt_rows, J, 3), float(FILL), device="cuda") if gt else None,
             px=torch.full((gt_rows, J, 2), float(FILL), dtype=torch.float64, device="cuda") if px else None,
             outside=torch.full((num,), FILL_COUNT, dtype=torch.int32, device="cuda") if count else None,
             status=torch.full((num,), -1, dtype=torch.int32, device="cuda"))
    p = {k: (v.data_ptr() if v is not None else None) for k, v in b.items()}
    _capi.clips_project(wd.data_ptr(), world.shape[0], J, enc, tab.data_ptr(), num, max_rows, p["x"], out_rows, p["xm"],
                        mirror_perm(J) if mirror else None, p["gt"], p["px"], gt_rows, p["outside"], p["status"], _stream())
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in b.items()}


def assert_same_as_hook(dev, hook, what):
    """Every buffer bit for bit - the rows no descriptor covers (FILL on both sides) included; the share of unequal elements is
    printed before it is asserted to be zero."""
    for name in NAMES:
        d, h = dev[name], hook[name]
        assert (d is None) == (h is None), (what, name)
        if d is None:
            continue
        w = np.int32 if d.dtype.itemsize == 4 else np.int64
        off = float((d.view(w) != h.view(w)).mean()) if d.shape == h.shape else 1.0
        print("%s %s: %d elements, share not bit-equal %.3e" % (what, name, d.size, off))
    for name in NAMES:
        if dev[name] is not None:
            assert same_bits(dev[name], hook[name]), (what, name)


# ------------------------------------------------------------------ 2. device against hook, bit for bit

@pytest.mark.parametrize("J", [1, 14, 17])
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_device_equals_the_host_hook(encoding, J):
    """Clips of 1 / 15 / 16 / 31 frames under RF 9 - centred, causal (8, 0) and surplus padding, three cameras on shared source
    frames, out of order with gaps: every output has the hook's bits, a padding row the bits of the frame it repeats."""
    frame = "camera" if J == 14 else "normalized"
    table, world, out_rows, max_rows, gt_rows, _ = layout(J, frame)
    dev = run_device(J, encoding, table, world, out_rows, max_rows, gt_rows)
    rc, hook = run_hook(J, encoding, table, world, out_rows, max_rows, gt_rows)
    assert rc == 0 and not hook["status"].any() and int(hook["outside"].sum()) > FILL_COUNT * len(table)
    assert_same_as_hook(dev, hook, "%s J %d" % (encoding, J))
    x = dev["x"]
    for d in table:
        at, pf, n, pb = int(d["out_first"]), int(d["pad_front"]), int(d["n_frames"]), int(d["pad_back"])
        assert all(same_bits(x[at + r], x[at + pf]) for r in range(pf))
        assert all(same_bits(x[at + pf + n + r], x[at + pf + n - 1]) for r in range(pb))


@pytest.mark.parametrize("outputs", ["none", "mirror", "gt", "px", "count", "gt+count"])
def test_device_optional_outputs(outputs):
    """With and without each optional output and the mirror: what is written has the hook's bits, nothing else exists to write."""
    table, world, out_rows, max_rows, gt_rows, _ = layout(17)
    kw = dict(mirror="mirror" in outputs, gt="gt" in outputs, px="px" in outputs, count="count" in outputs)
    dev = run_device(17, "ray", table, world, out_rows, max_rows, gt_rows, **kw)
    rc, hook = run_hook(17, "ray", table, world, out_rows, max_rows, gt_rows, **kw)
    assert rc == 0 and not hook["status"].any()
    assert_same_as_hook(dev, hook, outputs)


def test_device_invalid_descriptors_equal_the_host_hook():
    """One invalid descriptor of each kind (n < 1, a negative pad, rows over max_rows, source / output / gt out of range, ranges
    near 2^62) between the valid ones: status 1, none of its rows touched, its neighbours keep their bits."""
    table, world, out_rows, max_rows, gt_rows, _ = layout(17)
    clean = run_device(17, "ray", table, world, out_rows, max_rows, gt_rows)
    t, bad = with_invalid(table, world.shape[0], out_rows, max_rows, gt_rows)
    dev = run_device(17, "ray", t, world, out_rows, max_rows, gt_rows)
    rc, hook = run_hook(17, "ray", t, world, out_rows, max_rows, gt_rows)
    assert rc == 0 and dev["status"].tolist() == [1 if k in bad else 0 for k in range(len(t))]
    assert_same_as_hook(dev, hook, "with invalid descriptors")
    for name in ("x", "xm", "gt", "px"):
        assert same_bits(dev[name], clean[name]), name
    assert (dev["outside"][bad] == FILL_COUNT).all()


def test_device_nonfinite_points_equal_the_host_hook():
    """NaN / +-Inf world elements and a camera whose plane holds the points (h2 == 0): the device has the hook's bits - canonical
    NaNs included - and tests/test_clips_project_host.py shows on the hook that only the outputs that read them move."""
    table, world, out_rows, max_rows, gt_rows, _ = layout(17)
    w, _ = nonfinite_world(world, table)
    t = table.copy()
    t[0]["proj"][8:12] = 0.0
    for encoding in ENCODINGS:
        dev = run_device(17, encoding, t, w, out_rows, max_rows, gt_rows)
        rc, hook = run_hook(17, encoding, t, w, out_rows, max_rows, gt_rows)
        assert rc == 0 and not hook["status"].any() and np.isnan(hook["x"]).any() and np.isinf(hook["px"]).any()
        assert_same_as_hook(dev, hook, "non-finite %s" % encoding)
        for name in ("x", "gt", "px"):                   # (the mirrored copy negates component 0: a NaN's sign bit with it)
            got = dev[name]
            bits = got[np.isnan(got)].view(np.int32 if got.dtype == np.float32 else np.int64)
            assert (bits == (0x7fc00000 if got.dtype == np.float32 else 0x7ff8000000000000)).all(), name


# ------------------------------------------------------------------ guard bands

def test_guard_bands_around_every_buffer():
    """world, the table, x, x_mirror, gt, px, outside and status exact-size regions of one arena filled with NaN bits (world and
    the float32 outputs 4 bytes off their alignment), the layout of the bit test with every invalid descriptor in between: not a
    byte outside the regions written, the rows no valid descriptor covers keep the pattern, the rest has the hook's bits."""
    from ray3d_amd import _capi
    J, F = 17, 3
    table, world, out_rows, max_rows, gt_rows, _ = layout(J)
    t, bad = with_invalid(table, world.shape[0], out_rows, max_rows, gt_rows)
    world = np.ascontiguousarray(world)
    nx, ng, npx, nw = out_rows * J * F * 4, gt_rows * J * 3 * 4, gt_rows * J * 2 * 8, 4 * len(t)
    arena = Arena("cuda", NANS, Arena.capacity_for([world.nbytes, t.nbytes, nx, nx, ng, npx, nw, nw]))
    wd = arena.put(world, skew=4, name="world")()
    tab = arena.put(t.view(np.uint8), name="table")()
    x, xm = arena.carve(nx, skew=4, name="x"), arena.carve(nx, skew=4, name="x_mirror")
    gt, px = arena.carve(ng, skew=4, name="gt"), arena.carve(npx, name="px")
    outside, status = arena.carve(nw, name="outside"), arena.carve(nw, name="status")
    outside.view(torch.int32).fill_(FILL_COUNT)
    assert wd.data_ptr() % 8 == 4 and x.data_ptr() % 8 == 4 and gt.data_ptr() % 8 == 4 and tab.data_ptr() % 8 == 0 and px.data_ptr() % 8 == 0
    _capi.clips_project(wd.data_ptr(), world.shape[0], J, _capi.R3D_ENCODE_RAY, tab.data_ptr(), len(t), max_rows, x.data_ptr(), out_rows,
                        xm.data_ptr(), mirror_perm(J), gt.data_ptr(), px.data_ptr(), gt_rows, outside.data_ptr(), status.data_ptr(), _stream())
    arena.check()
    rc, hook = run_hook(J, "ray", t, world, out_rows, max_rows, gt_rows)
    assert rc == 0
    assert status.view(torch.int32).cpu().numpy().tolist() == hook["status"].tolist() == [1 if k in bad else 0 for k in range(len(t))]
    assert outside.view(torch.int32).cpu().numpy().tolist() == hook["outside"].tolist()
    for name, view, shape in (("x", x, (out_rows, J, F)), ("xm", xm, (out_rows, J, F)), ("gt", gt, (gt_rows, J, 3))):
        got = view.view(torch.int32).view(shape).cpu().numpy()
        covered = hook[name] != FILL
        assert (got[~covered] == -1).all(), name                                      # the arena's pattern (0xFFFFFFFF)
        assert np.array_equal(got[covered], hook[name].view(np.int32)[covered]), name
    got = px.view(torch.int64).view(gt_rows, J, 2).cpu().numpy()
    covered = hook["px"] != float(FILL)
    assert (got[~covered] == -1).all() and np.array_equal(got[covered], hook["px"].view(np.int64)[covered])


# ------------------------------------------------------------------ hipGraph

def test_the_call_captured_in_a_hip_graph_replays_on_new_contents():
    """shard_project_hip with every buffer given, captured (the memset of `outside` and the one launch), replayed twice after new
    world poses were written into the captured buffer: the outputs equal the hook on those poses, the counts do not pile up."""
    from ray3d_amd import evaluate
    J = 17
    table, world, out_rows, max_rows, gt_rows, _ = layout(J)
    dev = torch.device("cuda:0")
    new = np.array(world)
    new[~np.isnan(new)] += np.float32(0.125)
    tab = torch.from_numpy(np.array(table).view(np.uint8)).to(dev)
    wd = torch.from_numpy(np.array(world)).to(dev)
    x = torch.full((out_rows, J, 3), float(FILL), device=dev)
    xm, gt = torch.full_like(x, float(FILL)), torch.full((gt_rows, J, 3), float(FILL), device=dev)
    px = torch.full((gt_rows, J, 2), float(FILL), dtype=torch.float64, device=dev)
    outside = torch.full((len(table),), FILL_COUNT, dtype=torch.int32, device=dev)
    status = torch.full((len(table),), -1, dtype=torch.int32, device=dev)
    call = lambda: evaluate.shard_project_hip(wd, tab, len(table), out_rows, max_rows, gt_rows, "ray", mirror_perm(J), x_all=x, x_mirror_all=xm,
                                              gt_all=gt, px_all=px, outside=outside, status=status)
    call()                                                                              # (the code objects are loaded outside the capture)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call()
    wd.copy_(torch.from_numpy(new))
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    rc, hook = run_hook(J, "ray", table, new, out_rows, max_rows, gt_rows)
    hook["outside"] -= FILL_COUNT                                                       # shard_project_hip zeroes the counts itself
    got = dict(x=x, xm=xm, gt=gt, px=px, outside=outside, status=status)
    assert rc == 0
    assert_same_as_hook({k: v.cpu().numpy() for k, v in got.items()}, hook, "graph replay")
    del g
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. the sweep equals the host path

@functools.lru_cache(maxsize=None)
def _rf9():
    from test_gpu_clips_valid import _lifter
    lifter, cp = _lifter()
    assert cp.receptive_field == RF
    return lifter


def _hook_clips(lifter, frame="normalized"):
    """evaluate.Clip objects - camera-major, as the sweep orders its pairs - whose rays / gt_norm are the HOOK's outputs for the
    (clip, camera) pairs of project.npz: the host path's inputs with the sweep's bits."""
    from ray3d_amd import _capi, evaluate
    wc = _world_clips()
    pairs = [(k, ci) for ci in range(3) for k in range(2)]
    world = np.concatenate([c.world for c in wc], axis=0)
    table, out_first, out_rows, max_rows, gt_first, gt_rows = evaluate.clip_project_table(wc, pairs, cameras(), RF, frame=frame)
    rc, b = run_hook(17, "ray", table, world, out_rows, max_rows, gt_rows)
    _capi.use_hooks(False)
    assert rc == 0 and not b["status"].any()
    pad = (RF - 1) // 2
    clips = []
    for k, (ci_clip, ci) in enumerate(pairs):
        n = wc[ci_clip].world.shape[0]
        clips.append(evaluate.Clip(cameras()[ci], b["x"][out_first[k] + pad:out_first[k] + pad + n].copy(),
                                   b["gt"][gt_first[k]:gt_first[k] + n].copy(), wc[ci_clip].action, k, frame=frame))
    return wc, pairs, clips, [int(v) - FILL_COUNT for v in b["outside"]]


def _same_report(a, b):
    """Two reduce_camera_sweep results equal, a NaN (the velocity error of a one-frame clip) equal to a NaN."""
    flat = lambda rep: [(n, sorted(per), [v for k in sorted(per) for v in per[k]] + list(avg), out) for n, per, avg, out in rep]
    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(x[0] == y[0] and x[1] == y[1] and x[3] == y[3] and np.array_equal(x[2], y[2], equal_nan=True)
                                      for x, y in zip(fa, fb))


def _sorted(rows):
    """Sweep rows in (camera, clip) order."""
    from ray3d_amd import evaluate
    rows = rows.detach().cpu()
    key = rows[:, evaluate.PARTIAL_COLS] * 1000 + rows[:, 0]
    return rows[torch.argsort(key, stable=True)]


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_sweep_equals_the_host_path(flip, monkeypatch):
    """2 clips x 3 cameras of project.npz through the RF-9 model.  (a) The sweep's rows are BIT-EQUAL to those of
    evaluate_clips_batched(finish=True) on Clips that hold the hook's inputs and ground truth: bit-equal inputs, the same calls
    after them.  (b) Against Clips built on the host with Camera.rays_from_uv(Camera.project(...)) / world2normalized the
    per-camera errors agree to 1e-3 mm: the drift a one-ulp input difference can cause at this depth - looser on purpose, it
    catches a wrong grouping.  (c) cameras_per_pass 1 and None give the same rows.  (d) The third camera reports the fixture's
    count of keypoints outside the frame.  (e) Ranks 0 and 1 of two, the all_gather replaced by the rows the ranks made,
    reassemble the single-rank rows."""
    from ray3d_amd import evaluate
    lifter, dev = _rf9(), torch.device("cuda:0")
    z = golden()
    wc, pairs, hook_clips, hook_outside = _hook_clips(lifter)
    kw = dict(flip=flip, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    with torch.no_grad():
        report, rows = evaluate.evaluate_camera_sweep(lifter.forward_clip, wc, cameras(), RF, dev, **kw)
        report1, rows1 = evaluate.evaluate_camera_sweep(lifter.forward_clip, wc, cameras(), RF, dev, cameras_per_pass=1, **kw)
        _, _, host_rows = evaluate.evaluate_clips_batched(lifter.forward_clip, hook_clips, RF, dev, finish=True, **kw)
    torch.cuda.synchronize()
    assert rows.shape == (6, evaluate.SWEEP_COLS) and rows.dtype == torch.float64
    got = _sorted(rows)
    one_frame = got[:, 2] == 1                           # (the velocity error of a one-frame clip is NaN, as in r3d_clip_metrics)
    assert torch.isfinite(got[:, [3, 4, 5, 7, 8, 9]]).all() and torch.equal(torch.isnan(got[:, 6]), one_frame) and int(one_frame.sum()) == 3
    # (a) host_rows: clip id = index into hook_clips = camera-major pair index
    host_rows = host_rows.detach().cpu()
    host_rows = host_rows[torch.argsort(host_rows[:, 0], stable=True)]
    assert host_rows[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert got[:, 0].tolist() == [0.0, 1.0] * 3 and got[:, evaluate.PARTIAL_COLS].tolist() == [0.0, 0.0, 1.0, 1.0, 2.0, 2.0]
    diff = torch.nan_to_num(got[:, 1:evaluate.PARTIAL_COLS] - host_rows[:, 1:]).abs().max().item()       # (NaN velocity on both sides: 0)
    print("flip %d: sweep rows vs host path on the hook's inputs: max |diff| %.3e" % (flip, diff))
    assert torch.equal(got[:, 1:evaluate.PARTIAL_COLS].contiguous().view(torch.int64), host_rows[:, 1:].contiguous().view(torch.int64))
    # (c)
    assert torch.equal(_sorted(rows1).view(torch.int64), got.view(torch.int64)) and _same_report(report1, report)
    # (d)
    assert got[:, evaluate.PARTIAL_COLS + 1].tolist() == [float(v) for v in hook_outside]
    assert [r[0] for r in report] == [c.name for c in cameras()]
    assert [r[3] for r in report] == [0, 0, int(z["ref/one/2/outside"]) + int(z["ref/walk/2/outside"])] and report[2][3] > 0
    # (b) the host path proper: NumPy float64 projection, encoding and ground truth per (clip, camera)
    for ci, cam in enumerate(cameras()):
        clips = [evaluate.Clip(cam, cam.rays_from_uv(cam.project(c.world.astype(np.float64))).astype(np.float32),
                               cam.world2normalized(c.world.astype(np.float64)).astype(np.float32), c.action, k) for k, c in enumerate(wc)]
        with torch.no_grad():
            named, avg, _ = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, RF, dev, finish=True, **kw)
        name, per_action, average, _ = report[ci]
        assert set(per_action) == set(named) == {"A", "B"}
        a, b = (np.array([per[act] for act in ("A", "B")]) for per in (per_action, named))
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(a).sum() == 1        # action A is the one-frame clip: no velocity
        worst = float(np.nanmax(np.abs(a - b)))
        print("flip %d camera %s: per-action errors vs the NumPy host path: max |diff| %.3e mm" % (flip, name, worst))
        assert worst <= 1e-3 and float(np.nanmax(np.abs(np.array(average) - np.array(avg)))) <= 0.1 + 1e-9
    # (e)
    shards = evaluate.shard_clips([wc[k].world.shape[0] for k, _ in pairs], 2)
    assert all(shards) and sorted(shards[0] + shards[1]) == list(range(6))
    made = {}

    def gather(local_rows, counts, group=None, cols=evaluate.PARTIAL_COLS, rank=None):
        assert list(counts) == [len(s) for s in shards] and local_rows.shape == (counts[rank], cols) and cols == evaluate.SWEEP_COLS
        made[rank] = local_rows
        return torch.cat([made.get(r, local_rows.new_zeros((counts[r], cols))) for r in range(2)], dim=0)

    res = {}
    for rank in (0, 1, 0):                               # (rank 0 once more, now with rank 1's rows in the exchange)
        monkeypatch.setattr(evaluate, "gather_partials", functools.partial(gather, rank=rank))
        with torch.no_grad():
            res[rank] = evaluate.evaluate_camera_sweep(lifter.forward_clip, wc, cameras(), RF, dev, rank=rank, world_size=2,
                                                       cameras_per_pass=2, **kw)
    for rank in (0, 1):
        rep, r = res[rank]
        assert torch.equal(_sorted(r).view(torch.int64), got.view(torch.int64)) and _same_report(rep, report), rank


def test_sweep_camera_frame_and_argument_errors():
    """frame="camera": the ground truth is the hook's world2camera and the metrics go through Rc2w / Tc2w - bit-equal to the host
    path on camera-frame Clips; an unknown frame, finish=False and a lift_clip that is no lifter's forward_clip raise before
    anything is uploaded."""
    from ray3d_amd import evaluate
    lifter, dev = _rf9(), torch.device("cuda:0")
    wc, pairs, hook_clips, _ = _hook_clips(lifter, frame="camera")
    with torch.no_grad():
        _, rows = evaluate.evaluate_camera_sweep(lifter.forward_clip, wc, cameras(), RF, dev, frame="camera")
        _, _, host_rows = evaluate.evaluate_clips_batched(lifter.forward_clip, hook_clips, RF, dev, finish=True)
    got, host_rows = _sorted(rows), host_rows.detach().cpu()
    host_rows = host_rows[torch.argsort(host_rows[:, 0], stable=True)]
    assert torch.equal(got[:, 1:evaluate.PARTIAL_COLS].contiguous().view(torch.int64), host_rows[:, 1:].contiguous().view(torch.int64))
    with pytest.raises(ValueError, match="frame"):
        evaluate.evaluate_camera_sweep(lifter.forward_clip, wc, cameras(), RF, dev, frame="world")
    with pytest.raises(ValueError, match="finish"):
        evaluate.evaluate_camera_sweep(lifter.forward_clip, wc, cameras(), RF, dev, finish=False)
    with pytest.raises(ValueError, match="forward_clip"):
        evaluate.evaluate_camera_sweep(lambda x, p: x, wc, cameras(), RF, dev)
    report, rows = evaluate.evaluate_camera_sweep(lifter.forward_clip, [], cameras(), RF, dev)
    assert report == [] and rows.shape == (0, evaluate.SWEEP_COLS)
