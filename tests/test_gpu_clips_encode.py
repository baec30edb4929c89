"""-m gpu: r3d_clips_encode - a shard's padded, encoded (and mirrored) model inputs from its raw pixel archive in one launch over
a device-side clip table - against its host hook on the clips of tests/test_clips_encode_host.py, bit for bit against the
pre-pass of a R3D_INPUT_UV_DIST forward and (zero coefficients) against R3D_INPUT_UV, inside guard bands with descriptors that
point far outside, end to end through evaluate_clips_batched(encode=), and captured in a hipGraph."""
import os

import numpy as np
import pytest
import torch

from buffers_util import NANS, Arena
from conftest import GOLDEN, check_parity, record_parity
from test_clips_encode_host import (ENCODINGS, FILL, KPS, cameras, host_encode, invalid_cases, layout, mirror_perm, pixels, run_hook,
                                    same_bits, ulps, with_invalid)

pytestmark = pytest.mark.gpu

H36M_LEFT, H36M_RIGHT = KPS[17]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_device(J, encoding, table, px, out_rows, max_rows, mirror=True):
    """One r3d_clips_encode call (product library) on device tensors pre-filled with FILL -> (x, x_mirror or None, status), NumPy."""
    from ray3d_amd import _capi, evaluate
    enc = evaluate.ENCODINGS[encoding]
    F = _capi.ENCODE_FLOATS[enc]
    pxd = torch.from_numpy(np.array(px)).cuda()
    tab = torch.from_numpy(np.array(table).view(np.uint8)).cuda()
    x = torch.full((out_rows, J, F), float(FILL), device="cuda")
    xm = torch.full((out_rows, J, F), float(FILL), device="cuda") if mirror else None
    status = torch.full((table.shape[0],), -1, dtype=torch.int32, device="cuda")
    _capi.clips_encode(pxd.data_ptr(), px.shape[0], J, enc, tab.data_ptr(), table.shape[0], max_rows, x.data_ptr(), out_rows,
                       xm.data_ptr() if mirror else None, mirror_perm(J) if mirror else None, status.data_ptr(), _stream())
    torch.cuda.synchronize()
    return x.cpu().numpy(), xm.cpu().numpy() if mirror else None, status.cpu().numpy()


def _equal_within_one_ulp(got, want, what):
    """FILL where the hook left FILL, every other element within one float32 ulp."""
    fill = want == FILL
    assert np.array_equal(got == FILL, fill), what
    worst = ulps(got[~fill], want[~fill])
    print("%s: %.6f of %d elements equal, max %d ulp" % (what, float((got == want).mean()), got.size, worst))
    assert worst <= 1, (what, worst)


@pytest.mark.parametrize("J", [17, 14])
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_device_equals_the_host_hook(encoding, J):
    """The clips of the host test (1 .. 40 frames, pads 0 / 4 / 13, a causal shift, an extra pad_back, distorted and
    zero-coefficient rows, out of order with gaps): every element within one ulp of r3d_debug_clips_encode_host, the same
    status words, the mirrored copy exact, rows outside every clip untouched."""
    table, px, total, out_rows, max_rows, _ = layout(J)
    x, xm, status = run_device(J, encoding, table, px, out_rows, max_rows)
    rc, hx, hxm, hstatus = run_hook(J, encoding, table, px, out_rows, max_rows)
    assert rc == 0 and np.array_equal(status, hstatus) and not status.any()
    _equal_within_one_ulp(x, hx, "%s J %d" % (encoding, J))
    _equal_within_one_ulp(xm, hxm, "%s J %d mirrored" % (encoding, J))
    exp = x[:, mirror_perm(J)].copy()
    exp[..., 0] = -exp[..., 0]
    covered = (hx != FILL).all(axis=(1, 2))
    assert same_bits(xm[covered], exp[covered])
    for d in table:                                       # a padding row has the bits of the frame it repeats
        at, pf, n, pb = int(d["out_first"]), int(d["pad_front"]), int(d["n_frames"]), int(d["pad_back"])
        assert all(same_bits(x[at + r], x[at + pf]) for r in range(pf))
        assert all(same_bits(x[at + pf + n + r], x[at + pf + n - 1]) for r in range(pb))
    x2, _, status2 = run_device(J, encoding, table, px, out_rows, max_rows, mirror=False)
    assert same_bits(x2, x) and not status2.any()


def test_device_invalid_descriptors_equal_the_host_hook():
    """Each of the five invalidity conditions between valid clips: the hook's status words, nothing of those clips written, the
    other clips as in the all-valid run."""
    J = 17
    table, px, total, out_rows, max_rows, _ = layout(J)
    ref, ref_m, _ = run_device(J, "ray", table, px, out_rows, max_rows)
    for t, bad in with_invalid(J):
        x, xm, status = run_device(J, "ray", t, px, out_rows, max_rows)
        rc, hx, hxm, hstatus = run_hook(J, "ray", t, px, out_rows, max_rows)
        assert rc == 0 and np.array_equal(status, hstatus) and status.tolist() == [1 if c in bad else 0 for c in range(len(t))]
        want, want_m = ref.copy(), ref_m.copy()
        for c in bad:
            d = table[c]
            rows = slice(int(d["out_first"]), int(d["out_first"] + d["pad_front"] + d["n_frames"] + d["pad_back"]))
            want[rows], want_m[rows] = FILL, FILL
        assert same_bits(x, want) and same_bits(xm, want_m), bad


# ------------------------------------------------------------------ against the existing pre-pass and R3D_INPUT_UV

def _lifter():
    """The RF-27, J-17 ray pair of tests/test_gpu_clips_metrics.py (one per session)."""
    from test_gpu_clips_metrics import _lifter as make
    return make()


def _one_clip_table(n, cam, pad_front, pad_back):
    from ray3d_amd import _capi
    table = np.zeros(1, dtype=_capi.clip_input_desc_dtype())
    table[0]["n_frames"], table[0]["pad_front"], table[0]["pad_back"] = n, pad_front, pad_back
    table[0]["cam"] = cam.cam_row(distortion=True)
    return table


def test_bit_for_bit_with_the_pre_pass_of_a_uv_dist_forward():
    """RF 27, J 17, one distorted camera: the encoded rows of a clip are the rays an R3D_INPUT_UV_DIST forward with
    window_stride 1 over the padded raw pixels leaves in its workspace tail."""
    from ray3d_amd import _capi, evaluate
    from test_gpu_undistort import _ws_rays
    lifter, dev = _lifter(), torch.device("cuda:0")
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    n, cam = 100, cameras()[1]
    px = pixels("clips_encode.prepass", (n, 17, 2))
    padded = torch.from_numpy(evaluate.pad_clip(px, 13)).cuda()
    row = torch.from_numpy(cam.cam_row(distortion=True)).cuda()
    prow = torch.from_numpy(cam.param()).cuda()
    inp = _capi.make_input(_capi.R3D_INPUT_UV_DIST, padded.data_ptr(), 1, prow.data_ptr(), 0, row.data_ptr(), 0)
    want, _ = _ws_rays(lifter, hp, ht, inp, n, n + 26, 17, dev)
    x, _, status = run_device(17, "ray", _one_clip_table(n, cam, 13, 13), px, n + 26, n + 26, mirror=False)
    assert not status.any() and np.isfinite(want).all() and same_bits(x, want)


@pytest.mark.parametrize("n", [64, 40])
def test_zero_coefficient_rows_give_uv_mode_values_through_the_forward(n):
    """forward_clip on the encoded slice (an exact batch size, and one with surplus rows: forward_clip(n_windows=)) is
    forward_uv with the 8-wide row on the padded raw pixels, bit for bit."""
    from ray3d_amd import evaluate
    lifter, dev = _lifter(), torch.device("cuda:0")
    cam = cameras()[5]
    assert not cam.cam_row(distortion=True)[8:].any()
    px = pixels("clips_encode.zero.%d" % n, (n, 17, 2))
    surplus = sum(lifter.clip_batch_sizes(n)) - n
    assert (surplus > 0) == (n == 40)
    table = _one_clip_table(n, cam, 13, 13 + surplus)
    x_all, _, status = evaluate.shard_encode_hip(torch.from_numpy(px).cuda(), torch.from_numpy(table.view(np.uint8)).cuda(), 1,
                                                 n + 26 + surplus, n + 26 + surplus, "ray")
    prow = torch.from_numpy(cam.param()).cuda()
    with torch.no_grad():
        got = lifter.forward_clip(x_all, prow, n_windows=n)
        want = lifter.forward_uv(torch.from_numpy(evaluate.pad_clip(px, 13)).cuda(), torch.from_numpy(cam.cam_row()).cuda(), prow, window_stride=1)
    torch.cuda.synchronize()
    assert not status.any().item() and got.shape == want.shape == (n, 1, 17, 3)
    assert torch.isfinite(want).all() and torch.equal(got, want)


# ------------------------------------------------------------------ guard bands

def test_guard_bands_around_every_buffer():
    """px, the table, x, x_mirror and status exact-size regions of one arena (px and the outputs 4 bytes off their alignment):
    clips of 15 rows (255 points), 16 rows (272) and 31 rows (527: one row more than two workgroups of 256 points) of 17
    joints, and every invalid descriptor of the host test - ranges near +-2^62 included - in between: not a byte outside the
    regions written, the rows no valid clip covers keep the pattern, the valid clips are the hook's."""
    from ray3d_amd import _capi
    J, F = 17, 3
    lengths = (15, 16, 31)
    total, out_rows, max_rows = sum(lengths), sum(lengths) + 4, 31
    px = pixels("clips_encode.guard", (total, J, 2))
    cases = invalid_cases(total, out_rows, max_rows)
    table = np.zeros(len(lengths) + len(cases), dtype=_capi.clip_input_desc_dtype())
    valid, at = [], 0
    for k, n in enumerate(lengths):                       # valid clips at table positions 0, 6, 12: no pads, rows [at + 2, ...)
        c = 6 * k
        table[c]["first_frame"], table[c]["n_frames"], table[c]["out_first"] = at, n, at + 2
        valid.append(c)
        at += n
    bad = [c for c in range(len(table)) if c not in valid]
    for c, (_, over) in zip(bad, cases):
        table[c]["first_frame"], table[c]["n_frames"], table[c]["out_first"] = 0, 15, 2     # valid until overwritten
        for name, v in over.items():
            table[c][name] = v
    for c in range(len(table)):
        table[c]["cam"] = cameras()[c % 8].cam_row(distortion=True)
    nx = out_rows * J * F * 4
    arena = Arena("cuda", NANS, Arena.capacity_for([px.nbytes, table.nbytes, nx, nx, 4 * len(table)]))
    pxd = arena.put(px, skew=4, name="px")()
    tab = arena.put(table.view(np.uint8), name="table")()
    x, xm = arena.carve(nx, skew=4, name="x"), arena.carve(nx, skew=4, name="x_mirror")
    status = arena.carve(4 * len(table), name="status")
    assert pxd.data_ptr() % 8 == 4 and x.data_ptr() % 8 == 4 and tab.data_ptr() % 8 == 0
    _capi.clips_encode(pxd.data_ptr(), total, J, _capi.R3D_ENCODE_RAY, tab.data_ptr(), len(table), max_rows, x.data_ptr(), out_rows,
                       xm.data_ptr(), mirror_perm(J), status.data_ptr(), _stream())
    arena.check()
    got_status = status.view(torch.int32).cpu().numpy()
    assert got_status.tolist() == [0 if c in valid else 1 for c in range(len(table))]
    xi, xmi = x.view(torch.int32).view(out_rows, J, F).cpu().numpy(), xm.view(torch.int32).view(out_rows, J, F).cpu().numpy()
    untouched = [0, 1, out_rows - 2, out_rows - 1]
    assert (xi[untouched] == -1).all() and (xmi[untouched] == -1).all()              # the arena's pattern (0xFFFFFFFF)
    rc, hx, hxm, hstatus = run_hook(J, "ray", table, px, out_rows, max_rows)
    assert rc == 0 and np.array_equal(hstatus, got_status)
    body = slice(2, out_rows - 2)
    assert ulps(xi.view(np.float32)[body], hx[body]) <= 1 and ulps(xmi.view(np.float32)[body], hxm[body]) <= 1


# ------------------------------------------------------------------ end to end: evaluate_clips_batched(encode=)

def _pixel_clips():
    """Lengths 1, 40 (lifted as 64) and 100 (as 128) on three cameras - two distorted H36M ones and a zero-coefficient one -
    with seeded ground truth of the poses' size; raw pixels in Clip.rays."""
    from ray3d_amd import evaluate
    rng = np.random.default_rng(5)
    out = []
    for k, (n, cam) in enumerate(((1, 0), (40, 6), (100, 3))):
        gt = rng.normal(0, 0.5, (n, 17, 3)).astype(np.float32)
        out.append(evaluate.Clip(cameras()[cam], pixels("clips_encode.eval.%d" % k, (n, 17, 2)), gt, "AB"[k % 2], k))
    return out


def test_batched_evaluation_from_raw_pixels_equals_the_per_clip_forward_uv_path():
    """flip off: evaluate_clips_batched(encode="ray") gives the rows - bit for bit - of evaluate_clips with a lifter that calls
    forward_uv(padded, row16, prow) per clip (pad on the host, upload, the pre-pass in front of every forward)."""
    from ray3d_amd import evaluate
    lifter, dev = _lifter(), torch.device("cuda:0")
    clips = _pixel_clips()
    assert [sum(lifter.clip_batch_sizes(c.rays.shape[0])) for c in clips] == [1, 64, 128]
    row_of = {c.rays.shape[0] + 26: torch.from_numpy(c.camera.cam_row(distortion=True)).cuda() for c in clips}
    lift_a = lambda padded, prow: lifter.forward_uv(padded, row_of[padded.shape[0]], prow, window_stride=1)
    with torch.no_grad():
        named_a, avg_a, rows_a = evaluate.evaluate_clips(lift_a, clips, 27, dev)
        named_b, avg_b, rows_b = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, encode="ray")
        _, _, rows_d, detail = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, encode="ray", detail=True)
    torch.cuda.synchronize()
    assert rows_b.shape == (3, 8) and torch.isfinite(rows_a[:, 3:6]).all()
    assert torch.equal(rows_b.view(torch.int64), rows_a.view(torch.int64))
    # (the velocity of the one-frame clip is NaN in both, and with it action A's and the average's: compare NaN as equal)
    assert set(named_b) == set(named_a) == {"A", "B"}
    assert all(np.array_equal(named_b[k], named_a[k], equal_nan=True) for k in named_a) and np.array_equal(avg_b, avg_a, equal_nan=True)
    order = torch.argsort(rows_b[:, 0])
    assert torch.equal(rows_d.view(torch.int64), rows_b[order].view(torch.int64)) and detail["rows"].shape == (3, 82)
    with pytest.raises(ValueError, match="mirror"):
        evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, encode="ray", mirror=lambda x: x)
    with pytest.raises(ValueError, match="encode"):
        evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, encode="rays")
    with pytest.raises(ValueError, match="forward_clip"):
        evaluate.evaluate_clips_batched(lift_a, clips, 27, dev, encode="ray")
    # a rank whose shard is empty (3 clips on 4 ranks) refuses a bad `encode` like the others: decided before the shards are cut
    with pytest.raises(ValueError, match="encode"):
        evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, encode="rays", rank=3, world_size=4)


def test_batched_flip_on_distorted_cameras_mirrors_the_encoded_input():
    """flip=True from raw pixels of undistort=True cameras (which mirror_pixels refuses): the rows are those of the torch
    restatement - the host-encoded rays in Clip.rays, mirror_input on the padded encoded clip, the same forwards.  Bound: the
    inputs of the two differ by at most one ulp, the poses are HIP against HIP: 2e-5 * max(1, |ref|), as the lanes tests of
    tests/test_gpu_undistort.py bound two HIP results, on the per-frame means (sums / frames, metres)."""
    from ray3d_amd import evaluate
    lifter, dev = _lifter(), torch.device("cuda:0")
    clips = _pixel_clips()
    with pytest.raises(ValueError, match="undistort"):
        evaluate.mirror_pixels(clips[0].camera, "intrinsic", H36M_LEFT, H36M_RIGHT)
    encoded = [evaluate.Clip(c.camera, host_encode(c.camera, c.rays, "ray"), c.gt_norm, c.action, c.clip_id) for c in clips]
    kw = dict(flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    with torch.no_grad():
        _, _, rows_ref = evaluate.evaluate_clips(lifter.forward_clip, encoded, 27, dev, **kw)
        _, _, rows = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, encode="ray", **kw)
        _, _, rows_plain = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, encode="ray")
    torch.cuda.synchronize()
    assert torch.equal(rows[:, :3], rows_ref[:, :3])
    assert not torch.equal(rows[:, 3], rows_plain[:, 3])                    # the flip pass did something
    got, ref = (rows[:, 3:] / rows[:, 2:3]).cpu().numpy(), (rows_ref[:, 3:] / rows_ref[:, 2:3]).cpu().numpy()
    fin = np.isfinite(ref)                                                  # (the velocity of the one-frame clip is NaN in both)
    assert np.array_equal(np.isfinite(got), fin) and fin.sum() == 14
    tol = 2e-5 * max(1.0, float(np.abs(ref[fin]).max()))
    print("flip rows: max |diff| %.3e (tol %.3e)" % (float(np.abs(got[fin] - ref[fin]).max()), tol))
    check_parity(got[fin], ref[fin], "flip from raw pixels vs the torch restatement (HIP against HIP)", tol=tol)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case,keyword", [("screen_trj", "screen"), ("intrinsic_trj", "intrinsic")])
def test_batched_two_feature_encodings_reproduce_evaluate_core(case, keyword, flip):
    """Trainer.evaluate_core's five metrics with RAY_ENCODING False (tests/golden/px2d.npz) through
    evaluate_clips_batched(encode=) on the 2-feature pair, camera-frame ground truth; the bounds of tests/test_gpu_px2d.py."""
    import ray3d_amd
    from ray3d_amd import _capi, evaluate
    from test_gpu_px2d import MPJPE_MM, OTHERS_MM, _pair
    z = np.load(os.path.join(GOLDEN, "px2d.npz"))
    w, h = z["eval/res"]
    cam = ray3d_amd.Camera(z["eval/K"], z["eval/R"], z["eval/t"], res_w=w, res_h=h)
    lifter, _ = _pair("3,3,3")
    dev = torch.device("cuda:0")
    kl, kr = list(z["eval/kps_left"]), list(z["eval/kps_right"])
    clip = evaluate.Clip(cam, z["eval/uv"], z["eval/gt_cam"], "A", 0, frame="camera")
    with torch.no_grad():
        named, _, rows = evaluate.evaluate_clips_batched(lifter.forward_clip, [clip], 27, dev, flip=flip, kps_left=kl, kps_right=kr,
                                                         encode=keyword)
    got, ref = np.array(named["A"]), z["eval/%s/metrics_flip%d" % (case, int(flip))]
    print(case, "flip", flip, "got", got, "ref", ref, "diff", got - ref)
    for name, g, r, tol in zip(_capi.METRIC_NAMES, got, ref, (MPJPE_MM,) + (OTHERS_MM,) * 4):
        record_parity("clips_encode px2d evaluation %s flip%d %s (mm)" % (case, int(flip), name), abs(g - r), tol, abs(r))
    assert abs(got[0] - ref[0]) < MPJPE_MM, (got, ref)
    assert np.abs(got - ref).max() < OTHERS_MM, (got, ref)


def test_batched_evaluation_with_encode_on_lanes():
    """set_lanes(2): the encode call runs on the caller's stream, the clips' forwards (plain and mirrored slices of its buffers) on
    the lanes' streams behind it, joined once before the metrics call - the rows are those of the lane-less pass.  A lane has
    half the CUs (other tile schedules, other split-K sums): HIP against HIP, 2e-5 * max(1, |ref|) on the per-frame means, as
    the lanes tests of tests/test_gpu_undistort.py bound it."""
    from ray3d_amd import evaluate
    from test_gpu_clips_metrics import _lifter as make
    lifter = make.__wrapped__()                                      # (a pair of its own: the lanes are an option of its handles)
    dev = torch.device("cuda:0")
    clips = _pixel_clips()
    kw = dict(flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT, encode="ray")
    with torch.no_grad():
        _, _, rows_ref = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, **kw)
        torch.cuda.synchronize()
        lifter.set_lanes(2)
        try:
            _, _, rows = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 27, dev, **kw)
            torch.cuda.synchronize()
            lifter.check_status()
        finally:
            lifter.set_lanes(0)
    assert torch.equal(rows[:, :3], rows_ref[:, :3])
    got, ref = (rows[:, 3:] / rows[:, 2:3]).cpu().numpy(), (rows_ref[:, 3:] / rows_ref[:, 2:3]).cpu().numpy()
    fin = np.isfinite(ref)                                                  # (the velocity of the one-frame clip is NaN in both)
    assert np.array_equal(np.isfinite(got), fin) and fin.sum() == 14
    check_parity(got[fin], ref[fin], "encode + flip on 2 lanes vs no lanes (HIP against HIP)", tol=2e-5 * max(1.0, float(np.abs(ref[fin]).max())))


# ------------------------------------------------------------------ hipGraph

def test_encode_and_forward_clip_captured_in_a_hip_graph():
    """r3d_clips_encode and a forward_clip of a prepared size captured together (torch.cuda.graph, default queue settings):
    replayed after new pixels were written into the captured archive, the poses equal the eager run on those pixels."""
    from ray3d_amd import _capi, evaluate
    from test_gpu_clips_metrics import _lifter as make
    lifter = make.__wrapped__()                                      # (a pair of its own: it pins a schedule)
    dev = torch.device("cuda:0")
    n, cam = 64, cameras()[2]
    assert lifter.clip_batch_sizes(n) == [n]
    px = torch.from_numpy(pixels("clips_encode.graph.a", (n, 17, 2))).cuda()
    px2 = torch.from_numpy(pixels("clips_encode.graph.b", (n, 17, 2))).cuda()
    tab = torch.from_numpy(_one_clip_table(n, cam, 13, 13).view(np.uint8)).cuda()
    prow = torch.from_numpy(cam.param()).cuda()
    x = torch.zeros((n + 26, 17, 3), device=dev)
    xm = torch.zeros((n + 26, 17, 3), device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    out = torch.empty((n, 1, 17, 3), device=dev)
    perm = mirror_perm(17)
    lifter.prepare([n])
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    lifter._ws.get(_capi.workspace_bytes(hp, ht, n), dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            evaluate.shard_encode_hip(px, tab, 1, n + 26, n + 26, "ray", perm, x_all=x, x_mirror_all=xm, status=status)
            lifter.forward_clip(x, prow, out=out, n_windows=n)
    px.copy_(px2)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        ex, exm, est = evaluate.shard_encode_hip(px2, tab, 1, n + 26, n + 26, "ray", perm)
        eager = lifter.forward_clip(ex, prow, n_windows=n)
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(est[0]) == 0
    assert torch.equal(x, ex) and torch.equal(xm, exm)
    assert torch.isfinite(eager).all() and torch.equal(out, eager)
    del g
    torch.cuda.synchronize()
    _capi.release(hp, ht, n)
