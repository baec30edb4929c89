"""-m gpu: the HIP path (through the C ABI) against the reference-generated golden fixtures and
the CPU oracle.  Tolerance: the literal 1e-4 abs on fp32 3D joint positions (BASELINE.json north_star),
the deliberately over-scaled '_big' fixture (outputs of up to 108 m) included."""
import os
import numpy as np
import pytest
import torch

from conftest import MODEL_CASES, case_out_scale, check_parity, dev_switch, hooks_library, load_model_fixture, synth_states

pytestmark = pytest.mark.gpu

ATOL = 1e-4


def tol_for(ref):
    return ATOL


def build_modules(mc, out_scale=1.0, device="cuda:0"):
    import ray3d_amd
    (cp, sp), (ct, st) = synth_states(mc, out_scale)
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos.eval(), trj.eval()
    return pos, trj, (cp, sp), (ct, st)


# Calls of <= 48 windows run the library's un-fused "small" plan (r3d_plan.cpp, plan_is_small); the fixtures' few windows
# must hold on the fused plan too (partial first-level / pair tiles with a handful of valid rows): both are run.
PLANS = [pytest.param(False, id="small-plan"), pytest.param(True, id="fused-plan")]


@pytest.mark.parametrize("fused", PLANS)
@pytest.mark.parametrize("name", MODEL_CASES)
def test_modules_match_reference_fixture(name, fused, monkeypatch):
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")
    z, mc = load_model_fixture(name)
    pos, trj, _, _ = build_modules(mc, case_out_scale(name))
    x = torch.from_numpy(z["x"]).cuda()
    p = torch.from_numpy(z["param"]).cuda()
    with torch.no_grad():
        op = pos(x, p).cpu().numpy()
        ot = trj(x, p).cpu().numpy()
    assert op.shape == z["out_pos"].shape and ot.shape == z["out_trj"].shape
    check_parity(op, z["out_pos"], "pos vs reference fixture")
    check_parity(ot, z["out_trj"], "trj vs reference fixture")


@pytest.mark.parametrize("fused", PLANS)
@pytest.mark.parametrize("name", MODEL_CASES)
def test_lifter_pair_matches_reference_fixture(name, fused, monkeypatch):
    import ray3d_amd
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")
    z, mc = load_model_fixture(name)
    pos, trj, _, _ = build_modules(mc, case_out_scale(name))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x = torch.from_numpy(z["x"]).cuda()
    p = torch.from_numpy(z["param"]).cuda()
    with torch.no_grad():
        out, out_trj = lifter(x, p, return_trj=True)
    ref = z["out_pos"] + z["out_trj"]
    check_parity(out.cpu().numpy(), ref, "pos+trj vs reference fixture")
    check_parity(out_trj.cpu().numpy(), z["out_trj"], "trj vs reference fixture")


# Every reference fixture again in the modes the two tests above do not reach: the bf16x3 arithmetic (r3d_config.bf16x3
# through model_config['BF16X3']; its tiles run from 96 windows per call on, so the fixture's windows are tiled to 128 -
# which is also the fully fused plan) and the level-by-level form (R3D_OPT_STAGED through set_staged: the documented
# fallback for shared GPUs, and what models of more than 256 channels and the dense ablation always run).
MODES = [pytest.param(False, id="f32"), pytest.param(True, id="bf16x3")]
FORMS = [pytest.param(False, id="single-launch"), pytest.param(True, id="staged")]


@pytest.mark.parametrize("staged", FORMS)
@pytest.mark.parametrize("b3", MODES)
@pytest.mark.parametrize("name", MODEL_CASES)
def test_reference_fixture_in_every_mode_and_form(name, b3, staged):
    import ray3d_amd
    if os.environ.get("R3D_BF16X3") is not None and b3 != (os.environ["R3D_BF16X3"] == "1"):
        pytest.skip("R3D_BF16X3 in the environment overrides the configuration key")
    z, mc = load_model_fixture(name)
    pos, trj, _, _ = build_modules(dict(mc, BF16X3=b3), case_out_scale(name))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.set_staged(staged)
    reps = -(-128 // z["x"].shape[0])
    x = torch.from_numpy(np.tile(z["x"], (reps, 1, 1, 1))).cuda()
    p = torch.from_numpy(np.tile(z["param"], (reps, 1))).cuda()
    with torch.no_grad():
        out, out_trj = lifter(x, p, return_trj=True)
        op = pos(x, p)                                   # (the modules alone: one network per call)
    lifter.check_status()
    assert lifter.precision(x.device) == ("bf16x3" if b3 else "f32")
    # (the one exception to the literal bound: the opt-in bf16x3 arithmetic on the deliberately over-scaled fixture, outputs
    #  of up to 108 m - 1.05e-4 there, 1e-6 of the magnitude; the bound relative to 10 m, as the fixture was scaled)
    tol = ATOL * float(np.abs(z["out_pos"] + z["out_trj"]).max()) / 10.0 if (b3 and name.endswith("_big")) else None
    check_parity(out.cpu().numpy(), np.tile(z["out_pos"] + z["out_trj"], (reps, 1, 1, 1)), "pos+trj vs reference fixture", tol=tol)
    check_parity(out_trj.cpu().numpy(), np.tile(z["out_trj"], (reps, 1, 1, 1)), "trj vs reference fixture", tol=tol)
    check_parity(op.cpu().numpy(), np.tile(z["out_pos"], (reps, 1, 1, 1)), "pos vs reference fixture", tol=tol)


# ---------------------------------------------------------------- oracle parity beyond the fixtures

@pytest.mark.parametrize("fused", PLANS)
@pytest.mark.parametrize("arch,batch", [("3,3", 1), ("3,3", 37), ("3,3,3", 100), ("3,3,3,3", 33), ("3,3,3,3,3", 5)])
def test_lifter_matches_oracle_ragged_batches(arch, batch, fused, monkeypatch):
    """Batch sizes that are not multiples of any tile (row masking, partial schedules)."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")
    mc = ray3d_amd.default_model_config(ARCHITECTURE=arch)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x = synth.synth_rays(batch, cp, seed=21)
    p = synth.synth_param(batch, seed=22)
    with torch.no_grad():
        out = lifter(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()).cpu().numpy()
    ref = oracle.forward(cp, sp, x, p) + oracle.forward(ct, st, x, p)
    check_parity(out, ref)


@pytest.mark.parametrize("over", [dict(ARCHITECTURE="3,3,3,3,3"), dict(ARCHITECTURE="3,3", NUM_KPTS=14),
                                  dict(ARCHITECTURE="3,3,3", STAGE=1, CAMERA_EMBDDING=False)])
def test_calls_of_one_to_four_windows_run_the_gemv_tiles(over, monkeypatch):
    """Calls of up to four windows: every layer with at most four rows (the MLPs, the top of the pyramid) runs as
    32-column GEMV tiles (r3d_kernels.hip, gemv_tile: weights streamed once, K split over the wavefronts, no MFMA) -
    against the oracle, and against the MFMA split-K tiles the same call would use otherwise (R3D_NO_GEMV=1)."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    mc = ray3d_amd.default_model_config(**over)
    for B in (1, 2, 3, 4):
        outs = []
        for no_gemv in ("0", "1"):
            dev_switch(monkeypatch, "R3D_NO_GEMV", no_gemv)
            pos, trj, (cp, sp), (ct, st) = build_modules(mc)          # (the switch is read when a schedule is built: fresh handles)
            x, p = synth.synth_rays(B, cp, seed=91), synth.synth_param(B, seed=92)
            pt = torch.from_numpy(p).cuda() if cp.camera_embedding else None
            with torch.no_grad():
                outs.append(ray3d_amd.Ray3DLifter(pos, trj).eval()(torch.from_numpy(x).cuda(), pt).cpu().numpy())
        ref = oracle.forward(cp, sp, x, p) + oracle.forward(ct, st, x, p)
        check_parity(outs[0], ref, "%d windows, GEMV tiles" % B)
        check_parity(outs[1], ref, "%d windows, MFMA split-K tiles" % B)
        assert not np.array_equal(outs[0], outs[1])                  # (two different evaluations)


@pytest.mark.parametrize("over", [dict(ARCHITECTURE="3,3,3,3,3"), dict(ARCHITECTURE="3,3", NUM_KPTS=15, STAGE=2)])
def test_calls_of_five_to_32_windows_run_the_latency_tiles(over, monkeypatch):
    """Layers of 5 .. 32 rows (the MLPs and the pyramid's top in calls of up to 32 windows) run as 32-column latency tiles on
    the matrix cores (lat_tile: K split over the wavefronts, all operands requested up front) - against the oracle and
    against the split-K gemm tiles the call would use otherwise (R3D_NO_LAT=1)."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    mc = ray3d_amd.default_model_config(**over)
    for B in (5, 11, 32):
        outs = []
        for no_lat in ("0", "1"):
            dev_switch(monkeypatch, "R3D_NO_LAT", no_lat)
            pos, trj, (cp, sp), (ct, st) = build_modules(mc)
            x, p = synth.synth_rays(B, cp, seed=93), synth.synth_param(B, seed=94)
            with torch.no_grad():
                outs.append(ray3d_amd.Ray3DLifter(pos, trj).eval()(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()).cpu().numpy())
        ref = oracle.forward(cp, sp, x, p) + oracle.forward(ct, st, x, p)
        check_parity(outs[0], ref, "%d windows, latency tiles" % B)
        check_parity(outs[1], ref, "%d windows, split-K tiles" % B)
        assert not np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("per_frame", [True, False], ids=["per-frame-first-layers", "gathered"])
def test_forward_clip_equals_materialised_windows(per_frame, monkeypatch):
    """In-kernel sliding windows (window_stride = 1) == eval_data_prepare's copies (trainer.py:47-58).  A clip call
    evaluates expand_conv once per input FRAME (first_level_shared: E[first frame] + V[current frame] instead of one
    gathered product per window row - another summation order, same values to fp32 rounding); with that switched off
    (R3D_NO_SHARED_L0, hooks build) the two calls are the same arithmetic in the same order: bit-identical."""
    import ray3d_amd
    from ray3d_amd import synth
    if not per_frame:
        dev_switch(monkeypatch, "R3D_NO_SHARED_L0", "1")
    elif os.environ.get("R3D_BF16X3") == "1":
        pytest.skip("bf16x3 handles keep the gathered first level (the per-frame form exists for the fp32 tiles)")
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, _), _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    n, rf = 150, 27
    clip = synth.synth_rays(1, ray3d_amd.LiftConfig("pos", 17, 3, (3,) * 3), seed=5)[0]          # (27,17,3)
    clip = np.concatenate([clip] * 7, axis=0)[: n + rf - 1] + 0.01 * np.arange(n + rf - 1, dtype=np.float32)[:, None, None]
    windows = np.stack([clip[i:i + rf] for i in range(n)])
    prow = np.array([1.5, 0.2], np.float32)
    with torch.no_grad():
        lifter.CLIP_ROUND = 0                                     # one forward of exactly n windows
        a = lifter.forward_clip(torch.from_numpy(clip).cuda(), torch.from_numpy(prow).cuda()).cpu().numpy()
        b = lifter(torch.from_numpy(windows).cuda(), torch.from_numpy(np.tile(prow, (n, 1))).cuda()).cpu().numpy()
        assert a.shape == (n, 1, 17, 3)
        if per_frame:
            check_parity(a, b, "clip call (per-frame first layers) vs the same windows materialised", tol=1e-5 * max(1.0, float(np.abs(b).max())))
            assert not np.array_equal(a, b)    # (it did take the other path)
        else:
            assert np.array_equal(a, b)        # same arithmetic, same order: bit-identical
        # chunked: 64 windows per forward, the last chunk rounded up to a multiple of 32 over repeated last frames
        lifter.CLIP_CHUNK, lifter.CLIP_ROUND = 64, 32
        c = lifter.forward_clip(torch.from_numpy(clip).cuda(), torch.from_numpy(prow).cuda())
        assert c.shape == (n, 1, 17, 3) and c.is_contiguous()
        # other batch sizes, other split-K tiles: last-bit differences on outputs of several metres
        assert np.abs(c.cpu().numpy() - b).max() <= 1e-5 * max(1.0, np.abs(b).max())
        c += 1.0                                                   # caller-owned and writable (trainer.py:353)


def _reference_cameras():
    """The real H36M / 3DHP calibration tables of tests/golden/cameras.npz (reference-generated), as product cameras
    and as oracle cameras (the C restatement, pinned to the same fixture by tests/test_oracle.py)."""
    import os
    import ray3d_amd
    from conftest import GOLDEN
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    tags = [t for t in z["tags"]]
    return ([ray3d_amd.Camera(z[t + "/K"], z[t + "/R"], z[t + "/t"]) for t in tags],
            [oracle.Camera(z[t + "/K"], z[t + "/R"], z[t + "/t"]) for t in tags], z, tags)


def _dhp_cameras():
    """The 14 MPI-INF-3DHP cameras of tests/golden/cameras_3dhp.npz (lib/dataset/mpii_3dhp_dataset.py:9-251, generated by
    the reference's CameraInfoPacket) as product and as oracle cameras."""
    import os
    import ray3d_amd
    from conftest import GOLDEN
    from oracle import oracle
    z = np.load(os.path.join(GOLDEN, "cameras_3dhp.npz"))
    tags = [t for t in z["tags"]]
    assert len(tags) == 14
    return ([ray3d_amd.Camera(z[t + "/K"], z[t + "/R"], z[t + "/t"]) for t in tags],
            [oracle.Camera(z[t + "/K"], z[t + "/R"], z[t + "/t"]) for t in tags], z, tags)


@pytest.mark.parametrize("arch,B", [("3,3", 1024), ("3,3,3,3,3", 140)])
def test_cfg4_3dhp_mixed_intrinsics_one_of_the_14_cameras_per_window(arch, B):
    """BASELINE configs[3] as SURVEY 8(d) words it: J = 17, the shipped RF 9 architecture (cfg_ray3d_3dhp_stage3.py:77-89)
    AND RF 243, every window of the batch with its own camera drawn from the 14 3DHP cameras, undistort=False, input =
    pixels + per-window camera rows.  Parity vs the reference = encode each window with ITS CameraInfoPacket (here: the
    oracle camera, pinned to the reference's uv -> ray pairs of all 14) and run the model on the rays."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    cams, ocams, z, tags = _dhp_cameras()
    for oc, t in zip(ocams, tags):
        assert np.abs(oc.rays_from_uv(z[t + "/uv"]) - z[t + "/rays"]).max() < 1e-12
    mc = ray3d_amd.default_model_config(ARCHITECTURE=arch)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    rf = cp.receptive_field
    uv = (2048.0 * synth.hash_uniform("uvcfg4.%d" % rf, (B, rf, 17, 2), 13)).astype(np.float32)
    pick = [(5 * i + i // 14) % 14 for i in range(B)]
    assert len(set(pick)) == 14
    rays = np.stack([ocams[c].rays_from_uv(uv[i].astype(np.float64)) for i, c in enumerate(pick)]).astype(np.float32)
    rows = np.stack([cams[c].cam_row() for c in pick])
    par = np.stack([cams[c].param() for c in pick])
    with torch.no_grad():
        a = lifter.forward_uv(torch.from_numpy(uv).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(par).cuda())
    ref = _oracle_lift(((cp, sp), (ct, st)), rays, par)
    check_parity(a, ref, "UV mode, all windows vs torch port on oracle-encoded rays")
    idx = [0, 1, 13, 14, B // 2, B - 1]
    cref = oracle.forward(cp, sp, rays[idx], par[idx]) + oracle.forward(ct, st, rays[idx], par[idx])
    check_parity(a[idx], cref, "UV mode, 6 windows vs C oracle")


@pytest.mark.parametrize("fused", PLANS)
@pytest.mark.parametrize("arch,B", [("3,3", 24), ("3,3,3,3,3", 48)])
def test_forward_uv_matches_oracle_on_reference_cameras(arch, B, fused, monkeypatch):
    """BASELINE configs[3] (mixed intrinsics per batch) at RF 9 and RF 243: pixel keypoints + one camera row PER WINDOW in,
    rays encoded inside the first-level gather.  Comparand: the ORACLE chain - rays from the oracle's camera restatement
    (float64, pinned to the reference's uv -> ray pairs in cameras.npz), cast as lib/train_val/trainer.py:298 does, through
    oracle.forward.  Also: bit-identical to the HIP path fed with those rays (the encoding is the same float64 arithmetic),
    and no more launches than the rays mode (no separate encoding kernel)."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")     # (the gather inside the fused first level / inside r3d_gemm_enc_uv_f32)
    cams, ocams, z, tags = _reference_cameras()
    mc = ray3d_amd.default_model_config(ARCHITECTURE=arch)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    rf = cp.receptive_field
    uv = (1000.0 * synth.hash_uniform("uvtest%d" % rf, (B, rf, 17, 2), 9)).astype(np.float32)
    pick = [i % len(cams) for i in range(B)]
    rays = np.stack([ocams[c].rays_from_uv(uv[i].astype(np.float64)) for i, c in enumerate(pick)]).astype(np.float32)
    # the fixture's own uv -> ray pairs pin that encoding to the reference
    t0 = tags[0]
    assert np.abs(ocams[0].rays_from_uv(z[t0 + "/uv"]) - z[t0 + "/rays"]).max() < 1e-12
    rows = np.stack([cams[c].cam_row() for c in pick])
    par = np.stack([cams[c].param() for c in pick])
    uvd, rowsd, pard = torch.from_numpy(uv).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(par).cuda()
    with torch.no_grad():
        a = lifter.forward_uv(uvd, rowsd, pard)
        b = lifter(torch.from_numpy(rays).cuda(), pard)
    ref = oracle.forward(cp, sp, rays, par) + oracle.forward(ct, st, rays, par)
    check_parity(a.cpu().numpy(), ref)
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    h = lifter.pos.handle(uvd.device)
    counts = []
    for run in (lambda: lifter.forward_uv(uvd, rowsd, pard), lambda: lifter(torch.from_numpy(rays).cuda(), pard)):
        h.profile_enable(True)
        with torch.no_grad():
            run()
        recs = [r for r in h.profile_read() if r["stage"] >= 0]
        h.profile_enable(False)
        counts.append(len(recs))
        assert not any("prologue" in r["kernel"] for r in recs)
    assert counts[0] == counts[1], counts


@pytest.mark.parametrize("fused", PLANS)
def test_forward_uv_overlapping_windows_each_with_its_own_camera(fused, monkeypatch):
    """Windows that share frames but not the camera (window_stride < RF with per-window camera rows): every window's
    frames are encoded with THAT window's camera - equal to materialising the windows and encoding each on the host.
    Also the sliding-clip form (stride 1, one camera) against forward_clip on host-encoded rays."""
    import ray3d_amd
    from ray3d_amd import synth
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")
    cams, _, _, _ = _reference_cameras()
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, _), _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    rf, stride, B = 27, 5, 40
    T = (B - 1) * stride + rf
    seq = (1000.0 * synth.hash_uniform("uvseq", (T, 17, 2), 3)).astype(np.float32)
    pick = [cams[(3 * i) % len(cams)] for i in range(B)]
    windows = np.stack([pick[i].rays_from_uv(seq[i * stride:i * stride + rf].astype(np.float64)) for i in range(B)]).astype(np.float32)
    rows, par = np.stack([c.cam_row() for c in pick]), np.stack([c.param() for c in pick])
    with torch.no_grad():
        lifter.CLIP_ROUND = 0                                     # exact sizes: one forward of B windows
        a = lifter.forward_uv(torch.from_numpy(seq).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(par).cuda(),
                              window_stride=stride)
        b = lifter(torch.from_numpy(windows).cuda(), torch.from_numpy(par).cuda())
        assert a.shape == (B, 1, 17, 3) and np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        # a sequence is lifted in the batch sizes of clip_batch_sizes (every clip length would otherwise build its own
        # tile schedule): chunks of 16 windows + a tail rounded up to 8, surplus windows over repeated last frames with
        # the last camera, cut off - per-window camera and parameter rows follow their chunk
        lifter.CLIP_CHUNK, lifter.CLIP_ROUND = 16, 8
        assert lifter.clip_batch_sizes(B) == [16, 16, 8]
        a2 = lifter.forward_uv(torch.from_numpy(seq[:(B - 3 - 1) * stride + rf]).cuda(), torch.from_numpy(rows[:B - 3]).cuda(),
                               torch.from_numpy(par[:B - 3]).cuda(), window_stride=stride)       # 37 windows: 16 + 16 + 8 with 3 surplus
        assert a2.shape == (B - 3, 1, 17, 3) and a2.is_contiguous()
        assert np.abs(a2.cpu().numpy() - b[:B - 3].cpu().numpy()).max() <= 1e-5 * max(1.0, float(b.abs().max()))
        lifter.CLIP_CHUNK, lifter.CLIP_ROUND = 4096, 0
        cam = cams[1]
        n = 100
        clip_uv = (1000.0 * synth.hash_uniform("uvclip", (n + rf - 1, 17, 2), 4)).astype(np.float32)
        c = lifter.forward_uv(torch.from_numpy(clip_uv).cuda(), torch.from_numpy(cam.cam_row()).cuda(),
                              torch.from_numpy(cam.param()).cuda())
        d = lifter.forward_clip(torch.from_numpy(cam.rays_from_uv(clip_uv.astype(np.float64)).astype(np.float32)).cuda(),
                                torch.from_numpy(cam.param()).cuda())
    assert c.shape == (n, 1, 17, 3) and np.array_equal(c.cpu().numpy(), d.cpu().numpy())


def _oracle_lift(states, windows, prm, threads=None):
    """pos + trj through oracle/torch_port.py (the PyTorch-CPU restatement, pinned to the reference fixtures)."""
    from oracle import torch_port
    (cp, sp), (ct, st) = states
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]
    out = []
    with torch.no_grad():
        for i in range(0, windows.shape[0], 512):
            xw, pw = torch.from_numpy(windows[i:i + 512]), torch.from_numpy(prm[i:i + 512])
            out.append((torch_port.forward(cp, sds[0], xw, pw) + torch_port.forward(ct, sds[1], xw, pw)).numpy())
    return np.concatenate(out)


def test_h36m_shape_eval_rf243_against_the_oracle_chain():
    """BASELINE configs[2] on one GPU: the Human3.6M evaluation SHAPE (the data set is not in the image: synthetic clips,
    lengths ~ U(1000, 6000) frames, four cameras, fifteen actions) at RF 243 through evaluate_clips(forward_clip) with the
    default chunking (4096 windows per forward, tail rounded to 128) and r3d_clip_metrics.  Against the oracle chain
    (lib/train_val/trainer.py:283-405 restated: edge pad, materialised windows, CPU forward, float64 world transform,
    NumPy metrics): the per-clip partial rows of three whole clips, and 64 sampled frames of every other clip."""
    import ray3d_amd
    from ray3d_amd import evaluate
    from oracle import oracle, metrics_oracle as mo
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    assert (lifter.CLIP_CHUNK, lifter.CLIP_ROUND) == (4096, 128)
    rng = np.random.default_rng(0)
    cams = [ray3d_amd.synthetic_camera(yaw, 4.5, -12.0, name="cam%d" % i) for i, yaw in enumerate((20, 110, 200, 290))]
    clips = []
    n_clips = 40
    for i in range(n_clips):
        n = int(rng.integers(1000, 6001))
        cam = cams[i % 4]
        # a slowly moving skeleton: per-frame noise on a random walk, so that sliding windows differ from frame to frame
        world = rng.normal(0, 0.3, (1, 17, 3)) + np.array([0, 0, 1.0]) + 0.02 * np.cumsum(rng.normal(0, 1.0, (n, 1, 3)), axis=0) \
            + rng.normal(0, 0.02, (n, 17, 3))
        rays = cam.rays_from_uv(cam.project(world)).astype(np.float32)
        clips.append(evaluate.Clip(cam, rays, cam.world2normalized(world).astype(np.float32), "A%d" % (i % 15), i))
    dev = torch.device("cuda:0")
    with torch.no_grad():
        named, avg, rows = evaluate.evaluate_clips(lifter.forward_clip, clips, 243, dev)
        torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    assert rows.shape == (n_clips, evaluate.PARTIAL_COLS) and np.all(np.isfinite(rows))
    assert sorted(rows[:, 0].astype(int).tolist()) == list(range(n_clips))
    assert len(named) == 15
    by_id = {int(r[0]): r for r in rows}
    order = sorted(range(n_clips), key=lambda i: clips[i].rays.shape[0])
    whole = [order[0], order[1], order[len(order) // 3]]           # three whole clips (the two shortest and a mid-sized one)
    states = ((cp, sp), (ct, st))
    for cid in range(n_clips):
        c = clips[cid]
        n = c.rays.shape[0]
        assert int(by_id[cid][2]) == n
        padded = evaluate.pad_clip(c.rays, 121)                      # generators.py:213-216
        if cid in whole:
            frames = np.arange(n)
        else:
            # the seams of the 2048-window chunks and of the rounded tail, the clip's ends, and random frames
            seams = np.clip([0, 1, n - 2, n - 1, 2047, 2048, (n // 2048) * 2048 - 1, (n // 2048) * 2048], 0, n - 1)
            frames = np.unique(np.concatenate([seams, rng.integers(0, n, 64)]))[:64]
        windows = np.stack([padded[i:i + 243] for i in frames])    # trainer.py:47-58
        prm = np.tile(c.camera.param(), (len(frames), 1))            # trainer.py:297,324
        ref = _oracle_lift(states, windows, prm).reshape(len(frames), 17, 3)
        if cid in whole:
            pw, gw = c.camera.normalized2world(ref), c.camera.normalized2world(c.gt_norm)       # trainer.py:358-359
            want = np.array([mo.mpjpe(pw, gw), mo.p_mpjpe(pw, gw), mo.n_mpjpe(pw[:, None], gw[:, None]),
                             mo.mean_velocity_error(pw, gw), mo.mpjpe(pw[:, :1], gw[:, :1])]) * 1000.0
            got = by_id[cid][3:8] / n * 1000.0
            assert np.abs(got - want).max() < 0.1, (cid, n, got, want)                      # millimetres
            # the C restatement on a few of the same windows (the torch port is the bulk checker)
            few = [0, n // 2, n - 1]
            cref = (oracle.forward(cp, sp, windows[few], prm[few]) + oracle.forward(ct, st, windows[few], prm[few])).reshape(3, 17, 3)
            assert np.abs(cref - ref[few]).max() <= 1e-4
        else:
            with torch.no_grad():
                pred = evaluate.predict_clip(lifter.forward_clip, c, 243, dev)
            got = pred.reshape(n, 17, 3)[torch.from_numpy(frames).to(dev)].cpu().numpy()
            check_parity(got, ref)



def test_last_clock_reports_the_shader_clock_of_a_single_launch_forward():
    """r3d_last_clock: workgroup 0 of the persistent kernel stamps its cycle counter and the 100 MHz wall clock at both ends;
    the ratio is the shader clock of that forward (bench.py's roofline.clk_ghz).  0 for a level-by-level forward."""
    import ray3d_amd
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, _), _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x = torch.from_numpy(synth.synth_rays(256, cp, seed=1)).cuda()
    p = torch.from_numpy(synth.synth_param(256, seed=2)).cuda()
    assert lifter.last_clock_ghz("cuda:0") == 0.0                  # nothing ran yet
    with torch.no_grad():
        for _ in range(30):
            out = lifter(x, p)
        ghz = lifter.last_clock_ghz("cuda:0")
        if os.environ.get("R3D_STAGED") == "1":
            assert ghz == 0.0
            return
        assert 0.5 < ghz < 2.6, ghz                               # (MI355X: 2.4 GHz maximum)
        lifter.set_staged(True)
        assert torch.equal(lifter(x, p), out)
        assert lifter.last_clock_ghz("cuda:0") == 0.0


def test_clip_calls_run_the_per_frame_first_layers():
    """A call whose windows slide over a clip one frame at a time (trainer.py:47-58) evaluates expand_conv once per input
    frame: a launch of gathered GEMMs ahead of the forward, then r3d_forward_clip_f32 (first_level_shared).  Checked here:
    which kernels run (rays and pixel input; per-window cameras and independent windows keep the gathered path), the
    oracle on every window, the level-by-level form, and a captured call replayed on new clip contents."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import torch_port
    if os.environ.get("R3D_BF16X3") == "1":
        pytest.skip("bf16x3 handles keep the gathered first level (the per-frame form exists for the fp32 tiles)")
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.CLIP_ROUND = 0
    rf, n = 81, 200
    cams, ocams, _, _ = _dhp_cameras()
    cam = cams[2]
    rng = np.random.default_rng(11)
    uv = (rng.uniform(200, 1800, (1, 17, 2)) + np.cumsum(rng.normal(0, 3.0, (n + rf - 1, 17, 2)), axis=0)).astype(np.float32)
    rays = cam.rays_from_uv(uv.astype(np.float64)).astype(np.float32)
    prow = cam.param().astype(np.float32)
    windows = np.stack([rays[i:i + rf] for i in range(n)])
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
    with torch.no_grad():
        ref = (torch_port.forward(cp, sds[0], torch.from_numpy(windows), torch.from_numpy(np.tile(prow, (n, 1)))) +
               torch_port.forward(ct, sds[1], torch.from_numpy(windows), torch.from_numpy(np.tile(prow, (n, 1))))).numpy()
    names = lambda recs: [r["kernel"] for r in recs]
    clip_d, uv_d = torch.from_numpy(rays).cuda(), torch.from_numpy(uv).cuda()
    p_d, row_d = torch.from_numpy(prow).cuda(), torch.from_numpy(cam.cam_row()).cuda()
    staged_env = os.environ.get("R3D_STAGED") == "1"
    with torch.no_grad():
        a = lifter.forward_clip(clip_d, p_d)
        check_parity(a, ref, "rays clip")
        recs = names(lifter.profile_call(lambda: lifter.forward_clip(clip_d, p_d), "cuda:0"))
        if not staged_env:
            assert "r3d_forward_clip_f32" in recs and "r3d_forward_f32" not in recs and recs.count("r3d_gemm_f32") == 1, recs
        b = lifter.forward_uv(uv_d, row_d, p_d)                   # pixel clip, ONE camera: per-frame first layers too
        check_parity(b, ref, "pixel clip, one camera")
        recs = names(lifter.profile_call(lambda: lifter.forward_uv(uv_d, row_d, p_d), "cuda:0"))
        if not staged_env:
            assert "r3d_forward_clip_uv_f32" in recs and recs.count("r3d_gemm_uv_f32") == 1, recs
        rows = row_d.view(1, 8).expand(n, 8).contiguous()        # a camera row PER WINDOW: frames have no single camera - gathered path
        c = lifter.forward_uv(uv_d, rows, p_d)
        check_parity(c, ref, "pixel clip, a camera row per window")
        recs = names(lifter.profile_call(lambda: lifter.forward_uv(uv_d, rows, p_d), "cuda:0"))
        if not staged_env:
            assert "r3d_forward_uv_f32" in recs and "r3d_forward_clip_uv_f32" not in recs, recs
        w = lifter(torch.from_numpy(windows).cuda(), p_d.view(1, 2).expand(n, 2).contiguous())   # independent windows: nothing to share
        check_parity(w, ref, "materialised windows")
        # a captured clip call (per-frame launch + forward in the graph), replayed on another clip behind the same pointer
        lifter.prepare([n])
        out = torch.empty((n, 1, 17, 3), device="cuda")
        g, s_ = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        buf = clip_d.clone()
        with torch.cuda.stream(s_):
            with torch.cuda.graph(g, stream=s_):
                lifter._run(ray3d_amd._capi.R3D_INPUT_RAYS, buf, 1, n, p_d, 0, out=out)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)
        buf.copy_(torch.flip(clip_d, dims=[0]))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, lifter.forward_clip(torch.flip(clip_d, dims=[0]).contiguous(), p_d))
        # the level-by-level form (R3D_OPT_STAGED) reads the same per-frame buffer
        lifter.set_staged(True)
        check_parity(lifter.forward_clip(clip_d, p_d), ref, "rays clip, level by level")
        assert torch.equal(lifter.forward_clip(clip_d, p_d), a)


@pytest.mark.parametrize("over", [dict(ARCHITECTURE="3,3"), dict(ARCHITECTURE="3,3", NUM_KPTS=14, STAGE=2),
                                  dict(ARCHITECTURE="3,3,3", NUM_KPTS=15), dict(ARCHITECTURE="3,3,3", CHANNELS=128, LATENT_FEATURES_DIM=160),
                                  dict(ARCHITECTURE="3,3,3,3", DISABLE_OPTIMIZATIONS=True, CAUSAL=True),
                                  dict(ARCHITECTURE="3,3,3", INPUT_DIM=2, CAMERA_EMBDDING=False)],
                         ids=["rf9", "j14-rf9-s2", "j15-rf27", "c128", "rf81-causal-dilated", "f2-noemb"])
def test_clip_calls_of_many_lengths_equal_their_materialised_windows(over):
    """forward_clip over clips of 1 ... ~700 windows (every tail size of clip_batch_sizes, chunks of 256: the plans of
    small, medium and large calls; per-frame first layers where the plan has them) against the same windows materialised
    and lifted as independent windows - the two differ in summation order at most.  At 130 windows (a plan with the
    per-frame first layers where the variant has them) the clip call is also held to the ORACLE - the torch port of the
    reference graph on the materialised windows - so that the per-frame [E | V] fold of every variant's tables (J = 14 / 15
    groups, 128 channels, causal-dilated, two input features) is checked against the reference arithmetic, not only against
    this library's own window path."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import torch_port
    mc = ray3d_amd.default_model_config(**over)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.CLIP_CHUNK = 256
    rf, J, F = cp.receptive_field, cp.num_joints, cp.in_features
    rng = np.random.default_rng(123)
    prow = torch.from_numpy(np.array([1.4, 0.15], np.float32)).cuda()
    for n in (1, 2, 3, 5, 11, 17, 40, 64, 97, 130, 257, 300, 511, 700):
        clip = (rng.normal(0, 0.4, (1, J, F)) + np.cumsum(rng.normal(0, 0.03, (n + rf - 1, J, F)), axis=0)).astype(np.float32)
        windows = np.stack([clip[i:i + rf] for i in range(n)])
        with torch.no_grad():
            a = lifter.forward_clip(torch.from_numpy(clip).cuda(), prow)
            b = lifter(torch.from_numpy(windows).cuda(), prow.view(1, 2).expand(n, 2).contiguous() if cp.camera_embedding else None)
        assert a.shape == (n, 1, J, 3)
        check_parity(a, b.cpu().numpy(), "%d windows" % n, tol=2e-5 * max(1.0, float(b.abs().max())))
        if n == 130:
            with torch.no_grad():
                pw = torch.from_numpy(np.tile(prow.cpu().numpy(), (n, 1)))
                ref = (torch_port.forward(cp, sds[0], torch.from_numpy(windows), pw) +
                       torch_port.forward(ct, sds[1], torch.from_numpy(windows), pw)).numpy()
            check_parity(a, ref, "130 windows, clip call against the oracle")


def test_rf243_flip_tta_and_uv_clip_mode_against_the_oracle_chain():
    """RF 243 with what the h36m-shape test leaves out: (a) flip test-time augmentation (lib/train_val/trainer.py:299-302,
    338-353: mirrored input, mirrored output, mean) through evaluate_clips, against the oracle chain restated here with
    the torch port; (b) UV clip mode - an edge-padded PIXEL clip, window stride 1, one 3DHP camera, rays encoded in the
    first-level gather - against the oracle camera + torch port.  Decoder scale LITERAL_SCALE: every output below 10 m, so
    both run at the literal 1e-4 abs bound."""
    import ray3d_amd
    from ray3d_amd import evaluate
    from oracle import metrics_oracle as mo
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc, LITERAL_SCALE)
    states = ((cp, sp), (ct, st))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    cams, ocams, _, _ = _dhp_cameras()
    rng = np.random.default_rng(5)
    kl, kr = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
    dev = torch.device("cuda:0")
    clips, worlds = [], []
    for i, n in enumerate((150, 333)):
        cam = cams[3 + 5 * i]
        world = rng.normal(0, 0.3, (1, 17, 3)) + np.array([0, 0, 1.0]) + 0.02 * np.cumsum(rng.normal(0, 1.0, (n, 1, 3)), axis=0) \
            + rng.normal(0, 0.02, (n, 17, 3))
        # (3DHP's world frame is not the z-up frame of this synthetic walk: keep the skeleton in front of the camera by
        # placing it in the camera frame instead)
        pc = world + np.array([0.0, 0.0, 3.0])
        uvp = np.stack([pc[..., 0] / pc[..., 2] * cam.fx + cam.cx, pc[..., 1] / pc[..., 2] * cam.fy + cam.cy], -1)
        rays = cam.rays_from_uv(uvp).astype(np.float32)
        gt = (pc @ cam.Rc2n.T + cam.Tc2n.T).astype(np.float32)
        clips.append(evaluate.Clip(cam, rays, gt, "A%d" % i, i))
        worlds.append(uvp)
    # ---- (a) flip TTA
    with torch.no_grad():
        named, avg, rows = evaluate.evaluate_clips(lifter.forward_clip, clips, 243, dev, flip=True, kps_left=kl, kps_right=kr)
        preds = [evaluate.predict_clip(lifter.forward_clip, c, 243, dev, True, kl, kr).cpu().numpy() for c in clips]
    by_id = {int(r[0]): r for r in rows.cpu().numpy()}           # (rows come in shard order: longest clip first)
    for c, pred in zip(clips, preds):
        row = by_id[c.clip_id]
        n = c.rays.shape[0]
        padded = evaluate.pad_clip(c.rays, 121)
        windows = np.stack([padded[i:i + 243] for i in range(n)])
        prm = np.tile(c.camera.param(), (n, 1))
        ref = _oracle_lift(states, windows, prm)
        wm = windows.copy()                                       # trainer.py:299-302
        wm[..., 0] *= -1
        wm[:, :, kl + kr] = wm[:, :, kr + kl]
        refm = _oracle_lift(states, wm, prm)
        refm[..., 0] *= -1                                        # trainer.py:340-342
        refm[:, :, kl + kr] = refm[:, :, kr + kl]
        ref = (0.5 * (ref.astype(np.float64) + refm)).astype(np.float32)     # trainer.py:343-345 (mean of the two passes)
        assert np.abs(ref).max() <= 10.0
        check_parity(pred, ref, "RF 243 flip-TTA, clip of %d frames" % n)
        pw, gw = c.camera.normalized2world(ref.reshape(n, 17, 3)), c.camera.normalized2world(c.gt_norm)
        want = np.array([mo.mpjpe(pw, gw), mo.p_mpjpe(pw, gw), mo.n_mpjpe(pw[:, None], gw[:, None]),
                         mo.mean_velocity_error(pw, gw), mo.mpjpe(pw[:, :1], gw[:, :1])]) * 1000.0
        assert np.abs(row[3:8] / n * 1000.0 - want).max() < 0.1          # millimetres
    # ---- (b) UV clip mode: pixels in, stride 1, one camera for the clip
    for ci, (c, uvp) in enumerate(zip(clips, worlds)):
        n = uvp.shape[0]
        cam, ocam = c.camera, ocams[3 + 5 * ci]
        uv_pad = evaluate.pad_clip(uvp.astype(np.float32), 121)
        with torch.no_grad():
            got = lifter.forward_uv(torch.from_numpy(uv_pad).cuda(), torch.from_numpy(cam.cam_row()).cuda(),
                                    torch.from_numpy(cam.param()).cuda())
        assert got.shape == (n, 1, 17, 3)
        rays_pad = ocam.rays_from_uv(uv_pad.astype(np.float64)).astype(np.float32)       # the oracle's camera, float64 then cast
        windows = np.stack([rays_pad[i:i + 243] for i in range(n)])
        ref = _oracle_lift(states, windows, np.tile(cam.param(), (n, 1)))
        assert np.abs(ref).max() <= 10.0
        check_parity(got, ref, "RF 243 UV clip mode, clip of %d frames" % n)


@pytest.mark.parametrize("flip", [False, True])
def test_evaluate_clips_reproduces_reference_metrics(flip):
    """Whole eval loop on the GPU vs Trainer.evaluate_core's five metrics (tests/golden/evalcore.npz)."""
    import os
    import ray3d_amd
    from conftest import GOLDEN
    from ray3d_amd import evaluate
    z = np.load(os.path.join(GOLDEN, "evalcore.npz"))
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, _, _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    clips = [evaluate.Clip(ray3d_amd.Camera(z["clip%d/K" % i], z["clip%d/R" % i], z["clip%d/t" % i]),
                           z["clip%d/rays" % i], z["clip%d/gt_norm" % i], "A", i) for i in range(3)]
    with torch.no_grad():
        named, avg, rows = evaluate.evaluate_clips(lifter.forward_clip, clips, 27, torch.device("cuda:0"), flip=flip,
                                                   kps_left=list(z["kps_left"]), kps_right=list(z["kps_right"]))
    ref = z["metrics_flip%d" % int(flip)]
    assert np.abs(np.array(named["A"]) - ref).max() < 5e-2, (named["A"], ref)   # mm; MPJPE itself to 0.05 mm
    assert abs(named["A"][0] - ref[0]) < 2e-2


# ---------------------------------------------------------------- full-size properties (BASELINE sizes)

LITERAL_SCALE = 0.25     # decoder scale at which the RF-243 outputs stay below 10 m: the bound is then the literal 1e-4


@pytest.mark.parametrize("out_scale", [pytest.param(1.0, id="scale1"), pytest.param(LITERAL_SCALE, id="literal-1e-4")])
def test_full_size_batch_properties(out_scale):
    """B = 256, RF 243 (BASELINE configs[1]): permutation equivariance, split invariance, determinism,
    and oracle agreement on every window at the literal 1e-4 abs bound of north_star - with the synthetic decoders at scale 1
    (outputs of up to ~23 m) and at a scale that keeps every output below 10 m."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc, out_scale)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    B = 256
    x = synth.synth_rays(B, cp, seed=31)
    p = synth.synth_param(B, seed=32)
    xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    with torch.no_grad():
        full = lifter(xd, pd)
        again = lifter(xd, pd)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(0)).cuda()
        permuted = lifter(xd[perm].contiguous(), pd[perm].contiguous())
        halves = torch.cat([lifter(xd[:100].contiguous(), pd[:100].contiguous()),
                            lifter(xd[100:].contiguous(), pd[100:].contiguous())])
    assert torch.equal(full, again)                                   # deterministic (no atomics)
    # different batch sizes get different tile schedules (incl. split-K tiles), i.e. different fp32
    # summation orders: agreement is to rounding noise of the ~14-layer chain, not bit-exact
    assert (full[perm] - permuted).abs().max().item() <= 6e-5         # windows are independent
    assert (full - halves).abs().max().item() <= 6e-5
    # every window against the oracle chain (torch port: every tile class - first / last row unit of every launch, the
    # spilled first-level tiles, the split-K tiles of the M = B layers), and a spread of them against the C restatement
    ref_all = _oracle_lift(((cp, sp), (ct, st)), x, p)
    if out_scale != 1.0:
        assert np.abs(ref_all).max() <= 10.0                          # the literal bound applies
    check_parity(full.cpu().numpy(), ref_all, "all windows vs torch port")
    idx = [0, 31, 32, 77, 128, 200, 254, 255]
    ref = oracle.forward(cp, sp, x[idx], p[idx]) + oracle.forward(ct, st, x[idx], p[idx])
    check_parity(full[idx].cpu().numpy(), ref, "8 windows vs C oracle")
    # output buffer is fresh and caller-owned (callers mutate it in place, trainer.py:340-353)
    full += 1.0
    assert not torch.equal(full, again)


@pytest.mark.parametrize("out_scale", [pytest.param(1.0, id="scale1"), pytest.param(LITERAL_SCALE, id="literal-1e-4")])
def test_large_batch_1024(out_scale):
    """north_star's 1024 x 243 x 17 shape: finite, equal to four 256-window calls, and 134 windows spread over every tile
    class against the oracle (at decoder scale 1 and at the scale where the literal 1e-4 abs bound applies)."""
    import ray3d_amd
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    pos, trj, (cp, _), _ = build_modules(mc, out_scale)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x = torch.from_numpy(synth.synth_rays(1024, cp, seed=41)).cuda()
    p = torch.from_numpy(synth.synth_param(1024, seed=42)).cuda()
    with torch.no_grad():
        big = lifter(x, p)
        parts = torch.cat([lifter(x[i:i + 256].contiguous(), p[i:i + 256].contiguous()) for i in range(0, 1024, 256)])
    assert torch.isfinite(big).all()
    assert (big - parts).abs().max().item() <= 6e-5
    idx = np.unique(np.concatenate([np.arange(0, 1024, 8), [1, 31, 32, 33, 1022, 1023]]))      # 134 windows over every tile class
    (cp, sp), (ct, st) = synth_states(mc, out_scale)
    ref = _oracle_lift(((cp, sp), (ct, st)), x[idx].cpu().numpy(), p[idx].cpu().numpy())
    if out_scale != 1.0:
        assert np.abs(ref).max() <= 10.0
    check_parity(big[idx].cpu().numpy(), ref, "134 windows vs torch port")


def test_universal_14_joint_batch_4096():
    """BASELINE configs[4]: 14-joint layout (quirk Q2's permuted output order), RF 9, 4096 windows per step with a
    different synthetic camera per window: oracle agreement on a sample, equal to eight 512-window calls."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3", NUM_KPTS=14)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    B = 4096
    x = synth.synth_rays(B, cp, seed=51)
    p = synth.synth_param(B, seed=52)                              # per-window [height, pitch]
    xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    with torch.no_grad():
        big = lifter(xd, pd)
        parts = torch.cat([lifter(xd[i:i + 512].contiguous(), pd[i:i + 512].contiguous()) for i in range(0, B, 512)])
    assert big.shape == (B, 1, 14, 3) and torch.isfinite(big).all()
    assert (big - parts).abs().max().item() <= 6e-5
    ref_all = _oracle_lift(((cp, sp), (ct, st)), x, p)              # all 4096 windows against the torch port
    check_parity(big.cpu().numpy(), ref_all)
    idx = [0, 1, 31, 32, 511, 512, 2047, 4095]
    ref = oracle.forward(cp, sp, x[idx], p[idx]) + oracle.forward(ct, st, x[idx], p[idx])
    check_parity(big[idx].cpu().numpy(), ref)


def test_empty_batch_is_rejected():
    """The reference's forward fails on an empty batch (BatchNorm/Conv on zero rows is fine in torch, but main.py never
    produces one); the library names the problem instead of launching empty grids."""
    import ray3d_amd
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3")
    pos, trj, _, _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x = torch.zeros((0, 9, 17, 3), device="cuda")
    p = torch.zeros((0, 2), device="cuda")
    with pytest.raises((RuntimeError, AssertionError)):
        lifter(x, p)


def test_weight_update_is_picked_up():
    import ray3d_amd
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config()
    pos, trj, (cp, sp), _ = build_modules(mc)
    x = torch.from_numpy(synth.synth_rays(4, cp, seed=3)).cuda()
    p = torch.from_numpy(synth.synth_param(4, seed=4)).cuda()
    with torch.no_grad():
        a = pos(x, p)
        sd = {k: v.clone() for k, v in pos.state_dict().items()}
        key = [k for k in sd if k.endswith("Integration_Torso.fc_2.bias")][0]
        sd[key] += 1.0
        pos.load_state_dict(sd)
        b = pos(x, p)
    d = (b - a)[:, 0].cpu().numpy()
    torso_slots = [0, 7, 8, 9, 10]
    assert np.allclose(d[:, torso_slots], 1.0, atol=1e-5) and np.allclose(np.delete(d, torso_slots, axis=1), 0.0, atol=1e-6)


def test_integration_md_ctypes_stub_runs_against_the_library():
    """The reference-side binding shown in INTEGRATION.md section 2 is executed verbatim (only the
    library path is made absolute) and must reproduce the reference fixture through the C ABI."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", text, flags=re.S)
    stub = next(b for b in blocks if "class HipRIE" in b)
    lib = os.path.join(root, "ray3d_amd", "libray3d_hip.so")
    stub = stub.replace('C.CDLL("libray3d_hip.so")', "C.CDLL(%r)" % lib)
    ns = {}
    exec(compile(stub, "INTEGRATION.md:hip_backend", "exec"), ns)
    z, mc = load_model_fixture("j17_rf27_s3")
    (cp, sp), (ct, st) = synth_states(mc)
    torch.cuda.set_device(0)
    x = torch.from_numpy(z["x"]).cuda()
    p = torch.from_numpy(z["param"]).cuda()
    for kind, sd, ref in ((0, sp, z["out_pos"]), (1, st, z["out_trj"])):
        mod = ns["HipRIE"](kind, mc, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        out = mod(x, p)
        torch.cuda.synchronize()
        assert out.shape == ref.shape
        check_parity(out.cpu().numpy(), ref)


def test_overlapped_half_batches_equal_the_single_pass():
    import ray3d_amd
    from ray3d_amd import synth
    z, mc = load_model_fixture("j17_rf27_s3")
    pos, trj, (cp, _), _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x = torch.from_numpy(synth.synth_rays(200, cp, seed=11)).cuda()
    p = torch.from_numpy(synth.synth_param(200, seed=12, vary=True)).cuda()
    with torch.no_grad():
        one = lifter(x, p)
        two = lifter.forward_overlapped(x, p, parts=2)
        three = lifter.forward_overlapped(x, p, parts=3)
        torch.cuda.synchronize()
    assert two.shape == one.shape
    assert (one - two).abs().max().item() <= 6e-5
    assert (one - three).abs().max().item() <= 6e-5


@pytest.mark.parametrize("over", [
    dict(ARCHITECTURE="3,3,3", CHANNELS=128, LATENT_FEATURES_DIM=160, EMBEDD_DIM=32, STAGE=2),            # narrow fused-pair tiles
    dict(ARCHITECTURE="3,3,3", CHANNELS=512, LATENT_FEATURES_DIM=128, NUM_KPTS=15, STAGE=3),              # C > 256: levels not fused
    dict(ARCHITECTURE="3,3,3,3", CHANNELS=96, LATENT_FEATURES_DIM=96, NUM_KPTS=14, INPUT_DIM=2,
         CAMERA_EMBDDING=False, STAGE=1),                                                                   # 2D input, no embedding
    dict(ARCHITECTURE="3,3", CHANNELS=1024, LATENT_FEATURES_DIM=256, EXTRINSIC_DIM=3, EMBEDD_DIM=96),      # the class-default width
])
def test_other_widths_match_oracle(over):
    """Configurations no golden fixture has (the reference's cfg files all use C = 256): channel counts that
    are not a tile width, more channels than a tile, other latent / embedding sizes."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    mc = ray3d_amd.default_model_config(**over)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    batch = 70
    x = synth.synth_rays(batch, cp, seed=31)
    p = synth.synth_param(batch, seed=32)
    if cp.extrinsic_dim != 2:
        p = np.ascontiguousarray(np.tile(p, (1, 2))[:, : max(cp.extrinsic_dim, 1)])
    pt = torch.from_numpy(p).cuda() if cp.camera_embedding else None
    with torch.no_grad():
        out = lifter(torch.from_numpy(x).cuda(), pt).cpu().numpy()
    ref = oracle.forward(cp, sp, x, p if cp.camera_embedding else None) + oracle.forward(ct, st, x, p if cp.camera_embedding else None)
    check_parity(out, ref)


@pytest.mark.parametrize("no_lat", [False, True], ids=["latency-tiles", "split-k-tiles"])
@pytest.mark.parametrize("batch", [5, 11, 32])
@pytest.mark.parametrize("channels", [64, 96, 128])
def test_narrow_channels_at_5_to_32_windows_keep_the_residual(channels, batch, no_lat, monkeypatch):
    """A pyramid level's un-fused 1x1 convolution (K = CHANNELS < 256, residual = the level's input) on the latency tiles:
    with K < 256 some wavefronts have no K tile of their own and must still add the residual to the rows they emit
    (round-3 advisor finding: they added 0).  Checked against the oracle with and without the latency tiles."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    dev_switch(monkeypatch, "R3D_NO_LAT", "1" if no_lat else "0")
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3", CHANNELS=channels, LATENT_FEATURES_DIM=128)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x = synth.synth_rays(batch, cp, seed=41)
    p = synth.synth_param(batch, seed=42)
    with torch.no_grad():
        out = lifter(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()).cpu().numpy()
    ref = oracle.forward(cp, sp, x, p) + oracle.forward(ct, st, x, p)
    check_parity(out, ref)


@pytest.mark.parametrize("over", [dict(), dict(CHANNELS=128, LATENT_FEATURES_DIM=160, STAGE=2), dict(STAGE=1, CAMERA_EMBDDING=False),
                                  dict(DENSE=True, DISABLE_OPTIMIZATIONS=True)])
def test_shrink_folded_into_its_consumers_equals_the_separate_layer(over, monkeypatch):
    """r3d_finalize composes the TemporalBlocks' `shrink` (1x1 convolution + bias, no activation: rie.py:105) with the
    Linears that read it when channels <= latent size; R3D_NO_SHRINK_FOLD=1 (read at r3d_create) keeps it a layer of its
    own.  Both must agree with the oracle, and with each other far inside the tolerance (rounding of the composed
    weights only)."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import torch_port
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3", **over)
    outs = []
    for nofold in ("0", "1"):
        dev_switch(monkeypatch, "R3D_NO_SHRINK_FOLD", nofold)
        pos, trj, (cp, sp), (ct, st) = build_modules(mc)
        x, p = synth.synth_rays(75, cp, seed=71), synth.synth_param(75, seed=72)
        pt = torch.from_numpy(p).cuda() if cp.camera_embedding else None
        with torch.no_grad():
            outs.append(ray3d_amd.Ray3DLifter(pos, trj).eval()(torch.from_numpy(x).cuda(), pt).cpu().numpy())
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
    with torch.no_grad():
        pp = torch.from_numpy(p) if cp.camera_embedding else None
        ref = (torch_port.forward(cp, sds[0], torch.from_numpy(x), pp) + torch_port.forward(ct, sds[1], torch.from_numpy(x), pp)).numpy()
    for o in outs:
        check_parity(o, ref)
    assert np.abs(outs[0] - outs[1]).max() <= 0.2 * tol_for(ref)
    assert not np.array_equal(outs[0], outs[1])          # (the switch really selects two different evaluations)


@pytest.mark.parametrize("b3", [False, True])
def test_window_counts_where_the_plan_switches(b3):
    """The library picks one of four plans per call by its window count (<= 48 nothing fused, <= 96 first level only,
    < 1024 all but the top level, from 1024 on everything: r3d_plan.cpp, plan_kind) and, in bf16x3 mode, the fp32 tiles
    below 96 windows: every window of calls on both sides of every switch against the torch port of the reference graph."""
    import ray3d_amd
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3", BF16X3=b3)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    for B in (48, 49, 95, 96, 97, 1023, 1024, 1025):
        x, p = synth.synth_rays(B, cp, seed=B), synth.synth_param(B, seed=B + 1)
        with torch.no_grad():
            out = lifter(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()).cpu().numpy()
        ref = _oracle_lift(((cp, sp), (ct, st)), x, p)
        check_parity(out, ref)


def test_rccl_gather_of_clip_partials_single_rank():
    """The exchange step of the sharded evaluation on the real backend: one all_gather of device-resident
    per-clip rows through RCCL (backend "nccl"), here with a single rank (the GPU box has one device; the
    world_size-2 logic is covered on CPU with gloo in tests/test_host.py)."""
    import os
    import socket
    import torch.distributed as dist
    import ray3d_amd
    from conftest import GOLDEN
    from ray3d_amd import evaluate
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda:0"))
    try:
        z = np.load(os.path.join(GOLDEN, "evalcore.npz"))
        mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
        pos, trj, _, _ = build_modules(mc)
        lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
        clips = [evaluate.Clip(ray3d_amd.Camera(z["clip%d/K" % i], z["clip%d/R" % i], z["clip%d/t" % i]),
                               z["clip%d/rays" % i], z["clip%d/gt_norm" % i], "A", i) for i in range(3)]
        with torch.no_grad():
            named, avg, rows = evaluate.evaluate_clips(lifter.forward_clip, clips, 27, torch.device("cuda:0"))
            gathered = evaluate.gather_partials(rows, [rows.shape[0]])
        assert gathered.is_cuda and torch.equal(gathered, rows)
        ref = z["metrics_flip0"]
        assert np.abs(np.array(evaluate.reduce_partials(gathered)[0]) - ref).max() < 5e-2
    finally:
        dist.destroy_process_group()


def test_bf16x3_mode_keeps_parity(monkeypatch):
    """R3D_BF16X3=1 (read at r3d_create): the FCBlocks' 1024-wide Linears run on the bf16 matrix cores with every
    fp32 operand split exactly into three bf16 terms (six products, fp32 accumulate).  Same tolerance as fp32."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    monkeypatch.setenv("R3D_BF16X3", "1")
    # a reference fixture (outputs of the reference's PyTorch-CPU forward) ...
    z, mc = load_model_fixture("j17_rf27_s3")
    pos, trj, _, _ = build_modules(mc)
    reps = -(-128 // z["x"].shape[0])                     # (below 96 windows per call the mode runs the fp32 tiles)
    with torch.no_grad():
        got = ray3d_amd.Ray3DLifter(pos, trj).eval()(torch.from_numpy(np.tile(z["x"], (reps, 1, 1, 1))).cuda(),
                                                     torch.from_numpy(np.tile(z["param"], (reps, 1))).cuda())
    want = np.tile(z["out_pos"] + z["out_trj"], (reps, 1, 1, 1))
    check_parity(got.cpu().numpy(), want)
    # ... and a batch with multi-unit tiles against the oracle
    mc2 = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos2, trj2, (cp2, sp2), (ct2, st2) = build_modules(mc2)
    lifter = ray3d_amd.Ray3DLifter(pos2, trj2).eval()
    xb = synth.synth_rays(600, cp2, seed=41)
    pb = synth.synth_param(600, seed=42)
    with torch.no_grad():
        out = lifter(torch.from_numpy(xb).cuda(), torch.from_numpy(pb).cuda()).cpu().numpy()
    ref = oracle.forward(cp2, sp2, xb, pb) + oracle.forward(ct2, st2, xb, pb)
    check_parity(out, ref)


def test_bf16x3_through_the_configuration_key():
    """model_config['BF16X3'] -> r3d_config.bf16x3: the same mode without the environment variable; a reference fixture
    at the fp32 tolerance, and outputs that differ from the fp32 path's (so the mode is really on)."""
    import os
    import ray3d_amd
    if os.environ.get("R3D_BF16X3") is not None:
        pytest.skip("R3D_BF16X3 in the environment overrides the configuration key")
    z, mc = load_model_fixture("j17_rf27_s3")
    # (the mode switches itself off below 96 windows per call, where the fp32 tiles are the faster ones: the fixture's
    # windows are repeated up to a batch that uses it)
    reps = -(-128 // z["x"].shape[0])
    x, p = torch.from_numpy(np.tile(z["x"], (reps, 1, 1, 1))).cuda(), torch.from_numpy(np.tile(z["param"], (reps, 1))).cuda()
    outs = []
    for flag in (False, True):
        pos, trj, _, _ = build_modules(dict(mc, BF16X3=flag))
        with torch.no_grad():
            outs.append(ray3d_amd.Ray3DLifter(pos, trj).eval()(x, p).cpu().numpy())
    want = np.tile(z["out_pos"] + z["out_trj"], (reps, 1, 1, 1))
    check_parity(outs[0], want, "f32 vs reference fixture")
    check_parity(outs[1], want, "bf16x3 vs reference fixture")
    assert not np.array_equal(outs[0], outs[1])


def test_bf16x3_error_against_float64_is_the_fp32_paths(monkeypatch):
    """The claim behind "fp32-equivalent": measured against a FLOAT64 evaluation of the same network (the torch port run
    in double precision), the bf16x3 path's error is no larger than the fp32-MFMA path's - on the RF-243 network, whose
    first level, fused pairs and 1024-wide Linears all run on the bf16 matrix cores in that mode."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import torch_port
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    (cp, sp), (ct, st) = synth_states(mc)
    B = 96
    x, p = synth.synth_rays(B, cp, seed=61), synth.synth_param(B, seed=62)
    sd64 = [{k: torch.from_numpy(np.asarray(v)).double() for k, v in s_.items() if np.asarray(v).dtype == np.float32} for s_ in (sp, st)]
    with torch.no_grad():
        x64, p64 = torch.from_numpy(x).double(), torch.from_numpy(p).double()
        ref = (torch_port.forward(cp, sd64[0], x64, p64) + torch_port.forward(ct, sd64[1], x64, p64)).numpy()
    errs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("R3D_BF16X3", mode)
        pos, trj, _, _ = build_modules(mc)
        with torch.no_grad():
            out = ray3d_amd.Ray3DLifter(pos, trj).eval()(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()).cpu().numpy()
        errs[mode] = float(np.abs(out.astype(np.float64) - ref).max())
    print("max abs error vs float64: fp32 MFMA %.3e, bf16x3 %.3e (|ref| max %.2f)" % (errs["0"], errs["1"], np.abs(ref).max()))
    assert errs["0"] <= 1e-4 and errs["1"] <= 1e-4
    assert errs["1"] <= 1.25 * errs["0"] + 1e-6


# ---------------------------------------------------------------- library-owned lanes (R3D_OPT_LANES)

def test_lanes_share_one_weight_image_and_lift_side_by_side():
    """R3D_OPT_LANES = 2 on ONE pair of handles: two library-owned CU-masked streams (lane k: the CUs c of every XCD with c % 2 ==
    k), each with its own schedules and control regions, one packed weight image.  Two different batches lifted on the two lanes
    at once equal the plain forwards (other tile schedules: to fp32 rounding) and the oracle chain; enabling the lanes and
    running both adds device memory of the order of the two workspaces - not a second 200 MB weight image; a forward issued
    on a stream that is no lane's is relayed round-robin and ordered behind join_lanes; lanes off again restores the plain path
    bit for bit."""
    import ray3d_amd
    from ray3d_amd import synth, _capi
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    dev = torch.device("cuda:0")
    B = 256
    xs = [torch.from_numpy(synth.synth_rays(B, cp, seed=81 + i)).cuda() for i in range(3)]
    ps = [torch.from_numpy(synth.synth_param(B, seed=91 + i)).cuda() for i in range(3)]
    with torch.no_grad():
        plain = [lifter(x, p).clone() for x, p in zip(xs, ps)]
        torch.cuda.synchronize()
        hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
        ws_bytes = _capi.workspace_bytes(hp, ht, B)
        free0 = torch.cuda.mem_get_info(dev)[0]
        lifter.set_lanes(2)
        assert lifter.num_lanes() == 2 and lifter.lane_stream(0).cuda_stream != lifter.lane_stream(1).cuda_stream
        outs = [None, None]
        for rep in range(3):                                  # (both lanes busy at once, repeatedly)
            for k in range(2):
                with lifter.lane(k):
                    outs[k] = lifter(xs[k], ps[k])
        lifter.join_lanes()
        torch.cuda.synchronize()
        lifter.check_status()
        added = free0 - torch.cuda.mem_get_info(dev)[0]
        print("lanes: device memory added %.1f MB; one workspace %.1f MB" % (added / 1e6, ws_bytes / 1e6))
        assert added < 2 * ws_bytes + 48e6, (added, ws_bytes)        # two lane workspaces + outputs + schedules - no second weight image (202 MB)
        for k in range(2):
            check_parity(outs[k], plain[k].cpu().numpy(), "lane %d vs the whole-chip forward (HIP against HIP)" % k,
                         tol=2e-5 * max(1.0, float(plain[k].abs().max())))
        ref = _oracle_lift(((cp, sp), (ct, st)), xs[0][:6].cpu().numpy(), ps[0][:6].cpu().numpy())
        check_parity(outs[0][:6], ref, "lane 0 vs oracle chain")
        # a forward on the caller's stream: relayed to the next lane; its result is there after join_lanes
        o2 = lifter(xs[2], ps[2])
        lifter.join_lanes()
        torch.cuda.synchronize()
        check_parity(o2, plain[2].cpu().numpy(), "relayed forward vs the whole-chip forward (HIP against HIP)", tol=2e-5 * max(1.0, float(plain[2].abs().max())))
        # ... and the library's own relay (a C caller that passes a stream of its own): r3d_forward_pair + r3d_lanes_join
        out3 = torch.empty_like(plain[2])
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        inp = _capi.make_input(_capi.R3D_INPUT_RAYS, xs[2].data_ptr(), cp.receptive_field, ps[2].data_ptr(), 2)
        cur = torch.cuda.current_stream().cuda_stream
        for _ in range(3):                                    # (three calls: lanes 0, 1, 0 again - a lane is in order)
            _capi.forward_pair(hp, ht, inp, B, out3.data_ptr(), None, ws.data_ptr(), ws.numel(), cur)
            hp.lanes_join(cur)                                # (one workspace: join before the next call reuses it)
        torch.cuda.synchronize()
        check_parity(out3, plain[2].cpu().numpy(), "library-relayed forward vs the whole-chip forward (HIP against HIP)", tol=2e-5 * max(1.0, float(plain[2].abs().max())))
        # the lanes do run side by side: a round of two forwards on two lanes takes about as long as one forward on one lane
        # (half the chip each) - not twice as long.  From the legacy default stream AND from a stream of the caller's: an event
        # recorded on the default stream is behind every blocking stream's work, which is how lanes end up taking turns
        # (measured so in round 6 before lane() / the library stopped recording there).
        def round_ms(lanes_used, reps=20):
            def once():
                for k in lanes_used:
                    with lifter.lane(k):
                        outs[k] = lifter(xs[k], ps[k])
                lifter.join_lanes()
            for _ in range(5):
                once()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                once()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps
        for where in ("default stream", "side stream"):
            ctx = torch.cuda.stream(torch.cuda.Stream()) if where == "side stream" else torch.cuda.stream(torch.cuda.current_stream())
            with ctx:
                one, two = round_ms([0]), round_ms([0, 1])
            print("lanes from the %s: one forward on one lane %.3f ms, two forwards on two lanes %.3f ms per round" % (where, one, two))
            assert two < 1.5 * one, (where, one, two)
        lifter.set_lanes(0)
        again = lifter(xs[0], ps[0])
        assert torch.equal(again, plain[0])


def test_a_lanes_forward_is_captured_on_the_lanes_own_stream_and_a_relayed_capture_is_refused():
    """R3D_OPT_LANES and hipGraphs (include/ray3d_hip.h, lanes): with the lanes' schedules pinned (r3d_prepare builds every lane's), a
    forward issued on a lane's OWN stream can be captured there and the replay - on new input contents behind the same pointers -
    equals the plain forward; a forward on a capturing stream that is no lane's would have to be relayed across streams inside the
    capture, which the library refuses with R3D_ERR_STATE instead of recording half of it."""
    import ray3d_amd
    from ray3d_amd import synth, _capi
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, _), _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    dev = torch.device("cuda:0")
    B = 207                                                     # a batch size nothing else in this process has used
    xa = torch.from_numpy(synth.synth_rays(B, cp, seed=171)).cuda()
    xb = torch.from_numpy(synth.synth_rays(B, cp, seed=173)).cuda()
    p = torch.from_numpy(synth.synth_param(B, seed=172)).cuda()
    with torch.no_grad():
        want_a, want_b = lifter(xa, p).clone(), lifter(xb, p).clone()
        torch.cuda.synchronize()
        lifter.set_lanes(2)
        lifter.prepare([B])                                     # every lane's schedule of this size, uploaded and pinned
        with lifter.lane(1):                                    # (lane 1's workspace exists before anything is captured)
            eager = lifter(xa, p)
        lifter.join_lanes()
        torch.cuda.synchronize()
        tol = 2e-5 * max(1.0, float(want_a.abs().max()))
        check_parity(eager, want_a.cpu().numpy(), "lane 1, eager, vs the whole-chip forward (HIP against HIP)", tol=tol)
        x = xa.clone()
        out = torch.empty((B, 1, 17, 3), device=dev)
        s1 = lifter.lane_stream(1)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s1):
            with torch.cuda.graph(g, stream=s1):
                lifter._run(_capi.R3D_INPUT_RAYS, x, cp.receptive_field, B, p, 2, out=out)
        for src, want in ((xa, want_a), (xb, want_b), (xa, want_a)):
            x.copy_(src)
            out.zero_()
            torch.cuda.synchronize()
            with torch.cuda.stream(s1):
                g.replay()
            torch.cuda.synchronize()
            check_parity(out, want.cpu().numpy(), "lane 1, replayed capture, vs the whole-chip forward (HIP against HIP)", tol=tol)
        lifter.check_status()
        # a capturing stream that is no lane's: refused, nothing recorded, the handles stay usable
        hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
        ws = torch.empty(_capi.workspace_bytes(hp, ht, B), dtype=torch.uint8, device=dev)
        inp = _capi.make_input(_capi.R3D_INPUT_RAYS, x.data_ptr(), cp.receptive_field, p.data_ptr(), 2)
        side = torch.cuda.Stream()
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g2, stream=side):
                with pytest.raises(_capi_error(), match="cannot be captured from a caller's stream"):
                    _capi.forward_pair(hp, ht, inp, B, out.data_ptr(), None, ws.data_ptr(), ws.numel(), side.cuda_stream)
                out.add_(0.0)                                   # (a capture must not end empty)
        with lifter.lane(0):
            after = lifter(xb, p)
        lifter.join_lanes()
        torch.cuda.synchronize()
        check_parity(after, want_b.cpu().numpy(), "lane 0 after the refused capture (HIP against HIP)", tol=tol)
        lifter.release_prepared()
        lifter.set_lanes(0)
        assert torch.equal(lifter(xa, p), want_a)


def test_lanes_join_is_per_issuing_stream():
    """Two caller streams relay one forward each (lanes 0 and 1); stream A joins first.  A's join must not make lane 1 look joined
    to stream B: B's own join still has to wait for B's forward - a copy of its output enqueued on B right behind the join holds the
    poses, not the zeros the buffer held before.  (The first version kept one `pending` flag per lane and cleared it at ANY join.)
    Through the C ABI (r3d_forward_pair + r3d_lanes_join) and through Ray3DLifter (forward on a side stream + join_lanes)."""
    import ray3d_amd
    from ray3d_amd import synth, _capi
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    pos, trj, (cp, _), _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    dev = torch.device("cuda:0")
    B = 512                                                      # (a forward of about 2 ms on half the chip: long against a join)
    xa = torch.from_numpy(synth.synth_rays(B, cp, seed=181)).cuda()
    xb = torch.from_numpy(synth.synth_rays(B, cp, seed=183)).cuda()
    p = torch.from_numpy(synth.synth_param(B, seed=182)).cuda()
    with torch.no_grad():
        want_a, want_b = lifter(xa, p).clone(), lifter(xb, p).clone()
        torch.cuda.synchronize()
        tol = 2e-5 * max(1.0, float(want_a.abs().max()), float(want_b.abs().max()))
        lifter.set_lanes(2)
        hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
        nws = _capi.workspace_bytes(hp, ht, B)
        ws_a, ws_b = (torch.empty(nws, dtype=torch.uint8, device=dev) for _ in range(2))
        out_a, out_b = torch.zeros_like(want_a), torch.zeros_like(want_b)
        snap_a, snap_b = torch.empty_like(want_a), torch.empty_like(want_b)
        inp_a = _capi.make_input(_capi.R3D_INPUT_RAYS, xa.data_ptr(), cp.receptive_field, p.data_ptr(), 2)
        inp_b = _capi.make_input(_capi.R3D_INPUT_RAYS, xb.data_ptr(), cp.receptive_field, p.data_ptr(), 2)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        for rep in range(3):
            out_a.zero_()
            out_b.zero_()
            torch.cuda.synchronize()
            _capi.forward_pair(hp, ht, inp_a, B, out_a.data_ptr(), None, ws_a.data_ptr(), ws_a.numel(), sa.cuda_stream)
            _capi.forward_pair(hp, ht, inp_b, B, out_b.data_ptr(), None, ws_b.data_ptr(), ws_b.numel(), sb.cuda_stream)
            hp.lanes_join(sa.cuda_stream)                       # A first ...
            hp.lanes_join(sb.cuda_stream)                       # ... B's join still waits for B's forward
            with torch.cuda.stream(sb):
                snap_b.copy_(out_b)
            with torch.cuda.stream(sa):
                snap_a.copy_(out_a)
            torch.cuda.synchronize()
            check_parity(snap_b, want_b.cpu().numpy(), "C ABI, stream B behind its own join (HIP against HIP)", tol=tol)
            check_parity(snap_a, want_a.cpu().numpy(), "C ABI, stream A behind its own join (HIP against HIP)", tol=tol)
        # the same through the module: forwards issued on two side streams are relayed by Ray3DLifter.lane()
        for rep in range(3):
            torch.cuda.synchronize()
            with torch.cuda.stream(sa):
                oa = lifter(xa, p)
            with torch.cuda.stream(sb):
                ob = lifter(xb, p)
            with torch.cuda.stream(sa):
                lifter.join_lanes()
                ca = oa.clone()
            with torch.cuda.stream(sb):
                lifter.join_lanes()
                cb = ob.clone()
            torch.cuda.synchronize()
            check_parity(cb, want_b.cpu().numpy(), "module, stream B behind its own join (HIP against HIP)", tol=tol)
            check_parity(ca, want_a.cpu().numpy(), "module, stream A behind its own join (HIP against HIP)", tol=tol)
        lifter.check_status()
        lifter.set_lanes(0)


def test_two_threads_with_their_own_handles_and_streams():
    """include/ray3d_hip.h, threading: different handles may be driven from different threads.  Two threads, each with its own pair of
    handles and its own stream, issue single-launch forwards at the same time (ctypes releases the GIL inside the call): every result
    equals the one-thread result bit for bit and no forward gives up waiting for its tiles - the library's ordering of whole-device
    forwards (waits, launch, note of the last forward's stream) is one critical section, so two of them never share the chip."""
    import threading
    import ray3d_amd
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    B, reps = 256, 40
    lifters, xs, wants = [], [], []
    for t in range(2):
        pos, trj, (cp, _), _ = build_modules(mc)
        lifters.append(ray3d_amd.Ray3DLifter(pos, trj).eval())
        xs.append(torch.from_numpy(synth.synth_rays(B, cp, seed=191 + t)).cuda())
    p = torch.from_numpy(synth.synth_param(B, seed=190)).cuda()
    with torch.no_grad():
        for t in range(2):
            wants.append(lifters[t](xs[t], p).clone())
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    errors, gate = [], threading.Barrier(2)

    def work(t):
        try:
            with torch.no_grad(), torch.cuda.stream(streams[t]):
                gate.wait()
                for _ in range(reps):
                    out = lifters[t](xs[t], p)
                    if not torch.equal(out, wants[t]):          # (the comparison synchronises this thread's stream)
                        errors.append("thread %d: a forward differs from the one-thread result" % t)
                        return
                lifters[t].check_status()
        except Exception as e:                                   # noqa: BLE001 - reported by the assertion below
            errors.append("thread %d: %r" % (t, e))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    torch.cuda.synchronize()
    assert not any(th.is_alive() for th in threads), "a thread hangs"
    assert not errors, errors


def test_lanes_keep_the_abort_contract(monkeypatch):
    """A lane's forward that cannot finish (hooks build: R3D_FAULT_TILE makes a tile never report) ends as without lanes: bounded
    spin, NaN outputs, r3d_status (which waits for the lanes) raises through check_status - and checked() repeats the call level
    by level on the lane and gets the poses."""
    import ray3d_amd
    from ray3d_amd import synth
    if os.environ.get("R3D_STAGED") == "1":
        pytest.skip("one launch per level: stream order, no ready counters to miss")
    hooks_library()
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.set_spin_timeout_ms(100)
    B = 200
    x, p = torch.from_numpy(synth.synth_rays(B, cp, seed=5)).cuda(), torch.from_numpy(synth.synth_param(B, seed=6)).cuda()

    def call():
        with lifter.lane(1):
            return lifter(x, p)
    with torch.no_grad():
        lifter.set_lanes(2)
        good = call()
        lifter.join_lanes()
        torch.cuda.synchronize()
        dev_switch(monkeypatch, "R3D_FAULT_TILE", "0")
        bad = call()
        lifter.join_lanes()
        with pytest.raises(_capi_error(), match="gave up after 100 ms"):
            lifter.check_status()
        assert torch.isnan(bad).all()
        with pytest.warns(UserWarning, match="level-by-level"):
            fixed = lifter.checked(call)
        monkeypatch.delenv("R3D_FAULT_TILE")
    assert lifter.pos._staged
    check_parity(fixed, good.cpu().numpy(), "level by level on a lane vs the single launch on it (HIP against HIP)", tol=2e-5 * max(1.0, float(good.abs().max())))
    ref = _oracle_lift(((cp, sp), (ct, st)), x[:8].cpu().numpy(), p[:8].cpu().numpy())
    check_parity(fixed[:8], ref, "after the fault: vs oracle chain")


# ---------------------------------------------------------------- the fp32 tiles' error budget

def _f64_and_cpu_errors(cp, sp, ct, st, x, p):
    """(float64 evaluation of the torch port, max abs error of the torch-CPU fp32 evaluation against it)."""
    from oracle import torch_port
    sd32 = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
    sd64 = [{k: (v.double() if v.dtype == torch.float32 else v) for k, v in s_.items()} for s_ in sd32]
    with torch.no_grad():
        x32, p32 = torch.from_numpy(x), torch.from_numpy(p)
        ref = (torch_port.forward(cp, sd64[0], x32.double(), p32.double()) + torch_port.forward(ct, sd64[1], x32.double(), p32.double())).numpy()
        cpu = (torch_port.forward(cp, sd32[0], x32, p32) + torch_port.forward(ct, sd32[1], x32, p32)).numpy()
    return ref, cpu


# what "no worse than the CPU's fp32" means here: the reference's own arithmetic (ATen's blocked fp32 sums) against a float64
# evaluation of the same graph is the yardstick; a tile kind whose max error exceeds BUDGET x that yardstick (+ one fp32 ulp of
# the output magnitude) accumulates in a worse order than anything a PyTorch user of the reference would see.
# (Measured on the round-5 tiles, 42 fixture x plan-kind pairs: HIP / torch-CPU error ratios 0.6 .. 2.03 - the maxima are over a few
#  hundred outputs and noisy; 36 pairs are below 1.5, the dense-ablation fixture is the 2.03.  The guard is set where every existing
#  tile kind passes with a margin of the noise and a tile with a worse summation order - one long sequential chain where the others
#  block - does not: 2 x the CPU's error + one ulp of the output magnitude; 1.5 x on the benchmark batch, whose 13 k outputs
#  make the maxima stable (measured 1.31).)
F32_BUDGET = float(os.environ.get("R3D_F32_BUDGET", "2.0"))
F32_BUDGET_BENCH = 1.5
BUDGET_KINDS = ["small", "fused", "staged", "clip"]


@pytest.mark.parametrize("kind", BUDGET_KINDS)
@pytest.mark.parametrize("name", MODEL_CASES)
def test_f32_error_budget_against_float64_per_plan_kind(name, kind, monkeypatch):
    """The fp32 path is at 8.9e-5 of the literal 1e-4 on the over-scaled fixture: a tile with another summation order must
    be judged on ERROR GROWTH, not on luck with one fixture.  For every reference fixture and every plan kind - the un-fused
    plan of calls of a few windows, the fully fused single launch (windows tiled to 128), the level-by-level form, a clip
    call (per-frame first layers where the plan has them; 130 windows sliding over the fixture's frames) - the HIP result's
    max error against a FLOAT64 evaluation of the torch port is at most F32_BUDGET x the torch-CPU fp32 evaluation's error
    against the same float64 values, + one ulp of the output magnitude (lib/model/rie.py:94-97 is the arithmetic both evaluate)."""
    import ray3d_amd
    z, mc = load_model_fixture(name)
    scale = case_out_scale(name)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc, scale)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x, p = z["x"], z["param"]
    rf = cp.receptive_field
    if kind == "clip":
        # a clip made of the fixture's frames: window i = frames [i, i + rf)
        n = 130
        frames = np.concatenate([w for w in x], axis=0)
        reps = -(-(n + rf - 1) // frames.shape[0])
        clip = np.tile(frames, (reps, 1, 1))[: n + rf - 1].copy()
        clip += (0.002 * np.arange(clip.shape[0], dtype=np.float32))[:, None, None]        # (no two windows alike)
        xw = np.stack([clip[i:i + rf] for i in range(n)])
        pw = np.tile(p[:1], (n, 1))
        with torch.no_grad():
            out = lifter.forward_clip(torch.from_numpy(clip).cuda(), torch.from_numpy(p[0]).cuda()).cpu().numpy()
    else:
        reps = 1 if kind == "small" else -(-128 // x.shape[0])
        xw, pw = np.tile(x, (reps, 1, 1, 1)), np.tile(p, (reps, 1))
        lifter.set_staged(kind == "staged")
        with torch.no_grad():
            out = lifter(torch.from_numpy(xw).cuda(), torch.from_numpy(pw).cuda()).cpu().numpy()
    lifter.check_status()
    ref, cpu = _f64_and_cpu_errors(cp, sp, ct, st, xw, pw)
    e_hip = float(np.abs(out.astype(np.float64) - ref).max())
    e_cpu = float(np.abs(cpu.astype(np.float64) - ref).max())
    ulp = float(np.abs(ref).max()) * 2.0 ** -23
    print("%s %s: HIP %.3e, torch-CPU fp32 %.3e (ratio %.2f), |ref| max %.2f" % (name, kind, e_hip, e_cpu, e_hip / max(e_cpu, 1e-30), np.abs(ref).max()))
    from conftest import record_parity
    record_parity("f32-budget %s %s (HIP err vs float64; bound = %.1f x torch-CPU fp32 err + 1 ulp)" % (name, kind, F32_BUDGET),
                  e_hip, F32_BUDGET * e_cpu + ulp, float(np.abs(ref).max()))
    assert e_hip <= F32_BUDGET * e_cpu + ulp, (name, kind, e_hip, e_cpu)


def test_f32_error_budget_on_the_benchmark_batch():
    """The same budget on BASELINE configs[1] itself: 256 synthetic 243-frame windows, pos + trj, the default (single-launch)
    form and the level-by-level one."""
    import ray3d_amd
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    B = 256
    x, p = synth.synth_rays(B, cp, seed=3), synth.synth_param(B, seed=4)
    ref, cpu = _f64_and_cpu_errors(cp, sp, ct, st, x, p)
    e_cpu = float(np.abs(cpu.astype(np.float64) - ref).max())
    ulp = float(np.abs(ref).max()) * 2.0 ** -23
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    from conftest import record_parity
    for staged in (False, True):
        lifter.set_staged(staged)
        with torch.no_grad():
            out = lifter(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()).cpu().numpy()
        lifter.check_status()
        e_hip = float(np.abs(out.astype(np.float64) - ref).max())
        print("cfg 2, %s: HIP %.3e, torch-CPU fp32 %.3e (ratio %.2f)" % ("staged" if staged else "single launch", e_hip, e_cpu, e_hip / max(e_cpu, 1e-30)))
        record_parity("f32-budget cfg2 256 windows %s (bound = %.1f x torch-CPU fp32 err + 1 ulp)" % ("staged" if staged else "single-launch", F32_BUDGET_BENCH),
                      e_hip, F32_BUDGET_BENCH * e_cpu + ulp, float(np.abs(ref).max()))
        assert e_hip <= 1e-4
        assert e_hip <= F32_BUDGET_BENCH * e_cpu + ulp, (staged, e_hip, e_cpu)


# ---------------------------------------------------------------- per-clip error sums on the device

def _metric_sums_hip(pred, gt, R, T):
    from ray3d_amd import _capi
    p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).cuda()
    g = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).cuda()
    out = torch.full((_capi.METRIC_OUT_DOUBLES,), -1.0, dtype=torch.float64, device="cuda")
    _capi.clip_metrics(p.data_ptr(), g.data_ptr(), p.shape[0], p.shape[1], R, T, out.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out[:5].cpu().numpy()


def _metric_sums_oracle(pred, gt, R, T):
    from oracle import metrics_oracle as mo
    pw = np.asarray(pred, np.float32).astype(np.float64) @ R.T + T.reshape(1, 1, 3)
    gw = np.asarray(gt, np.float32).astype(np.float64) @ R.T + T.reshape(1, 1, 3)
    n = pw.shape[0]
    vel = n * mo.mean_velocity_error(pw, gw) if n > 1 else float("nan")
    return np.array([n * mo.mpjpe(pw, gw), n * mo.p_mpjpe(pw, gw), n * mo.n_mpjpe(pw[:, None], gw[:, None]), vel,
                     n * mo.mpjpe(pw[:, :1], gw[:, :1])])


@pytest.mark.gpu
@pytest.mark.parametrize("n,J", [(1, 17), (2, 17), (300, 17), (5000, 17), (40000, 14), (777, 15)])
def test_clip_metrics_kernel_matches_oracle(n, J):
    """r3d_clip_metrics vs the NumPy restatement of lib/loss/loss.py (pinned to the reference by losses.npz)."""
    rng = np.random.default_rng(n + J)
    gt = rng.normal(0, 0.4, (n, J, 3)).astype(np.float32) + np.array([0, 0, 1.0], np.float32)
    pred = gt + rng.normal(0, 0.05, (n, J, 3)).astype(np.float32)
    if n >= 300:
        pred[7] = gt[7] * np.array([-1, 1, 1], np.float32)          # a mirrored pose: the fit must not reflect
        pred[11] = gt[11]                                            # exact prediction: zero error, no NaN
        gt[13, :, 2] = 1.0                                           # planar ground truth: rank-2 correlation
        pred[13, :, 2] = 1.0
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R, T = q * np.sign(np.linalg.det(q)), rng.normal(size=3)
    got, want = _metric_sums_hip(pred, gt, R, T), _metric_sums_oracle(pred, gt, R, T)
    if n == 1:
        assert np.isnan(got[3]) and np.isnan(want[3])
        got, want = np.delete(got, 3), np.delete(want, 3)
    assert np.all(np.isfinite(got))
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (got, want)
    again = _metric_sums_hip(pred, gt, R, T)
    assert np.array_equal(np.delete(again, 3) if n == 1 else again, got)      # fixed summation order


@pytest.mark.gpu
def test_clip_metrics_known_answers_and_errors():
    import os
    from conftest import GOLDEN
    from ray3d_amd import _capi
    z = np.load(os.path.join(GOLDEN, "losses.npz"))            # values computed by the reference's lib/loss/loss.py
    a, b = z["pred"].reshape(-1, 17, 3), z["target"].reshape(-1, 17, 3)
    n = a.shape[0]
    got = _metric_sums_hip(a, b, np.eye(3), np.zeros(3))
    # the fixture's inputs are float64; the kernel takes the model's float32 outputs
    assert abs(got[0] / n - float(z["mpjpe"])) < 1e-6
    assert abs(got[1] / n - float(z["p_mpjpe"])) < 1e-6
    assert abs(got[2] / n - float(z["n_mpjpe"])) < 1e-6
    assert abs(got[3] / n - float(z["mpjve"])) < 1e-6
    t = torch.zeros(_capi.METRIC_OUT_DOUBLES, dtype=torch.float64, device="cuda")
    with pytest.raises(_capi.Ray3DHipError, match="num_joints"):
        _capi.clip_metrics(t.data_ptr(), t.data_ptr(), 4, 18, np.eye(3), np.zeros(3), t.data_ptr(), 0)
    with pytest.raises(_capi.Ray3DHipError, match="n_frames"):
        _capi.clip_metrics(t.data_ptr(), t.data_ptr(), 0, 17, np.eye(3), np.zeros(3), t.data_ptr(), 0)


@pytest.mark.gpu
def test_archives_to_metrics_end_to_end(tmp_path):
    """Pose archives (the reference's npz layout) -> clips -> in-kernel sliding windows -> device metrics, against the
    same chain done with the oracle: windows materialised on the host, C oracle forward, NumPy metrics."""
    import os
    import ray3d_amd
    from conftest import GOLDEN
    from ray3d_amd import dataset, evaluate
    from oracle import oracle, metrics_oracle as mo
    z = np.load(os.path.join(GOLDEN, "dataset.npz"))
    acts = [str(a) for a in z["actions"]]
    p3, p2 = str(tmp_path / "d3.npz"), str(tmp_path / "d2.npz")
    np.savez_compressed(p3, positions_3d={"TS1": {a: z["in3d/%d" % i] for i, a in enumerate(acts)}})
    np.savez_compressed(p2, positions_2d={"TS1": {a: [z["in2d/%d" % i]] for i, a in enumerate(acts)}},
                        metadata={"layout_name": "3dhp", "num_joints": 17,
                                  "keypoints_symmetry": [[4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]]})
    cams = dataset.cameras_from_tables({"TS1": [{"R": z["table_R"], "translation": z["table_translation"],
                                                 "focal_length": z["table_focal_length"], "center": z["table_center"]}]})
    pd = dataset.load_pose_data(p3, p2, cams, ["TS1"])
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    with torch.no_grad():
        named, avg, rows = evaluate.evaluate_clips(lifter.forward_clip, pd.clips, 27, torch.device("cuda:0"),
                                                   kps_left=pd.kps_left, kps_right=pd.kps_right,
                                                   joints_left=pd.joints_left, joints_right=pd.joints_right)
    # the same numbers the long way round
    want = {}
    for key, ids in pd.actions.items():
        tot = np.zeros(5)
        frames = 0
        for cid in ids:
            c = pd.clips[cid]
            n = c.rays.shape[0]
            padded = evaluate.pad_clip(c.rays, 13)
            windows = np.stack([padded[i:i + 27] for i in range(n)])
            prm = np.tile(c.camera.param(), (n, 1))
            pred = (oracle.forward(cp, sp, windows, prm) + oracle.forward(ct, st, windows, prm)).reshape(n, 17, 3)
            pw, gw = c.camera.normalized2world(pred), c.camera.normalized2world(c.gt_norm)
            tot += n * np.array([mo.mpjpe(pw, gw), mo.p_mpjpe(pw, gw), mo.n_mpjpe(pw[:, None], gw[:, None]),
                                 mo.mean_velocity_error(pw, gw), mo.mpjpe(pw[:, :1], gw[:, :1])])
            frames += n
        want[key] = tot / frames * 1000.0
    assert set(named) == set(want)
    for key in want:
        # millimetres; the lifted poses differ from the oracle's by <= 1e-4 m, i.e. 0.1 mm per joint at worst
        assert np.abs(np.array(named[key]) - want[key]).max() < 0.1, (key, named[key], want[key])
    assert evaluate.format_report(named, avg)[-5].startswith("Protocol #1   (MPJPE) action-wise average:")


# ---------------------------------------------------------------- bench.py's evaluation mode / multi-GPU

def _bench_eval(gpus, clips=10):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--mode", "eval", "--gpus", str(gpus),
                          "--clips", str(clips), "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_eval_mode_single_gpu():
    """bench.py --mode eval (BASELINE configs[2] stand-in) runs end to end on one GPU and reports a finite MPJPE."""
    line = _bench_eval(1)
    assert line["n_gpus"] == 1 and line["scaling"] == "strong" and line["value"] > 0
    assert np.isfinite(line["mpjpe_mm"]["action_average"]) and line["config"]["clips"] == 10


@pytest.mark.parametrize("mode", ["windows", "eval"])
def test_bench_under_the_drivers_launcher_with_one_rank(mode):
    """The driver starts N > 1 as `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`.  One GPU is what a
    test box has: the same launch form with N = 1 initialises RCCL and runs every collective of the N > 1 path (barrier, MAX
    all_reduce, the per-rank all_gathers, in eval mode the all_gather of the per-clip rows) with one rank."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    extra = ["--full", "--no-cpu-baseline", "--no-bf16x3", "--no-shipped-cfgs", "--no-b1024", "--no-c1024"] if mode == "windows" else ["--mode", "eval", "--clips", "6"]
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"] + extra,
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["config"]["world_size_observed"] == 1
    if mode == "windows":
        assert line["parity_max_abs_err"] <= 1e-4 and len(line["config"]["ms_per_step_per_rank"]) == 1
        # the driver's multi-GPU command carries north_star's split: the 240-clip set sharded over the ranks + ONE all_gather
        ep = line["eval_pass"]
        assert ep["world_size_observed"] == 1 and ep["backend"] == "nccl" and ep["clips"] == 240 and ep["value"] > 0
        assert len(ep["shard_frames"]) == 1 and len(ep["pass_ms_per_rank"]) == 1 and ep["pass_ms_imbalance"] == 1.0
        assert ep["all_gather_ms"] >= 0 and ep["mpjpe_mm"]["checksum"] > 0 and ep["scaling"] == "strong"
    else:
        assert line["config"]["shard_imbalance"] == 1.0 and len(line["config"]["pass_ms_per_rank"]) == 1


def test_bench_plain_run_times_its_steps_and_dumps_the_last_output(tmp_path):
    """bench.py --gpus 1 --steps K --warmup W (no --full): the headline line only - none of the --full objects - and
    --dump-outputs writes the last timed step's poses, which equal those of a second run with the same arguments."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    poses = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                              "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        assert line["higher_is_better"] is True and line["unit"] == "poses/s"
        assert abs(line["value"] - 256 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
        for key in ("roofline", "roofline_b1024", "cfg4", "cfg5", "c1024", "bf16x3", "cpu_baseline", "parity", "eval_pass"):
            assert key not in line, key
        assert sorted(os.listdir(d)) == ["poses.npy"]
        poses.append(np.load(d / "poses.npy"))
    assert poses[0].shape == (256, 1, 17, 3) and poses[0].dtype == np.float32 and np.isfinite(poses[0]).all()
    assert np.array_equal(poses[0], poses[1])


def test_clip_sharded_eval_over_rccl_two_gpus():
    """Two ranks over RCCL (started by bench.py itself through torch.distributed.run): whole clips sharded longest
    first, ONE all_gather of the per-clip rows; the gathered errors must equal the single-rank run's.  Skipped on a
    box with one GPU (the CPU suite covers the same logic with gloo, tests/test_host.py)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    one, two = _bench_eval(1), _bench_eval(2)
    assert two["n_gpus"] == 2
    assert two["mpjpe_mm"] == one["mpjpe_mm"]            # same clips, same kernels, fixed summation order: identical


def test_camera_augmented_14_joint_batch_uv_mode():
    """BASELINE configs[4] with the reference's camera grid: 14-joint layout, RF 9, 4096 windows per step, every window
    seen by one of the 342 cameras of the 'Train' set of data/camera_augmentation.py (yaw x distance ratio x pitch around
    H36M S1 / camera 1, restated by ray3d_amd.camera_grid and pinned to the script's own functions in tests/test_host.py),
    pixel keypoints in (UV mode), against the oracle chain on every window."""
    import os
    import ray3d_amd
    from conftest import GOLDEN
    z = np.load(os.path.join(GOLDEN, "frontends.npz"))
    K = np.array([[1145.51133842, 0, 514.968197319], [0, 1144.77392808, 501.882018537], [0, 0, 1.0]])   # H36M camera 1 intrinsics
    cams = ray3d_amd.camera_grid(K, z["grid/R0"], z["grid/T0"])
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3", NUM_KPTS=14)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    B = 4096
    rng = np.random.default_rng(14)
    pick = [cams[i % len(cams)] for i in range(B)]
    # a 14-joint skeleton near the centre point, moving a little over the 9 frames, projected by each window's camera
    world = rng.normal(0, 0.25, (B, 1, 14, 3)) + np.array([0, 0, 1.0]) + 0.01 * np.cumsum(rng.normal(0, 1, (B, 9, 1, 3)), axis=1)
    uv = np.stack([c.project(world[i]) for i, c in enumerate(pick)]).astype(np.float32)
    rays = np.stack([c.rays_from_uv(uv[i].astype(np.float64)) for i, c in enumerate(pick)]).astype(np.float32)
    rows, par = np.stack([c.cam_row() for c in pick]), np.stack([c.param() for c in pick])
    with torch.no_grad():
        out = lifter.forward_uv(torch.from_numpy(uv).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(par).cuda())
    assert out.shape == (B, 1, 14, 3) and torch.isfinite(out).all()
    ref = _oracle_lift(((cp, sp), (ct, st)), rays, par)
    check_parity(out.cpu().numpy(), ref)


def test_forward_captured_in_a_hip_graph_after_prepare():
    """r3d_prepare moves the schedule build (hipMalloc + blocking copy) out of the forward, so a forward of a batch size
    the library has not seen can be captured into a hipGraph; the replay equals the eager result."""
    import ray3d_amd
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, _), _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    B = 203                                                     # a batch size nothing else in this process has used
    x = torch.from_numpy(synth.synth_rays(B, cp, seed=71)).cuda()
    p = torch.from_numpy(synth.synth_param(B, seed=72)).cuda()
    lifter.prepare([B])
    out = torch.empty((B, 1, 17, 3), device="cuda")
    lifter._ws.get(ray3d_amd._capi.workspace_bytes(lifter.pos.handle(x.device), lifter.trj.handle(x.device), B), x.device)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            lifter._run(ray3d_amd._capi.R3D_INPUT_RAYS, x, 27, B, p, 2, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = lifter(x, p)
    assert torch.equal(out, eager)
    # The captured kernels hold pointers into B's tile schedule and never call the library again: a size named in
    # r3d_prepare stays resident however many other sizes pass through the 64-entry cache, until r3d_release.
    hp, ht = lifter.pos.handle(x.device), lifter.trj.handle(x.device)
    with torch.no_grad():
        x2, p2 = torch.cat([x, x]), torch.cat([p, p])
        for b in range(B + 1, B + 71):                           # 70 other batch sizes of the same plan: more than the cache keeps
            lifter(x2[:b].contiguous(), p2[:b].contiguous())
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    ray3d_amd._capi.release(hp, ht, B)
    with pytest.raises(ray3d_amd._capi.Ray3DHipError, match="never prepared"):
        ray3d_amd._capi.release(hp, ht, B)


def test_a_call_on_the_buffers_of_the_previous_one_skips_the_bind_kernel():
    """Eager calls keep their ready counters and bound problem table in a control region the schedule owns: a call whose
    input / parameter / workspace pointers are the previous call's runs WITHOUT r3d_bind_f32, on the counter bank the
    previous launch zeroed (r3d_forward.cpp).  Outputs must not depend on which path a call took: repeated calls, calls that
    alternate between two inputs (bind every time), new contents behind the same pointer, and eager calls around the
    replay of a captured graph - which binds inside the graph, in the caller's workspace - all give the same bits."""
    import ray3d_amd
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    B = 150
    x1 = torch.from_numpy(synth.synth_rays(B, cp, seed=201)).cuda()
    x2 = torch.from_numpy(synth.synth_rays(B, cp, seed=202)).cuda()
    p = torch.from_numpy(synth.synth_param(B, seed=203)).cuda()
    names = lambda recs: [r["kernel"] for r in recs]
    with torch.no_grad():
        first = lifter(x1, p)
        recs = lifter.profile_call(lambda: lifter(x1, p), x1.device)
        single = "r3d_forward_f32" in names(recs)           # (R3D_STAGED=1: one launch per level, nothing to bind)
        assert "r3d_bind_f32" not in names(recs), names(recs)
        for _ in range(4):                                   # both counter banks, twice
            assert torch.equal(lifter(x1, p), first)
        other = lifter(x2, p)                                # another input pointer: bound again
        recs = lifter.profile_call(lambda: lifter(x1, p), x1.device)
        assert "r3d_bind_f32" in names(recs) or not single, names(recs)
        for _ in range(3):
            assert torch.equal(lifter(x2, p), other)
            assert torch.equal(lifter(x1, p), first)
        check_parity(first, _oracle_lift(((cp, sp), (ct, st)), x1.cpu().numpy(), p.cpu().numpy()), "bind skipped, %d windows" % B)
        # new contents behind the pointer the table is bound to
        keep = x1.clone()
        x1.copy_(x2)
        assert torch.equal(lifter(x1, p), other)
        x1.copy_(keep)
        assert torch.equal(lifter(x1, p), first)
        # a captured forward of the other input between eager calls
        out = torch.empty((B, 1, 17, 3), device="cuda")
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                lifter._run(ray3d_amd._capi.R3D_INPUT_RAYS, x2, 27, B, p, 2, out=out)
        assert torch.equal(lifter(x1, p), first)
        assert torch.equal(lifter(x1, p), first)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, other)
            assert torch.equal(lifter(x1, p), first)        # (table still bound to x1: the replay used the workspace's region)


def test_a_tile_that_never_reports_ends_in_nan_not_in_a_hang(monkeypatch):
    """The single-launch forward orders its tiles by ready counters; a counter that never fills must not hang the GPU.
    R3D_FAULT_TILE makes one tile of workgroup 0 skip its counter update: its consumers spin, give up after ~1 s, raise the
    launch's abort flag, every later wait returns at once and the decoder turns the outputs into NaN.  The next forward
    (bind kernel: fresh counters) is correct again."""
    import time
    import ray3d_amd
    from ray3d_amd import synth
    if os.environ.get("R3D_STAGED") == "1":
        pytest.skip("one launch per level: stream order, no ready counters to miss")
    hooks_library()                                 # (fault injection exists in the hooks build only; handles stay with their library)
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    B = 200
    x = torch.from_numpy(synth.synth_rays(B, cp, seed=97)).cuda()
    p = torch.from_numpy(synth.synth_param(B, seed=98)).cuda()
    with torch.no_grad():
        good = lifter(x, p)
        torch.cuda.synchronize()
        dev_switch(monkeypatch, "R3D_FAULT_TILE", "0")
        t0 = time.perf_counter()
        bad = lifter(x, p)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        monkeypatch.delenv("R3D_FAULT_TILE")
        again = lifter(x, p)
        torch.cuda.synchronize()
    assert torch.isnan(bad).all(), "a forward with a missing counter update must be poisoned"
    assert 0.5 < dt < 20.0, dt                      # it waited for the bounded spins, and no longer
    assert torch.equal(good, again)
    # ... and it is an ERROR at the boundary, not only a NaN: r3d_status reports the aborted forward (once), the Python
    # mirror raises; with a shorter spin timeout (R3D_OPT_SPIN_TIMEOUT_MS) the wait is shorter
    with pytest.raises(_capi_error(), match="gave up"):
        lifter.check_status()
    lifter.check_status()                           # (cleared by the call that reported it)
    lifter.set_spin_timeout_ms(100)
    with torch.no_grad():
        dev_switch(monkeypatch, "R3D_FAULT_TILE", "0")
        t0 = time.perf_counter()
        bad = lifter(x, p)
        with pytest.raises(_capi_error(), match="gave up after 100 ms"):
            lifter.check_status()
        dt = time.perf_counter() - t0
        monkeypatch.delenv("R3D_FAULT_TILE")
    assert torch.isnan(bad).all() and dt < 0.9, dt
    # checked(): notices, switches the pair to the level-by-level form, repeats - the caller gets correct poses
    with torch.no_grad(), pytest.warns(UserWarning, match="level-by-level"):
        dev_switch(monkeypatch, "R3D_FAULT_TILE", "0")
        fixed = lifter.checked(lambda: lifter(x, p))
        monkeypatch.delenv("R3D_FAULT_TILE")
    assert torch.equal(fixed, good) and lifter.pos._staged


def _capi_error():
    from ray3d_amd import _capi
    return _capi.Ray3DHipError


TWO_PROC_SCRIPT = r"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.environ["R3D_ROOT"]); sys.path.insert(0, os.path.join(os.environ["R3D_ROOT"], "tests"))
import ray3d_amd
from ray3d_amd import synth
from conftest import synth_states
tag, go = sys.argv[1], sys.argv[2]
mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
(cp, sp), (ct, st) = synth_states(mc)
fac = ray3d_amd.Model(mc, {}, is_train=False)
pos, trj = fac.get_pos_model(), fac.get_trj_model()
ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
lifter.set_spin_timeout_ms(200)
B = 1024
x = torch.from_numpy(synth.synth_rays(B, cp, seed=5)).cuda()
p = torch.from_numpy(synth.synth_param(B, seed=6)).cuda()
ref = ray3d_amd.Ray3DLifter(pos, trj).eval()
with torch.no_grad():
    want = lifter(x, p).clone()           # alone on the GPU (the other process waits for the go file too)
    lifter.check_status()
    open(go + "." + tag, "w").close()
    t0 = time.time()
    while not (os.path.exists(go + ".a") and os.path.exists(go + ".b")) and time.time() - t0 < 120:
        time.sleep(0.01)
    bad = 0
    import warnings
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for i in range(300):
            out = lifter.checked(lambda: lifter(x, p))
            if not torch.isfinite(out).all() or (out - want).abs().max().item() > 1e-5:
                bad += 1
print("RESULT", tag, "bad", bad, "switched_to_staged", int(lifter.pos._staged), "warnings", len(w))
"""


def test_two_processes_lifting_on_one_gpu_both_get_correct_poses(tmp_path):
    """Two single-launch forwards of two PROCESSES can each hold part of the chip and wait for the rest (within a process the
    library orders them).  No environment variable: a forward that gives up raises the handle's status, checked() switches
    the lifter to the level-by-level form and repeats the call - every result of both processes is correct."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "two_proc.py"
    script.write_text(TWO_PROC_SCRIPT)
    env = dict(os.environ, R3D_ROOT=root)
    env.pop("R3D_STAGED", None)
    go = str(tmp_path / "go")
    procs = [subprocess.Popen([sys.executable, str(script), tag, go], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for tag in ("a", "b")]
    outs = [pr.communicate(timeout=600)[0] for pr in procs]
    for pr, o in zip(procs, outs):
        assert pr.returncode == 0, o[-3000:]
        res = [l for l in o.splitlines() if l.startswith("RESULT")]
        assert res and " bad 0 " in res[0], o[-3000:]
        print(res[0])


@pytest.mark.parametrize("B", [1, 3, 12])
def test_calls_of_a_few_windows_take_data_as_its_own_ready_flag(B, monkeypatch):
    """Up to 16 windows, eager: the schedule owns two banks of activations, each filled with sentinels by the launch that
    runs on the other one, and the GEMV / latency tiles read their operands until no sentinel is left instead of waiting for
    ready counters (r3d_kernels.hip, ACT_SENTINEL).  Same bits as the counter path - which a captured call of the same
    size still takes, in the caller's workspace - call after call; and a tile that never stores ends in NaN after the
    bounded spins, not in a hang, with the next call correct again."""
    import time
    import ray3d_amd
    from ray3d_amd import synth
    if B <= 4 and os.environ.get("R3D_STAGED") != "1":
        hooks_library()                             # (the fault injection at the end exists in the hooks build only)
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x = torch.from_numpy(synth.synth_rays(B, cp, seed=301)).cuda()
    x2 = torch.from_numpy(synth.synth_rays(B, cp, seed=302)).cuda()
    p = torch.from_numpy(synth.synth_param(B, seed=303)).cuda()
    with torch.no_grad():
        first = lifter(x, p)
        check_parity(first, _oracle_lift(((cp, sp), (ct, st)), x.cpu().numpy(), p.cpu().numpy()), "poll mode, %d windows" % B)
        for _ in range(5):                                   # both banks, armed by the launch before
            assert torch.equal(lifter(x, p), first)
        other = lifter(x2, p)
        assert torch.equal(lifter(x, p), first) and torch.equal(lifter(x2, p), other)
        # the counter path of the same schedule: a captured call
        lifter.prepare([B])
        out = torch.empty((B, 1, 17, 3), device="cuda")
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                lifter._run(ray3d_amd._capi.R3D_INPUT_RAYS, x2, 27, B, p, 2, out=out)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, other)
            assert torch.equal(lifter(x, p), first)
        if B > 4 or os.environ.get("R3D_STAGED") == "1":
            return
        # a GEMV tile of workgroup 0 that never stores
        torch.cuda.synchronize()
        dev_switch(monkeypatch, "R3D_FAULT_TILE", "0")
        t0 = time.perf_counter()
        bad = lifter(x, p)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        monkeypatch.delenv("R3D_FAULT_TILE")
        again = lifter(x, p)
        torch.cuda.synchronize()
    assert torch.isnan(bad).all(), "a forward with a missing tile must be poisoned"
    assert 0.5 < dt < 30.0, dt
    assert torch.equal(again, first)


@pytest.mark.parametrize("B", [3, 200])
def test_two_streams_share_a_lifter(B):
    """Eager calls of one batch size share the schedule's control region (and, for a few windows, its activation banks)
    whatever stream they are on; the library orders single-launch forwards of different streams with an event, a call
    that finds the table bound to other buffers binds again behind that event.  Two streams taking turns on one lifter
    with different inputs, nothing synchronised in between, get what each gets alone."""
    import ray3d_amd
    from ray3d_amd import synth
    if os.environ.get("R3D_STAGED") == "1":
        pytest.skip("launch by launch nothing orders two streams: they need a lifter (a workspace) each")
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, _), _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    xa = torch.from_numpy(synth.synth_rays(B, cp, seed=401)).cuda()
    xb = torch.from_numpy(synth.synth_rays(B, cp, seed=402)).cuda()
    p = torch.from_numpy(synth.synth_param(B, seed=403)).cuda()
    with torch.no_grad():
        ra, rb = lifter(xa, p), lifter(xb, p)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for it in range(8):
            with torch.cuda.stream(s1):
                oa = lifter(xa, p)
            with torch.cuda.stream(s2):
                ob = lifter(xb, p)
                if it % 3 == 2:
                    ob2 = lifter(xb, p)                      # (the same stream and buffers twice in a row: no bind)
                    outs.append((ob2, rb))
            outs += [(oa, ra), (ob, rb)]
        torch.cuda.synchronize()
    for got, want in outs:
        assert torch.equal(got, want)


@pytest.mark.parametrize("arch,B", [("3,3,3", 130), ("3,3,3", 192), ("3,3,3", 200), ("3,3,3", 250), ("3,3", 300), ("3,3,3,3", 224)])
def test_narrow_column_tiles_against_the_oracle(arch, B, monkeypatch):
    """Calls whose M = B levels are one tile deep run them as single-unit tiles of 4 .. 7 column blocks (gemm_tile_nb: whole blocks
    on wavefronts 0-3, quarter blocks on 4-7, partial sums through LDS): every width, ragged last units (130 = 4 units + 2 rows,
    250 = 7 units + 26 rows), the residual layers, concatenated operands - all windows against the torch port at the literal
    bound, the level-by-level form bit-identical (same tiles), and the whole-tile packing (R3D_NO_NB, hooks build) within rounding."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import torch_port
    if os.environ.get("R3D_BF16X3") == "1":
        pytest.skip("bf16x3 handles run these layers on the bf16 matrix cores")
    mc = ray3d_amd.default_model_config(ARCHITECTURE=arch)

    def lift(staged=False):
        pos, trj, (cp, sp), (ct, st) = build_modules(mc)
        lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
        lifter.set_staged(staged)
        x = synth.synth_rays(B, cp, seed=77)
        p = synth.synth_param(B, seed=78)
        with torch.no_grad():
            out = lifter(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda())
        lifter.check_status()
        return out, (cp, sp, ct, st, x, p)
    out, (cp, sp, ct, st, x, p) = lift()
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
    with torch.no_grad():
        ref = (torch_port.forward(cp, sds[0], torch.from_numpy(x), torch.from_numpy(p)) +
               torch_port.forward(ct, sds[1], torch.from_numpy(x), torch.from_numpy(p))).numpy()
    check_parity(out, ref, "narrow tiles vs torch port")
    if os.environ.get("R3D_STAGED") != "1":
        assert torch.equal(lift(staged=True)[0], out)
    dev_switch(monkeypatch, "R3D_NO_NB", "1")
    whole, _ = lift()
    check_parity(whole, ref, "whole tiles vs torch port")
    assert not torch.equal(whole, out)                        # (the switch really selects the other tiling)
    assert (whole - out).abs().max().item() <= 2e-5 * max(1.0, float(np.abs(ref).max()))


def test_two_lifters_side_by_side_on_half_chip_streams():
    """R3D_OPT_CU_LIMIT (Ray3DLifter.set_cu_limit) + ray3d_amd.masked_stream: two pairs of handles, each on a CU-masked stream
    of 128 CUs (disjoint halves of the chip), lift different batches at the same time - the single persistent launch with at
    most 128 workgroups each, not ordered against the other stream.  Both get the oracle's poses (the literal bound), every
    time, nothing aborts; the forward kernel's grid is <= 128; back on an unmasked stream with the limit lifted the same
    lifter runs on the whole chip again."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import torch_port
    if os.environ.get("R3D_STAGED") == "1":
        pytest.skip("the limit concerns the single-launch form")
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3")
    B = 256
    streams = [ray3d_amd.masked_stream(range(0, 128)), ray3d_amd.masked_stream(range(128, 256))]
    lifters, xs, refs = [], [], []
    p = torch.from_numpy(synth.synth_param(B, seed=9)).cuda()
    for i in range(2):
        pos, trj, (cp, sp), (ct, st) = build_modules(mc)
        l = ray3d_amd.Ray3DLifter(pos, trj).eval()
        l.set_cu_limit(128)
        lifters.append(l)
        x = synth.synth_rays(B, cp, seed=500 + i)
        xs.append(torch.from_numpy(x).cuda())
        sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
        with torch.no_grad():
            refs.append((torch_port.forward(cp, sds[0], torch.from_numpy(x), p.cpu()) +
                         torch_port.forward(ct, sds[1], torch.from_numpy(x), p.cpu())).numpy())
    outs = [[], []]
    with torch.no_grad():
        for it in range(12):
            for i in range(2):
                with torch.cuda.stream(streams[i]):
                    outs[i].append(lifters[i](xs[i], p))
        torch.cuda.synchronize()
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                lifters[i].check_status()
                recs = lifters[i].profile_call(lambda: lifters[i](xs[i], p), "cuda:0")
            fw = [r for r in recs if r["kernel"].startswith("r3d_forward")]
            assert fw and all(r["blocks"] <= 128 for r in fw), recs
    for i in range(2):
        check_parity(outs[i][0], refs[i], "half-chip stream %d vs torch port" % i)
        for o in outs[i][1:]:
            assert torch.equal(o, outs[i][0])
    with torch.no_grad():
        lifters[0].set_cu_limit(0)
        whole = lifters[0](xs[0], p)
        recs = lifters[0].profile_call(lambda: lifters[0](xs[0], p), "cuda:0")
    assert max(r["blocks"] for r in recs if r["kernel"].startswith("r3d_forward")) > 128
    check_parity(whole, refs[0], "the same lifter on the whole chip again")


def test_pos_and_trj_with_different_channel_counts():
    """CHANNELS may differ between the two networks (separate model_configs in the reference): one of them fusable
    (<= 256 channels), the other not - the pair then runs the un-fused first level for both (r3d_plan.cpp) instead of
    failing with a mixed launch."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import oracle
    mcp = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    mct = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3", CHANNELS=512)
    pos, _, (cp, sp), _ = build_modules(mcp)
    _, trj, _, (ct, st) = build_modules(mct)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    for B in (5, 130):
        x, p = synth.synth_rays(B, cp, seed=81), synth.synth_param(B, seed=82)
        with torch.no_grad():
            out = lifter(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda())
        ref = oracle.forward(cp, sp, x, p) + oracle.forward(ct, st, x, p)
        check_parity(out, ref, "pos C=256 + trj C=512, %d windows" % B)


@pytest.mark.parametrize("over", [dict(ARCHITECTURE="3"), dict(ARCHITECTURE="3,3,3", CHANNELS=512),
                                  dict(ARCHITECTURE="3,3", DENSE=True, DISABLE_OPTIMIZATIONS=True)])
def test_forward_uv_on_the_unfused_first_layer_kernel(over):
    """UV mode where the first level is not fused (one-level architecture, C > 256, the dense ablation): the gathers of
    r3d_gemm_enc_uv_f32 encode the rays; bit-identical to the rays mode, and equal to the oracle chain."""
    import ray3d_amd
    from ray3d_amd import synth
    cams, ocams, _, _ = _reference_cameras()
    mc = ray3d_amd.default_model_config(**over)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    rf, B = cp.receptive_field, 45
    uv = (1000.0 * synth.hash_uniform("uvenc%d" % rf, (B, rf, 17, 2), 5)).astype(np.float32)
    pick = [i % len(cams) for i in range(B)]
    rays = np.stack([ocams[c].rays_from_uv(uv[i].astype(np.float64)) for i, c in enumerate(pick)]).astype(np.float32)
    rows, par = np.stack([cams[c].cam_row() for c in pick]), np.stack([cams[c].param() for c in pick])
    with torch.no_grad():
        a = lifter.forward_uv(torch.from_numpy(uv).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(par).cuda())
        b = lifter(torch.from_numpy(rays).cuda(), torch.from_numpy(par).cuda())
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    ref = _oracle_lift(((cp, sp), (ct, st)), rays, par)
    check_parity(a.cpu().numpy(), ref)


@pytest.mark.parametrize("seed", list(range(10)))
def test_random_configurations_match_the_oracle_chain(seed):
    """Seeded random configurations over everything the reference's factory reads (joints, input dimension, depth,
    channels, latent size, stage, camera embedding, dilated / causal / dense geometry), random batch sizes, both
    precisions: HIP path vs the torch port of the reference graph on every window."""
    import ray3d_amd
    from ray3d_amd import synth
    rng = np.random.default_rng(1000 + seed)
    levels = int(rng.integers(1, 5))
    over = dict(ARCHITECTURE=",".join(["3"] * levels), NUM_KPTS=int(rng.choice([14, 15, 17])),
                INPUT_DIM=int(rng.choice([2, 3])), CHANNELS=int(rng.choice([64, 96, 128, 256, 256, 384])),
                LATENT_FEATURES_DIM=int(rng.choice([64, 128, 256])), STAGE=int(rng.choice([1, 2, 3])),
                CAMERA_EMBDDING=bool(rng.integers(0, 2)), EMBEDD_DIM=int(rng.choice([32, 64])),
                BF16X3=bool(rng.integers(0, 2)))
    geom = int(rng.integers(0, 4))                  # strided | dilated | dilated + causal | dense (short receptive fields)
    if geom >= 1:
        over["DISABLE_OPTIMIZATIONS"] = True
    if geom == 2:
        over["CAUSAL"] = True
    if geom == 3 and levels <= 3:
        over["DENSE"] = True
    mc = ray3d_amd.default_model_config(**over)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    B = int(rng.choice([1, 7, 33, 100, 257]))
    x = synth.synth_rays(B, cp, seed=seed)
    p = synth.synth_param(B, seed=seed + 1)
    pt = torch.from_numpy(p).cuda() if cp.camera_embedding else None
    with torch.no_grad():
        out = lifter(torch.from_numpy(x).cuda(), pt).cpu().numpy()
    from oracle import torch_port
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
    with torch.no_grad():
        pp = torch.from_numpy(p) if cp.camera_embedding else None
        ref = (torch_port.forward(cp, sds[0], torch.from_numpy(x), pp) + torch_port.forward(ct, sds[1], torch.from_numpy(x), pp)).numpy()
    assert out.shape == ref.shape
    check_parity(out, ref)
