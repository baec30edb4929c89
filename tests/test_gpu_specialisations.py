"""-m gpu: every case of tests/specialisation_cases.py - the table that tests/test_specialisations_host.py proves to reach every
(kernel, tile kind) pair the library's calls can reach - run on the GPU through handles of the hooks library:

  census against reality   the kernel names and grids of the call's launch records equal the census's launches, in order: the
                           host-side census (r3d_debug_forward_census) is held to what the product launches;
  parity                   pos + trj and trj against the oracle chain at the literal 1e-4: oracle.forward for small independent
                           windows, the torch port of the reference graph (pinned to the reference fixtures) otherwise;
  pixel input              bit-identical to the same handle fed the rays the oracle's cameras give for those pixels;
  clip calls               against their materialised windows at 2e-5 * max(1, |out|) (another summation order at most);
  captured                 the graph's replay has the bits of the eager call.

A case at 128 workgroups runs on a lifter with set_lanes(2), one at 64 with set_lanes(4) (R3D_OPT_LANES: device CUs / lanes
workgroups per forward): every call of the case is issued on lane 0's own stream (lifter.lane(0)), then join_lanes() and
check_status() - a forward that gave up (R3D_ERR_ABORTED) fails the case, nothing is repeated - and set_lanes(0) in a finally.
Lane forwards do give launch records (the records' events are recorded on the stream the forward runs on, the lane's), so the
census is held to them exactly as on the whole chip: kernel names and grids, asked of r3d_debug_forward_census at CUs / lanes.

Rays are synth_rays; pixels are uniform over a 1000-pixel image through the reference cameras of tests/golden/cameras.npz;
per-window cameras cycle over its four H36M S9 rows.

First reached here: the 126 of the sweep's 246 (kernel, tile kind) pairs that the census finds in none of the earlier GPU
parametrisations that are cheap to enumerate - test_gpu_buffers.py's _EAGER, staged, _VARIANTS and input cases, the fixtures in
every mode and form and at their own sizes, the ragged-batch list, test_gpu_nonfinite.py's BATCHES, the narrow-column list, the UV
parity sizes, the 200-window clip calls.  (Partial: the random configurations, the clip-length sweep, the 1024 / 4096-window and
evaluation tests were not enumerated; they reach some of the tall fp32 tiles below.)
r3d_forward_b3: enc_tile<3,rays>, first_level_taps_b3<2,K>64,rays>, gemm_tile<5,1>, gemm_tile<6,1>, gemm_tile_b3<2>,
    gemm_tile_b3<3>, gemm_tile_b3<4>, gemm_tile_b3t<2>, gemm_tile_b3t<3>
r3d_forward_clip_f32: enc_tile<3,rays>, gemm_tile<2,1,pair>, gemm_tile<3,1,pair>, gemm_tile<3,1>, gemm_tile<4,1,pair>,
    gemm_tile<4,1>, gemm_tile<5,1>, gemm_tile<6,1>, gemm_tile_nb<4>
r3d_forward_clip_uv_f32: enc_tile<3,UV>, gemm_tile<1,2>, gemm_tile<2,1,pair>, gemm_tile<3,1,pair>, gemm_tile<3,1>,
    gemm_tile<4,1,pair>, gemm_tile<4,1>, gemm_tile<5,1>, gemm_tile<6,1>, gemm_tile_nb<4>
r3d_forward_f32: first_level_taps<2,K>64,rays>, gemm_tile<3,1,pair>, gemm_tile<4,1,pair>, gemm_tile<5,1>, gemm_tile<6,1>
r3d_forward_lat: enc_tile<2,rays>
r3d_forward_uv_b3: enc_tile<1,UV>, enc_tile<2,UV>, enc_tile<3,UV>, first_level_taps_b3<1,K<=64,UV>,
    first_level_taps_b3<1,K>64,UV>, first_level_taps_b3<2,K<=64,UV>, first_level_taps_b3<2,K>64,UV>, gemm_tile<1,1>,
    gemm_tile<1,2>, gemm_tile<1,4>, gemm_tile<2,1>, gemm_tile<3,1>, gemm_tile<4,1>, gemm_tile<5,1>, gemm_tile<6,1>,
    gemm_tile_b3<2>, gemm_tile_b3<3>, gemm_tile_b3<4>, gemm_tile_b3p<1>, gemm_tile_b3t<1>, gemm_tile_b3t<2>,
    gemm_tile_b3t<3>
r3d_forward_uv_f32: first_level_taps<2,K>64,UV>, gemm_tile<2,1,pair>, gemm_tile<3,1,pair>, gemm_tile<4,1,pair>,
    gemm_tile<5,1>, gemm_tile<6,1>
r3d_forward_uv_lat: enc_tile<2,UV>, gemm_tile<1,2>, gemm_tile<1,4>, gemv_run
r3d_gemm_b3: enc_tile<3,rays>, first_level_taps_b3<2,K>64,rays>, gemm_tile<5,1>, gemm_tile<6,1>, gemm_tile_b3<3>,
    gemm_tile_b3<4>, gemm_tile_b3t<2>, gemm_tile_b3t<3>, gemm_tile_nb<5>, gemm_tile_nb<6>
r3d_gemm_enc_f32: enc_tile<3,rays>
r3d_gemm_enc_uv_f32: enc_tile<1,UV>, enc_tile<2,UV>, enc_tile<3,UV>
r3d_gemm_f32: enc_tile<3,rays>, first_level_taps<2,K>64,rays>, gemm_tile<2,1,pair>, gemm_tile<3,1,pair>,
    gemm_tile<4,1,pair>, gemm_tile<5,1>, gemm_tile<6,1>
r3d_gemm_uv_b3: enc_tile<1,UV>, enc_tile<2,UV>, enc_tile<3,UV>, first_level_taps_b3<1,K<=64,UV>,
    first_level_taps_b3<1,K>64,UV>, first_level_taps_b3<2,K<=64,UV>, first_level_taps_b3<2,K>64,UV>, gemm_tile<1,1>,
    gemm_tile<2,1>, gemm_tile<3,1>, gemm_tile<4,1>, gemm_tile<5,1>, gemm_tile<6,1>, gemm_tile_b3<2>, gemm_tile_b3<3>,
    gemm_tile_b3p<1>, gemm_tile_b3t<1>, gemm_tile_b3t<2>, gemm_tile_b3t<3>
r3d_gemm_uv_f32: enc_tile<2,UV>, enc_tile<3,UV>, first_level_shared<1>, first_level_shared<2>, first_level_taps<1,K<=64,UV>,
    first_level_taps<1,K>64,UV>, first_level_taps<2,K<=64,UV>, first_level_taps<2,K>64,UV>, gemm_tile<1,1,pair>,
    gemm_tile<1,1>, gemm_tile<1,2>, gemm_tile<1,4>, gemm_tile<2,1,pair>, gemm_tile<2,1>, gemm_tile<3,1,pair>,
    gemm_tile<3,1>, gemm_tile<4,1,pair>, gemm_tile<4,1>, gemm_tile<5,1>, gemm_tile<6,1>

First executed under test with the workgroup axis (128 / 64: lanes) and the wider configuration domain (six levels, latent 512, 640
and 768 channels) - 28 more pairs, 274 in all; before, no test of any kind selected them (the case that reaches each):
r3d_forward_lat / r3d_forward_uv_lat: enc_tile<3,*>, gemm_tile<2,1> (rf729, 26 windows), gemm_tile<3,1>, gemm_tile<4,1> (rf729,
    31 windows, 128 workgroups), gemm_tile<5,1>, gemm_tile<6,1> (rf729, 23 windows, 64 workgroups), gemm_tile_nb<4>, <5>, <6>
    (c512, 22 windows, 64 workgroups), gemm_tile_nb<7> (c640 bf16x3, 22 windows, 64 workgroups)
r3d_forward_b3 / r3d_forward_uv_b3: gemm_tile_nb<5>, gemm_tile_nb<6> (n512 bf16x3, 292 windows)
r3d_gemm_b3: gemm_tile_nb<4> (c768_rf9 bf16x3, 196 windows), gemm_tile_nb<7> (c640 bf16x3, 292 windows)
r3d_gemm_uv_b3: gemm_tile<1,2> (j17_rf243_s3 bf16x3 staged, 96 windows, 128 workgroups), gemm_tile<1,4> (the same at 64)
"""
import functools
import os

import numpy as np
import pytest
import torch

import specialisation_cases as sc
from conftest import check_parity, hooks_library, synth_states

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _states(config):
    """(cfg, state) of pos and trj: synthetic weights at scale 1, the same for both precisions of a configuration."""
    return synth_states(sc.model_config(config))


@functools.lru_cache(maxsize=None)
def _cameras():
    from test_gpu_parity import _reference_cameras
    cams, ocams, z, tags = _reference_cameras()
    assert all(str(t).startswith("h36m_S9_") for t in tags[:4])
    t0 = tags[0]
    assert np.abs(ocams[0].rays_from_uv(z[t0 + "/uv"]) - z[t0 + "/rays"]).max() < 1e-12      # (the oracle's encoding, pinned to the reference's pairs)
    return cams[:4], ocams[:4]


@functools.lru_cache(maxsize=None)
def _inputs(config, shape, B):
    """What the call reads - x (rays or pixels, windows or a frame sequence), window stride, parameter rows, camera rows - and
    the same windows materialised as rays (B, RF, J, F) with their (B, 2) parameter rows, for the references."""
    from ray3d_amd import synth
    (cp, _), _ = _states(config)
    uv, per_window, stride = sc.SHAPES[shape]
    rf, J, F = cp.receptive_field, cp.num_joints, cp.in_features
    stride = stride or rf
    frames = (B - 1) * stride + rf
    seed = 1000 + B
    if not uv:
        if stride == rf:
            x = synth.synth_rays(B, cp, seed=seed)
            windows = x
            par = synth.synth_param(B, seed=seed + 1)
        else:                                           # a clip: one parameter row for all windows
            # (synth_rays windows laid end to end: every frame in the range of the model's inputs however long the clip - a ramp
            #  over 1000 frames would put the outputs at 100 m, where 1e-4 is below fp32's rounding of the result)
            x = np.ascontiguousarray(synth.synth_rays(frames // rf + 1, cp, seed=seed).reshape(-1, J, F)[:frames])
            windows = np.stack([x[i:i + rf] for i in range(B)])
            par = np.tile(np.array([[1.5, 0.2]], np.float32), (B, 1))
        rows, seq_rays = None, None
    else:
        cams, ocams = _cameras()
        pick = [i % 4 for i in range(B)] if per_window else [1] * B
        x = (1000.0 * synth.hash_uniform("specialisations.%s.%s" % (config, shape), (frames, J, 2), 3)).astype(np.float32)
        windows = np.stack([ocams[c].rays_from_uv(x[i * stride:i * stride + rf].astype(np.float64)) for i, c in enumerate(pick)]).astype(np.float32)
        par = np.stack([cams[c].param() for c in pick]).astype(np.float32)
        rows = np.stack([cams[c].cam_row() for c in pick]) if per_window else cams[1].cam_row()
        # the rays the same call shape reads (one camera: the sequence itself; own cameras: the materialised windows)
        seq_rays = None if per_window else ocams[1].rays_from_uv(x.astype(np.float64)).astype(np.float32)
    out = dict(x=x, stride=stride, windows=windows, par=par if cp.camera_embedding else None, rows=rows, seq_rays=seq_rays,
               one_row=(not uv and stride != rf))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(config, shape, B):
    """(pos + trj, trj) of the oracle chain on the call's windows: computed once per (configuration, input, B), shared by the
    precisions and forms, read-only."""
    from oracle import oracle, torch_port
    (cp, sp), (ct, st) = _states(config)
    inp = _inputs(config, shape, B)
    w = np.array(inp["windows"])
    p = np.array(inp["par"]) if inp["par"] is not None else np.zeros((B, 2), np.float32)
    clip = sc.SHAPES[shape][2] == 1
    if not clip and B * cp.receptive_field <= 64 * 27:
        pos, trj = oracle.forward(cp, sp, w, p), oracle.forward(ct, st, w, p)
    else:
        outs = []
        with torch.no_grad():
            for c, s in ((cp, sp), (ct, st)):
                sd = {k: torch.from_numpy(np.asarray(v)) for k, v in s.items()}
                outs.append(torch.cat([torch_port.forward(c, sd, torch.from_numpy(w[i:i + 512]), torch.from_numpy(p[i:i + 512]))
                                       for i in range(0, B, 512)]).numpy())
        pos, trj = outs
    both = pos + trj
    both.setflags(write=False), trj.setflags(write=False)
    return both, trj


def _lifter(config, b3, staged):
    """A fresh pair on the hooks library (the census is asked of the handles that run the call)."""
    import ray3d_amd
    hooks_library()
    (cp, sp), (ct, st) = _states(config)
    fac = ray3d_amd.Model(sc.model_config(config, b3), {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    pos.eval(), trj.eval()
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.CLIP_ROUND = 0
    lifter.set_staged(staged)
    return lifter


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV) if a is not None else None


def _call(lifter, mode, x, stride, B, p=None, cam=None, **kw):
    """One r3d_forward_pair with out_trj through Ray3DLifter._run on device tensors -> (out, out_trj).  p: (B, E) rows, (E,) one
    row for all windows, or None; cam: (B, 8) rows, (8,) one row, or None."""
    with torch.no_grad():
        return lifter._run(mode, x, stride, B, p, 0 if (p is None or p.dim() == 1) else lifter.pos.extrinsic_dim, cam,
                           0 if (cam is None or cam.dim() == 1) else cam.shape[1], return_trj=True, **kw)


def _on_lane(lifter, fn):
    """fn() - forwards through `lifter` - on lane 0's own stream when the lifter has lanes (on the current stream otherwise), joined
    and checked: an aborted forward raises here."""
    with lifter.lane(0):
        res = fn()
    lifter.join_lanes()
    lifter.check_status(DEV)
    return res


@pytest.mark.parametrize("case", sc.CASES, ids=[sc.case_id(c) for c in sc.CASES])
def test_case_runs_what_the_census_says_and_matches_the_oracle(case):
    config, b3, form, shape, B, case_nwg = case
    lifter = _lifter(config, b3, form == "staged")
    lanes = sc.NWG // case_nwg
    assert lanes in (1, 2, 4) and (lanes == 1 or form != "captured")
    try:
        if lanes > 1:
            lifter.set_lanes(lanes, DEV)
            assert lifter.num_lanes() == lanes
        _run_case(case, lifter, lanes)
    finally:
        if lanes > 1:
            lifter.set_lanes(0, DEV)


def _run_case(case, lifter, lanes):
    from ray3d_amd import _capi
    config, b3, form, shape, B, _ = case
    if os.environ.get("R3D_BF16X3") is not None and b3 != (os.environ["R3D_BF16X3"] == "1"):
        pytest.skip("R3D_BF16X3 in the environment overrides the configuration key")
    uv, per_window, _ = sc.SHAPES[shape]
    assert lifter.precision(DEV) == ("bf16x3" if b3 else "f32")
    inp = _inputs(config, shape, B)
    rf, stride = lifter.receptive_field(), inp["stride"]
    mode = _capi.R3D_INPUT_UV if uv else _capi.R3D_INPUT_RAYS
    x, cam, p_rows = _dev(inp["x"]), _dev(inp["rows"]), _dev(inp["par"])
    p = p_rows[0].contiguous() if (inp["one_row"] and p_rows is not None) else p_rows
    dev = torch.device(DEV)
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)

    # ---- census against reality: the FIRST call on these buffers (it binds), with launch records
    got = {}
    recs = lifter.profile_call(lambda: got.update(out=_on_lane(lifter, lambda: _call(lifter, mode, x, stride, B, p, cam))), DEV)
    out, out_trj = got["out"]
    nwg = torch.cuda.get_device_properties(dev).multi_processor_count // lanes
    census = _capi.debug_forward_census(hp, ht, B, stride, nwg=nwg, uv=uv, cam_stride=8 if per_window else 0,
                                        staged=form == "staged", captured=form == "captured")
    launched = [(r["kernel"], r["blocks"]) for r in recs if r["stage"] >= 0]
    print("launches of %s: %s" % (sc.case_id(case), launched))
    assert launched == [(k, blocks) for k, blocks, _ in census], (launched, census)
    kernels = [k for k, _ in launched]
    if case == ("j17_rf81_s2_big", True, "single", "uv-clip", 200, sc.NWG) and os.environ.get("R3D_STAGED") != "1":
        # a clip call on a bf16x3 handle keeps the gathered first level: no per-frame launch, no clip kernel
        assert kernels == ["r3d_bind_f32", "r3d_forward_uv_b3", "r3d_decode_w4_f32"], kernels

    # ---- parity against the oracle chain
    both, trj = _reference(config, shape, B)
    check_parity(out, both, "pos+trj vs the oracle chain")
    check_parity(out_trj, trj, "trj vs the oracle chain")

    # ---- pixel input: the bits of the same handle fed the rays of those pixels
    if uv:
        if inp["seq_rays"] is not None:
            seq = _dev(inp["seq_rays"])
            r_out, r_trj = _on_lane(lifter, lambda: _call(lifter, _capi.R3D_INPUT_RAYS, seq, stride, B, p_rows))
        else:
            wins = _dev(inp["windows"])
            r_out, r_trj = _on_lane(lifter, lambda: _call(lifter, _capi.R3D_INPUT_RAYS, wins, rf, B, p_rows))
        assert torch.equal(out, r_out) and torch.equal(out_trj, r_trj), float((out - r_out).abs().max())

    # ---- clip calls: their materialised windows
    if stride == 1:
        wins = _dev(inp["windows"])
        w_out, w_trj = _on_lane(lifter, lambda: _call(lifter, _capi.R3D_INPUT_RAYS, wins, rf, B, p_rows))
        check_parity(out, w_out.cpu().numpy(), "clip call vs its materialised windows", tol=2e-5 * max(1.0, float(w_out.abs().max())))
        check_parity(out_trj, w_trj.cpu().numpy(), "clip call vs its materialised windows, trj", tol=2e-5 * max(1.0, float(w_trj.abs().max())))

    # ---- captured: the replay has the eager call's bits
    if form == "captured":
        lifter.prepare([B])
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        c_out, c_trj = torch.zeros_like(out), torch.zeros_like(out_trj)
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    _call(lifter, mode, x, stride, B, p, cam, out=c_out, out_trj=c_trj)
                g.replay()
            torch.cuda.synchronize()
            lifter.check_status(DEV)
            assert torch.equal(c_out, out) and torch.equal(c_trj, out_trj)
        finally:
            del g
            torch.cuda.synchronize()
            lifter.release_prepared()
