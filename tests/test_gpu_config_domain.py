"""-m gpu: configurations of the domain model_create accepts that no other GPU test builds - six levels (RF 729: every per-level
table one entry deeper than any other run), a latent size of 512 at 256 channels, 640 channels, 768 channels at RF 9 - held to the
torch port of the reference graph in every plan kind, at the smallest size that selects it, under the project's two bounds:

  check_parity     pos + trj against the fp32 torch port at the literal 1e-4;
  the error budget (test_f32_error_budget_against_float64_per_plan_kind's rule, fp32 handles): HIP error against the FLOAT64 torch
                   port <= F32_BUDGET x the fp32 torch port's error against it + one ulp of |ref| max.  The HIP / CPU ratios are
                   printed and recorded in the parity summary.

Weights are synth_states, inputs synth_rays(seed=5) / synth_param(seed=6).  For the reference alone (fp32 port against float64, this
CPU): six levels, 26 windows: |ref| max 37.3 m, 3.2e-5; latent 512 / 640 channels / 768 channels, 64 windows: 16.9 / 12.6 / 12.5 m,
1.1e-5 / 1.2e-5 / 8.8e-6 - so 2 x + ulp stays under 1e-4 everywhere (6.9e-5 for six levels).

The references are computed once per module (97 six-level windows: about 12 s of CPU for both dtypes) and sliced: windows are
independent, so the first B rows of the 97-window reference are the reference of a B-window call.

Also here: four lanes at once (R3D_OPT_LANES = 4) on the default RF 27 pair."""
import functools

import numpy as np
import pytest
import torch

from conftest import check_parity, record_parity, synth_states
from test_gpu_parity import F32_BUDGET, _f64_and_cpu_errors, build_modules

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CONFIGS = {
    "six-levels": dict(ARCHITECTURE="3,3,3,3,3,3"),
    "latent-512": dict(ARCHITECTURE="3,3,3", LATENT_FEATURES_DIM=512),
    "c640-n320": dict(ARCHITECTURE="3,3,3", CHANNELS=640, LATENT_FEATURES_DIM=320),
    "c768-n512-rf9": dict(ARCHITECTURE="3,3", CHANNELS=768, LATENT_FEATURES_DIM=512),
}
REF_WINDOWS = {"six-levels": 97, "latent-512": 292, "c640-n320": 292, "c768-n512-rf9": 196}     # (the largest call of each)


def _mc(name, b3=False):
    import ray3d_amd
    mc = ray3d_amd.default_model_config(**CONFIGS[name])
    mc["BF16X3"] = bool(b3)
    return mc


@functools.lru_cache(maxsize=None)
def _states(name):
    """((cfg, state) of pos, (cfg, state) of trj): synthetic weights at scale 1, on the host, the same for both precisions."""
    return synth_states(_mc(name))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(x, p, float64 torch port, fp32 torch port) of the configuration's REF_WINDOWS windows: once per module, read-only."""
    from ray3d_amd import synth
    (cp, sp), (ct, st) = _states(name)
    n = REF_WINDOWS[name]
    x, p = synth.synth_rays(n, cp, seed=5), synth.synth_param(n, seed=6)
    ref, cpu = _f64_and_cpu_errors(cp, sp, ct, st, x, p)
    for a in (x, p, ref, cpu):
        a.setflags(write=False)
    return x, p, ref, cpu


def _lifter(name, b3=False, staged=False):
    import ray3d_amd
    (_, sp), (_, st) = _states(name)
    fac = ray3d_amd.Model(_mc(name, b3), {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
    ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    lifter = ray3d_amd.Ray3DLifter(pos.eval(), trj.eval()).eval()
    lifter.set_staged(staged)
    assert lifter.precision(DEV) == ("bf16x3" if b3 else "f32")
    return lifter


def _hold(name, what, out, B, budget):
    """out (B windows, the first B of the reference's) against the fp32 port at 1e-4 and - fp32 handles - under the error budget."""
    _, _, ref, cpu = _reference(name)
    ref, cpu = ref[:B], cpu[:B]
    out = out.detach().cpu().numpy()
    e_hip = float(np.abs(out.astype(np.float64) - ref).max())
    e_cpu = float(np.abs(cpu.astype(np.float64) - ref).max())
    ulp = float(np.abs(ref).max()) * 2.0 ** -23
    print("%s %s, %d windows: HIP %.3e, torch-CPU fp32 %.3e (ratio %.2f), |ref| max %.2f"
          % (name, what, B, e_hip, e_cpu, e_hip / max(e_cpu, 1e-30), np.abs(ref).max()))
    check_parity(out, cpu, "%s %s %d windows vs torch port" % (name, what, B))
    if budget:
        record_parity("f32-budget %s %s %d windows (HIP err vs float64; bound = %.1f x torch-CPU fp32 err + 1 ulp)" % (name, what, B, F32_BUDGET),
                      e_hip, F32_BUDGET * e_cpu + ulp, float(np.abs(ref).max()))
        assert e_hip <= F32_BUDGET * e_cpu + ulp, (name, what, B, e_hip, e_cpu)


def _forward(lifter, name, B):
    x, p, _, _ = _reference(name)
    with torch.no_grad():
        out = lifter(torch.from_numpy(np.array(x[:B])).to(DEV), torch.from_numpy(np.array(p[:B])).to(DEV))
    lifter.check_status(DEV)
    return out


# ---------------------------------------------------------------- six levels

# (plan kind, B, staged, bf16x3): the small plan (<= 48 windows; 12: one-unit tiles, 26: the first two-unit ones), the medium plan
# (<= 96), the fused single launch, the level-by-level form, the bf16x3 tiles (from 96 windows)
SIX_LEVEL_KINDS = [("small", 12, False, False), ("small", 26, False, False), ("medium", 64, False, False),
                   ("fused", 97, False, False), ("staged", 97, True, False), ("bf16x3", 97, False, True)]


@pytest.mark.parametrize("kind,B,staged,b3", SIX_LEVEL_KINDS, ids=["%s-%d" % (k[0], k[1]) for k in SIX_LEVEL_KINDS])
def test_six_levels_in_every_plan_kind(kind, B, staged, b3):
    lifter = _lifter("six-levels", b3, staged)
    assert lifter.receptive_field() == 729
    _hold("six-levels", kind, _forward(lifter, "six-levels", B), B, budget=not b3)


def test_six_level_clip_call_against_its_materialised_windows():
    """97 windows sliding over 97 + 728 frames (one call, exact size): against the same handle fed the materialised windows at
    2e-5 * max(1, |out|) (another summation order at most), and eight of the windows against the torch port at 1e-4."""
    from oracle import torch_port
    from ray3d_amd import _capi
    from test_gpu_specialisations import _call
    lifter = _lifter("six-levels")
    lifter.CLIP_ROUND = 0
    (cp, sp), (ct, st) = _states("six-levels")
    x, p, _, _ = _reference("six-levels")
    n, rf = 97, 729
    # (the reference's windows laid end to end: every frame in the range of the model's inputs)
    clip = np.ascontiguousarray(np.array(x[:3]).reshape(-1, cp.num_joints, cp.in_features)[:n + rf - 1])
    assert clip.shape[0] == n + 728
    windows = np.stack([clip[i:i + rf] for i in range(n)])
    row = np.array(p[0])
    rows = np.tile(row[None], (n, 1))
    d_clip, d_win, d_row, d_rows = (torch.from_numpy(a).to(DEV) for a in (clip, windows, row, rows))
    out, out_trj = _call(lifter, _capi.R3D_INPUT_RAYS, d_clip, 1, n, d_row)
    lifter.check_status(DEV)
    w_out, w_trj = _call(lifter, _capi.R3D_INPUT_RAYS, d_win, rf, n, d_rows)
    lifter.check_status(DEV)
    check_parity(out, w_out.cpu().numpy(), "clip call vs its materialised windows", tol=2e-5 * max(1.0, float(w_out.abs().max())))
    check_parity(out_trj, w_trj.cpu().numpy(), "clip call vs its materialised windows, trj", tol=2e-5 * max(1.0, float(w_trj.abs().max())))
    pick = [0, 1, 31, 32, 48, 64, 95, 96]
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]
    with torch.no_grad():
        xw, pw = torch.from_numpy(windows[pick]), torch.from_numpy(rows[pick])
        ref = (torch_port.forward(cp, sds[0], xw, pw) + torch_port.forward(ct, sds[1], xw, pw)).numpy()
    check_parity(out[pick], ref, "clip call, eight windows vs torch port")


def test_six_levels_with_pixel_input():
    """26 windows of pixels, one camera row (uv-cam0): the bits of the same handle fed the rays of those pixels, and the torch
    port on those rays at 1e-4."""
    from oracle import torch_port
    from ray3d_amd import _capi, synth
    from test_gpu_specialisations import _call, _cameras
    lifter = _lifter("six-levels")
    (cp, sp), (ct, st) = _states("six-levels")
    cams, ocams = _cameras()
    B, rf = 26, 729
    uv = (1000.0 * synth.hash_uniform("config_domain.six-levels.uv-cam0", (B * rf, cp.num_joints, 2), 3)).astype(np.float32)
    rays = ocams[1].rays_from_uv(uv.astype(np.float64)).astype(np.float32)
    par = np.tile(np.asarray(cams[1].param(), np.float32)[None], (B, 1))
    d_uv, d_rays, d_par = (torch.from_numpy(a).to(DEV) for a in (uv, rays, par))
    d_cam = torch.from_numpy(np.asarray(cams[1].cam_row())).to(DEV)
    out, out_trj = _call(lifter, _capi.R3D_INPUT_UV, d_uv, rf, B, d_par, d_cam)
    lifter.check_status(DEV)
    r_out, r_trj = _call(lifter, _capi.R3D_INPUT_RAYS, d_rays, rf, B, d_par)
    lifter.check_status(DEV)
    assert torch.equal(out, r_out) and torch.equal(out_trj, r_trj), float((out - r_out).abs().max())
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in (sp, st)]
    with torch.no_grad():
        xw, pw = torch.from_numpy(rays.reshape(B, rf, cp.num_joints, 3)), torch.from_numpy(par)
        ref = (torch_port.forward(cp, sds[0], xw, pw) + torch_port.forward(ct, sds[1], xw, pw)).numpy()
    check_parity(out, ref, "six-levels uv-cam0 26 windows vs torch port")


# ---------------------------------------------------------------- the widths

# 70 windows (the medium plan; launch by launch above 256 channels) and the size at which the census finds the configuration's own
# tile kinds in bf16x3 (gemm_tile_nb<5>, <6> in r3d_forward_b3; <7> and <4> in r3d_gemm_b3)
WIDTH_CASES = [(name, B, b3) for name in ("latent-512", "c640-n320", "c768-n512-rf9") for B in (70, REF_WINDOWS[name]) for b3 in (False, True)]


@pytest.mark.parametrize("name,B,b3", WIDTH_CASES, ids=["%s-%d-%s" % (n, B, "bf16x3" if b3 else "f32") for n, B, b3 in WIDTH_CASES])
def test_wide_configurations_in_both_precisions(name, B, b3):
    lifter = _lifter(name, b3)
    _hold(name, "bf16x3" if b3 else "f32", _forward(lifter, name, B), B, budget=not b3)


# ---------------------------------------------------------------- four lanes

def test_four_lanes_lift_four_different_batches_at_once():
    """R3D_OPT_LANES = 4 on the default RF 27 pair: batches of 3, 12, 31 and 130 windows - the polled activation banks, the latency
    tiles and the fused list, each cut for 64 workgroups - issued on the four lanes' own streams three times round, joined, checked:
    every result equals the whole-chip forward to 2e-5 * max(1, |out|) (other tile schedules: fp32 rounding) and the oracle chain
    at 1e-4; with the lanes off again the plain forward has its earlier bits."""
    import ray3d_amd
    from oracle import oracle
    from ray3d_amd import synth
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    sizes = [3, 12, 31, 130]
    xs = [synth.synth_rays(B, cp, seed=41 + i) for i, B in enumerate(sizes)]
    ps = [synth.synth_param(B, seed=51 + i) for i, B in enumerate(sizes)]
    refs = [oracle.forward(cp, sp, x, p) + oracle.forward(ct, st, x, p) for x, p in zip(xs, ps)]
    dx, dp = [torch.from_numpy(x).to(DEV) for x in xs], [torch.from_numpy(p).to(DEV) for p in ps]
    with torch.no_grad():
        plain = [lifter(x, p).clone() for x, p in zip(dx, dp)]
        lifter.check_status(DEV)
        try:
            lifter.set_lanes(4, DEV)
            assert lifter.num_lanes() == 4 and len({lifter.lane_stream(k).cuda_stream for k in range(4)}) == 4
            outs = [[], [], [], []]
            for rep in range(3):
                for k in range(4):
                    with lifter.lane(k):
                        outs[k].append(lifter(dx[k], dp[k]))
            lifter.join_lanes()
            lifter.check_status(DEV)
            for k, B in enumerate(sizes):
                for rep, o in enumerate(outs[k]):
                    check_parity(o, plain[k].cpu().numpy(), "lane %d of 4, %d windows, vs the whole-chip forward (HIP against HIP)" % (k, B),
                                 tol=2e-5 * max(1.0, float(plain[k].abs().max())))
                    check_parity(o, refs[k], "lane %d of 4, %d windows, vs the oracle chain" % (k, B))
        finally:
            lifter.set_lanes(0, DEV)
        for k in range(4):
            assert torch.equal(lifter(dx[k], dp[k]), plain[k]), k
        lifter.check_status(DEV)
