"""-m gpu: every HIP path under weights with the BatchNorm statistics of a trained checkpoint (tests/trained_stats.py: dead
channels with variances far below eps, variances far above 1, negative and pruned gammas).  On the synthetic weights of the
rest of the suite an eps wrong by a third - in the fold (r3d_model.cpp, Folder::scale_shift), in one class of layer, or a fold
that is right for positive gammas only - stays below the 1e-4 bound; here an eps wrong by 1 % misses it by two orders of
magnitude (tests/test_trained_stats_host.py).

Comparand: the reference's own outputs (tests/golden/model_trained_*.npz) where a fixture exists, otherwise the torch port on
every window; bound: check_parity's literal 1e-4.  tests/test_trained_stats_host.py holds each network's float64 output to
<= 10 m and the torch port's fp32 error to <= 1e-5 for every input used here; each case asserts the 10 m again.  Each case also
records e_hip / e_cpu - the HIP result's error against the float64 torch port over the torch-CPU fp32 evaluation's error
against the same values - in its parity row: REPORTED, not asserted (F32_BUDGET was calibrated on the synthetic weights; the
measured ratios are in DESIGN.md)."""
import os

import numpy as np
import pytest
import torch

import trained_stats as ts
from conftest import check_parity, dev_switch, load_model_fixture, record_parity
from test_gpu_parity import FORMS, MODES, PLANS, _reference_cameras, build_modules

pytestmark = pytest.mark.gpu

LITERAL = 1e-4
_REFS = {}


def _mc(over):
    import ray3d_amd
    return ray3d_amd.default_model_config(**over)


def _refs(key, states, x, p):
    """The torch port on (x, p), once per key: each network in float64 and in fp32 on the CPU, and their sums."""
    if key not in _REFS:
        (p64, p32), (t64, t32) = [ts.f64_and_cpu((s,), x, p) for s in states]
        assert max(float(np.abs(p64).max()), float(np.abs(t64).max())) <= 10.0, key        # the scale the literal bound is meant at
        r = dict(pos64=p64, trj64=t64, pos32=p32, trj32=t32, sum64=p64 + t64, sum32=p32 + t32)
        for v in r.values():
            v.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _ratio(kind, what, out, r, part="sum"):
    """Report e_hip / e_cpu of one result in a parity row of its own (bound column: the literal 1e-4, on e_hip)."""
    if hasattr(out, "detach"):
        out = out.detach().cpu().numpy()
    ref64 = r[part + "64"]
    e_hip = float(np.abs(out.astype(np.float64) - ref64).max())
    e_cpu = float(np.abs(r[part + "32"].astype(np.float64) - ref64).max())
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split("::", 1)[-1].split(" (")[0]
    record_parity("trained-ratio [%s] %s %s: e_hip / e_cpu = %.2f (torch-CPU fp32 err %.2e)" % (kind, test, what, e_hip / max(e_cpu, 1e-30), e_cpu),
                  e_hip, LITERAL, float(np.abs(ref64).max()))
    return e_hip / max(e_cpu, 1e-30)


def _cuda(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _lifter(mc, scale=1.0):
    import ray3d_amd
    pos, trj, sp, st = ts.build_trained_modules(mc, scale)
    return ray3d_amd.Ray3DLifter(pos, trj).eval(), pos, trj, (sp, st)


# ---------------------------------------------------------------- (a), (b): the reference fixtures

@pytest.mark.parametrize("fused", PLANS)
@pytest.mark.parametrize("name", list(ts.TRAINED_CASES))
def test_trained_fixture_modules_and_pair_on_both_plans(name, fused, monkeypatch):
    """The modules alone and the lifter pair against the reference's outputs, on the un-fused plan of calls of a few windows and
    (R3D_NO_SMALL_PLAN) on the fused plan."""
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")
    z, mc = load_model_fixture(name)
    lifter, pos, trj, states = _lifter(mc)
    r = _refs(name, states, z["x"], z["param"])
    x, p = _cuda(z["x"], z["param"])
    with torch.no_grad():
        op, ot = pos(x, p).cpu().numpy(), trj(x, p).cpu().numpy()
        out, out_trj = lifter(x, p, return_trj=True)
    lifter.check_status()
    assert float(np.abs(z["out_pos"]).max()) <= 10.0 and float(np.abs(z["out_trj"]).max()) <= 10.0
    check_parity(op, z["out_pos"], "pos module vs reference fixture")
    check_parity(ot, z["out_trj"], "trj module vs reference fixture")
    check_parity(out, z["out_pos"] + z["out_trj"], "pair, pos+trj vs reference fixture")
    check_parity(out_trj, z["out_trj"], "pair, trj vs reference fixture")
    _ratio("fused" if fused else "small", "pair", out, r)
    _ratio("fused" if fused else "small", "pos module", op, r, "pos")


@pytest.mark.parametrize("staged", FORMS)
@pytest.mark.parametrize("b3", MODES)
@pytest.mark.parametrize("name", list(ts.TRAINED_CASES))
def test_trained_fixture_in_every_mode_and_form(name, b3, staged):
    """The fixture's windows tiled to 128 (the fully fused plan, and enough rows for the bf16x3 tiles) in fp32 and bf16x3
    (planes read back from the folded copy), as one launch and level by level: pos alone, trj and the sum."""
    if os.environ.get("R3D_BF16X3") is not None and b3 != (os.environ["R3D_BF16X3"] == "1"):
        pytest.skip("R3D_BF16X3 in the environment overrides the configuration key")
    z, mc = load_model_fixture(name)
    lifter, pos, trj, states = _lifter(dict(mc, BF16X3=b3))
    lifter.set_staged(staged)
    reps = -(-128 // z["x"].shape[0])
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))
    r = _refs(name + "/128", states, tile(z["x"]), tile(z["param"]))
    x, p = _cuda(tile(z["x"]), tile(z["param"]))
    with torch.no_grad():
        out, out_trj = lifter(x, p, return_trj=True)
        op = pos(x, p)
    lifter.check_status()
    assert lifter.precision(x.device) == ("bf16x3" if b3 else "f32")
    check_parity(out, tile(z["out_pos"] + z["out_trj"]), "pos+trj vs reference fixture")
    check_parity(out_trj, tile(z["out_trj"]), "trj vs reference fixture")
    check_parity(op, tile(z["out_pos"]), "pos vs reference fixture")
    _ratio(("staged" if staged else "fused") + ("-bf16x3" if b3 else ""), "pair", out, r)


# ---------------------------------------------------------------- (c): calls of a few windows

def _few_windows(B, monkeypatch, switch, value):
    dev_switch(monkeypatch, switch, value)
    lifter, _, _, states = _lifter(_mc(ts.RF27))                  # (the switch is read when a schedule is built: fresh handles)
    x, p = ts.window_inputs(states[0][0], B)
    r = _refs("rf27/%d" % B, states, x, p)
    xd, pd = _cuda(x, p)
    with torch.no_grad():
        out = lifter(xd, pd)
    lifter.check_status()
    return lifter, out, r, xd, pd


@pytest.mark.parametrize("no_gemv", ["0", "1"], ids=["gemv-tiles", "mfma-split-k-tiles"])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_trained_calls_of_one_to_four_windows(B, no_gemv, monkeypatch):
    _, out, r, _, _ = _few_windows(B, monkeypatch, "R3D_NO_GEMV", no_gemv)
    check_parity(out, r["sum32"], "%d windows vs torch port" % B)
    _ratio("gemv" if no_gemv == "0" else "split-k", "%d windows" % B, out, r)


@pytest.mark.parametrize("no_lat", ["0", "1"], ids=["latency-tiles", "split-k-tiles"])
@pytest.mark.parametrize("B", [5, 11, 32])
def test_trained_calls_of_five_to_32_windows(B, no_lat, monkeypatch):
    _, out, r, _, _ = _few_windows(B, monkeypatch, "R3D_NO_LAT", no_lat)
    check_parity(out, r["sum32"], "%d windows vs torch port" % B)
    _ratio("latency" if no_lat == "0" else "split-k", "%d windows" % B, out, r)


def test_trained_call_of_12_windows_captured_in_a_graph():
    """Eager calls of up to 16 windows poll their operands (data as its own ready flag); a captured call of the same size
    takes the ready counters, in the caller's workspace: the replay against the torch port, and the bits of the eager call."""
    import ray3d_amd
    B = 12
    lifter, _, _, states = _lifter(_mc(ts.RF27))
    x, p = ts.window_inputs(states[0][0], B)
    r = _refs("rf27/%d" % B, states, x, p)
    xd, pd = _cuda(x, p)
    with torch.no_grad():
        eager = lifter(xd, pd)
        lifter.check_status()
        check_parity(eager, r["sum32"], "eager (poll mode) vs torch port")
        lifter.prepare([B])
        out = torch.empty((B, 1, 17, 3), device="cuda")
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                lifter._run(ray3d_amd._capi.R3D_INPUT_RAYS, xd, 27, B, pd, 2, out=out)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
    lifter.check_status()
    check_parity(out, r["sum32"], "captured (counter path) vs torch port")
    assert torch.equal(out, eager)
    _ratio("latency", "captured", out, r)


# ---------------------------------------------------------------- (d): clip calls

@pytest.mark.parametrize("per_frame", [True, False], ids=["per-frame-first-layers", "gathered"])
@pytest.mark.parametrize("config", list(ts.CLIP_CONFIGS))
def test_trained_clip_call_of_130_windows(config, per_frame, monkeypatch):
    """forward_clip over exactly 130 sliding windows: the per-frame [E | V] tables are copies of the folded first layers.  Against
    the torch port on the materialised windows; with the per-frame first layers switched off (R3D_NO_SHARED_L0) the call is the
    window call's arithmetic in its order: bit-equal."""
    if not per_frame:
        dev_switch(monkeypatch, "R3D_NO_SHARED_L0", "1")
    elif os.environ.get("R3D_BF16X3") == "1":
        pytest.skip("bf16x3 handles keep the gathered first level (the per-frame form exists for the fp32 tiles)")
    lifter, _, _, states = _lifter(_mc(ts.CLIP_CONFIGS[config]))
    cp = states[0][0]
    clip, windows, prow, pw = ts.clip_inputs(cp)
    n = ts.CLIP_WINDOWS
    r = _refs("clip/" + config, states, windows, pw)
    clip_d, win_d, prow_d, pw_d = _cuda(clip, windows, prow, pw)
    lifter.CLIP_ROUND = 0                                            # one forward of exactly n windows
    with torch.no_grad():
        a = lifter.forward_clip(clip_d, prow_d)
        b = lifter(win_d, pw_d if cp.camera_embedding else None)
    lifter.check_status()
    assert a.shape == (n, 1, cp.num_joints, 3)
    check_parity(a, r["sum32"], "clip call vs torch port on the materialised windows")
    check_parity(b, r["sum32"], "window call vs torch port")
    if not per_frame:
        assert torch.equal(a, b)
    _ratio("clip" if per_frame else "clip-gathered", config, a, r)


# ---------------------------------------------------------------- (e): pixel input

@pytest.mark.parametrize("fused", PLANS)
@pytest.mark.parametrize("config", list(ts.UV_CONFIGS))
def test_trained_forward_uv_with_a_camera_row_per_window(config, fused, monkeypatch):
    """Pixels and one reference camera per window in, rays encoded in the first-level gather: the bits of the rays forward on
    host-encoded rays, and within the bound of the oracle chain (oracle cameras in float64, cast, torch port)."""
    if fused:
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")
    cams, ocams, z, tags = _reference_cameras()
    assert np.abs(ocams[0].rays_from_uv(z[tags[0] + "/uv"]) - z[tags[0] + "/rays"]).max() < 1e-12   # the encoding, pinned to the reference
    lifter, _, _, states = _lifter(_mc(ts.UV_CONFIGS[config]))
    uv, rays, rows, par = ts.uv_inputs(states[0][0], cams, ocams)
    par = par.astype(np.float32)
    r = _refs("uv/" + config, states, rays, par)
    uv_d, rays_d, rows_d, par_d = _cuda(uv, rays, rows, par)
    with torch.no_grad():
        a = lifter.forward_uv(uv_d, rows_d, par_d)
        b = lifter(rays_d, par_d)
    lifter.check_status()
    assert torch.equal(a, b)
    check_parity(a, r["sum32"], "pixel input vs the oracle chain")
    _ratio("uv-fused" if fused else "uv-small", config, a, r)


# ---------------------------------------------------------------- (f), (g), (h): shrink fold, widths, RF 243

@pytest.mark.parametrize("config", list(ts.SHRINK_CONFIGS))
def test_trained_shrink_folded_into_its_consumers_and_kept_apart(config, monkeypatch):
    """Layer::pre composes `shrink` with the Linears that read it, then scales the composed row by the consumer's BatchNorm:
    R3D_NO_SHRINK_FOLD=1 keeps the layer.  Both within the bound, within a fifth of it of each other, and not the same bits."""
    outs = []
    for nofold in ("0", "1"):
        dev_switch(monkeypatch, "R3D_NO_SHRINK_FOLD", nofold)
        lifter, _, _, states = _lifter(_mc(ts.SHRINK_CONFIGS[config]))
        x, p = ts.window_inputs(states[0][0], ts.SHRINK_WINDOWS)
        r = _refs("windows/%s/%d" % (config, ts.SHRINK_WINDOWS), states, x, p)
        with torch.no_grad():
            outs.append(lifter(*_cuda(x, p)).cpu().numpy())
        lifter.check_status()
        check_parity(outs[-1], r["sum32"], "shrink %s vs torch port" % ("kept apart" if nofold == "1" else "folded"))
        _ratio("fused-first-level" + ("-no-shrink-fold" if nofold == "1" else ""), config, outs[-1], r)
    assert np.abs(outs[0] - outs[1]).max() <= 0.2 * LITERAL
    assert not np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("config", list(ts.WIDTH_CONFIGS))
def test_trained_channel_widths(config):
    """Channel counts that are no tile width (column padding of the folded rows) and above 256 (the un-fused first level)."""
    lifter, _, _, states = _lifter(_mc(ts.WIDTH_CONFIGS[config]))
    x, p = ts.window_inputs(states[0][0], ts.WIDTH_WINDOWS)
    r = _refs("width/" + config, states, x, p)
    with torch.no_grad():
        out = lifter(*_cuda(x, p))
    lifter.check_status()
    check_parity(out, r["sum32"], "vs torch port")
    _ratio("width", config, out, r)


@pytest.mark.parametrize("staged", FORMS)
def test_trained_rf243(staged):
    """Five levels at 40 windows (decoder scale RF243_SCALE: the trajectory output would pass 10 m at 1.0)."""
    lifter, _, _, states = _lifter(_mc(ts.RF243), ts.RF243_SCALE)
    lifter.set_staged(staged)
    x, p = ts.window_inputs(states[0][0], ts.RF243_WINDOWS)
    r = _refs("rf243", states, x, p)
    with torch.no_grad():
        out = lifter(*_cuda(x, p))
    lifter.check_status()
    check_parity(out, r["sum32"], "vs torch port")
    _ratio("rf243-staged" if staged else "rf243-small", "40 windows", out, r)


# ---------------------------------------------------------------- (i): seeded random configurations

@pytest.mark.parametrize("b3", MODES)
@pytest.mark.parametrize("seed", ts.RANDOM_SEEDS)
def test_trained_random_configurations(seed, b3):
    over, B = ts.random_configuration(seed)
    lifter, _, _, states = _lifter(_mc(dict(over, BF16X3=b3)))
    cp = states[0][0]
    x, p = ts.window_inputs(cp, B, seed=seed)
    r = _refs("random/%d" % seed, states, x, p)
    xd, pd = _cuda(x, p)
    with torch.no_grad():
        out = lifter(xd, pd if cp.camera_embedding else None)
    lifter.check_status()
    check_parity(out, r["sum32"], "%d windows vs torch port" % B)
    _ratio("random" + ("-bf16x3" if b3 else ""), "seed %d" % seed, out, r)


# ---------------------------------------------------------------- (j): re-fold on update

def test_trained_state_loaded_over_synthetic_weights_is_folded_again():
    """Modules that have run on the synthetic weights, then load_state_dict of the trained-like state: every table derived from the
    fold (shrink composition, column sums, [E | V], bf16x3 planes) is rebuilt - the bits of fresh modules built from that state,
    on the un-fused plan (4 windows), the fused first level (75) and a clip call (130)."""
    import ray3d_amd
    mc = _mc(ts.RF27)
    pos, trj, _, _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    fresh, fpos, ftrj, states = _lifter(mc)
    cp = states[0][0]
    clip, windows, prow, pw = ts.clip_inputs(cp)
    calls = []
    for B in (4, ts.SHRINK_WINDOWS):
        x, p = ts.window_inputs(cp, B)
        calls.append(("%d windows" % B, _refs("rf27/%d" % B, states, x, p), _cuda(x, p)))
    clip_d, prow_d = _cuda(clip, prow)
    lifter.CLIP_ROUND = fresh.CLIP_ROUND = 0
    with torch.no_grad():
        before = [lifter(*a).clone() for _, _, a in calls] + [lifter.forward_clip(clip_d, prow_d).clone()]
        ts.load_states(pos, trj, states[0][1], states[1][1])
        after = [lifter(*a) for _, _, a in calls] + [lifter.forward_clip(clip_d, prow_d)]
        want = [fresh(*a) for _, _, a in calls] + [fresh.forward_clip(clip_d, prow_d)]
        one = (pos(*calls[0][2]), fpos(*calls[0][2]), trj(*calls[0][2]), ftrj(*calls[0][2]))
    lifter.check_status(), fresh.check_status()
    refs = [r for _, r, _ in calls] + [_refs("clip/rf27", states, windows, pw)]
    for what, b, a, w, r in zip([c[0] for c in calls] + ["clip call"], before, after, want, refs):
        assert not torch.equal(a, b), what                             # (the update was picked up)
        assert torch.equal(a, w), what
        check_parity(a, r["sum32"], what + " after the update vs torch port")
        _ratio("re-fold", what, a, r)
    assert torch.equal(one[0], one[1]) and torch.equal(one[2], one[3])
