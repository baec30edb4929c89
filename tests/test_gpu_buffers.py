"""-m gpu: WHERE the library reads and writes.  Every device buffer of a call - input, parameter rows, camera rows, outputs,
workspace - is carved to its exact size out of one pattern-filled allocation with 1 MiB guards (tests/buffers_util.py); the
workspace is exactly r3d_workspace_bytes / r3d_input_workspace_bytes.  After the call the guards must still hold the
pattern, the outputs must be finite, and they must be the same bits whatever the scratch and the memory around the
buffers held: zeros, NaN, +Inf, or the library's own "not produced yet" word (ACT_SENTINEL).  Values are checked against
the oracle once per case at the literal 1e-4 bound of the parity suite."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from buffers_util import ACT_SENTINEL, NANS, PATTERN_IDS, PATTERNS, Arena, ExactWorkspace, fill_pattern
from conftest import check_parity, dev_switch, load_model_fixture
from test_gpu_parity import _oracle_lift, _reference_cameras, build_modules

pytestmark = pytest.mark.gpu

OUT_SENTINEL = 12345.678           # finite, and nothing a forward of these weights produces (outputs are a few metres)
DEV = "cuda:0"


# ---------------------------------------------------------------- models

def _model_config(name):
    """Named configurations of the path tables (defaults: ARCHITECTURE "3,3,3", 17 joints)."""
    import ray3d_amd
    fixtures = {"f2-noemb": "j17_f2_rf27_noemb_s3", "dense": "j17_rf27_dense_s3", "dense-causal": "j14_rf9_dense_causal_s2",
                "dilated": "j17_rf27_dilated_s3", "causal-rf81": "j17_rf81_causal_s3"}
    if name in fixtures:
        return load_model_fixture(fixtures[name])[1]
    over = {"default": dict(), "rf9": dict(ARCHITECTURE="3,3"),
            "f2-noemb-rf9": dict(ARCHITECTURE="3,3", INPUT_DIM=2, CAMERA_EMBDDING=False),
            "j14-rf9": dict(ARCHITECTURE="3,3", NUM_KPTS=14), "j15-s2": dict(NUM_KPTS=15, STAGE=2),
            "s1-noemb": dict(STAGE=1, CAMERA_EMBDDING=False), "c64": dict(CHANNELS=64, LATENT_FEATURES_DIM=128),
            "c96": dict(CHANNELS=96, LATENT_FEATURES_DIM=128), "c512": dict(CHANNELS=512, LATENT_FEATURES_DIM=128),
            "bf16x3": dict(BF16X3=True), "bf16x3-rf9": dict(ARCHITECTURE="3,3", BF16X3=True)}[name]
    return ray3d_amd.default_model_config(**dict(dict(ARCHITECTURE="3,3,3"), **over))


def _fresh_pair(name, staged=False):
    """(lifter, ((cfg, state) pos, (cfg, state) trj)) on the library that is selected NOW."""
    import ray3d_amd
    pos, trj, sp, st = build_modules(_model_config(name))
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.CLIP_ROUND = 0                              # sequences are lifted in ONE forward of exactly their window count
    lifter.set_staged(staged)
    return lifter, (sp, st)


@functools.lru_cache(maxsize=None)
def _pair(name, staged=False):
    """... of the product library, built once per session."""
    return _fresh_pair(name, staged)


def _rays_call(cfg, B, seed):
    """A (B, RF, J, F) batch with its (B, 2) parameter rows (None without the camera embedding) as a call description."""
    from ray3d_amd import _capi, synth
    x = synth.synth_rays(B, cfg, seed=seed)
    p = synth.synth_param(B, seed=seed + 1) if cfg.camera_embedding else None
    return dict(mode=_capi.R3D_INPUT_RAYS, x=x, stride=cfg.receptive_field, B=B, param=p, pstride=2 if p is not None else 0,
                cam=None, cstride=0)


# ---------------------------------------------------------------- one guarded call, once per pattern

def _input(call, x, p, cam):
    from ray3d_amd import _capi
    return _capi.make_input(call["mode"], x.data_ptr(), call["stride"], p.data_ptr() if p is not None else None, call["pstride"],
                            cam.data_ptr() if cam is not None else None, call["cstride"])


def _need(handles, call):
    """The workspace the library asks for for this call: r3d_input_workspace_bytes in the pixel pre-pass modes."""
    from ray3d_amd import _capi
    hp, ht = handles
    if call["mode"] in _capi.PX_MODES:
        probe = _capi.make_input(call["mode"], 256, call["stride"], None, call["pstride"], 256, call["cstride"])   # (pointers are not read)
        return _capi.input_workspace_bytes(hp, ht, probe, call["B"])
    return _capi.workspace_bytes(hp, ht, call["B"])


def guarded(lifter, call, entry="pair+trj", patterns=PATTERNS, skew=0):
    """The call once per pattern with every buffer carved exactly from an arena filled with that pattern ->
    [(out, out_trj or None)] per pattern, after assertions a (guards clean) and b (outputs finite, sentinel gone).
    entry: "pair+trj" r3d_forward_pair with out_trj (C ABI), "pair" the same with out_trj NULL through Ray3DLifter._run and
    the workspace adapter, "pos" / "trj" r3d_forward of one network (C ABI)."""
    from ray3d_amd import _capi
    dev = torch.device(DEV)
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    handles = {"pos": (hp, None), "trj": (None, ht)}.get(entry, (hp, ht))
    B, J = call["B"], lifter.pos.num_joints_in
    out_shape = (B, 1, 1 if entry == "trj" else J, 3)
    nbytes = _need(handles, call)
    inputs = [(k, np.ascontiguousarray(call[k], dtype=np.float64 if k == "cam" else np.float32)) for k in ("x", "param", "cam") if call[k] is not None]
    sizes = [np.asarray(a).nbytes for _, a in inputs] + [int(np.prod(out_shape)) * 4, B * 3 * 4, nbytes]
    arena = Arena(dev, patterns[0], Arena.capacity_for(sizes))
    put = {k: arena.put(a, skew=skew if k != "cam" else 0, name=k + "_dev") for k, a in inputs}
    out = arena.carve(int(np.prod(out_shape)) * 4, skew=skew, name="out_dev").view(torch.float32).view(out_shape)
    out_trj = arena.carve(B * 3 * 4, skew=skew, name="out_trj_dev").view(torch.float32).view(B, 1, 1, 3) if entry == "pair+trj" else None
    ws = ExactWorkspace(arena, "workspace_dev")
    wsv = ws.get(nbytes, dev)
    assert wsv.data_ptr() % 256 == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    results = []
    for pattern in patterns:
        arena.refill(pattern)
        t = {k: w() for k, w in put.items()}
        x, p, cam = t["x"], t.get("param"), t.get("cam")
        out.fill_(OUT_SENTINEL)
        if out_trj is not None:
            out_trj.fill_(OUT_SENTINEL)
        with torch.no_grad(), torch.cuda.device(dev):
            if entry == "pair+trj":
                _capi.forward_pair(hp, ht, _input(call, x, p, cam), B, out.data_ptr(), out_trj.data_ptr(), wsv.data_ptr(), nbytes, stream)
            elif entry == "pair":
                res = lifter._run(call["mode"], x, call["stride"], B, p, call["pstride"], cam, call["cstride"], out=out, workspace=ws)
                assert res is out
            else:
                _capi.forward(hp if entry == "pos" else ht, _input(call, x, p, cam), B, out.data_ptr(), wsv.data_ptr(), nbytes, stream)
        what = "%s, pattern 0x%08X" % (entry, pattern)
        arena.check()                                                                    # a. (synchronises)
        lifter.check_status(dev)
        for o in (out, out_trj):                                                         # b.
            if o is not None:
                assert torch.isfinite(o).all(), what
                assert not (o == OUT_SENTINEL).any(), what
        results.append((out.clone(), out_trj.clone() if out_trj is not None else None))
    return results


def _all_equal(results, plain, plain_trj, what):
    """c. the outputs of all patterns equal each other and the ordinary call's, bit for bit."""
    for pid, (o, t) in zip(PATTERN_IDS, results):
        assert torch.equal(o, plain), (what, pid, float((o - plain).abs().max()))
        if t is not None and plain_trj is not None:
            assert torch.equal(t, plain_trj), (what, pid, "trj", float((t - plain_trj).abs().max()))


def _reference(states, call_windows, param, B):
    """pos + trj of the oracle chain (the torch port of the reference graph, pinned to the reference fixtures) and trj alone."""
    from oracle import torch_port
    (cp, sp), (ct, st) = states
    prm = np.asarray(param, np.float32) if param is not None else np.zeros((B, 2), dtype=np.float32)
    both = _oracle_lift(states, call_windows, prm)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}
    with torch.no_grad():
        trj = np.concatenate([torch_port.forward(ct, sd, torch.from_numpy(call_windows[i:i + 512]), torch.from_numpy(prm[i:i + 512])).numpy()
                              for i in range(0, B, 512)])
    return both, trj


def _reference_pos(states, call_windows, param, B):
    """... and the pos network alone."""
    from oracle import torch_port
    (cp, sp), _ = states
    prm = np.asarray(param, np.float32) if param is not None else np.zeros((B, 2), dtype=np.float32)
    with torch.no_grad():
        return torch_port.forward(cp, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()}, torch.from_numpy(call_windows),
                                  torch.from_numpy(prm)).numpy()


# ---------------------------------------------------------------- 5. (first: a wrong size formula shows here, not as a dirty guard)

@pytest.mark.parametrize("staged", [False, True], ids=["single-launch", "staged"])
@pytest.mark.parametrize("B", [3, 37, 97, 200, 1025])
def test_too_small_a_workspace_is_refused_before_anything_runs(B, staged):
    """One byte less than r3d_workspace_bytes(B): R3D_ERR_WORKSPACE, nothing launched (the output keeps its sentinel, the
    guards their pattern); exactly r3d_workspace_bytes(B): the call runs.  One call per plan kind, both forms."""
    from ray3d_amd import _capi
    lifter, ((cp, _), _) = _pair("default", staged)
    dev = torch.device(DEV)
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    call = _rays_call(cp, B, seed=500 + B)
    nbytes = _capi.workspace_bytes(hp, ht, B)
    out_shape = (B, 1, lifter.pos.num_joints_in, 3)
    out_bytes = int(np.prod(out_shape)) * 4
    arena = Arena(dev, NANS, Arena.capacity_for([call["x"].nbytes, call["param"].nbytes, out_bytes, nbytes]))
    x, p = arena.put(call["x"], name="x_dev")(), arena.put(call["param"], name="param_dev")()
    out = arena.carve(out_bytes, name="out_dev").view(torch.float32).view(out_shape)
    ws = arena.carve(nbytes, name="workspace_dev")
    out.fill_(OUT_SENTINEL)
    inp = _input(call, x, p, None)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib = hp._lib
    rc = lib.r3d_forward_pair(hp.ptr, ht.ptr, C.byref(inp), B, out.data_ptr(), None, ws.data_ptr(), nbytes - 1, stream)
    assert rc == _capi.R3D_ERR_WORKSPACE, (rc, lib.r3d_last_error())
    arena.check()
    assert (out == OUT_SENTINEL).all()
    rc = lib.r3d_forward_pair(hp.ptr, ht.ptr, C.byref(inp), B, out.data_ptr(), None, ws.data_ptr(), nbytes, stream)
    assert rc == 0, (rc, lib.r3d_last_error())
    arena.check()
    lifter.check_status(dev)
    assert torch.isfinite(out).all() and not (out == OUT_SENTINEL).any()


# ---------------------------------------------------------------- 1. the forward's path tables

_EAGER = [1, 3, 5, 16, 17, 33, 37, 48, 49, 95, 97, 130, 200, 1025]
_VARIANTS = [("j14-rf9", 37), ("j15-s2", 11), ("s1-noemb", 37), ("f2-noemb", 37), ("dense", 9), ("dense", 37), ("dense-causal", 9),
             ("dense-causal", 37), ("dilated", 37), ("causal-rf81", 5), ("c64", 11), ("c96", 11), ("c512", 37), ("bf16x3", 97), ("bf16x3", 130)]
FORWARD_CASES = ([pytest.param("default", "single", B, "pair+trj", id="single-launch-%d" % B) for B in _EAGER] +
                 [pytest.param("default", "staged", B, "pair+trj", id="staged-%d" % B) for B in (3, 37, 97)] +
                 [pytest.param("default", "fused", B, "pair+trj", id="no-small-plan-%d" % B) for B in (3, 37)] +
                 [pytest.param(name, "single", B, "pair+trj", id="%s-%d" % (name, B)) for name, B in _VARIANTS] +
                 [pytest.param("default", "single", 37, entry, id="entry-%s-37" % entry) for entry in ("pair", "pos", "trj")] +
                 [pytest.param("s1-noemb", "single", 3, entry, id="entry-%s-noemb-3" % entry) for entry in ("pos", "trj")])


@pytest.mark.parametrize("name,form,B,entry", FORWARD_CASES)
def test_forward_stays_inside_its_buffers_and_ignores_scratch_contents(name, form, B, entry, monkeypatch):
    if form == "fused":
        dev_switch(monkeypatch, "R3D_NO_SMALL_PLAN", "1")       # (read when a schedule is built: handles of the hooks build, made now)
        lifter, states = _fresh_pair(name)
    else:
        lifter, states = _pair(name, form == "staged")
    (cp, _), _ = states
    call = _rays_call(cp, B, seed=300 + B)
    results = guarded(lifter, call, entry)
    xt = torch.from_numpy(call["x"]).to(DEV)
    pt = torch.from_numpy(call["param"]).to(DEV) if call["param"] is not None else None
    both, trj = _reference(states, call["x"], call["param"], B)
    what = "%s %s B=%d %s" % (name, form, B, entry)
    with torch.no_grad():
        if entry in ("pos", "trj"):
            # r3d_forward of one network: the module's own forward (LiftModule.forward) on the exact workspace too
            module = lifter.pos if entry == "pos" else lifter.trj
            plain = module(xt, pt)
            h = module.handle(torch.device(DEV))
            arena = Arena(DEV, NANS, Arena.capacity_for([_need((h, None) if entry == "pos" else (None, h), call)]))
            keep, module._ws = module._ws, ExactWorkspace(arena, "workspace_dev")
            try:
                exact = module(xt, pt)
                arena.check()
            finally:
                module._ws = keep
            assert torch.equal(exact, plain), what
            _all_equal(results, plain, None, what)
            check_parity(plain, trj if entry == "trj" else _reference_pos(states, call["x"], call["param"], B), what + " vs the oracle chain")   # d.
            return
        plain, plain_trj = lifter(xt, pt, return_trj=True)
    lifter.check_status(DEV)
    _all_equal(results, plain, plain_trj, what)
    check_parity(plain, both, what + " pos+trj vs the oracle chain")                                        # d.
    check_parity(plain_trj, trj, what + " trj vs the oracle chain")


# ---------------------------------------------------------------- 2. clip and pixel inputs

def _clip_case(B, per_window):
    from ray3d_amd import _capi, synth
    lifter, states = _pair("default")
    (cp, _), _ = states
    rf = cp.receptive_field
    frames = (B - 1) + rf                                          # exactly: the last window ends with the clip
    clip = synth.synth_rays(1, cp, seed=7)[0]
    clip = np.concatenate([clip] * (frames // rf + 1), axis=0)[:frames] + 0.01 * np.arange(frames, dtype=np.float32)[:, None, None]
    prm = synth.synth_param(B, seed=8) if per_window else np.tile(np.array([[1.5, 0.2]], np.float32), (B, 1))
    call = dict(mode=_capi.R3D_INPUT_RAYS, x=np.ascontiguousarray(clip), stride=1, B=B, param=prm if per_window else prm[0], pstride=2 if per_window else 0,
                cam=None, cstride=0)
    windows = np.stack([clip[i:i + rf] for i in range(B)])

    def plain():
        if not per_window:
            return lifter.forward_clip(torch.from_numpy(clip).to(DEV), torch.from_numpy(prm[0]).to(DEV))
        return lifter._run(_capi.R3D_INPUT_RAYS, torch.from_numpy(clip).to(DEV), 1, B, torch.from_numpy(prm).to(DEV), 2)
    return lifter, states, call, windows, prm, plain


def _uv_case(arch_name, B, stride, per_window):
    """R3D_INPUT_UV: pixels of the reference cameras, 8-double rows: exactly B of them, or exactly one."""
    from ray3d_amd import _capi, synth
    lifter, states = _pair(arch_name)
    (cp, _), _ = states
    rf = cp.receptive_field
    cams, _, _, _ = _reference_cameras()
    frames = (B - 1) * stride + rf
    seq = (1000.0 * synth.hash_uniform("buffers.uv.%s.%d" % (arch_name, stride), (frames, lifter.pos.num_joints_in, 2), 3)).astype(np.float32)
    pick = [cams[(3 * i) % len(cams)] for i in range(B)] if per_window else [cams[1]] * B
    windows = np.stack([pick[i].rays_from_uv(seq[i * stride:i * stride + rf].astype(np.float64)) for i in range(B)]).astype(np.float32)
    prm = np.stack([c.param() for c in pick]).astype(np.float32)
    rows = np.stack([c.cam_row() for c in pick]) if per_window else pick[0].cam_row()
    assert rows.shape == ((B, 8) if per_window else (8,))
    call = dict(mode=_capi.R3D_INPUT_UV, x=seq, stride=stride, B=B, param=prm, pstride=2, cam=rows, cstride=8 if per_window else 0)

    def plain():
        x = torch.from_numpy(seq).to(DEV)
        return lifter.forward_uv(x.view(B, rf, -1, 2) if stride == rf else x, torch.from_numpy(rows).to(DEV), torch.from_numpy(prm).to(DEV),
                                 window_stride=None if stride == rf else stride)
    return lifter, states, call, windows, prm, plain


def _dist_case(B, stride, per_window):
    """R3D_INPUT_UV_DIST: raw pixels of the distorted H36M cameras, rows of exactly 16 doubles; the oracle chain's rays."""
    from ray3d_amd import _capi
    from test_gpu_undistort import _h36m_distorted_cameras, _oracle_rays, _pixels
    lifter, states = _pair("default")
    (cp, _), _ = states
    rf = cp.receptive_field
    cams, ocams = _h36m_distorted_cameras()
    frames = (B - 1) * stride + rf
    seq = _pixels("buffers.dist.%d.%d" % (stride, B), (frames, lifter.pos.num_joints_in, 2))
    pick = [(i + stride) % 4 for i in range(B)] if per_window else [3] * B
    windows = np.stack([_oracle_rays(ocams[c], seq[i * stride:i * stride + rf]) for i, c in enumerate(pick)])
    prm = np.stack([cams[c].param() for c in pick]).astype(np.float32)
    rows = np.stack([cams[c].cam_row(distortion=True) for c in pick]) if per_window else cams[3].cam_row(distortion=True)
    assert rows.shape == ((B, 16) if per_window else (16,))
    call = dict(mode=_capi.R3D_INPUT_UV_DIST, x=seq, stride=stride, B=B, param=prm, pstride=2, cam=rows, cstride=16 if per_window else 0)

    def plain():
        x = torch.from_numpy(seq).to(DEV)
        return lifter.forward_uv(x.view(B, rf, -1, 2) if stride == rf else x, torch.from_numpy(rows).to(DEV), torch.from_numpy(prm).to(DEV),
                                 window_stride=None if stride == rf else stride)
    return lifter, states, call, windows, prm, plain


def _px_case(keyword, B, stride, per_window):
    """R3D_INPUT_PX_INTRINSIC / _SCREEN on the 2-feature pair without the camera embedding (param_dev NULL): the host's
    float64 -> float32 encoding of the windows, as tests/test_gpu_px2d.py obtains it."""
    from test_gpu_px2d import _cameras, _host, _mode
    from test_gpu_undistort import _pixels
    lifter, states = _pair("f2-noemb-rf9")                        # (this module's own pair: CLIP_ROUND = 0 stays here)
    rf = lifter.receptive_field()
    cams = _cameras(True)
    frames = (B - 1) * stride + rf
    seq = _pixels("buffers.px.%s.%d.%d" % (keyword, stride, B), (frames, lifter.pos.num_joints_in, 2))
    pick = [(3 * i + 1) % 4 for i in range(B)] if per_window else [2] * B
    windows = np.stack([_host(cams[c], seq[i * stride:i * stride + rf], keyword) for i, c in enumerate(pick)])
    rows = np.stack([cams[c].cam_row(distortion=True) for c in pick]) if per_window else cams[2].cam_row(distortion=True)
    call = dict(mode=_mode(keyword), x=seq, stride=stride, B=B, param=None, pstride=0, cam=rows, cstride=16 if per_window else 0)

    def plain():
        x = torch.from_numpy(seq).to(DEV)
        return lifter.forward_uv(x.view(B, rf, -1, 2) if stride == rf else x, torch.from_numpy(rows).to(DEV),
                                 window_stride=None if stride == rf else stride, encoding=keyword)
    return lifter, states, call, windows, None, plain


INPUT_CASES = ([pytest.param(lambda B=B: _clip_case(B, False), id="clip-one-row-%d" % B) for B in (1, 40, 300)] +
               [pytest.param(lambda: _clip_case(40, True), id="clip-per-window-rows-40")] +
               [pytest.param(lambda a=a, pw=pw: _uv_case(a, 37, 9 if a == "rf9" else 27, pw), id="uv-%s-%s" % (a, "cam8" if pw else "cam0"))
                for a in ("rf9", "default") for pw in (True, False)] +
               [pytest.param(lambda: _uv_case("default", 40, 5, True), id="uv-overlapping-own-cameras")] +
               # pixel input on a bf16x3 handle from 96 windows on: r3d_forward_uv_b3 (first_level_taps_b3 with the UV gather)
               [pytest.param(lambda: _uv_case("bf16x3-rf9", 97, 9, True), id="uv-bf16x3")] +
               # the pre-pass modes: one ray per input frame (one camera; stride >= RF), and materialised (B, RF, J, F) windows
               [pytest.param(lambda: _dist_case(40, 1, False), id="uv-dist-per-frame-clip-one-camera"),
                pytest.param(lambda: _dist_case(37, 27, True), id="uv-dist-per-frame-batch-own-cameras"),
                pytest.param(lambda: _dist_case(12, 5, True), id="uv-dist-materialised")] +
               [pytest.param(lambda k=k, args=args: _px_case(k, *args), id="px-%s-%s" % (k, lid))
                for k in ("intrinsic", "screen")
                for lid, args in (("per-frame-clip-one-camera", (40, 1, False)), ("per-frame-batch-own-cameras", (37, 9, True)),
                                  ("materialised", (12, 2, True)))])


@pytest.mark.parametrize("make", INPUT_CASES)
def test_clip_and_pixel_inputs_are_read_inside_their_extent(make):
    """Sliding clips that end with their last window, camera rows of exactly B (or one) rows, and the pixel pre-pass's
    tail of the workspace (exactly r3d_input_workspace_bytes), in both of its layouts."""
    lifter, states, call, windows, prm, plain = make()
    results = guarded(lifter, call, "pair+trj")
    with torch.no_grad():
        want = plain()
    lifter.check_status(DEV)
    _all_equal(results, want, None, "inputs")
    both, trj = _reference(states, windows, prm, call["B"])
    check_parity(want, both, "pos+trj vs the oracle chain")
    check_parity(results[0][1], trj, "trj vs the oracle chain")
    for _, t in results[1:]:
        assert torch.equal(t, results[0][1])


# ---------------------------------------------------------------- 3. captured forwards

@pytest.mark.parametrize("B", [12, 203])
def test_a_captured_forward_owns_nothing_between_replays(B):
    """A graph's workspace must exist and be left alone while the graph RUNS; between replays it may hold anything: the
    captured forward binds for itself (ready counters, abort flag, problem table live in the workspace).  At 12 windows an
    eager call would use the library's own polled activation banks; a captured one must not."""
    import ray3d_amd
    from ray3d_amd import _capi
    lifter, ((cp, _), _) = _fresh_pair("default")                 # (its own handles: prepared sizes are pinned per pair)
    dev = torch.device(DEV)
    hp, ht = lifter.pos.handle(dev), lifter.trj.handle(dev)
    call, other = _rays_call(cp, B, seed=900 + B), _rays_call(cp, B, seed=950 + B)
    x2, p2 = torch.from_numpy(other["x"]).to(dev), torch.from_numpy(other["param"]).to(dev)
    nbytes = _capi.workspace_bytes(hp, ht, B)
    out_shape = (B, 1, lifter.pos.num_joints_in, 3)
    out_bytes = int(np.prod(out_shape)) * 4
    arena = Arena(dev, NANS, Arena.capacity_for([call["x"].nbytes, call["param"].nbytes, out_bytes, nbytes]))
    wx, wp = arena.put(call["x"], name="x_dev"), arena.put(call["param"], name="param_dev")
    x, p = wx(), wp()
    out = arena.carve(out_bytes, name="out_dev").view(torch.float32).view(out_shape)
    ws = ExactWorkspace(arena, "workspace_dev")
    wsv = ws.get(nbytes, dev)
    with torch.no_grad():
        eager = lifter(x.clone(), p.clone())
        eager2 = lifter(x2, p2)
    lifter.prepare([B])
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    try:
        torch.cuda.synchronize()
        with torch.no_grad(), torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                lifter._run(_capi.R3D_INPUT_RAYS, x, cp.receptive_field, B, p, 2, out=out, workspace=ws)
        for pattern in PATTERNS + (ACT_SENTINEL, NANS):
            with torch.no_grad():
                assert torch.equal(lifter(x2, p2), eager2)          # an eager call on other buffers between the replays
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                fill_pattern(wsv, pattern)                           # the whole workspace, control region included
                out.fill_(OUT_SENTINEL)
                g.replay()
            torch.cuda.synchronize()
            arena.check()
            assert torch.equal(out, eager), ("pattern 0x%08X" % pattern, float((out - eager).abs().max()))
        lifter.check_status(dev)
    finally:
        del g                                                        # the graph before the size it pins and the handles
        torch.cuda.synchronize()
        lifter.release_prepared()


# ---------------------------------------------------------------- 4. alignment

@pytest.mark.parametrize("B", [37, 3])
def test_pointers_need_only_their_types_alignment(B):
    """Nothing that touches x_dev, param_dev, out_dev or out_trj_dev needs more than dword alignment: the first level's
    gathers read x_dev with 4-byte buffer loads (r3d_tiles.hpp: enc_tile, first_level_*; the per-frame launch of clip
    calls), the pre-pass reads its pixels one float at a time, r3d_decode_f32 / _w4 store out_dev and out_trj_dev one float
    at a time, and r3d_bind_f32 only copies the pointers.  The parameter rows are the A operand of embedder.w1: the GEMM
    tiles stage them with 16-byte buffer loads through a bounded descriptor based at the row (rows of 2 floats are 8 bytes
    apart as it is) - a buffer load needs dword alignment whatever its width, and the descriptor's bound clips it per
    dword.  So a float pointer needs 4-byte alignment and no more: every buffer 4 bytes off a 256-byte boundary gives the
    bits of the aligned call."""
    lifter, ((cp, _), _) = _pair("default")
    call = _rays_call(cp, B, seed=700 + B)
    aligned = guarded(lifter, call, "pair+trj", patterns=(NANS,))[0]
    skewed = guarded(lifter, call, "pair+trj", patterns=(NANS, ACT_SENTINEL), skew=4)
    for o, t in skewed:
        assert torch.equal(o, aligned[0]) and torch.equal(t, aligned[1])
    # what LiftModule / Ray3DLifter pass through as it is: x[1:] of a (B + 1)-window tensor is contiguous, and with RF 27 and
    # 17 joints (4131 floats per window) 4 bytes off a 16-byte boundary
    bigger = _rays_call(cp, B + 1, seed=700 + B)
    xb, pb = torch.from_numpy(bigger["x"]).to(DEV), torch.from_numpy(bigger["param"]).to(DEV)
    assert xb[1:].is_contiguous() and xb[1:].data_ptr() % 16 == 4
    with torch.no_grad():
        a = lifter(xb[1:], pb[1:])
        b = lifter(xb[1:].clone(), pb[1:].clone())
    assert torch.equal(a, b)


# ---------------------------------------------------------------- 6. the metric calls

def _metric_inputs(n, J):
    rng = np.random.default_rng(4000 + n + J)
    gt = rng.normal(0, 0.4, (n, J, 3)).astype(np.float32) + np.array([0, 0, 1.0], np.float32)
    pred = gt + rng.normal(0, 0.05, (n, J, 3)).astype(np.float32)
    trj = rng.normal(0, 0.5, (n, 3)).astype(np.float32) + np.array([0, 0, 4.0], np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return pred, gt, trj, q * np.sign(np.linalg.det(q)), rng.normal(size=3)


@pytest.mark.parametrize("J", [14, 17])
@pytest.mark.parametrize("n", [1, 2, 64, 65, 257, 33100])
def test_metric_calls_stay_inside_their_buffers(n, J):
    """r3d_clip_metrics, r3d_clip_metrics_detail and r3d_clip_valid_losses on inputs, output rows and per-frame tables of
    exactly their documented sizes, inside a NaN arena (the velocity terms read frame f + 1: not past the clip's end).
    Result slots are bit-identical to the ordinary call on plain tensors, which the metric suites pin to their oracles."""
    import valid_oracle as vo
    from ray3d_amd import _capi
    dev = torch.device(DEV)
    pred, gt, trj, R, T = _metric_inputs(n, J)
    stream = torch.cuda.current_stream(dev).cuda_stream
    parents = vo.tree_for(J)

    def run(alloc_in, alloc_out, check):
        """Every call variant with buffers from the two allocators -> the result slots, in a fixed order."""
        got = []
        p, g, t = alloc_in(pred, "pred_dev"), alloc_in(gt, "gt_dev"), alloc_in(trj, "trj_dev")
        out = alloc_out(_capi.METRIC_OUT_DOUBLES, "out_dev")
        _capi.clip_metrics(p.data_ptr(), g.data_ptr(), n, J, R, T, out.data_ptr(), stream)
        check()
        got.append(out[:5].clone())
        for frames in (True, False):
            out, det = alloc_out(_capi.METRIC_OUT_DOUBLES, "out_dev"), alloc_out(_capi.DETAIL_OUT_DOUBLES, "detail_dev")
            fr = alloc_out(n * 5, "frame_dev") if frames else None
            _capi.clip_metrics_detail(p.data_ptr(), g.data_ptr(), n, J, R, T, out.data_ptr(), fr.data_ptr() if frames else None,
                                      det.data_ptr(), stream)
            check()
            got += [out[:5].clone(), det[:_capi.DETAIL_DOUBLES].clone()] + ([fr.clone()] if frames else [])
        for with_trj, with_parents, frames in ((True, True, True), (False, True, False), (True, False, True), (False, False, False)):
            out = alloc_out(_capi.VALID_OUT_DOUBLES, "out_dev")
            fr = alloc_out(n * _capi.VALID_COUNT, "frame_dev") if frames else None
            _capi.clip_valid_losses(p.data_ptr(), t.data_ptr() if with_trj else None, g.data_ptr(), n, J, parents if with_parents else None, 0,
                                    out.data_ptr(), fr.data_ptr() if frames else None, stream)
            check()
            got += [out[:_capi.VALID_DOUBLES].clone()] + ([fr.clone()] if frames else [])
        return got

    def plain_out(count, name):
        return torch.full((count,), -7.0, dtype=torch.float64, device=dev)

    want = run(lambda a, name: torch.from_numpy(a).to(dev), plain_out, torch.cuda.synchronize)
    M, D, V = _capi.METRIC_OUT_DOUBLES, _capi.DETAIL_OUT_DOUBLES, _capi.VALID_OUT_DOUBLES
    arena = Arena(dev, NANS, Arena.capacity_for([pred.nbytes, gt.nbytes, trj.nbytes] +
                                                [8 * c for c in (M, M, D, n * 5, M, D, V, n * _capi.VALID_COUNT, V, V, n * _capi.VALID_COUNT, V)]))

    def guarded_out(count, name):
        o = arena.carve(count * 8, name=name).view(torch.float64)
        o.fill_(-7.0)
        return o

    got = run(lambda a, name: arena.put(a, name=name)(), guarded_out, arena.check)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (k, a, b)
