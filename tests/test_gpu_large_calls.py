"""Forwards whose buffers cross 2^31 and 2^32 bytes (tests/large_call_cases.py reads the crossings from the library): every window
against the same library in calls of 4096 windows, a sample around every crossing against the oracle, everything finite.

The forward kernels mix 64-bit bases with 32-bit offsets, bounds and row indices; a wrapped one is invisible below 2 GiB per buffer,
which is where the rest of the suite runs.  Inputs are generated on the device from a hash of the element index (any window can be
re-created on the host); nothing of this size is uploaded or stored.  One case is alive at a time: a case frees its lifter, its
workspace and the allocator's cache when it ends.

Sizes, with the default channels (r3d_debug_plan_buffers; DESIGN.md section 2 has the table and the figures of a run): the RF-9 pair
needs 132 872 bytes of workspace per window and its widest buffer (mix5, 1280 floats per window) reaches 2^31 bytes at 419 431
windows (55.7 GB of workspace) and 2^32 bytes at 838 861 (111.5 GB, under half an MI355X's 288 GB).  2^31 FLOATS in one buffer
need 1 677 722 windows: as materialised windows the raw-input rule refuses that (1 169 653 at most), as a clip call it needs 223 GB
- more than half the card - so no case runs it.  A case takes 1 - 6 s, most of it the allocation and the 100 - 200 calls of 4096.
The clip cases use RF 27, the smallest receptive field at which a clip call takes the per-frame first layers at all (RF 9 has
too few rows per window for them to pay: call_shares_first_layers)."""
import os
import time

import numpy as np
import pytest
import torch

import large_call_cases as lc
from conftest import check_parity, record_parity

pytestmark = pytest.mark.gpu

HIP_BOUND = 6e-5          # another batch size, another summation order: the bound of test_large_batch_1024 / test_universal_14_joint_batch_4096
RUN_LOG = []              # (case, windows, workspace bytes, seconds, max HIP-against-HIP difference) - printed at the end of a case


def _tables(mc, batch, clip=False):
    """The hook's view of a call of `batch` windows: (crossed limits, workspace bytes, per-frame answer, RF, J)."""
    from ray3d_amd import _capi
    with lc.HostPair(mc) as pr:
        out = (lc.crossed(pr, batch, clip), pr.workspace_bytes(batch), pr.call_check(batch, 1 if clip else pr.rf)[2], pr.rf, pr.joints)
    _capi.use_hooks(False)
    return out


def _first_crossing(mc, limit_name, clip=False, per_frame_only=False):
    from ray3d_amd import _capi
    with lc.HostPair(mc) as pr:
        out = lc.first_crossing(pr, limit_name, clip, per_frame_only)
    _capi.use_hooks(False)
    return out


def _need_memory(nbytes, what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # an earlier case left the device in an error state: nothing more is started on it
        pytest.exit("the device reported an error before %s: %s" % (what, e), returncode=3)
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("%s needs %d bytes of device memory, torch.cuda.mem_get_info reports %d free (of %d)" % (what, nbytes, free, total))


def _release():
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _lifter(mc):
    import ray3d_amd
    from test_gpu_parity import build_modules
    pos, trj, sp, st = build_modules(mc)
    return ray3d_amd.Ray3DLifter(pos, trj).eval(), (sp, st)


def _oracle(states, windows, prm):
    """The torch port on the sampled windows.  check_parity holds the result to the literal 1e-4 abs whatever its magnitude: at the
    default decoder scale the RF-9 and RF-27 pairs put out up to ~13 m and ~14.5 m on these inputs (12.2 m on synth_rays), the
    RF-243 pair at LITERAL_SCALE stays below 10 m."""
    from test_gpu_parity import _oracle_lift
    return _oracle_lift(states, windows, prm)


def _finish(case, lifter, big, worst, batch, ws_bytes, t0):
    assert torch.isfinite(big).all()
    lifter.check_status("cuda:0")
    err = float(worst)
    record_parity("test_gpu_large_calls %s: %d windows against calls of %d" % (case, batch, lc.CHUNK), err, HIP_BOUND)
    RUN_LOG.append((case, batch, ws_bytes, time.time() - t0, err))
    print("\nlarge call %-28s %8d windows  workspace %13d bytes  %.1f s  max |big - chunks| %.2e" % RUN_LOG[-1])
    assert err <= HIP_BOUND, (case, err)


def _assert_crossings(crossings, want_limit, what):
    assert any(l == want_limit for _, _, l, _, _, _ in crossings), "%s: no buffer reaches %s at this batch: %s" % (what, want_limit, crossings)


# ---------------------------------------------------------------- a, b, d: materialised windows, RF 9

def _windows_case(case, mc, limit_name, staged=False, margin=37):
    from ray3d_amd import _capi
    batch = _first_crossing(mc, limit_name)[0] + margin
    crossings, ws_bytes, _, rf, J = _tables(mc, batch)
    _assert_crossings(crossings, limit_name, case)
    width = rf * J * 3
    _need_memory(ws_bytes + batch * (width + 2 + J * 3 + 3) * 4 + (1 << 30), "%s (%d windows)" % (case, batch))
    t0 = time.time()
    lifter, states = _lifter(mc)
    try:
        lifter.set_staged(staged or os.environ.get("R3D_STAGED") == "1")
        x = torch.empty((batch, width), dtype=torch.float32, device="cuda")
        p = torch.empty((batch, 2), dtype=torch.float32, device="cuda")
        lc.fill_hashed(x, "rays")
        lc.fill_hashed(p, "param")
        x = x.view(batch, rf, J, 3)
        with torch.no_grad():
            big = lifter(x, p)
            worst = torch.zeros((), device="cuda")
            for i in range(0, batch, lc.CHUNK):
                part = lifter(x[i:i + lc.CHUNK], p[i:i + lc.CHUNK])
                worst = torch.maximum(worst, (big[i:i + lc.CHUNK] - part).abs().max())
        idx = lc.sample_windows(batch, crossings)
        xs = np.stack([lc.hashed_rows_host(w, 1, width, "rays")[0] for w in idx]).reshape(len(idx), rf, J, 3)
        ps = np.stack([lc.hashed_rows_host(w, 1, 2, "param")[0] for w in idx])
        sel = torch.tensor(idx, device="cuda")
        assert np.array_equal(x[sel].cpu().numpy(), xs) and np.array_equal(p[sel].cpu().numpy(), ps)      # the host re-creates the device's input
        check_parity(big[sel].cpu().numpy(), _oracle(states, xs, ps), "%s: %d windows around the crossings vs torch port" % (case, len(idx)))
        _finish(case, lifter, big, worst, batch, ws_bytes, t0)
        return lifter.precision("cuda:0")
    finally:
        del lifter
        x = p = big = part = None
        _release()


@pytest.mark.parametrize("limit_name", ["2^31 bytes", "2^32 bytes"])
def test_pair_forward_single_launch_across(limit_name):
    """a. r3d_forward_pair, RF 9, one persistent launch, just above the first buffer to reach 2^31 / 2^32 bytes."""
    _windows_case("a single launch, " + limit_name, lc.model_config("3,3"), limit_name)


@pytest.mark.parametrize("limit_name", ["2^31 bytes", "2^32 bytes"])
def test_pair_forward_level_by_level_across(limit_name):
    """b. the same batches level by level (R3D_OPT_STAGED): the r3d_gemm* kernels on the same buffers."""
    _windows_case("b level by level, " + limit_name, lc.model_config("3,3"), limit_name, staged=True)


def test_bf16x3_pair_forward_across_2_31_bytes():
    """d. bf16x3 (its own first-level and tile families) just above the first buffer to reach 2^31 bytes."""
    if os.environ.get("R3D_BF16X3") is None:
        mc = dict(lc.model_config("3,3"), BF16X3=True)
    else:
        mc = lc.model_config("3,3")
    precision = _windows_case("d bf16x3, 2^31 bytes", mc, "2^31 bytes")
    assert precision == "bf16x3" or os.environ.get("R3D_BF16X3") == "0", precision


# ---------------------------------------------------------------- c: pixel input, a camera row per window

def test_pixel_input_with_a_camera_row_per_window_across_2_31_bytes():
    """c. forward_uv on (B, RF, J, 2) pixels with one of the 14 3DHP cameras per window: the gather that encodes in flight, the
    camera row found from the 64-bit window index and cam_stride."""
    from test_gpu_parity import _dhp_cameras
    case, mc = "c pixels, camera per window", lc.model_config("3,3")
    batch = _first_crossing(mc, "2^31 bytes")[0] + 41
    crossings, ws_bytes, _, rf, J = _tables(mc, batch)
    _assert_crossings(crossings, "2^31 bytes", case)
    width = rf * J * 2
    _need_memory(ws_bytes + batch * (width + 2 + 16 + J * 3) * 4 + (1 << 30), "%s (%d windows)" % (case, batch))
    t0 = time.time()
    cams, ocams, _, _ = _dhp_cameras()
    lifter, states = _lifter(mc)
    try:
        lifter.set_staged(os.environ.get("R3D_STAGED") == "1")
        uv = torch.empty((batch, width), dtype=torch.float32, device="cuda")
        lc.fill_hashed(uv, "pixels")
        uv = uv.view(batch, rf, J, 2)
        rows14 = torch.from_numpy(np.stack([c.cam_row() for c in cams])).cuda()
        prm14 = torch.from_numpy(np.stack([c.param() for c in cams]).astype(np.float32)).cuda()
        which = torch.arange(batch, device="cuda") % 14
        rows, p = rows14[which].contiguous(), prm14[which].contiguous()
        with torch.no_grad():
            big = lifter.forward_uv(uv, rows, p)
            worst = torch.zeros((), device="cuda")
            for i in range(0, batch, lc.CHUNK):
                part = lifter.forward_uv(uv[i:i + lc.CHUNK], rows[i:i + lc.CHUNK], p[i:i + lc.CHUNK])
                worst = torch.maximum(worst, (big[i:i + lc.CHUNK] - part).abs().max())
        idx = lc.sample_windows(batch, crossings)
        uvs = np.stack([lc.hashed_rows_host(w, 1, width, "pixels")[0] for w in idx]).reshape(len(idx), rf, J, 2)
        assert np.array_equal(uv[torch.tensor(idx, device="cuda")].cpu().numpy(), uvs)
        xs = np.stack([ocams[w % 14].rays_from_uv(uvs[k].astype(np.float64)).astype(np.float32) for k, w in enumerate(idx)])
        ps = np.stack([cams[w % 14].param() for w in idx]).astype(np.float32)
        check_parity(big[torch.tensor(idx, device="cuda")].cpu().numpy(), _oracle(states, xs, ps),
                     "%s: %d windows around the crossings vs oracle camera + torch port" % (case, len(idx)))
        _finish(case, lifter, big, worst, batch, ws_bytes, t0)
    finally:
        del lifter
        uv = rows = p = big = part = None
        _release()


# ---------------------------------------------------------------- e: clip calls through the C ABI, RF 27

@pytest.mark.parametrize("which", ["per-frame buffer past 2^31 bytes", "just above the fallback"])
def test_clip_call_through_the_c_abi(which):
    """e. One r3d_forward_pair with window_stride 1 over a long clip (lifter._run, not the chunking forward_clip): with the
    per-frame buffer between 2^31 and 2^32 bytes the call runs the per-frame first layers (r3d_gemm_f32 once, then
    r3d_forward_clip_f32); at the first frame count whose buffer reaches 2^32 - 1 bytes it runs the gathered first levels."""
    from ray3d_amd import _capi
    case, mc = "e clip, " + which, lc.model_config("3,3,3")
    with lc.HostPair(mc) as pr:
        rf, J = pr.rf, pr.joints
        ld = [r[1] for r in pr.buffers(1 << 20)[0] if r[4]][0]
        if which.startswith("per-frame"):
            batch = lc.first_crossing(pr, "2^31 bytes", clip=True, per_frame_only=True)[0] + 29
        else:
            batch = lc.first_gathered_frames(ld) - (rf - 1) + 3
        crossings, ws_bytes, per_frame = lc.crossed(pr, batch, clip=True), pr.workspace_bytes(batch), pr.call_check(batch, 1)[2]
    _capi.use_hooks(False)
    frames = batch + rf - 1
    pf = [c for c in crossings if c[5]]
    if which.startswith("per-frame"):
        assert any(l == "2^31 bytes" for _, _, l, _, _, _ in pf) and not any(l == "2^32 bytes" for _, _, l, _, _, _ in pf), pf
        assert 2 ** 31 <= frames * ld * 4 < 2 ** 32
    else:
        assert frames * ld * 4 >= lc.PER_FRAME_GUARD and (frames - 4) * ld * 4 < lc.PER_FRAME_GUARD
    _need_memory(ws_bytes + frames * J * 3 * 4 + batch * (J * 3 + 3) * 4 + (1 << 30), "%s (%d windows)" % (case, batch))
    t0 = time.time()
    lifter, states = _lifter(mc)
    try:
        staged_env = os.environ.get("R3D_STAGED") == "1"
        lifter.set_staged(staged_env)
        f32 = lifter.precision("cuda:0") == "f32"              # (bf16x3 handles keep the gathered first level)
        assert per_frame == which.startswith("per-frame") or not f32
        clip = torch.empty((frames, J * 3), dtype=torch.float32, device="cuda")
        lc.fill_hashed(clip, "rays")
        clip = clip.view(frames, J, 3)
        prow = torch.tensor([1.4, 0.15], dtype=torch.float32, device="cuda")
        run = lambda c, b, out=None: lifter._run(_capi.R3D_INPUT_RAYS, c, 1, b, prow, 0, out=out)
        with torch.no_grad():
            big = run(clip, batch)
            recs = [r["kernel"] for r in lifter.profile_call(lambda: run(clip, batch, big), "cuda:0")]
            if not staged_env:
                if which.startswith("per-frame") and f32:
                    assert "r3d_forward_clip_f32" in recs and "r3d_forward_f32" not in recs and recs.count("r3d_gemm_f32") == 1, recs
                else:
                    assert not any("clip" in k for k in recs) and "r3d_gemm_f32" not in recs, recs
            worst = torch.zeros((), device="cuda")
            for i in range(0, batch, lc.CHUNK):
                b = min(lc.CHUNK, batch - i)
                worst = torch.maximum(worst, (big[i:i + b] - run(clip[i:], b)).abs().max())
        idx = lc.sample_windows(batch, crossings)
        xs =np.stack([lc.hashed_rows_host(w, rf, J * 3, "rays") for w in idx]).reshape(len(idx), rf, J, 3)
        sel = torch.tensor(idx, device="cuda")
        assert np.array_equal(torch.stack([clip[w:w + rf] for w in idx]).cpu().numpy(), xs)
        ps = np.tile(np.array([1.4, 0.15], np.float32), (len(idx), 1))
        check_parity(big[sel].cpu().numpy(), _oracle(states, xs, ps), "%s: %d windows around the crossings vs torch port" % (case, len(idx)))
        _finish(case, lifter, big, worst, batch, ws_bytes, t0)
    finally:
        del lifter
        clip = big = None
        _release()


# ---------------------------------------------------------------- f: a raw input just under the 2 GiB guard, RF 243

def test_raw_input_just_under_the_2_gib_guard_rf243():
    """f. The largest batch of materialised RF-243 windows the raw-input rule accepts (computed from the documented rule, and the
    library must accept it): the only case where the first-level gather's unsigned byte offsets exceed 2^31."""
    from ray3d_amd import _capi
    from test_gpu_parity import LITERAL_SCALE, build_modules
    import ray3d_amd
    case, mc = "f raw input under 2 GiB, RF 243", lc.model_config("3,3,3,3,3")
    with lc.HostPair(mc) as pr:
        rf, J = pr.rf, pr.joints
        batch = lc.last_accepted_batch(rf, rf, J)
        assert pr.call_check(batch, rf)[0] == 0
        crossings, ws_bytes = lc.crossed(pr, batch), pr.workspace_bytes(batch)
    _capi.use_hooks(False)
    width = rf * J * 3
    assert 2 ** 31 - width * 4 <= batch * width * 4 < 2 ** 31 - 1
    _need_memory(ws_bytes + batch * (width + 2 + J * 3 + 3) * 4 + (1 << 30), "%s (%d windows)" % (case, batch))
    t0 = time.time()
    pos, trj, sp, st = build_modules(mc, LITERAL_SCALE)          # (the decoder scale at which RF-243 outputs stay below 10 m)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    try:
        lifter.set_staged(os.environ.get("R3D_STAGED") == "1")
        x = torch.empty((batch, width), dtype=torch.float32, device="cuda")
        p = torch.empty((batch, 2), dtype=torch.float32, device="cuda")
        lc.fill_hashed(x, "rays", rows_per_step=1 << 12)
        lc.fill_hashed(p, "param")
        x = x.view(batch, rf, J, 3)
        with torch.no_grad():
            big = lifter(x, p)
            worst = torch.zeros((), device="cuda")
            for i in range(0, batch, lc.CHUNK):
                part = lifter(x[i:i + lc.CHUNK], p[i:i + lc.CHUNK])
                worst = torch.maximum(worst, (big[i:i + lc.CHUNK] - part).abs().max())
        # the window whose first byte is the last one below 2^31, its neighbours, the last windows of the input, a spread
        w31 = 2 ** 31 // (width * 4)
        idx = sorted({0, batch - 1, batch - 2, w31 - 1, w31, w31 + 1, w31 - 32, w31 + 32} | {int(v) for v in np.linspace(0, batch - 1, 16).round()})
        idx = [w for w in idx if 0 <= w < batch]
        xs = np.stack([lc.hashed_rows_host(w, 1, width, "rays")[0] for w in idx]).reshape(len(idx), rf, J, 3)
        ps = np.stack([lc.hashed_rows_host(w, 1, 2, "param")[0] for w in idx])
        sel = torch.tensor(idx, device="cuda")
        assert np.array_equal(x[sel].cpu().numpy(), xs)
        check_parity(big[sel].cpu().numpy(), _oracle((sp, st), xs, ps), "%s: %d windows vs torch port" % (case, len(idx)))
        _finish(case, lifter, big, worst, batch, ws_bytes, t0)
    finally:
        del lifter
        x = p = big = part = None
        _release()
