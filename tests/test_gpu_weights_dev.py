"""GPU suite: r3d_finalize_dev - a handle packed on the device from device-resident tensors - against r3d_finalize from host arrays:
the packed images byte for byte, the forwards bit for bit, one row per configuration against the reference fixture; refresh in
place through the module switches, under a pinned schedule and with lanes; guard bands round the source tensors.  Small batches
only (3 and 33 windows).  The host half is tests/test_weights_dev_host.py."""
import numpy as np
import pytest
import torch

from conftest import MODEL_CASES, check_parity, hooks_library, load_model_fixture

import buffers_util
import weights_dev_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = (3, 33)


def _load(model, state):
    import ray3d_amd
    ray3d_amd.load_weight(model, {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})


def _pair(mc, sp, st, device_weights, fuse_pair=False):
    """(factory, pos, trj) of the hooks library with the given states loaded, in eval mode."""
    import ray3d_amd
    fac = ray3d_amd.Model(mc, {}, is_train=False, fuse_pair=fuse_pair, device_weights=device_weights)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    _load(pos, sp[1])
    _load(trj, st[1])
    pos.eval(), trj.eval()
    return fac, pos, trj


def _inputs(cfg, B, seed=5):
    from ray3d_amd import synth
    return torch.from_numpy(synth.synth_rays(B, cfg, seed=seed)).to(DEV), torch.from_numpy(synth.synth_param(B, seed=seed + 1)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape and np.array_equal(a, b), "%s: %d of %d floats differ" % (what, int((a != b).sum()), a.size)


def _image(module):
    from ray3d_amd.modules import _unwrap
    return _unwrap(module).handle(torch.device(DEV)).debug_weights_image().view(np.int32)


def _edit_in_place(module):
    """Scale a few parameters and one running_var where they live."""
    from ray3d_amd.modules import _unwrap
    m = _unwrap(module)
    sd = dict(m.named_parameters())
    sd.update(dict(m.named_buffers()))
    with torch.no_grad():
        for key, factor in (("GlobalInfo.fc_1.weight", 1.25), ("GlobalInfo.bn_1.bias", -0.5), ("GlobalInfo.bn_1.running_var", 3.0)):
            sd[key].mul_(factor)
        first = [k for k in sd if k.endswith("expand_conv.weight")][0]
        sd[first].mul_(0.75)
    m.refresh_weights()


@pytest.mark.parametrize("weights", wc.WEIGHTS)
@pytest.mark.parametrize("case", wc.CASES + wc.GPU_EXTRA, ids=wc.case_id)
def test_device_pack_equals_host_pack(case, weights):
    import ray3d_amd
    hooks_library()
    mc, sp, st = wc.states_of(case, weights)
    _, hpos, htrj = _pair(mc, sp, st, device_weights=False)
    _, dpos, dtrj = _pair(mc, sp, st, device_weights=True)
    host, dev = ray3d_amd.Ray3DLifter(hpos, htrj).eval(), ray3d_amd.Ray3DLifter(dpos, dtrj).eval()
    with torch.no_grad():
        for B in BATCHES:
            x, p = _inputs(sp[0], B)
            (hp, ht), (dp, dt) = host.forward_split(x, p), dev.forward_split(x, p)
            _same_bits(dp, hp, "pos, %d windows" % B)
            _same_bits(dt, ht, "trj, %d windows" % B)
            _same_bits(dpos(x, p), hpos(x, p), "pos alone, %d windows" % B)
    for name, h, d in (("pos", hpos, dpos), ("trj", htrj, dtrj)):
        hi, di = _image(h), _image(d)
        assert hi.shape == di.shape and hi.size > 0
        assert np.array_equal(hi, di), "%s image: %d of %d floats differ, first at %d" % (name, int((hi != di).sum()), hi.size, int(np.argmax(hi != di)))
    if weights == "synth":       # the row of the parity table: the device-packed pair against the reference (fixture, or the CPU oracle)
        with torch.no_grad():
            if case[0] in MODEL_CASES:
                z, _ = load_model_fixture(case[0])
                x, p = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["param"]).to(DEV)
                if case[1]:      # (the bf16x3 tiles run from 96 windows per call on: the fixture's windows tiled, as test_gpu_parity does)
                    reps = -(-128 // x.shape[0])
                    n = x.shape[0]
                    out = dev(x.repeat(reps, 1, 1, 1)[:128].contiguous(), p.repeat(reps, 1)[:128].contiguous())[:n]
                else:
                    out = dev(x, p)
                ref = z["out_pos"] + z["out_trj"]
            else:
                from oracle import oracle
                x, p = _inputs(sp[0], 3)
                out = dev(x, p)
                ref = oracle.forward(sp[0], sp[1], x.cpu().numpy(), p.cpu().numpy()) + oracle.forward(st[0], st[1], x.cpu().numpy(), p.cpu().numpy())
        check_parity(out, ref, "device-packed pos+trj vs reference")       # (the literal 1e-4, bf16x3 included: outputs of O(1 m))


@pytest.mark.parametrize("fuse_pair", [False, True], ids=["modules", "pair-seam"])
def test_refresh_in_place_through_the_module_switches(fuse_pair):
    hooks_library()
    mc, sp, st = wc.states_of(("j14_rf9_s3", False), "trained")
    fac, pos, trj = _pair(mc, sp, st, device_weights=True, fuse_pair=fuse_pair)
    x, p = _inputs(sp[0], 33)
    with torch.no_grad():
        before = (pos(x, p).clone(), trj(x, p).clone())
        parked = pos(x, p)                  # (pair seam: parks a trajectory computed with the OLD weights)
        _edit_in_place(pos)
        _edit_in_place(trj)
        after_trj = trj(x, p).clone()       # must not be the parked one
        after_pos = pos(x, p).clone()
        after_trj2 = trj(x, p).clone()
    _same_bits(parked, before[0], "pos before the edit, repeated")
    # a module that loads the modified state_dict through the host path
    from ray3d_amd.modules import _unwrap
    mod_p = {k: v.detach().cpu().numpy() for k, v in _unwrap(pos).state_dict().items()}
    mod_t = {k: v.detach().cpu().numpy() for k, v in _unwrap(trj).state_dict().items()}
    _, hpos, htrj = _pair(mc, (sp[0], mod_p), (st[0], mod_t), device_weights=False)
    with torch.no_grad():
        want = (hpos(x, p), htrj(x, p))
    _same_bits(after_pos, want[0], "pos after refresh_weights()")
    _same_bits(after_trj, want[1], "trj after refresh_weights()")
    _same_bits(after_trj2, want[1], "trj after refresh_weights(), behind pos")
    assert not np.array_equal(_bits(after_pos), _bits(before[0])) and not np.array_equal(_bits(after_trj), _bits(before[1]))
    assert np.array_equal(_image(pos), _image(hpos)) and np.array_equal(_image(trj), _image(htrj))


@pytest.mark.parametrize("lanes", [0, 2], ids=["pinned-schedule", "two-lanes"])
def test_refresh_under_a_pinned_schedule_and_with_lanes(lanes):
    import ray3d_amd
    hooks_library()
    mc, sp, st = wc.states_of(("j17_rf9_s1", False), "synth")
    _, pos, trj = _pair(mc, sp, st, device_weights=True)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    x, p = _inputs(sp[0], 33)
    if lanes:
        lifter.set_lanes(lanes, DEV)
    lifter.prepare([33], DEV)
    with torch.no_grad():
        before = lifter(x, p)
        lifter.join_lanes()
        before = before.clone()
        _edit_in_place(pos)
        _edit_in_place(trj)
        after = lifter(x, p)                 # (two lanes: relayed to a lane behind the pack, which joined the lanes first)
        lifter.join_lanes()
        after = after.clone()
    from ray3d_amd.modules import _unwrap
    mod_p = {k: v.detach().cpu().numpy() for k, v in _unwrap(pos).state_dict().items()}
    mod_t = {k: v.detach().cpu().numpy() for k, v in _unwrap(trj).state_dict().items()}
    _, hpos, htrj = _pair(mc, (sp[0], mod_p), (st[0], mod_t), device_weights=False)
    hl = ray3d_amd.Ray3DLifter(hpos, htrj).eval()
    if lanes:
        hl.set_lanes(lanes, DEV)
    hl.prepare([33], DEV)
    with torch.no_grad():
        want = hl(x, p)
        hl.join_lanes()
    _same_bits(after, want, "forward after a device refresh")
    assert not np.array_equal(_bits(after), _bits(before))
    torch.cuda.synchronize()
    lifter.release_prepared()
    hl.release_prepared()
    if lanes:
        lifter.set_lanes(0, DEV)
        hl.set_lanes(0, DEV)


def test_sources_are_only_read_and_nothing_round_them_is_written():
    """Every source tensor carved exact-sized out of one NaN-patterned allocation (tests/buffers_util.py): after the call the
    tensors hold their bytes, the guards their pattern, and the image is the host path's."""
    from ray3d_amd import _capi
    hooks_library()
    mc, sp, st = wc.states_of(("j17_rf9_s1", False), "trained")
    cfg, state = st
    hd, hh = _capi.Handle(cfg), _capi.Handle(cfg)
    keys = hd.keys()
    arrays = [np.ascontiguousarray(state[k], dtype=np.float32) for k in keys]
    arena = buffers_util.Arena(DEV, buffers_util.NANS, buffers_util.Arena.capacity_for([a.nbytes for a in arrays]))
    tensors = [arena.put(a, skew=4 * (i % 3), name=k)() for i, (k, a) in enumerate(zip(keys, arrays))]
    with torch.cuda.device(DEV):
        hd.finalize_dev(tensors, torch.cuda.current_stream(DEV).cuda_stream)
        hd.finalize_dev(tensors, torch.cuda.current_stream(DEV).cuda_stream)       # in place, on the finalized handle
        arena.check()
        for k, t, a in zip(keys, tensors, arrays):
            assert np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32)), k
        wc.set_host_weights(hh, state)
        hh.finalize()
        assert np.array_equal(hd.debug_weights_image().view(np.int32), hh.debug_weights_image().view(np.int32))
        # r3d_set_weight + r3d_finalize keep working afterwards: the last finalize wins
        wc.set_host_weights(hd, {k: a * np.float32(2.0) for k, a in zip(keys, arrays)})
        hd.finalize()
        assert not np.array_equal(hd.debug_weights_image().view(np.int32), hh.debug_weights_image().view(np.int32))
        hd.finalize_dev(tensors, torch.cuda.current_stream(DEV).cuda_stream)
        assert np.array_equal(hd.debug_weights_image().view(np.int32), hh.debug_weights_image().view(np.int32))
    hd.close(), hh.close()


def test_a_parameter_left_on_the_cpu_raises_and_names_the_key():
    from ray3d_amd.modules import _unwrap
    hooks_library()
    mc, sp, st = wc.states_of(("j17_rf9_s1", False), "synth")
    _, pos, trj = _pair(mc, sp, st, device_weights=True)
    m = _unwrap(trj)
    m.GlobalInfo.fc_1.weight.data = m.GlobalInfo.fc_1.weight.data.cpu()
    m.refresh_weights()
    x, p = _inputs(st[0], 3)
    with pytest.raises(RuntimeError, match=r"'GlobalInfo\.fc_1\.weight' is on cpu"):
        trj(x, p)
