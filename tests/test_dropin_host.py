"""The drop-in seam without a GPU: r3d_forward_pair_split's declaration and argument rules, and the rules of the park that puts
one pair launch behind the reference's pos(x, p) / trj(x, p) calls - with the device forward replaced by a counting stub."""
import ctypes as C
import os
import re

import pytest
import torch

import ray3d_amd
from ray3d_amd import _capi, modules
from ray3d_amd.spec import config_from_dicts, default_model_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the C ABI

def test_header_declares_the_split_call_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
    assert re.search(r"^int\s+r3d_forward_pair_split\s*\(", text, re.M)
    assert "trainer.py:337-353" in text
    assert "r3d_forward_pair_split" in _capi.EXPORTS
    assert re.search(r"#define\s+R3D_ABI_VERSION\s+6\b", text)
    assert _capi.ABI_VERSION == 6
    lib = _capi.load()
    assert lib.r3d_abi_version() == 6
    assert hasattr(lib, "r3d_forward_pair_split")


BOGUS = 0x1000     # a non-null pointer into a page nobody maps: following it would end the test with a segmentation fault


@pytest.mark.parametrize("pos,trj,out_pos,out_trj", [
    (None, BOGUS, BOGUS, BOGUS), (BOGUS, None, BOGUS, BOGUS), (None, None, BOGUS, BOGUS),
    (BOGUS, BOGUS, None, BOGUS), (BOGUS, BOGUS, BOGUS, None), (BOGUS, BOGUS, None, None),
], ids=["no-pos", "no-trj", "no-models", "no-out-pos", "no-out-trj", "no-outputs"])
def test_split_call_refuses_null_models_and_null_outputs_before_it_follows_a_pointer(pos, trj, out_pos, out_trj):
    lib = _capi.load()
    inp = _capi.make_input(_capi.R3D_INPUT_RAYS, BOGUS, 27, BOGUS, 2)
    rc = lib.r3d_forward_pair_split(pos, trj, C.byref(inp), 4, out_pos, out_trj, BOGUS, 1 << 20, None)
    assert rc == _capi.R3D_ERR_ARG
    assert b"r3d_forward_pair_split" in lib.r3d_last_error()


# ---------------------------------------------------------------- the park

class Rig:
    """The two wrappers Model(...) returns, around bare CPU modules, sharing one seam whose device forward, trj-alone forward and
    upload are counting stubs: `split` / `alone` / `uploads` count calls, every stub output is a new tensor tagged with the
    number of the call that made it."""

    def __init__(self, on=True):
        mc = default_model_config(ARCHITECTURE="3,3")
        self.pos = ray3d_amd.RIEModel(config_from_dicts(mc, "pos")).eval()
        self.trj = ray3d_amd.RIETrajectoryModel(config_from_dicts(mc, "trj")).eval()
        self.seam = modules._PairSeam(self.pos, self.trj, on)
        self.wpos = modules._SingleDeviceParallel(self.pos, self.seam)
        self.wtrj = modules._SingleDeviceParallel(self.trj, self.seam)
        self.split = self.alone = self.pos_alone = self.uploads = 0
        self.seen = []
        self.seam._split = self._split
        self.seam._upload = self._upload
        self.trj.forward = self._trj_alone
        self.pos.forward = self._pos_alone

    def _split(self, x, p):
        self.split += 1
        self.seen.append((x, p))
        return torch.full((x.shape[0], 1, 17, 3), float(self.split)), torch.full((x.shape[0], 1, 1, 3), 100.0 + self.split)

    def _trj_alone(self, x, p):
        self.alone += 1
        return torch.full((x.shape[0], 1, 1, 3), -1.0)

    def _pos_alone(self, x, p):
        self.pos_alone += 1
        return torch.full((x.shape[0], 1, 17, 3), -2.0)

    def _upload(self, t, dev):
        self.uploads += 1
        return t.clone()          # (a new object, as a copy to a device is)

    def inputs(self, B=2):
        return torch.zeros(B, 9, 17, 3), torch.zeros(B, 2)


def test_a_trj_call_on_the_pos_calls_inputs_is_a_hit():
    r = Rig()
    x, p = r.inputs()
    assert float(r.wpos(x, p)[0, 0, 0, 0]) == 1.0
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == 101.0
    assert (r.split, r.alone, r.pos_alone) == (1, 0, 0)
    # the entry is dropped by the hit: the same call again runs the trj network alone
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == -1.0
    assert (r.split, r.alone) == (1, 1)


def test_off_by_default_every_call_runs_its_own_network():
    r = Rig(on=False)
    x, p = r.inputs()
    r.wpos(x, p), r.wtrj(x, p)
    assert (r.split, r.pos_alone, r.alone) == (0, 1, 1)
    assert ray3d_amd.fuse_pair_default() is False
    fac = ray3d_amd.Model(default_model_config(ARCHITECTURE="3,3"), {}, is_train=False)
    assert fac._seam.on is False
    try:
        assert ray3d_amd.fuse_pair_default(True) is True
        assert ray3d_amd.Model(default_model_config(ARCHITECTURE="3,3"), {}, is_train=False)._seam.on is True
        assert ray3d_amd.Model(default_model_config(ARCHITECTURE="3,3"), {}, is_train=False, fuse_pair=False)._seam.on is False
    finally:
        ray3d_amd.fuse_pair_default(False)
    assert ray3d_amd.Model(default_model_config(ARCHITECTURE="3,3"), {}, is_train=False, fuse_pair=True)._seam.on is True
    assert ray3d_amd.Model(default_model_config(ARCHITECTURE="3,3", TRAJECTORY_MODEL=False), {}, is_train=False, fuse_pair=True)._seam is None


def test_the_park_holds_two_pos_calls_in_the_references_order():
    r = Rig()
    x, p = r.inputs()
    xf = x.clone()
    r.wpos(x, p), r.wpos(xf, p)                          # pos, pos_flip
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == 101.0      # trj
    assert float(r.wtrj(xf, p)[0, 0, 0, 0]) == 102.0     # trj_flip
    assert (r.split, r.alone) == (2, 0)
    # ... and only two: a third pos call pushes the oldest entry out
    x3 = x.clone()
    r.wpos(x, p), r.wpos(xf, p), r.wpos(x3, p)
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == -1.0
    assert float(r.wtrj(x3, p)[0, 0, 0, 0]) == 105.0
    assert float(r.wtrj(xf, p)[0, 0, 0, 0]) == 104.0
    assert (r.split, r.alone) == (5, 1)


def test_an_in_place_edit_between_the_calls_is_a_miss():
    r = Rig()
    x, p = r.inputs()
    r.wpos(x, p)
    x.mul_(1)
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == -1.0
    r.wpos(x, p)
    p.add_(0)
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == -1.0
    assert (r.split, r.alone) == (2, 2)


def test_new_weights_between_the_calls_are_a_miss():
    r = Rig()
    x, p = r.inputs()
    for change in (lambda: r.wtrj.load_state_dict(r.wtrj.state_dict()), lambda: r.pos.load_state_dict(r.pos.state_dict()),
                   lambda: r.trj.refresh_weights(), lambda: r.pos._invalidate()):
        r.wpos(x, p)
        change()
        assert float(r.wtrj(x, p)[0, 0, 0, 0]) == -1.0
    assert (r.split, r.alone) == (4, 4)


def test_another_tensor_of_equal_contents_is_a_miss():
    r = Rig()
    x, p = r.inputs()
    r.wpos(x, p)
    assert float(r.wtrj(x.clone(), p)[0, 0, 0, 0]) == -1.0
    assert float(r.wtrj(x, p.clone())[0, 0, 0, 0]) == -1.0
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == 101.0      # (the misses left the entry where it was)
    assert (r.split, r.alone) == (1, 2)


def test_a_module_in_training_mode_is_not_fused():
    r = Rig()
    x, p = r.inputs()
    r.wpos(x, p)
    r.trj.train()
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == -1.0
    assert (r.split, r.alone) == (1, 1)


def test_cpu_callers_are_keyed_by_their_cpu_tensors_and_upload_once():
    """CPU inputs (the return_predictions branch): the pos call uploads x and param - one upload each - and the entry keeps the
    device copies; the trj call on the same CPU tensors is a hit and uploads nothing."""
    r = Rig()
    x, p = r.inputs()
    assert x.device.type == "cpu"
    r.wpos(x, p)
    assert r.uploads == 2 and r.seen[0][0] is not x and r.seen[0][1] is not p       # the forward read the copies
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == 101.0
    assert (r.split, r.alone, r.uploads) == (1, 0, 2)
    entry_free = r.seam._park == []
    assert entry_free


def test_lanes_or_a_cu_limit_on_either_handle_mean_no_fusing():
    class FakeHandle:
        options = {_capi.R3D_OPT_LANES: 2}

    r = Rig()
    x, p = r.inputs()
    r.trj._handle = FakeHandle()
    r.wpos(x, p), r.wtrj(x, p)
    assert (r.split, r.pos_alone, r.alone) == (0, 1, 1)
    FakeHandle.options = {_capi.R3D_OPT_LANES: 0}
    r.wpos(x, p), r.wtrj(x, p)
    assert (r.split, r.pos_alone, r.alone) == (1, 1, 1)
    r.trj._handle = None
    r.pos._cu_limit = 128
    r.wpos(x, p), r.wtrj(x, p)
    assert (r.split, r.pos_alone, r.alone) == (1, 2, 2)


def test_release_parked_drops_the_entries():
    fac = ray3d_amd.Model(default_model_config(ARCHITECTURE="3,3"), {}, is_train=False, fuse_pair=True)
    x, p = torch.zeros(2, 9, 17, 3), torch.zeros(2, 2)
    fac._seam._park.append((x, p, None, torch.zeros(2, 1, 1, 3), x, p))
    fac.release_parked()
    assert fac._seam._park == []
    r = Rig()
    r.wpos(x, p)
    r.seam.release()
    assert float(r.wtrj(x, p)[0, 0, 0, 0]) == -1.0
    assert (r.split, r.alone) == (1, 1)


def test_wrapper_state_dict_and_bare_module_guard_are_unchanged():
    r = Rig()
    assert all(k.startswith("module.") for k in r.wpos.state_dict())
    assert set(r.wpos.state_dict()) == {"module." + k for k in r.pos.state_dict()}
    bare = ray3d_amd.RIEModel(config_from_dicts(default_model_config(ARCHITECTURE="3,3"), "pos")).eval()
    with pytest.raises(RuntimeError, match="no.*CPU fallback|AMD GPU"):
        bare(torch.zeros(2, 9, 17, 3), torch.zeros(2, 2))
