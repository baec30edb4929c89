"""CPU suite: r3d_finalize_dev without a device - the exports, the argument rules (all answered before any device call) and the
device path's descriptor / inverse / segment tables and per-element routines (ray3d_amd/csrc/r3d_pack.hpp) replayed on the CPU
against the host pack, bit for bit (r3d_debug_pack_replay_host).  The GPU half is tests/test_gpu_weights_dev.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, hooks_library

from ray3d_amd import _capi
from ray3d_amd.spec import config_from_dicts, default_model_config

import weights_dev_cases as wc


def test_header_binding_and_libraries_agree_on_the_new_exports():
    hdr = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()
    m = re.search(r"#ifdef R3D_TEST_HOOKS(.*?)#endif /\* R3D_TEST_HOOKS \*/", hdr, flags=re.S)
    product = hdr.replace(m.group(0), "")
    assert re.search(r"\bint r3d_finalize_dev\(r3d_model \*m, const float \*const \*weights_dev, const int64_t \*numel, int32_t count, "
                     r"void \*hip_stream\);", product)
    for hook in ("r3d_debug_pack_replay_host", "r3d_debug_weights_image"):
        assert re.search(r"\bint %s\(" % hook, m.group(1)) and not re.search(r"\b%s\(" % hook, product)
        assert hook in _capi.HOOK_EXPORTS and hook not in _capi.EXPORTS
    assert "r3d_finalize_dev" in _capi.EXPORTS and "r3d_finalize_dev" not in _capi.HOOK_EXPORTS
    product_lib, hooks_lib = ctypes.CDLL(_capi.LIB_PATH), ctypes.CDLL(_capi.HOOKS_LIB_PATH)
    assert hasattr(product_lib, "r3d_finalize_dev") and hasattr(hooks_lib, "r3d_finalize_dev")
    for hook in ("r3d_debug_pack_replay_host", "r3d_debug_weights_image"):
        assert hasattr(hooks_lib, hook) and not hasattr(product_lib, hook)
    # every struct stays as it was: the ABI version several tests pin
    assert re.search(r"#define R3D_ABI_VERSION 6\b", hdr) and _capi.ABI_VERSION == 6
    assert product_lib.r3d_abi_version() == 6 and hooks_lib.r3d_abi_version() == 6
    # the ordering contract is written out where callers read it
    for phrase in ("ordered on `hip_stream`", "R3D_OPT_LANES", "no device-wide synchronisation", "BIT FOR BIT", "non-finite"):
        assert phrase in product, phrase


@pytest.mark.parametrize("hooks", [False, True], ids=["product", "hooks"])
def test_argument_rules_are_answered_before_any_device_call(hooks, monkeypatch):
    """Wrong count, null table, null entry, one wrong numel (the key named): R3D_ERR_ARG / R3D_ERR_SHAPE with no device in sight
    (HIP_VISIBLE_DEVICES=-1: any HIP call would fail with R3D_ERR_HIP instead)."""
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")
    if hooks:
        hooks_library()
    h = _capi.Handle(config_from_dicts(default_model_config(ARCHITECTURE="3,3"), "trj"))
    keys = h.keys()
    n = len(keys)
    sizes = [int(np.prod(h.shape(i))) for i in range(n)]
    err = lambda: h._lib.r3d_last_error().decode()
    ptrs = (ctypes.c_void_p * n)(*[0x1000 + 64 * i for i in range(n)])      # (never followed: every case ends at the checks)
    numel = (ctypes.c_int64 * n)(*sizes)
    assert h.finalize_dev_raw(ptrs, numel, n - 1, None) == _capi.R3D_ERR_ARG and "count is %d" % (n - 1) in err()
    assert h.finalize_dev_raw(ptrs, numel, n + 1, None) == _capi.R3D_ERR_ARG
    assert h.finalize_dev_raw(None, numel, n, None) == _capi.R3D_ERR_ARG and "null argument" in err()
    assert h.finalize_dev_raw(ptrs, None, n, None) == _capi.R3D_ERR_ARG and "null argument" in err()
    assert h._lib.r3d_finalize_dev(None, ptrs, numel, n, None) == _capi.R3D_ERR_ARG
    at = keys.index("GlobalInfo.fc_1.weight")
    holed = (ctypes.c_void_p * n)(*[(0 if i == at else 0x1000 + 64 * i) for i in range(n)])
    assert h.finalize_dev_raw(holed, numel, n, None) == _capi.R3D_ERR_ARG and "'GlobalInfo.fc_1.weight'" in err()
    at = keys.index("LocalLayer.expand_bn.running_var")
    wrong = (ctypes.c_int64 * n)(*[(s + 1 if i == at else s) for i, s in enumerate(sizes)])
    assert h.finalize_dev_raw(ptrs, wrong, n, None) == _capi.R3D_ERR_SHAPE and "'LocalLayer.expand_bn.running_var'" in err()
    with pytest.raises(_capi.Ray3DHipError, match="size mismatch for 'LocalLayer.expand_bn.running_var'"):
        _capi.check(h.finalize_dev_raw(ptrs, wrong, n, None), "r3d_finalize_dev")
    h.close()


@pytest.mark.parametrize("weights", wc.WEIGHTS)
@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_device_tables_and_routines_replay_the_host_pack_bit_for_bit(case, weights, monkeypatch):
    """The trained-like statistics carry zero and negated gammas and variances down to 1e-7 of the synthetic ones: where a fold
    goes wrong.  Both networks of the pair; no device call (HIP_VISIBLE_DEVICES=-1)."""
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")
    hooks_library()
    mc, sp, st = wc.states_of(case, weights)
    for cfg, state in (sp, st):
        h = _capi.Handle(cfg)
        if os.environ.get("R3D_BF16X3") is None:         # (in the environment it overrides the configuration key)
            assert h.precision() == ("bf16x3" if case[1] else "f32")
        wc.set_host_weights(h, state)
        mismatches, first = h.debug_pack_replay_host()
        assert (mismatches, first) == (0, -1), (wc.case_id(case), cfg.kind, mismatches, first)
        h.close()


def test_replay_needs_every_weight():
    hooks_library()
    h = _capi.Handle(config_from_dicts(default_model_config(ARCHITECTURE="3,3"), "trj"))
    with pytest.raises(_capi.Ray3DHipError, match="Missing key"):
        h.debug_pack_replay_host()
    h.close()


def test_python_switches_exist_and_are_off_by_default():
    import inspect
    import ray3d_amd
    from ray3d_amd import modules
    m = modules.RIETrajectoryModel(config_from_dicts(default_model_config(ARCHITECTURE="3,3"), "trj"))
    assert m._device_weights is False
    gen = m._generation
    m.set_device_weights(True)
    assert m._device_weights is True and m._generation > gen and not m._synced
    assert inspect.signature(ray3d_amd.Model.__init__).parameters["device_weights"].default is False
    assert hasattr(modules.Ray3DLifter, "set_device_weights") and hasattr(_capi.Handle, "finalize_dev")
