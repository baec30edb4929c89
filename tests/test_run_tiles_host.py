"""The run cut of one-tile-deep M = B launches (r3d_schedule.cpp, pack_runs) on the host: the hooks library builds the tile lists of the
default RF 27 and RF 243 pairs for every call size from 129 to 300 windows, and they are checked cell by cell.  No GPU."""
import collections
import ctypes

import pytest

from conftest import dev_switch, hooks_library
from run_tiles_util import NB_CODE, forward_lists, sources_of

ARCHS = {"rf27": "3,3,3", "rf243": "3,3,3,3,3"}


def _check_lists(probs, tiles):
    """Every cell (32-row unit, 32-column block) of every problem that holds gemm_tile_nb tiles is computed exactly once; a run is 4 .. 7
    cells wide and has at most two sources; a run crosses into another problem only when both have one A segment and the same K.
    Returns the two-source tiles."""
    cover = collections.defaultdict(collections.Counter)
    two = []
    for t in tiles:
        p = probs[t["prob"]]
        if t["code"] <= NB_CODE:
            assert t["src2"] < 0, t                                   # (only gemm_tile_nb has a second source)
            if p["N"] >= 512 and t["code"] <= 4:                      # whole and split-K tiles of the problems that are re-cut elsewhere
                for u in range(t["units"]):
                    for b in range(t["col0"] // 32, min(t["col0"] + 256 // t["code"], p["N"]) // 32):
                        cover[t["prob"]][(t["row0"] // 32 + u, b)] += 1
            continue
        nb = t["code"] - NB_CODE
        assert 4 <= nb <= 7 and t["units"] == 1, t
        srcs = sources_of(t, probs)
        assert 1 <= len(srcs) <= 2 and sum(s[3] for s in srcs) == nb
        for prob, unit, b0, n in srcs:
            q = probs[prob]
            assert n >= 1 and unit * 32 < q["M"] and (b0 + n) * 32 <= q["N"], (t, srcs)
            for b in range(b0, b0 + n):
                cover[prob][(unit, b)] += 1
        if len(srcs) == 2:
            two.append(t)
            a, b = probs[srcs[0][0]], probs[srcs[1][0]]
            assert srcs[0][2] + srcs[0][3] == a["N"] // 32 and a["K"] == b["K"], (t, srcs)        # the end of a row; one K loop
            if srcs[1][0] != srcs[0][0]:
                assert a["nseg"] == 1 and b["nseg"] == 1, (a, b)
                assert srcs[0][1] == (a["M"] + 31) // 32 - 1 and srcs[1][1] == 0                    # last unit -> first unit
    for prob, cells in cover.items():
        if not any(t["prob"] == prob and t["code"] > NB_CODE for t in tiles) and not any(t["src2"] == prob for t in two):
            continue
        q = probs[prob]
        want = {(u, b) for u in range((q["M"] + 31) // 32) for b in range(q["N"] // 32)}
        assert set(cells) == want and set(cells.values()) == {1}, (prob, q["name"])
    return two


@pytest.mark.parametrize("model", sorted(ARCHS))
def test_every_cell_once_for_129_to_300_windows(model, tmp_path):
    """Single-launch lists (r3d_debug_forward_check: a sound dependency machine with both sources' producers and counters) and the
    launch-by-launch form (r3d_debug_plan_check: the same tiles, exact cover per launch order) for every B in 129 .. 300."""
    import ray3d_amd
    from ray3d_amd import _capi
    from ray3d_amd.spec import config_from_dicts
    mc = ray3d_amd.default_model_config(ARCHITECTURE=ARCHS[model])
    lib = hooks_library()
    plan_check = lib.r3d_debug_plan_check
    plan_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    plan_check.restype = ctypes.c_int
    hp, ht = _capi.Handle(config_from_dicts(mc, "pos")), _capi.Handle(config_from_dicts(mc, "trj"))
    sizes_with_runs = []
    for B in range(129, 301):
        probs, tiles, rc = forward_lists(mc, B, tmp_path)
        assert rc == 0, (model, B, rc)
        if _check_lists(probs, tiles):
            sizes_with_runs.append(B)
        n, sp = ctypes.c_int(), ctypes.c_int()
        assert plan_check(hp.ptr, ht.ptr, B, 256, ctypes.byref(n), ctypes.byref(sp)) == 0, (model, B)
    hp.close()
    ht.close()
    print("%s: two-source tiles at B = %s" % (model, sizes_with_runs))
    assert 256 in sizes_with_runs and all(B <= 256 for B in sizes_with_runs)


def _launch_runs(probs, tiles, block, layer):
    """The gemm_tile_nb tiles of the launch that holds `block`'s `layer` problems (and whatever rides along): widths and workgroups."""
    mine = {i for i, q in probs.items() if q["name"].split(".")[0].split("_")[0] == block and q["name"].split(".")[-2] == layer and q["N"] >= 512}
    assert mine
    level = [t for t in tiles if t["code"] > NB_CODE and (t["prob"] in mine or t["src2"] in mine)]
    riders = {t["prob"] for t in level} | {t["src2"] for t in level if t["src2"] >= 0}
    level = [t for t in tiles if t["code"] > NB_CODE and t["prob"] in riders]
    return [t["code"] - NB_CODE for t in level], {t["wg"] for t in level}


@pytest.mark.parametrize("model", sorted(ARCHS))
def test_the_256_window_call_is_cut_into_256_equal_runs(model, tmp_path, monkeypatch):
    """At 256 windows the Integration w1 / w2 launches (six problems, 1536 cells) are 256 runs of 6 cells, and the FuseBlocks w1 / w2
    launches (the five FuseBlocks and both GlobalInfo layers: seven problems, 1792 cells) 256 runs of 7 - one per workgroup.
    The RF 243 pair's default plan moves the trajectory model's pyramid one launch late (r3d_plan.cpp, the row spill), which puts 24
    fused-pair units of that pyramid into the FuseBlocks launches: they need 24 workgroups of their own, 232 are left for 1792
    cells, and no run of at most 7 cells fits - those launches keep their whole tiles.  The seven problems alone (R3D_NO_SPILL,
    hooks build) are cut as above."""
    import ray3d_amd
    mc = ray3d_amd.default_model_config(ARCHITECTURE=ARCHS[model])
    probs, tiles, rc = forward_lists(mc, 256, tmp_path)
    assert rc == 0
    for layer in ("w1", "w2"):
        widths, wgs = _launch_runs(probs, tiles, "Integration", layer)
        assert widths == [6] * 256 and len(wgs) == 256, (layer, collections.Counter(widths))
    if model == "rf243":
        # the plan this call runs: whole tiles for the seven 1024-wide problems of each FuseBlocks launch, beside the rider's units
        for layer in ("w1", "w2"):
            mine = {i for i, q in probs.items() if q["name"].startswith("FuseBlocks.") and q["name"].split(".")[-2] == layer}
            kinds = collections.Counter((t["code"], t["units"]) for t in tiles if t["prob"] in mine)
            assert len(mine) == 5 and kinds == {(1, 1): 5 * 32}, (layer, kinds)
        dev_switch(monkeypatch, "R3D_NO_SPILL", "1")
        probs, tiles, rc = forward_lists(mc, 256, tmp_path)
        assert rc == 0
        _check_lists(probs, tiles)
    for layer in ("w1", "w2"):
        widths, wgs = _launch_runs(probs, tiles, "FuseBlocks", layer)
        assert widths == [7] * 256 and len(wgs) == 256, (layer, collections.Counter(widths))


def test_the_switches_keep_selecting_the_other_packings(tmp_path, monkeypatch):
    """R3D_NO_RUNS (hooks build) gives the row-by-row cut back, R3D_NO_NB the whole tiles."""
    import ray3d_amd
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    dev_switch(monkeypatch, "R3D_NO_RUNS", "1")
    probs, tiles, rc = forward_lists(mc, 256, tmp_path)
    assert rc == 0 and not any(t["src2"] >= 0 for t in tiles) and any(t["code"] > NB_CODE for t in tiles)
    dev_switch(monkeypatch, "R3D_NO_NB", "1")
    probs, tiles, rc = forward_lists(mc, 256, tmp_path)
    assert rc == 0 and not any(t["code"] > NB_CODE for t in tiles)
