"""CPU suite: the host side of r3d_streams_link (one person across cameras) - the exports, the state's documented layout, the
argument rules (all checked before any device call: they run without a GPU), and the host hook r3d_debug_streams_link_host, bit for
bit, outputs AND state after every tick, against the NumPy restatement of the header's rule (tests/streams_link_cases.py) on seeded
multi-tick cases, plus a constructed scene checked against literal expectations and the member table fed to the fuse hook.  Every
buffer lies inside guard bands with poisoned outputs (tests/buffers_util.py).  tests/test_gpu_streams_link.py runs the kernel on
the same cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, hooks_library

import streams_link_cases as lc
from streams_link_cases import LinkRig, agree
from ray3d_amd import _capi

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()


# ------------------------------------------------------------------------------------ header, binding, exports

def test_exports_header_and_abi():
    assert {"r3d_streams_link", "r3d_streams_link_bytes"} <= set(_capi.EXPORTS)
    assert "r3d_debug_streams_link_host" in _capi.HOOK_EXPORTS
    assert re.search(r"#define R3D_LINK_MAX_PEOPLE +%d\b" % _capi.LINK_MAX_PEOPLE, HDR) and _capi.LINK_MAX_PEOPLE == 32
    assert HDR.index("int r3d_debug_streams_link_host(") > HDR.index("#ifdef R3D_TEST_HOOKS") > HDR.index("int r3d_streams_link(")
    block = HDR[HDR.index("one call between a tick's r3d_streams_poses"):HDR.index("int r3d_streams_link(")]
    for word in ("THE WHOLE BOUNDS STORY", "R3D_ERR_ARG", "THE STATE", "GREEDY MATCHING", "BIRTHS", "only after its range check"):
        assert word in block, word
    # the struct the binding passes is the header's: the same fields in the same order, 56 bytes
    fields = HDR[:HDR.index("} r3d_link_params;")].rsplit("typedef struct {", 1)[1]
    names = [n.strip() for decl in re.findall(r"(?:int32_t|float|double)\s+([a-z_, ]+);", fields) for n in decl.split(",")]
    assert names == [f[0] for f in _capi.LinkParams._fields_] and C.sizeof(_capi.LinkParams) == 56
    product = C.CDLL(_capi.LIB_PATH)
    assert hasattr(product, "r3d_streams_link") and not hasattr(product, "r3d_debug_streams_link_host")
    hooks = hooks_library()
    assert hasattr(hooks, "r3d_streams_link") and hasattr(hooks, "r3d_debug_streams_link_host")
    assert hooks.r3d_abi_version() == 6 == _capi.ABI_VERSION            # no existing struct changed


def test_state_bytes_equal_the_documented_layout():
    for N, Cn, G, J in [(1, 1, 1, 1), (1, 2, 4, 17), (2, 3, 3, 14), (1, 16, 32, 17), (7, 1, 5, 3), (2047, 16, 32, 17), (65535, 1, 1, 1)]:
        NG = N * G
        want = (8 * N + 8 * NG + 8 * NG * Cn + 8 * NG * J * 3 + 4 * NG + 4 * NG + 4 * NG * Cn + 4 * NG + 7) // 8 * 8
        assert _capi.streams_link_bytes(N, Cn, G, J) == want == lc.state_bytes(N, Cn, G, J), (N, Cn, G, J)
    for shape in [(0, 1, 1, 17), (1, 0, 1, 17), (1, 17, 1, 17), (1, 1, 0, 17), (1, 1, 33, 17), (1, 1, 1, 0), (1, 1, 1, 18), (-1, 1, 1, 17),
                  (2049, 1, 32, 17), (65536, 1, 1, 17), (4097, 16, 1, 17)]:
        assert _capi.streams_link_bytes(*shape) == 0, shape
    st = lc.unpack_state(np.arange(lc.state_bytes(2, 3, 4, 5), dtype=np.int64).astype(np.uint8), 2, 3, 4, 5)
    assert st["link_id"].shape == (8, 3) and st["ref"].shape == (8, 5, 3) and st["link"].shape == (8, 3)
    assert np.array_equal(lc.pack_state(st, 2, 3, 4, 5), np.arange(lc.state_bytes(2, 3, 4, 5), dtype=np.int64).astype(np.uint8))


# ------------------------------------------------------------------------------------ the hook against the restatement

@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "N%d-C%d-P%d-G%d" % s)
def test_hook_equals_the_restatement_bit_for_bit(shape):
    """Outputs and state after every tick of every case of the shape."""
    keys = [k for k in lc.case_ids() if k[:4] == shape]
    assert len(keys) == 2
    for key in keys:
        case, outs = lc.host_run(*key)
        for t, (got, exp) in enumerate(zip(outs, lc.restate_case(case))):
            agree(got, exp, (key, t))
            assert (got["member"][:, case["C"]:] == -1).all()


def test_the_cases_do_what_they_are_there_for():
    """Over the seeded cases: J 1, 14 and 17, M = C and M = 16, the break test off and on, the three first states; people are born,
    matched, unlinked, freed; births overflow the free people; people have several members; streams did not finish, rows are not
    finite, identities go to -1 and change; two candidates are bit-identical."""
    keys = lc.case_ids()
    assert {k[4] for k in keys} == {1, 14, 17} and {k[5] == k[1] for k in keys} == {False, True} and {k[5] for k in keys} >= {16}
    assert {k[6] for k in keys} == {False, True} and {k[7] for k in keys} == {"zero", "a5", "twice"}
    assert {k[:4] for k in keys} == set(lc.SHAPES)
    born = linked = dropped = freed = several = unfinished = nonfinite = gone = changed = twins = broken = 0
    for key in keys:
        case, outs = lc.host_run(*key)
        N, Cn, P, G, J = (case[k] for k in "NCPGJ")
        before = None
        for t, (tick, got) in enumerate(zip(case["ticks"], outs)):
            linked += int(got["stats"][:, 1].sum())
            born += int(got["stats"][:, 2].sum())
            dropped += int(got["stats"][:, 3].sum())
            several += int(((got["member"] >= 0).sum(1) >= 2).sum())
            fin = (tick["status"] == 0) & (tick["emit"] >= 0)
            unfinished += int((~fin & (tick["id"] >= 0)).sum())
            nonfinite += int((~np.isfinite(tick["world"][fin])).sum())
            for c in range(N * Cn):
                rows = tick["world"][c * P:(c + 1) * P].view(np.uint64).reshape(P, -1)
                twins += int(P >= 2 and fin[c * P] and fin[c * P + 1] and np.array_equal(rows[0], rows[1]))
            if before is not None:
                freed += int(((before["person"] >= 0) & (got["person"] < 0)).sum())
                held = before["group"] >= 0
                gone += int((held & (tick["id"] < 0)).sum())
                changed += int((held & (tick["id"] >= 0) & (tick["id"] != case["ticks"][t - 1]["id"])).sum())
                s = tick["jumped"]
                if case["break_dist"] > 0 and s >= 0:
                    broken += int(held[s] and tick["id"][s] == case["ticks"][t - 1]["id"][s] and fin[s] and got["group"][s] != before["group"][s])
            before = got
    print("born %d linked %d dropped %d freed %d several %d unfinished %d nonfinite %d gone %d changed %d twins %d broken %d"
          % (born, linked, dropped, freed, several, unfinished, nonfinite, gone, changed, twins, broken))
    assert min(born, linked, dropped, freed, several, unfinished, nonfinite, gone, changed, twins, broken) > 0


def test_a_state_with_one_stream_linked_twice_keeps_the_smaller_person():
    key = [k for k in lc.case_ids() if k[7] == "twice" and k[2] >= 2][0]
    case, outs = lc.host_run(*key)
    st0 = lc.unpack_state(case["state0"], case["N"], case["C"], case["G"], case["J"])
    assert (st0["link"][:, 0] == 1).sum() >= 2 or case["G"] == 1
    for got in outs:
        held = got["member"][got["member"] >= 0]
        assert len(set(held.tolist())) == held.size                  # no stream is ever in two rows of the member table
        for gi, row in enumerate(got["member"]):
            for s in row[row >= 0]:
                assert got["group"][s] == gi


# ------------------------------------------------------------------------------------ the argument rules

def test_every_argument_error_is_err_arg_and_leaves_the_buffers_alone():
    case = lc.make_case(2, 3, 5, 3, 17, 16, True, "zero")
    rig = LinkRig("cpu", case)
    rig.load(case["ticks"][0])
    good = dict(num_scenes=2, num_cameras=3, slots=5, people=3, max_members=16, num_joints=17, min_joints=4, min_common=3, max_missed=2,
                max_dist=0.5, break_dist=1.0)
    bad_prm = [dict(num_scenes=0), dict(num_cameras=0), dict(num_cameras=17, max_members=17), dict(slots=0), dict(slots=33), dict(people=0),
               dict(people=33), dict(num_joints=0), dict(num_joints=18), dict(max_members=2), dict(max_members=17), dict(min_joints=0),
               dict(min_joints=18), dict(min_common=0), dict(min_common=18), dict(max_missed=-1), dict(max_dist=0.0), dict(max_dist=-1.0),
               dict(max_dist=float("inf")), dict(max_dist=float("nan")), dict(break_dist=0.25), dict(break_dist=float("inf")),
               dict(break_dist=float("nan")), dict(num_scenes=4370, num_cameras=1, slots=15, people=1), dict(num_scenes=2048, people=32)]
    for over in bad_prm:
        rc, out = rig.run(prm=_capi.link_params(**dict(good, **over)))
        assert rc == _capi.R3D_ERR_ARG, over
        assert all(lc.poisoned(out[k]) for k in lc.OUT_KEYS) and np.array_equal(out["state"], case["state0"]), over
    p = _capi.link_params(**good)
    p.struct_size = 48
    assert rig.run(prm=p)[0] == _capi.R3D_ERR_ARG
    for name in ("state", "prm", "world", "emit", "status", "id", "member", "person"):
        assert rig.run(**{name: None})[0] == _capi.R3D_ERR_ARG, name
    for name in ("state", "world", "emit", "id", "person"):          # 8-byte alignment
        assert rig.run(**{name: rig.t[name].data_ptr() + 4})[0] == _capi.R3D_ERR_ARG, name
    t = rig.t
    nbytes = {k: v.numel() * v.element_size() for k, v in t.items()}
    for out_name in lc.OUT_KEYS:                                     # an output inside, or ending inside, an input, the state or another output
        for other in ("world", "emit", "status", "id", "state") + tuple(k for k in lc.OUT_KEYS if k != out_name):
            assert rig.run(**{out_name: t[other].data_ptr()})[0] == _capi.R3D_ERR_ARG, (out_name, other)
            assert rig.run(**{out_name: t[other].data_ptr() + nbytes[other] - 8})[0] == _capi.R3D_ERR_ARG, (out_name, other)
            assert rig.run(**{out_name: t[other].data_ptr() - nbytes[out_name] + 8})[0] == _capi.R3D_ERR_ARG, (out_name, other)
    rc, out = rig.run()                                              # the good call still passes, with break_dist == max_dist too
    assert rc == 0 and not any(lc.poisoned(out[k]) for k in lc.OUT_KEYS)
    assert rig.run(prm=_capi.link_params(**dict(good, break_dist=0.5)))[0] == 0
    assert rig.run(prm=_capi.link_params(**dict(good, break_dist=-3.0)))[0] == 0


def test_optional_outputs_left_out_change_nothing_else():
    case = lc.make_case(2, 3, 5, 3, 17, 16, True, "zero")
    full, bare = LinkRig("cpu", case), LinkRig("cpu", case)
    for t, tick in enumerate(case["ticks"]):
        (_, a), (_, b) = full.run(tick), bare.run(tick, group=None, stats=None)
        agree(b, a, t, keys=("member", "person", "state"))
        assert lc.poisoned(b["group"]) and lc.poisoned(b["stats"])


def test_the_product_entry_refuses_on_the_host_before_any_device_call():
    """Without a GPU: R3D_ERR_ARG comes back from the product library's r3d_streams_link itself."""
    _capi.use_hooks(False)
    bogus = 1 << 24
    good = dict(num_scenes=2, num_cameras=3, slots=5, people=3, max_members=16, num_joints=17, min_joints=4, min_common=3, max_missed=2,
                max_dist=0.5, break_dist=0.0)
    ptrs = [bogus * k for k in range(2, 10)]
    for over, word in ((dict(people=33), "people"), (dict(max_dist=0.0), "max_dist"), (dict(max_members=2), "max_members")):
        with pytest.raises(_capi.Ray3DHipError, match=word):
            _capi.streams_link(bogus, _capi.link_params(**dict(good, **over)), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], None, None, 0)
    with pytest.raises(_capi.Ray3DHipError, match="overlaps"):
        _capi.streams_link(bogus, _capi.link_params(**good), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[4] + 8, None, None, 0)
    with pytest.raises(_capi.Ray3DHipError, match="struct_size"):
        p = _capi.link_params(**good)
        p.struct_size = 48
        _capi.streams_link(bogus, p, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], None, None, 0)


# ------------------------------------------------------------------------------------ a constructed scene

Cn, P, G, J, MAX_MISSED = 3, 2, 3, 17, 2
S = Cn * P
SKELETON = np.random.RandomState(3).uniform(-0.4, 0.4, (J, 3))
HOMES = np.array([[0.0, 0.0, 3.0], [1.5, 0.0, 3.0]])                  # two people 1.5 m apart
OFFSETS = np.array([[0.03, 0.0, 0.0], [0.0, -0.05, 0.0], [0.0, 0.0, 0.04]])      # per camera, <= 5 cm
SLOT = {0: (0, 1), 1: (1, 0), 2: (0, 1)}                             # camera -> the slots of person 0 and person 1


def scene_tick(t, finished=True, ids=None, moved=None):
    """Both people in all three cameras, walking 1 cm per tick; `ids`: (camera, person) -> identity overrides (None: no track);
    `moved`: (camera, person) -> metres added."""
    world = np.full((S, J, 3), np.nan)
    emit = np.full(S, t if finished else -1, np.int64)
    status = np.zeros(S, np.int32)
    idv = np.zeros(S, np.int64)
    for c in range(Cn):
        for k in range(2):
            s = c * P + SLOT[c][k]
            world[s] = HOMES[k] + 0.01 * t + SKELETON + OFFSETS[c] + (moved or {}).get((c, k), 0.0)
            idv[s] = k
            if ids and (c, k) in ids:
                idv[s] = -1 if ids[(c, k)] is None else ids[(c, k)]
    return dict(world=world, emit=emit, status=status, id=idv)


def scene_case(ticks, break_dist=0.0):
    return dict(N=1, C=Cn, P=P, G=G, M=4, J=J, min_joints=4, min_common=3, max_missed=MAX_MISSED, max_dist=0.5, break_dist=break_dist,
                state0=np.zeros(lc.state_bytes(1, Cn, G, J), np.uint8), ticks=ticks)


def play(case):
    rig = LinkRig("cpu", case)
    outs = []
    for tick in case["ticks"]:
        rc, out = rig.run(tick)
        assert rc == 0
        outs.append(out)
    for t, (got, exp) in enumerate(zip(outs, lc.restate_case(case))):
        agree(got, exp, t)
    return outs


def streams_of(k):
    return [c * P + SLOT[c][k] for c in range(Cn)]


def test_a_constructed_scene_against_literal_expectations():
    # nothing finished on tick 0; both people are born on tick 1 with three members each and no candidate is dropped
    ticks = [scene_tick(0, finished=False), scene_tick(1), scene_tick(2),
             scene_tick(3, ids={(1, 0): 7}),                         # camera 1's track of person 0 has a new identity, not finished ...
             scene_tick(4, ids={(1, 0): 7})]                         # ... and finishes: it re-joins the same pid
    ticks[3]["emit"][1 * P + SLOT[1][0]] = -1
    outs = play(scene_case(ticks))
    assert (outs[0]["person"] == -1).all() and (outs[0]["member"] == -1).all() and outs[0]["stats"].tolist() == [[0, 0, 0, 0]]
    # camera 0 bears both people - slot 0 (person 0) first -, cameras 1 and 2 link to them
    assert outs[1]["person"].tolist() == [0, 1, -1] and outs[1]["stats"].tolist() == [[2, 4, 2, 0]]
    assert outs[1]["member"].tolist() == [streams_of(0) + [-1], streams_of(1) + [-1], [-1] * 4]
    assert outs[1]["group"].tolist() == [0, 1, 1, 0, 0, 1]
    assert outs[2]["member"].tolist() == outs[1]["member"].tolist() and outs[2]["stats"].tolist() == [[2, 0, 0, 0]]
    s = 1 * P + SLOT[1][0]
    assert outs[3]["member"][0].tolist() == [streams_of(0)[0], -1, streams_of(0)[2], -1] and outs[3]["group"][s] == -1
    assert outs[3]["person"].tolist() == [0, 1, -1] and outs[3]["stats"].tolist() == [[2, 0, 0, 0]]
    assert outs[4]["member"].tolist() == outs[1]["member"].tolist() and outs[4]["stats"].tolist() == [[2, 1, 0, 0]]
    assert outs[4]["person"].tolist() == [0, 1, -1]
    # the reference pose is the mean of the members' points
    st = lc.unpack_state(outs[2]["state"], 1, Cn, G, J)
    want = np.mean([ticks[2]["world"][s] for s in streams_of(1)], 0)
    assert np.abs(st["ref"][1] - want).max() < 1e-15 and st["seen"][1] == (1 << J) - 1 and st["next_id"][0] == 2


def test_a_person_with_no_link_is_freed_after_exactly_max_missed_plus_one_ticks():
    gone = {(c, 1): None for c in range(Cn)}                          # person 1's tracks end everywhere
    ticks = [scene_tick(0)] + [scene_tick(t, ids=gone) for t in range(1, MAX_MISSED + 3)]
    outs = play(scene_case(ticks))
    assert outs[0]["person"].tolist() == [0, 1, -1]
    for t in range(1, MAX_MISSED + 1):                                # no link, still live
        assert outs[t]["person"].tolist() == [0, 1, -1] and (outs[t]["member"][1] == -1).all(), t
        assert outs[t]["stats"][0, 0] == 2
    assert outs[MAX_MISSED + 1]["person"].tolist() == [0, -1, -1] and outs[MAX_MISSED + 1]["stats"][0, 0] == 1
    assert outs[MAX_MISSED + 2]["person"].tolist() == [0, -1, -1]
    # a person that comes back within max_missed, with new identities, re-joins its pid; one tick later it is a new person
    back = {(c, 1): 40 + c for c in range(Cn)}
    for idle, pid in ((MAX_MISSED, 1), (MAX_MISSED + 1, 2)):
        ticks = [scene_tick(0)] + [scene_tick(t, ids=gone) for t in range(1, idle + 1)] + [scene_tick(idle + 1, ids=back)]
        outs = play(scene_case(ticks))
        assert sorted(outs[-1]["person"].tolist()) == sorted([0, pid, -1]), idle
        row = outs[-1]["person"].tolist().index(pid)
        assert outs[-1]["member"][row].tolist() == streams_of(1) + [-1]


def test_with_break_dist_a_member_moved_away_is_unlinked():
    ticks = [scene_tick(0), scene_tick(1, moved={(2, 0): 2.0}), scene_tick(2)]
    s = 2 * P + SLOT[2][0]
    kept = play(scene_case(ticks, break_dist=0.0))
    assert kept[1]["member"][0].tolist() == streams_of(0) + [-1]     # without the break test the identity keeps the link
    cut = play(scene_case(ticks, break_dist=1.0))
    # unlinked on the tick it moved; 2 m from everybody, it is born as a third person that tick
    assert cut[1]["member"][0].tolist() == streams_of(0)[:2] + [-1, -1]
    assert cut[1]["person"].tolist() == [0, 1, 2] and cut[1]["group"][s] == 2 and cut[1]["stats"].tolist() == [[3, 0, 1, 0]]


def test_the_member_table_feeds_the_fuse_hook_like_hand_written_groups():
    ticks = [scene_tick(0), scene_tick(1)]
    outs = play(scene_case(ticks))
    hooks_library()
    M = 4
    hand = np.array([streams_of(0) + [-1], streams_of(1) + [-1], [-1] * M], np.int32)
    tick = ticks[1]
    res = []
    for member in (np.ascontiguousarray(outs[1]["member"]), hand):
        world, emit, status = np.ascontiguousarray(tick["world"]), tick["emit"].copy(), tick["status"].copy()
        fused, spread = np.zeros((G, J, 3)), np.zeros((G, J))
        count, used = np.zeros((G, J), np.int32), np.zeros((G, M), np.uint32)
        rc = _capi.debug_streams_fuse_host(world.ctypes.data, None, emit.ctypes.data, status.ctypes.data, None, S, J, member.ctypes.data, G, M,
                                           2.0, 0.0, 0.0, fused.ctypes.data, spread.ctypes.data, count.ctypes.data, used.ctypes.data)
        assert rc == 0
        res.append((fused.view(np.uint64), spread.view(np.uint64), count, used))
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert (res[0][2][:2] == 3).all() and (res[0][2][2] == 0).all()
    _capi.use_hooks(False)
