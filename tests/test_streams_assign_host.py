"""CPU suite: the host side of r3d_streams_assign (detections to live streams) - the exports, the state's documented layout, the
argument rules (all checked before any device call: they run without a GPU), and the host hook r3d_debug_streams_assign_host, bit
for bit, outputs AND state after every tick, against the NumPy restatement of the header's rule (tests/streams_assign_cases.py) on
seeded multi-tick cases, plus the identity property on a seeded scene.  Every buffer lies inside guard bands with poisoned outputs
(tests/buffers_util.py).  tests/test_gpu_streams_assign.py runs the kernel on the same cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, hooks_library

import streams_assign_cases as ac
from streams_assign_cases import AssignRig, DRAIN, IDLE, PUSH, QNAN32, RESTART, agree
from ray3d_amd import _capi

HDR = open(os.path.join(ROOT, "include", "ray3d_hip.h")).read()


# ------------------------------------------------------------------------------------ header, binding, exports

def test_exports_header_and_abi():
    assert {"r3d_streams_assign", "r3d_streams_assign_bytes"} <= set(_capi.EXPORTS)
    assert "r3d_debug_streams_assign_host" in _capi.HOOK_EXPORTS
    for name, value in (("R3D_ASSIGN_MAX_SLOTS", _capi.ASSIGN_MAX_SLOTS), ("R3D_ASSIGN_MAX_DETECTIONS", _capi.ASSIGN_MAX_DETECTIONS),
                        ("R3D_ASSIGN_FILL_NAN", _capi.R3D_ASSIGN_FILL_NAN), ("R3D_ASSIGN_FILL_HOLD", _capi.R3D_ASSIGN_FILL_HOLD)):
        assert re.search(r"#define %s +%d\b" % (name, value), HDR), name
    assert HDR.index("int r3d_debug_streams_assign_host(") > HDR.index("#ifdef R3D_TEST_HOOKS") > HDR.index("int r3d_streams_assign(")
    block = HDR[HDR.index("one call in front of a tick's r3d_streams_repair"):HDR.index("int r3d_streams_assign(")]
    for word in ("THE WHOLE BOUNDS STORY", "R3D_ERR_ARG", "THE STATE", "GREEDY MATCHING", "BIRTHS", "Nothing in the state is ever used as an index"):
        assert word in block, word
    # the struct the binding passes is the header's: the same fields in the same order, 56 bytes
    fields = HDR[:HDR.index("} r3d_assign_params;")].rsplit("typedef struct {", 1)[1]
    names = [n.strip() for decl in re.findall(r"(?:int32_t|float|double)\s+([a-z_, ]+);", fields) for n in decl.split(",")]
    assert names == [f[0] for f in _capi.AssignParams._fields_] and C.sizeof(_capi.AssignParams) == 56
    product = C.CDLL(_capi.LIB_PATH)
    assert hasattr(product, "r3d_streams_assign") and not hasattr(product, "r3d_debug_streams_assign_host")
    hooks = hooks_library()
    assert hasattr(hooks, "r3d_streams_assign") and hasattr(hooks, "r3d_debug_streams_assign_host")
    assert hooks.r3d_abi_version() == 6 == _capi.ABI_VERSION            # no existing struct changed


def test_state_bytes_equal_the_documented_layout():
    for Cn, P, J, W in [(1, 1, 1, 2), (2, 3, 17, 3), (3, 5, 14, 2), (1, 32, 17, 3), (7, 1, 3, 3), (2047, 32, 17, 3)]:
        S = Cn * P
        want = (8 * Cn + 8 * S + 4 * S + 4 * S + 4 * S + 4 * S + 4 * S * J * W + 7) // 8 * 8
        assert _capi.streams_assign_bytes(Cn, P, J, W) == want == ac.state_bytes(Cn, P, J, W)
    for shape in [(0, 1, 17, 2), (1, 0, 17, 2), (1, 33, 17, 2), (2048, 32, 17, 2), (1, 1, 0, 2), (1, 1, 18, 2), (1, 1, 17, 1), (1, 1, 17, 4),
                  (-1, 1, 17, 2)]:
        assert _capi.streams_assign_bytes(*shape) == 0, shape


# ------------------------------------------------------------------------------------ the hook against the restatement

@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: "C%d-P%d-D%d" % s)
def test_hook_equals_the_restatement_bit_for_bit(shape):
    """Outputs and state after every tick of every case of the shape: J 14 and 17, width 2 and 3."""
    keys = [k for k in ac.case_ids() if k[:3] == shape]
    assert sorted(k[3:5] for k in keys) == [(14, 2), (14, 3), (17, 2), (17, 3)]
    for key in keys:
        case, outs = ac.host_run(*key)
        assert len(case["ticks"]) >= case["lag"] + case["max_missed"] + 3
        for t, (got, exp) in enumerate(zip(outs, ac.restate_case(case))):
            agree(got, exp, (key, t))
            idle = (got["action"] == IDLE) | (got["action"] == DRAIN)
            assert (got["frame_out"][idle] == QNAN32).all() and (got["conf_out"][idle] == 0).all() and (got["match"][idle] == -1).all()


def test_the_cases_do_what_they_are_there_for():
    """Over the seeded cases: every action occurs, tracks are matched, pushed synthetically, end, drain for exactly `lag` ticks and
    their slots are reused; births overflow the free slots; every lag, both fills, confidences and a 0xA5 state are played; and the
    clamped det_count ticks are there."""
    actions, reused, dropped, synthetic, matched = set(), 0, 0, 0, 0
    keys = ac.case_ids()
    assert {k[5] for k in keys} == set(ac.LAGS) and {k[6] for k in keys} == {0, 1} and {k[7] for k in keys} == {False, True}
    assert any(k[8] for k in keys)
    counts = set()                                       # det_count below 0, 0, D and above D
    for key in keys:
        case, outs = ac.host_run(*key)
        lag, P = case["lag"], case["P"]
        ended, drains = set(), {}
        for t, got in enumerate(outs):
            counts |= {"<0" if v < 0 else "0" if v == 0 else "D" if v == case["D"] else ">D" if v > case["D"] else "" for v in case["ticks"][t]["count"]}
            actions |= set(got["action"].tolist())
            dropped += int(got["stats"][:, 3].sum())
            matched += int(got["stats"][:, 1].sum())
            synthetic += int(((got["action"] == PUSH) & (got["match"] < 0)).sum())
            for s in range(case["C"] * P):
                a = int(got["action"][s])
                if a == RESTART:
                    reused += s in ended
                    assert drains.pop(s, lag) == lag, (key, t, s)      # an ended track got exactly `lag` DRAIN ticks first
                elif a == DRAIN:
                    drains[s] = drains.get(s, 0) + 1
                    ended.add(s)
                    assert drains[s] <= lag
                elif a == IDLE and got["id"][s] >= 0:                   # (lag 0: the tick a track ends)
                    ended.add(s)
    assert actions == {IDLE, PUSH, RESTART, DRAIN} and reused > 0 and dropped > 0 and synthetic > 0 and matched > 0
    assert {"<0", "0", "D", ">D"} <= counts


def test_a_track_is_born_missed_ends_drains_and_its_slot_is_reused():
    """One person, P = 1, lag 2, max_missed 2, by hand: RESTART, PUSH, two synthetic PUSHes, then DRAIN x 2, IDLE, and a RESTART of
    the same slot with the next identity."""
    J, W = 17, 2
    person = (300.0 + 200.0 * ac.BONES).astype(np.float32)
    none = np.full((1, 1, J, W), np.nan, np.float32)
    seq = [person, person + 3, None, None, None, None, None, person + 900, person + 905]
    ticks = [dict(det=none if d is None else d.reshape(1, 1, J, W), conf=None, count=np.array([0 if d is None else 1], np.int32)) for d in seq]
    case = dict(C=1, P=1, D=1, J=J, width=W, lag=2, min_joints=4, min_common=3, max_missed=2, fill=ac.FILL_HOLD, min_conf=0.0, max_cost=0.5,
                with_conf=False, state0=np.zeros(ac.state_bytes(1, 1, J, W), np.uint8), ticks=ticks)
    rig = AssignRig("cpu", case)
    outs = [rig.run(t)[1] for t in ticks]
    for t, (got, exp) in enumerate(zip(outs, ac.restate_case(case))):
        agree(got, exp, t)
    assert [int(o["action"][0]) for o in outs] == [RESTART, PUSH, PUSH, PUSH, DRAIN, DRAIN, IDLE, RESTART, PUSH]
    assert [int(o["id"][0]) for o in outs] == [0, 0, 0, 0, 0, 0, -1, 1, 1]
    assert [int(o["match"][0]) for o in outs] == [0, 0, -1, -1, -1, -1, -1, 0, 0]
    assert [o["stats"][0].tolist() for o in outs[:3]] == [[1, 0, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0]]
    held = ac.bits32(person + 3)
    assert np.array_equal(outs[2]["frame_out"][0], held) and np.array_equal(outs[3]["frame_out"][0], held)       # FILL_HOLD
    assert (outs[2]["conf_out"] == 0).all() and (outs[1]["conf_out"] == ac.ONE32).all()
    # the same ticks with FILL_NAN: only the synthetic frames differ
    rig = AssignRig("cpu", dict(case, fill=ac.FILL_NAN))
    nan_outs = [rig.run(t)[1] for t in ticks]
    for t, (a, b) in enumerate(zip(nan_outs, outs)):
        if t in (2, 3):
            assert (a["frame_out"] == QNAN32).all()
        agree(a, b, t, keys=("action", "conf_out", "match", "id", "stats", "state") + (() if t in (2, 3) else ("frame_out",)))


def test_the_tie_rule_and_the_greedy_order():
    """Two live slots with the same reference and two bit-identical detections: every cost is equal, the smaller p takes the smaller
    d.  A third detection that is closer to slot 1 than the twins are is matched first."""
    J, W = 14, 3
    base = np.concatenate([500.0 + 200.0 * ac.BONES[:J], np.ones((J, 1))], -1).astype(np.float32)
    mk = lambda rows, n: dict(det=np.stack(rows).reshape(1, 3, J, W), conf=None, count=np.array([n], np.int32))
    far = base + np.float32(5000)
    case = dict(C=1, P=2, D=3, J=J, width=W, lag=0, min_joints=4, min_common=3, max_missed=3, fill=ac.FILL_NAN, min_conf=0.0, max_cost=0.5,
                with_conf=False, state0=np.zeros(ac.state_bytes(1, 2, J, W), np.uint8),
                ticks=[mk([base, base, far], 2), mk([base + 4, base + 4, far], 2), mk([base + 9, base + 9, base + 5], 3)])
    rig = AssignRig("cpu", case)
    outs = [rig.run(t)[1] for t in case["ticks"]]
    for t, (got, exp) in enumerate(zip(outs, ac.restate_case(case))):
        agree(got, exp, t)
    assert outs[0]["action"].tolist() == [RESTART, RESTART] and outs[0]["match"].tolist() == [0, 1] and outs[0]["id"].tolist() == [0, 1]
    assert outs[1]["action"].tolist() == [PUSH, PUSH] and outs[1]["match"].tolist() == [0, 1]
    # tick 2: the references are both base + 4; detection 2 (1 px away) costs less than the twins (5 px): slot 0 takes it
    assert outs[2]["match"].tolist() == [2, 0] and outs[2]["stats"][0].tolist() == [3, 2, 0, 1]


# ------------------------------------------------------------------------------------ R3D_ERR_ARG

def test_every_argument_error():
    case = ac.make_case(2, 3, 5, 17, 3, 4, ac.FILL_NAN, True, False)
    rig = AssignRig("cpu", case)
    assert rig.run(case["ticks"][0])[0] == 0
    t = {n: v.data_ptr() for n, v in rig.t.items()}

    def prm(**over):
        p = _capi.AssignParams.from_buffer_copy(rig.prm)
        for k, v in over.items():
            setattr(p, k, v)
        return dict(prm=p)
    S, J, W, Cn, D = 6, 17, 3, 2, 5
    bad = [dict(state=None), dict(prm=None), dict(det=None), dict(count=None), dict(action=None), dict(frame_out=None), dict(match=None),
           dict(id=None),
           prm(struct_size=0), prm(struct_size=52), prm(struct_size=64),
           prm(num_cameras=0), prm(num_cameras=-1), prm(slots=0), prm(slots=33), prm(max_detections=0), prm(max_detections=33),
           prm(num_cameras=_capi.CLIPS_MAX // 3 + 1), prm(num_joints=0), prm(num_joints=18), prm(width=1), prm(width=4), prm(lag=-1),
           prm(min_joints=0), prm(min_joints=18), prm(min_common=0), prm(min_common=18), prm(max_missed=-1), prm(fill=2), prm(fill=-1),
           prm(min_conf=float("nan")), prm(min_conf=float("inf")), prm(max_cost=0.0), prm(max_cost=-1.0), prm(max_cost=float("nan")),
           prm(max_cost=float("inf")),
           dict(state=t["state"] + 4), dict(id=t["id"] + 4),
           # an output over an input, the state, another output - at the first and at the last byte
           dict(action=t["det"]), dict(frame_out=t["det"] + 4 * (Cn * D * J * W - 1)), dict(conf_out=t["conf"]), dict(match=t["count"] + 4),
           dict(stats=t["det"]), dict(id=t["det"] + 8),
           dict(action=t["state"]), dict(frame_out=t["state"] + ac.state_bytes(2, 3, J, W) - 4), dict(id=t["state"] + 8), dict(stats=t["state"] + 16),
           dict(action=t["match"]), dict(match=t["action"] + 4 * (S - 1)), dict(conf_out=t["frame_out"] + 4 * (S * J * W - 1)),
           dict(id=t["frame_out"]), dict(stats=t["id"] + 8 * (S - 1)), dict(frame_out=t["conf_out"] - 4 * (S * J * W - 1)),
           dict(stats=t["action"] - 4 * 7)]
    for over in bad:
        before = rig.read()
        rc = _capi.debug_streams_assign_host(*rig.ptrs(**over))
        assert rc == _capi.R3D_ERR_ARG, over
        assert _capi.load().r3d_last_error()
        agree(rig.read(), before, over)          # nothing is written by a refused call, the state included
    ok = [dict(conf_out=None), dict(stats=None), dict(conf=None), dict(conf_out=None, stats=None), prm(lag=0), prm(max_missed=0),
          prm(min_joints=17, min_common=17), prm(fill=1), prm(min_conf=-1.0), prm(max_cost=1e300)]
    for over in ok:
        assert _capi.debug_streams_assign_host(*rig.ptrs(**over)) == 0, over
    rig.arena.check()


def test_optional_outputs_left_out_change_nothing_else():
    key = (2, 3, 5, 17, 2, 1, ac.FILL_HOLD, True, False)
    case = ac.make_case(*key)
    full, bare = AssignRig("cpu", case), AssignRig("cpu", case)
    for t, tick in enumerate(case["ticks"]):
        (_, a), (_, b) = full.run(tick), bare.run(tick, conf_out=None, stats=None)
        agree(b, a, t, keys=("action", "frame_out", "match", "id", "state"))
        assert (b["conf_out"] == ac.FILL32).all() and (b["stats"].view(np.uint32) == ac.FILL32).all()


def test_the_product_entry_refuses_on_the_host_before_any_device_call():
    """Without a GPU: R3D_ERR_ARG comes back from the product library's r3d_streams_assign itself."""
    _capi.use_hooks(False)
    bogus = 1 << 24
    good = dict(num_cameras=2, slots=3, max_detections=4, num_joints=17, width=2, lag=4, min_joints=4, min_common=3, max_missed=5,
                fill=0, min_conf=0.0, max_cost=0.5)
    ptrs = [bogus * k for k in range(2, 10)]
    for over, word in ((dict(slots=33), "slots"), (dict(max_cost=0.0), "max_cost"), (dict(fill=7), "fill")):
        with pytest.raises(_capi.Ray3DHipError, match=word):
            _capi.streams_assign(bogus, _capi.assign_params(**dict(good, **over)), ptrs[0], None, ptrs[1], ptrs[2], ptrs[3], None, ptrs[4],
                                 ptrs[5], None, 0)
    with pytest.raises(_capi.Ray3DHipError, match="overlaps"):
        _capi.streams_assign(bogus, _capi.assign_params(**good), ptrs[0], None, ptrs[1], ptrs[2], ptrs[3], None, ptrs[2] + 8, ptrs[5], None, 0)
    with pytest.raises(_capi.Ray3DHipError, match="struct_size"):
        p = _capi.assign_params(**good)
        p.struct_size = 48
        _capi.streams_assign(bogus, p, ptrs[0], None, ptrs[1], ptrs[2], ptrs[3], None, ptrs[4], ptrs[5], None, 0)


# ------------------------------------------------------------------------------------ the identity property

SCENE_BONES = ac.BONES.copy()      # head, feet, hands: six joints on the skeleton's outline, so that dropped joints rarely shrink its size
SCENE_BONES[:6] = [[-0.5, -0.5], [0.5, 0.5], [-0.5, 0.5], [0.5, -0.5], [0.0, -0.5], [0.0, 0.5]]


def scene(seed, joint_drop, det_drop, ticks=300, people=5, J=17):
    """5 people, skeleton size 200 px, 260 px apart, each walking 6 - 10 px per tick (the direction turns slowly; they walk in step,
    so they stay 260 px apart), 2 px noise; `joint_drop` of the joints and `det_drop` of the detections dropped - nobody for more
    than 2 ticks in a row: at 10 px per tick, with stale joints and a size that shrinks when the outermost joints are missing, a
    longer gap carries a right pair past max_cost / 2 -; the detections
    shuffled every tick -> (per tick: det (1, 8, J, 2), count, who (the person behind detection d)), the clean skeletons (T, people,
    J, 2)."""
    rng = np.random.RandomState(seed)
    home = np.stack([[260.0 * k, 130.0 * (k % 2)] for k in range(people)]) + 400.0
    centre = np.zeros(2)
    heading = rng.uniform(0, 2 * np.pi)
    out, clean, gone = [], np.zeros((ticks, people, J, 2)), [0] * people
    for t in range(ticks):
        heading += rng.uniform(-0.2, 0.2)
        centre = centre + rng.uniform(6, 10) * np.array([np.cos(heading), np.sin(heading)])
        det = np.full((1, 8, J, 2), np.nan, np.float32)
        rows = []
        for k in range(people):
            clean[t, k] = home[k] + centre + 200.0 * SCENE_BONES[:J]
            if t > 0 and rng.uniform() < det_drop and gone[k] < 2:         # (everybody is seen on the first tick)
                gone[k] += 1
                continue
            gone[k] = 0
            pts = (clean[t, k] + rng.normal(0, 2.0, (J, 2))).astype(np.float32)
            pts[rng.uniform(size=J) < joint_drop] = np.nan
            rows.append((k, pts))
        order = rng.permutation(len(rows))
        who = []
        for d, i in enumerate(order):
            det[0, d] = rows[i][1]
            who.append(rows[i][0])
        out.append(dict(det=det, conf=None, count=np.array([len(rows)], np.int32), who=who))
    return out, clean


@pytest.mark.parametrize("joint_drop,det_drop,max_missed", [(0.2, 0.1, 5), (0.4, 0.2, 5), (0.3, 0.3, 10)])
def test_identities_survive_a_seeded_scene(joint_drop, det_drop, max_missed):
    """First the scene's own margins - the cost of every right pair (a detection against its person's last observation) is below
    max_cost / 2, of every wrong pair above 2 * max_cost -, then: zero identity switches and exactly 5 births over 300 ticks."""
    J, P, D, max_cost = 17, 8, 8, 0.5
    ticks, _ = scene(1234, joint_drop, det_drop)
    # the margins, with the rule's own cost on the rule's own references (the last observation per joint)
    last = {}
    right, wrong = [], []
    for tick in ticks:
        for d, k in enumerate(tick["who"]):
            pts = tick["det"][0, d].astype(np.float64)
            obs = np.isfinite(pts).all(-1)
            size = max(np.ptp(pts[obs, 0]), np.ptp(pts[obs, 1]))
            for k2, ref in last.items():
                common = obs & np.isfinite(ref).all(-1)
                if common.sum() >= 3:
                    (right if k2 == k else wrong).append(np.sqrt(((pts[common] - ref[common]) ** 2).sum(-1)).mean() / size)
        for d, k in enumerate(tick["who"]):
            pts = tick["det"][0, d].astype(np.float64)
            ref = last.setdefault(k, np.full((J, 2), np.nan))
            obs = np.isfinite(pts).all(-1)
            ref[obs] = pts[obs]
    print("right pairs: max cost %.3f; wrong pairs: min cost %.3f" % (max(right), min(wrong)))
    assert max(right) < max_cost / 2 and min(wrong) > 2 * max_cost
    case = dict(C=1, P=P, D=D, J=J, width=2, lag=4, min_joints=4, min_common=3, max_missed=max_missed, fill=ac.FILL_NAN, min_conf=0.0,
                max_cost=max_cost, with_conf=False, state0=np.zeros(ac.state_bytes(1, P, J, 2), np.uint8), ticks=ticks)
    rig = AssignRig("cpu", case)
    owner, births, switches = {}, 0, 0                   # track identity -> the person it was born from
    for tick in ticks:
        rc, out = rig.run(tick)
        assert rc == 0
        births += int(out["stats"][0, 2])
        for s in range(P):
            d = int(out["match"][s])
            if d < 0:
                continue
            person = tick["who"][d]
            switches += owner.setdefault(int(out["id"][s]), person) != person
    assert births == 5 and switches == 0 and sorted(owner.values()) == [0, 1, 2, 3, 4]
