#!/usr/bin/env python3
"""A/B of the cross-camera seam of one live multi-person tick - one scene of C cameras x P stream slots of the RF-243 pair
(ARCHITECTURE 3,3,3,3,3, synthetic weights), raw pixels in, `repair=5`, `world=True`, G = P people: every tick the cameras' tracks
(r3d_streams_assign) have to be grouped into people so that r3d_streams_fuse can write one world skeleton per person:

  A `people`: OnlineLifter(cameras=C, people=G).track - ONE r3d_streams_link launch between r3d_streams_poses and r3d_streams_fuse;
              nothing comes back to the host, and the fuse call of the SAME tick reads the table;
  B `host`:   what a caller writes without it - OnlineLifter(cameras=C, groups=...).track, then track_id, frames and world copied
              back to the host (the tick's synchronisation), the SAME rule there in plain C++ (r3d_debug_streams_link_host of the
              hooks library, on host arrays and a host state), then set_groups.  The table is ONE TICK STALE: this tick's fuse call
              has already run on the previous one.

Both eager and captured (OnlineLifter.capture(); B's copy-back, association and set_groups stay outside the graph).  The sides
first run rf // 2 + SETTLE untimed ticks on the same detections - a centred model's first pose, and with it the first person, comes
rf // 2 ticks after a track's first frame -, then their people and member tables are recorded (not asserted).  `link_alone`: the
one launch without the tick, between device events.

Timing: B synchronises by construction, so a side's run is TICKS ticks on the HOST clock between two device synchronisations; the
four sides alternate, REPS repetitions after an untimed round; the MEDIAN, min and max of ms per tick are kept.  The shader clock of
the last single-launch forward (r3d_last_clock) is recorded around every configuration.  No ratio is a pass condition.
usage:  python tools/online_link_ab.py [--out FILE] [--cameras 2,4,8] [--slots 8,32] [--ticks N] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clips_ab_common import write_out                              # noqa: E402
from online_ab import J, make_lifter, timed                        # noqa: E402
from online_assign_ab import MAX_COST, MAX_MISSED, PERIOD, REPAIR, scene     # noqa: E402
from online_finish_ab import cameras                               # noqa: E402
from online_finish_ab import timed as timed_events                 # noqa: E402

LINK_MAX_DIST, LINK_MAX_MISSED = 0.5, 25
SETTLE = 16            # untimed ticks behind the model's lag: tracks have finished poses, people are born and linked


def one(lifter, hooks, Cn, P, ticks, reps, dev):
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import _capi
    S, D, G, M = Cn * P, P, P, _capi.FUSE_MAX_MEMBERS
    rf = lifter.receptive_field()
    rows, params, trans = cameras(S, dev)
    slot_camera = (torch.arange(S, device=dev) // P) % 4            # a camera's row is repeated over its P slots
    rows, params, trans = rows[slot_camera], params[slot_camera], trans[slot_camera]
    det_host, counts_host = scene(Cn, P, D, 7 * Cn + P)
    det, counts = torch.from_numpy(det_host).to(dev), torch.from_numpy(counts_host).to(dev)
    at = [0]

    def advance():
        at[0] = (at[0] + 1) % PERIOD
        return at[0]

    def lifters(**options):
        pair = [ray3d_amd.OnlineLifter(lifter, S, encoding="ray", device=dev, repair=REPAIR, world=True, cameras=Cn, max_detections=D,
                                       assign_max_cost=MAX_COST, assign_max_missed=MAX_MISSED, assign_fill="nan", **options) for _ in range(2)]
        for ol in pair:
            ol.set_cameras(rows, params, trans)
        pair[1].capture()
        return pair

    a_eager, a_cap = lifters(people=G, link_max_dist=LINK_MAX_DIST, link_max_missed=LINK_MAX_MISSED)
    b_eager, b_cap = lifters(groups=[[] for _ in range(G)])
    prm = a_eager._link["prm"]

    class Host:                                 # side B's association: pinned landing buffers, a host state, the rule in plain C++
        def __init__(self):
            self.world = torch.empty((S, J, 3), dtype=torch.float64).pin_memory()
            self.emit = torch.empty((S,), dtype=torch.int64).pin_memory()
            self.ids = torch.empty((S,), dtype=torch.int64).pin_memory()
            self.status = np.zeros(S, np.int32)
            self.state = np.zeros(_capi.streams_link_bytes(1, Cn, G, J), np.uint8)
            self.member, self.person = np.zeros((G, M), np.int32), np.zeros(G, np.int64)

        def tick(self, ol, t):
            ol.track(det[t], counts[t], check=False)
            self.world.copy_(ol._finish["world"], non_blocking=True)
            self.emit.copy_(ol.emit, non_blocking=True)
            self.ids.copy_(ol._assign["track_id"], non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()          # the copy-back is the tick's synchronisation
            rc = hooks.r3d_debug_streams_link_host(C.c_void_p(self.state.ctypes.data), C.byref(prm), C.c_void_p(self.world.data_ptr()),
                                                   C.c_void_p(self.emit.data_ptr()), C.c_void_p(self.status.ctypes.data),
                                                   C.c_void_p(self.ids.data_ptr()), C.c_void_p(self.member.ctypes.data),
                                                   C.c_void_p(self.person.ctypes.data), None, None)
            assert rc == 0, rc
            ol.set_groups([[int(v) for v in row if v >= 0] for row in self.member])     # (the NEXT tick fuses them)

    hosts = [Host(), Host()]
    sides = [lambda: a_eager.track(det[advance()], counts[at[0]], check=False), lambda: a_cap.track(det[advance()], counts[at[0]], check=False),
             lambda: hosts[0].tick(b_eager, advance()), lambda: hosts[1].tick(b_cap, advance())]
    with torch.no_grad():
        warm = rf // 2 + SETTLE                 # (a centred model's first pose comes rf // 2 ticks after the track's first frame)
        for t in range(warm):                   # the same detections through all four: tracks and people are born and linked
            for run in sides:
                at[0] = (t - 1) % PERIOD
                run()
        torch.cuda.synchronize(dev)
        k = a_eager._link
        tables = [a_eager.member.cpu().numpy(), a_cap.member.cpu().numpy(), hosts[0].member, hosts[1].member]
        same = {"member_tables_equal": [bool(np.array_equal(tb, tables[0])) for tb in tables],
                "live_people": int((k["person_id"] >= 0).sum()), "linked_streams": int((k["stream_person"] >= 0).sum()),
                "last_stats": k["link_stats"].sum(0).tolist()}
        clock0 = lifter.last_clock_ghz(dev)
        res = timed(sides, ticks, reps, dev)
        ol, z, stream = a_eager, a_eager._assign, torch.cuda.current_stream(dev).cuda_stream

        def link_alone():
            _capi.streams_link(k["state"].data_ptr(), k["prm"], ol._finish["world"].data_ptr(), ol.emit.data_ptr(), ol.status.data_ptr(),
                               z["track_id"].data_ptr(), ol.member.data_ptr(), k["person_id"].data_ptr(), k["stream_person"].data_ptr(),
                               k["link_stats"].data_ptr(), stream)
        (alone,) = timed_events([link_alone], ticks, reps, 0.2, dev)
    lifter.check_status(dev)
    a_cap.release(), b_cap.release()
    torch.cuda.synchronize(dev)
    lifter.release_prepared()
    pe, pc, he, hc = res
    return {"receptive_field": rf, "cameras": Cn, "slots": P, "people": G, "streams": S, "people_eager": pe, "people_captured": pc,
            "host_eager": he, "host_captured": hc, "link_alone": alone,
            "ratio_people_over_host_eager": round(pe["median_ms"] / he["median_ms"], 4),
            "ratio_people_over_host_captured": round(pc["median_ms"] / hc["median_ms"], 4),
            "saved_us_per_tick_eager": round(1e3 * (he["median_ms"] - pe["median_ms"]), 1),
            "saved_us_per_tick_captured": round(1e3 * (hc["median_ms"] - pc["median_ms"]), 1),
            "warm_ticks": warm, "state_after_warm (people_eager, people_captured, host_eager, host_captured)": same,
            "shader_clock_ghz_before_after": [clock0, lifter.last_clock_ghz(dev)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_link_ab.json"))
    ap.add_argument("--cameras", default="2,4,8")
    ap.add_argument("--slots", default="8,32")
    ap.add_argument("--arch", default="3,3,3,3,3")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from ray3d_amd import _capi
    if not torch.cuda.is_available():
        raise SystemExit("online_link_ab.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hooks = C.CDLL(_capi.HOOKS_LIB_PATH)        # side B's plain C++ association; the lifters run on the product library
    hooks.r3d_debug_streams_link_host.restype = C.c_int
    lifter = make_lifter(args.arch, dev)
    rows = []
    for Cn in (int(v) for v in args.cameras.split(",")):
        for P in (int(v) for v in args.slots.split(",")):
            rows.append(one(lifter, hooks, Cn, P, args.ticks, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    head = {"what": "ms per tick of a live multi-camera, multi-person caller: OnlineLifter(cameras=, people=).track (one r3d_streams_link "
                    "launch between r3d_streams_poses and r3d_streams_fuse) against OnlineLifter(cameras=, groups=).track + track_id, frames "
                    "and world copied back + the same rule in plain C++ on the host + set_groups (one tick stale); eager and captured; "
                    "RF-243 pair, raw pixels, repair=%d, world, one scene, people = slots, link_max_dist %g, link_max_missed %d"
                    % (REPAIR, LINK_MAX_DIST, LINK_MAX_MISSED),
            "timing": "an untimed round, then the host clock around %d ticks between device synchronisations, four sides alternating, %d "
                      "repetitions: median / min / max of ms per tick; link_alone between device events" % (args.ticks, args.reps),
            "device": torch.cuda.get_device_name(dev), "rows": rows}
    return write_out(args.out, head)


if __name__ == "__main__":
    sys.exit(main())
