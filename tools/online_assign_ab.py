#!/usr/bin/env python3
"""A/B of the front of one live multi-person tick - C cameras x P stream slots of the RF-243 pair (ARCHITECTURE 3,3,3,3,3, synthetic
weights), raw pixels in, `repair=5`: per camera and tick a 2D detector's unordered list of up to D = P skeletons (P - 2 people in
view, a tenth of the joints and of the detections missing, the rows shuffled) lies in DEVICE memory, and every tick has to turn it
into the per-stream frame rows, confidences and actions r3d_streams_repair / r3d_streams_step read:

  A `track`:  OnlineLifter(cameras=C, max_detections=D).track - ONE r3d_streams_assign launch in front of the tick; nothing comes
              back to the host;
  B `host`:   what a caller writes without it - the detections and counts copied back to the host (the tick's synchronisation), the
              SAME rule there in plain C++ (r3d_debug_streams_assign_host of the hooks library, on host arrays and a host state),
              then frame / conf / actions uploaded into OnlineLifter.step.

Both eager and captured (OnlineLifter.capture(); B's copy-back and association stay outside the graph).  After WARM ticks on the same
detections the sides' actions and frame rows are compared (recorded, not asserted).  `assign_alone`: the one launch without the tick,
between device events.

Timing: B synchronises by construction, so a side's run is TICKS ticks on the HOST clock between two device synchronisations; the
four sides alternate, REPS repetitions after an untimed round; the MEDIAN, min and max of ms per tick are kept.  The shader clock of
the last single-launch forward (r3d_last_clock) is recorded around every configuration.  No ratio is a pass condition.
usage:  python tools/online_assign_ab.py [--out FILE] [--cameras 1,2,4,8] [--slots 8,32] [--ticks N] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clips_ab_common import write_out                              # noqa: E402
from online_ab import J, cameras, make_lifter, timed               # noqa: E402
from online_finish_ab import timed as timed_events                 # noqa: E402

PERIOD, WARM = 64, 12
MAX_COST, MAX_MISSED, REPAIR = 0.5, 5, 5


def scene(Cn, P, D, seed):
    """-> (det (PERIOD, C, D, J, 2) float32 pixels, counts (PERIOD, C) int32): P - 2 people per camera (at least one), skeletons of
    120 px on a grid 150 px apart, swaying 20 px with the period of the sequence (so that it can be cycled), 1.5 px noise; a tenth
    of the joints NaN, a tenth of the detections missing; the rows shuffled."""
    import numpy as np
    rng = np.random.RandomState(seed)
    people = max(P - 2, 1)
    bones = rng.uniform(-0.5, 0.5, (J, 2))
    bones[:4] = [[-0.5, -0.5], [0.5, 0.5], [-0.5, 0.5], [0.5, -0.5]]
    det = np.full((PERIOD, Cn, D, J, 2), np.nan, np.float32)
    counts = np.zeros((PERIOD, Cn), np.int32)
    for t in range(PERIOD):
        sway = 20.0 * np.array([np.sin(2 * np.pi * t / PERIOD), np.cos(2 * np.pi * t / PERIOD)])
        for c in range(Cn):
            rows = []
            for k in range(people):
                if rng.uniform() < 0.1:
                    continue
                pts = np.array([150.0 * (k % 6) + 100, 150.0 * (k // 6) + 100]) + sway + 120.0 * bones + rng.normal(0, 1.5, (J, 2))
                pts[rng.uniform(size=J) < 0.1] = np.nan
                rows.append(pts)
            rng.shuffle(rows)
            for d, row in enumerate(rows[:D]):
                det[t, c, d] = row
            counts[t, c] = min(len(rows), D)
    return det, counts


def one(lifter, hooks, Cn, P, ticks, reps, dev):
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import _capi
    S, D = Cn * P, P
    rf = lifter.receptive_field()
    rows, params = cameras(S, dev)
    slot_camera = (torch.arange(S, device=dev) // P) % 4            # a camera's row is repeated over its P slots
    rows, params = rows[slot_camera], params[slot_camera]
    det_host, counts_host = scene(Cn, P, D, 7 * Cn + P)
    det, counts = torch.from_numpy(det_host).to(dev), torch.from_numpy(counts_host).to(dev)
    at = [0]

    def advance():
        at[0] = (at[0] + 1) % PERIOD
        return at[0]

    def lifters(**options):
        pair = [ray3d_amd.OnlineLifter(lifter, S, encoding="ray", device=dev, repair=REPAIR, **options) for _ in range(2)]
        for ol in pair:
            ol.set_cameras(rows, params)
        return pair

    a_eager, a_cap = lifters(cameras=Cn, max_detections=D, assign_max_cost=MAX_COST, assign_max_missed=MAX_MISSED, assign_fill="nan")
    b_eager, b_cap = lifters()
    for ol in (a_cap, b_cap):                   # (B is captured with confidences: it gets them on every tick)
        if ol is b_cap:
            ol.step(np.zeros((S, J, 2), np.float32), np.zeros(S, np.int32), conf=np.zeros((S, J), np.float32))
        ol.capture()
    prm = a_eager._assign["prm"]

    class Host:                                 # side B's association: pinned landing buffers, a host state, the rule in plain C++
        def __init__(self):
            self.det = torch.empty((Cn, D, J, 2), dtype=torch.float32).pin_memory()
            self.counts = torch.empty((Cn,), dtype=torch.int32).pin_memory()
            self.state = np.zeros(_capi.streams_assign_bytes(Cn, P, J, 2), np.uint8)
            self.action, self.match = np.zeros(S, np.int32), np.zeros(S, np.int32)
            self.frame, self.conf = np.zeros((S, J, 2), np.float32), np.zeros((S, J), np.float32)
            self.ids = np.zeros(S, np.int64)

        def tick(self, ol, t):
            self.det.copy_(det[t], non_blocking=True)
            self.counts.copy_(counts[t], non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()          # the copy-back is the tick's synchronisation
            rc = hooks.r3d_debug_streams_assign_host(C.c_void_p(self.state.ctypes.data), C.byref(prm), C.c_void_p(self.det.data_ptr()), None,
                                                     C.c_void_p(self.counts.data_ptr()), C.c_void_p(self.action.ctypes.data),
                                                     C.c_void_p(self.frame.ctypes.data), C.c_void_p(self.conf.ctypes.data),
                                                     C.c_void_p(self.match.ctypes.data), C.c_void_p(self.ids.ctypes.data), None)
            assert rc == 0, rc
            return ol.step(self.frame, self.action, check=False, conf=self.conf)

    hosts = [Host(), Host()]
    sides = [lambda: a_eager.track(det[advance()], counts[at[0]], check=False), lambda: a_cap.track(det[advance()], counts[at[0]], check=False),
             lambda: hosts[0].tick(b_eager, advance()), lambda: hosts[1].tick(b_cap, advance())]
    with torch.no_grad():
        for t in range(WARM):                   # the same detections through all four: tracks are born, matched and missed
            for run in sides:
                at[0] = t - 1
                run()
        torch.cuda.synchronize(dev)
        same = {"actions_equal": [bool(torch.equal(ol.action, a_eager.action)) for ol in (a_eager, a_cap, b_eager, b_cap)],
                "frame_rows_equal": [bool(torch.equal(ol.frame_out.view(torch.int32), a_eager.frame_out.view(torch.int32)))
                                     for ol in (a_eager, a_cap, b_eager, b_cap)],
                "live_slots": int((a_eager._assign["track_id"] >= 0).sum()), "last_stats": a_eager._assign["assign_stats"].sum(0).tolist()}
        clock0 = lifter.last_clock_ghz(dev)
        res = timed(sides, ticks, reps, dev)
        ol, z, stream = a_eager, a_eager._assign, torch.cuda.current_stream(dev).cuda_stream

        def assign_alone():
            _capi.streams_assign(z["state"].data_ptr(), z["prm"], det[advance()].data_ptr(), None, counts[at[0]].data_ptr(), ol.action.data_ptr(),
                                 ol.frame.data_ptr(), ol.conf.data_ptr(), z["match"].data_ptr(), z["track_id"].data_ptr(),
                                 z["assign_stats"].data_ptr(), stream)
        (alone,) = timed_events([assign_alone], ticks, reps, 0.2, dev)
    lifter.check_status(dev)
    a_cap.release(), b_cap.release()
    torch.cuda.synchronize(dev)
    lifter.release_prepared()
    te, tc, he, hc = res
    return {"receptive_field": rf, "cameras": Cn, "slots": P, "max_detections": D, "streams": S, "track_eager": te, "track_captured": tc,
            "host_eager": he, "host_captured": hc, "assign_alone": alone,
            "ratio_track_over_host_eager": round(te["median_ms"] / he["median_ms"], 4),
            "ratio_track_over_host_captured": round(tc["median_ms"] / hc["median_ms"], 4),
            "saved_us_per_tick_eager": round(1e3 * (he["median_ms"] - te["median_ms"]), 1),
            "saved_us_per_tick_captured": round(1e3 * (hc["median_ms"] - tc["median_ms"]), 1),
            "state_after_warm (track_eager, track_captured, host_eager, host_captured)": same,
            "shader_clock_ghz_before_after": [clock0, lifter.last_clock_ghz(dev)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_assign_ab.json"))
    ap.add_argument("--cameras", default="1,2,4,8")
    ap.add_argument("--slots", default="8,32")
    ap.add_argument("--arch", default="3,3,3,3,3")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from ray3d_amd import _capi
    if not torch.cuda.is_available():
        raise SystemExit("online_assign_ab.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hooks = C.CDLL(_capi.HOOKS_LIB_PATH)        # side B's plain C++ association; the lifters run on the product library
    hooks.r3d_debug_streams_assign_host.restype = C.c_int
    lifter = make_lifter(args.arch, dev)
    rows = []
    for Cn in (int(v) for v in args.cameras.split(",")):
        for P in (int(v) for v in args.slots.split(",")):
            rows.append(one(lifter, hooks, Cn, P, args.ticks, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    head = {"what": "ms per tick of a live multi-person caller whose detector output lies on the device: OnlineLifter(cameras=).track (one "
                    "r3d_streams_assign launch in front of the tick) against detections copied back + the same rule in plain C++ on the "
                    "host + frame / conf / actions uploaded into OnlineLifter.step; eager and captured; RF-243 pair, raw pixels, repair=%d, "
                    "max_cost %g, max_missed %d" % (REPAIR, MAX_COST, MAX_MISSED),
            "timing": "an untimed round, then the host clock around %d ticks between device synchronisations, four sides alternating, %d "
                      "repetitions: median / min / max of ms per tick; assign_alone between device events" % (args.ticks, args.reps),
            "device": torch.cuda.get_device_name(dev), "rows": rows}
    return write_out(args.out, head)


if __name__ == "__main__":
    sys.exit(main())
