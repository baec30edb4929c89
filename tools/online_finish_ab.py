#!/usr/bin/env python3
"""A/B of the OUTPUT side of one live tick - S streams of the RF-243 pair (ARCHITECTURE 3,3,3,3,3, synthetic weights), flip on, one
new frame of rays per stream, and per stream the finished pose, its world coordinates and the re-projection residual with its mean
and maximum:

  A `torch`:  what a user writes without r3d_streams_poses - OnlineLifter.step (r3d_streams_step, two forwards, the torch flip
              finish), then torch ops on the device: a float64 normalized2world (matmul + add) and the residual of
              include/ray3d_hip.h's arithmetic (about twenty small elementwise launches, a mean and a max);
  B `call`:   OnlineLifter(world=True, quality=True).step - the same step and forwards, then ONE r3d_streams_poses launch.

Both eager and captured (A: OnlineLifter.capture() for the step and a second torch.cuda.graph around the torch tail; B:
OnlineLifter.capture()).  The new frame is a device tensor on all sides.  After RF + 2 ticks on the same frames the sides' outputs
are compared (poses expected equal bit for bit, world and residual to rounding: recorded, not asserted).

Timing: the clocks are settled by WARM seconds of ticks first; a side's run is TICKS ticks between two device events on the current
stream, read after a synchronise; the four sides alternate, REPS repetitions; the MEDIAN, min and max of ms per tick are kept.  The
shader clock of the last single-launch forward (r3d_last_clock) is recorded around every configuration.  No ratio is a pass condition.
usage:  python tools/online_finish_ab.py [--out FILE] [--streams 1,8,32,256] [--ticks N] [--reps R] [--warm SECONDS]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clips_ab_common import write_out      # noqa: E402
from online_ab import J, make_lifter       # noqa: E402

LEFT, RIGHT = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]


def cameras(S, dev):
    """-> (cam_rows (S, 16) float64, params (S, 2) float32, transforms (S, 14) float64) on `dev`: four synthetic cameras round-robin."""
    import numpy as np
    import torch
    import ray3d_amd
    cams = [ray3d_amd.synthetic_camera(yaw, 4.5, -12.0, name="cam%d" % i) for i, yaw in enumerate((20, 110, 200, 290))]
    pick = [cams[s % 4] for s in range(S)]
    rows = np.stack([c.cam_row(distortion=True) for c in pick])
    params = np.stack([np.asarray(c.param(), dtype=np.float32) for c in pick])
    trans = np.stack([c.stream_pose_row() for c in pick])
    return torch.from_numpy(rows).to(dev), torch.from_numpy(params).to(dev), torch.from_numpy(trans).to(dev)


def torch_tail(poses, x_row, rows, trans):
    """(S, J, 3) float32 poses -> (world, reproj, quality) with torch ops, float64, the stated arithmetic."""
    import torch
    p = poses.double()
    R, T, h = trans[:, :9].reshape(-1, 3, 3), trans[:, None, 9:12], trans[:, None, 12]
    world = torch.matmul(p, R.transpose(1, 2)) + T
    fx, fy, c, sn = rows[:, None, 0], rows[:, None, 1], rows[:, None, 4], rows[:, None, 5]
    yy, z = p[..., 1] + h, p[..., 2]
    zc = sn * yy + c * z
    a, b = p[..., 0] / zc, (c * yy - sn * z) / zc
    r = x_row.double()
    du, dv = fx * (a - r[..., 0]), fy * (b - (c * r[..., 1] - sn * r[..., 2]))
    res = torch.sqrt(du * du + dv * dv)
    return world, res, torch.stack([res.mean(1), res.max(1).values], 1)


def timed(sides, ticks, reps, warm, dev):
    """`warm` seconds of ticks (all sides in turn), then reps x (every side in turn: `ticks` ticks between two device events)
    -> per side {median, min, max} of ms per tick."""
    import torch
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm:
        for run in sides:
            for _ in range(5):
                run()
        torch.cuda.synchronize(dev)
    acc = [[] for _ in sides]
    for _ in range(reps):
        for run, a in zip(sides, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(ticks):
                run()
            e1.record()
            torch.cuda.synchronize(dev)
            a.append(e0.elapsed_time(e1) / ticks)
    return [{"median_ms": round(statistics.median(a), 4), "min_ms": round(min(a), 4), "max_ms": round(max(a), 4),
             "reps_ms": [round(v, 4) for v in a]} for a in acc]


def one(lifter, S, ticks, reps, warm, dev):
    import torch
    import ray3d_amd
    rf = lifter.receptive_field()
    rows, params, trans = cameras(S, dev)
    gen = torch.Generator(device="cpu").manual_seed(S)
    frames = torch.rand((rf + 4, S, J, 3), generator=gen) - 0.5
    frames[..., 2] = 1.0
    frames = frames.to(dev)                    # the ticks' new frames (rays), device-resident
    at = [0]

    def new_frame():
        at[0] = (at[0] + 1) % frames.shape[0]
        return frames[at[0]]

    def lifters(**options):
        pair = [ray3d_amd.OnlineLifter(lifter, S, flip=True, kps_left=LEFT, kps_right=RIGHT, device=dev, **options) for _ in range(2)]
        for ol in pair:
            ol.set_cameras(rows if options else None, params, trans if options else None)
        pair[1].capture()
        return pair

    a_eager, a_cap = lifters()
    b_eager, b_cap = lifters(world=True, quality=True)
    row = rf - 1 - a_eager.lag

    def torch_eager():
        poses, _ = a_eager.step(new_frame(), check=False)
        return (poses,) + torch_tail(poses, a_eager.x[:, row], rows, trans)

    # A captured: the step's own graph, then a graph around the tail that reads the step's captured pose buffer
    with torch.no_grad():
        static = a_cap._captured[0][:, 0]
        torch_tail(static, a_cap.x[:, row], rows, trans)
        torch.cuda.synchronize(dev)
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                tail_c = torch_tail(static, a_cap.x[:, row], rows, trans)
    torch.cuda.synchronize(dev)

    def torch_captured():
        poses, _ = a_cap.step(new_frame(), check=False)
        g.replay()
        return (poses,) + tail_c

    def call(ol):
        poses, _, extras = ol.step(new_frame(), check=False)
        return poses, extras["world"], extras["reproj"], extras["quality"]

    sides = [torch_eager, torch_captured, lambda: call(b_eager), lambda: call(b_cap)]
    with torch.no_grad():
        for t in range(rf + 2):                # the same frames through all four (every stream emits from tick `lag` on)
            outs = []
            for run in sides:
                at[0] = t - 1
                outs.append([v.clone() for v in run()])
        torch.cuda.synchronize(dev)
        ref = outs[2]
        same = {"poses_bit_equal": [bool(torch.equal(o[0], ref[0])) for o in outs],
                "worst_world_difference_m": [float((o[1] - ref[1]).abs().max()) for o in outs],
                "worst_residual_difference_px": [float((o[2] - ref[2]).abs().nan_to_num(0.0).max()) for o in outs],
                "median_residual_px": float(ref[2].nan_to_num(0.0).median())}
        clock0 = lifter.last_clock_ghz(dev)
        res = timed(sides, ticks, reps, warm, dev)
    lifter.check_status(dev)
    a_cap.release(), b_cap.release()
    del g
    torch.cuda.synchronize(dev)
    lifter.release_prepared()
    te, tc, ce, cc = res
    return {"receptive_field": rf, "streams": S, "torch_eager": te, "torch_captured": tc, "call_eager": ce, "call_captured": cc,
            "ratio_call_over_torch_eager": round(ce["median_ms"] / te["median_ms"], 4),
            "ratio_call_over_torch_captured": round(cc["median_ms"] / tc["median_ms"], 4),
            "saved_us_per_tick_eager": round(1e3 * (te["median_ms"] - ce["median_ms"]), 1),
            "saved_us_per_tick_captured": round(1e3 * (tc["median_ms"] - cc["median_ms"]), 1),
            "outputs_against_call_eager (torch_eager, torch_captured, call_eager, call_captured)": same,
            "shader_clock_ghz_before_after": [clock0, lifter.last_clock_ghz(dev)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_finish_ab.json"))
    ap.add_argument("--streams", default="1,8,32,256")
    ap.add_argument("--arch", default="3,3,3,3,3")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=float, default=2.0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("online_finish_ab.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lifter = make_lifter(args.arch, dev)
    rows = []
    for S in (int(v) for v in args.streams.split(",")):
        rows.append(one(lifter, S, args.ticks, args.reps, args.warm, dev))
        print(json.dumps(rows[-1]), flush=True)
    head = {"what": "ms per tick of a live caller that wants poses, world poses and the re-projection residual: OnlineLifter.step + a torch "
                    "tail, against OnlineLifter(world=True, quality=True).step (one r3d_streams_poses launch); eager and captured",
            "timing": "%g s of ticks first, then device events around %d ticks, four sides alternating, %d repetitions: median / min / max "
                      "of ms per tick" % (args.warm, args.ticks, args.reps),
            "device": torch.cuda.get_device_name(dev), "rows": rows}
    return write_out(args.out, head)


if __name__ == "__main__":
    sys.exit(main())
