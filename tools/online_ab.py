#!/usr/bin/env python3
"""A/B of one tick of a live caller - S cameras, one new frame of raw pixel keypoints each, the newest pose back - on synthetic
weights (ray3d_amd.synth), distorted synthetic cameras, S in {1, 4, 32, 256, 1024}, for the RF-243 pair (ARCHITECTURE 3,3,3,3,3)
and an RF-9 pair (3,3):

  `history`: what a live caller had before r3d_streams_step - a device-resident (S, RF, J, 2) pixel history rolled with torch ops
             every tick (torch.roll + the new frame into the last row), then forward_uv on it (the pre-pass encodes all RF frames
             of every stream again, 16-double camera rows);
  `streams`: OnlineLifter.step(check=False) - r3d_streams_step (the new frame encoded once into the ring, the window gathered) and
             the plain forward.

Both eager and captured into a hipGraph (torch.cuda.graph around the history tick; OnlineLifter.capture()).  The new frame is a
device tensor on both sides.  After RF ticks on the same frames the two sides' poses are compared (they run the same encoding
routine and the same forward: expected equal bit for bit; the result is recorded, not asserted).  `step_alone`: r3d_streams_step's
two launches without the forward.

Timing: a side's run is TICKS ticks on a host clock with the device synchronised before it starts and before it stops; the four
sides alternate, one untimed round first, REPS repetitions; the MEDIAN, min and max of ms per tick are kept.  The shader clock of
the last single-launch forward (r3d_last_clock) is recorded before and after each configuration.  No ratio is a pass condition.
usage:  python tools/online_ab.py [--out FILE] [--streams 1,4,32] [--ticks N] [--reps R] [--configs rf243,rf9]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clips_ab_common import DIST, write_out      # noqa: E402

CONFIGS = {"rf243": "3,3,3,3,3", "rf9": "3,3"}
J = 17


def make_lifter(arch, dev):
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import synth
    from ray3d_amd.spec import config_from_dicts
    mc = ray3d_amd.default_model_config(ARCHITECTURE=arch)
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    for m, kind, seed in ((pos, "pos", 1), (trj, "trj", 2)):
        cfg = config_from_dicts(mc, kind)
        ray3d_amd.load_weight(m, {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(cfg, seed=seed).items()})
        m.eval()
    return ray3d_amd.Ray3DLifter(pos, trj).eval()


def cameras(S, dev):
    """-> (cam_rows (S, 16) float64, params (S, 2) float32) on `dev`: four distorted synthetic cameras dealt round-robin."""
    import numpy as np
    import torch
    import ray3d_amd
    cams = []
    for i, yaw in enumerate((20, 110, 200, 290)):
        c = ray3d_amd.synthetic_camera(yaw, 4.5, -12.0, name="cam%d" % i)
        cams.append(ray3d_amd.Camera(c.K, c.Rw2c, c.Tw2c, dist_coeff=DIST[i], undistort=True, name="cam%d" % i, res_w=1024, res_h=1024))
    rows = np.stack([cams[s % 4].cam_row(distortion=True) for s in range(S)])
    params = np.stack([np.asarray(cams[s % 4].param(), dtype=np.float32) for s in range(S)])
    return torch.from_numpy(rows).to(dev), torch.from_numpy(params).to(dev)


def timed(sides, ticks, reps, dev):
    """reps x (every side in turn: `ticks` ticks on the host clock between two device synchronisations), one untimed round first
    -> per side {median, min, max} of ms per tick."""
    import torch
    for run in sides:
        for _ in range(3):
            run()
    torch.cuda.synchronize(dev)
    acc = [[] for _ in sides]
    for _ in range(reps):
        for run, a in zip(sides, acc):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(ticks):
                run()
            torch.cuda.synchronize(dev)
            a.append((time.perf_counter() - t0) * 1e3 / ticks)
    return [{"median_ms": round(statistics.median(a), 4), "min_ms": round(min(a), 4), "max_ms": round(max(a), 4),
             "reps_ms": [round(v, 4) for v in a]} for a in acc]


def one(lifter, name, S, ticks, reps, dev):
    import torch
    import ray3d_amd
    from ray3d_amd import _capi
    rf = lifter.receptive_field()
    rows, params = cameras(S, dev)
    gen = torch.Generator(device="cpu").manual_seed(S)
    frames = (1024.0 * torch.rand((rf + 4, S, J, 2), generator=gen)).to(dev)      # the ticks' new frames, device-resident
    at = [0]

    def new_frame():
        at[0] = (at[0] + 1) % frames.shape[0]
        return frames[at[0]]

    # ---- the history side: eager, and one tick captured around a fixed `fresh` buffer
    hist = frames[0].unsqueeze(1).repeat(1, rf, 1, 1).contiguous()
    lifter.prepare([S], dev)

    def history_tick(fresh, h=hist):
        h.copy_(torch.roll(h, -1, 1))
        h[:, -1] = fresh
        return lifter.forward_uv(h, rows, params)

    hist_c, fresh_c = hist.clone(), frames[0].clone()
    with torch.no_grad():
        history_tick(fresh_c, hist_c)                      # (the workspace exists before the capture)
        torch.cuda.synchronize(dev)
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out_c = history_tick(fresh_c, hist_c)
    torch.cuda.synchronize(dev)

    def history_captured():
        fresh_c.copy_(new_frame())
        g.replay()
        return out_c

    # ---- the streams side
    eager = ray3d_amd.OnlineLifter(lifter, S, encoding="ray", device=dev)
    cap = ray3d_amd.OnlineLifter(lifter, S, encoding="ray", device=dev)
    for ol in (eager, cap):
        ol.set_cameras(rows, params)
    cap.capture()

    # ---- the same RF + 2 frames through all four: their poses (all streams emit from tick `lag` on; the windows are full after RF)
    hist.copy_(frames[0].unsqueeze(1).expand(-1, rf, -1, -1))
    hist_c.copy_(hist)
    with torch.no_grad():
        for t in range(rf + 2):
            f = frames[t]
            a = history_tick(f)
            fresh_c.copy_(f)
            g.replay()
            b, _ = eager.step(f, check=False)
            c, emit = cap.step(f, check=False)
    torch.cuda.synchronize(dev)
    assert int(eager.status.abs().sum()) == 0 and int(cap.status.abs().sum()) == 0 and bool((emit >= 0).all())
    same = {"history_captured": bool(torch.equal(a, out_c)), "streams": bool(torch.equal(a[:, 0], b)), "streams_captured": bool(torch.equal(a[:, 0], c))}
    worst = float(max((a[:, 0] - b).abs().max(), (a[:, 0] - c).abs().max(), (a - out_c).abs().max()))

    clock0 = lifter.last_clock_ghz(dev)
    with torch.no_grad():
        res = timed([lambda: history_tick(new_frame()), history_captured, lambda: eager.step(new_frame(), check=False),
                     lambda: cap.step(new_frame(), check=False)], ticks, reps, dev)
        # r3d_streams_step alone: its two launches, no forward
        stream = torch.cuda.current_stream(dev).cuda_stream
        eager.action.fill_(_capi.R3D_STREAM_PUSH)

        def step_alone():
            _capi.streams_step(eager.state.data_ptr(), S, rf, eager.lag, J, 3, eager.encoding, eager.frame.data_ptr(), eager.cam.data_ptr(),
                               eager.action.data_ptr(), eager.x.data_ptr(), None, None, eager.emit.data_ptr(), eager.status.data_ptr(), stream)
        (alone,) = timed([step_alone], ticks, reps, dev)
    lifter.check_status(dev)
    cap.release()
    del g
    torch.cuda.synchronize(dev)
    lifter.release_prepared()
    h, hc, s, sc = res
    return {"config": name, "receptive_field": rf, "streams": S, "history": h, "history_captured": hc, "streams_step": s,
            "streams_step_captured": sc, "step_alone": alone,
            "ratio_streams_over_history": round(s["median_ms"] / h["median_ms"], 4),
            "ratio_captured_streams_over_captured_history": round(sc["median_ms"] / hc["median_ms"], 4),
            "poses_equal_to_history_eager": same, "worst_pose_difference_m": worst,
            "window_bytes_rebuilt_per_stream_and_tick_history": rf * J * 2 * 4, "shader_clock_ghz_before_after": [clock0, lifter.last_clock_ghz(dev)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_ab.json"))
    ap.add_argument("--streams", default="1,4,32,256,1024")
    ap.add_argument("--configs", default="rf243,rf9")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("online_ab.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    for name in args.configs.split(","):
        lifter = make_lifter(CONFIGS[name], dev)
        for S in (int(v) for v in args.streams.split(",")):
            rows.append(one(lifter, name, S, args.ticks, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    head = {"what": "ms per tick of a live caller: pixel history rolled with torch ops + forward_uv, against OnlineLifter.step; eager and captured",
            "timing": "host clock around %d ticks, device synchronised before start and stop, four sides alternating, one untimed round first, "
                      "%d repetitions: median / min / max of ms per tick" % (args.ticks, args.reps),
            "device": torch.cuda.get_device_name(dev), "rows": rows}
    return write_out(args.out, head)


if __name__ == "__main__":
    sys.exit(main())
