#!/usr/bin/env python3
"""A/B of lifting a shard of clips clip by clip (evaluate_clips_batched(finish=True): forward_clip per clip, call sizes rounded up
per clip) against the pooled path (pool_below=: one r3d_clips_windows gather and one full-batch forward per 4096 windows), RF 243,
17 joints, flip on, synthetic weights (ray3d_amd.synth), seeded synthetic shards:

  (a) `short`:  2 000 clips of lengths U(40, 400), seed 1 - per clip against everything pooled;
  (b) `long`:   the 240-clip U(1000, 6000) set of the other A/B tools, seed 0 - per clip against everything pooled;
      `gather`: r3d_clips_windows alone at 4096 windows per call on shard (a)'s pool, plain and flip runs: device events around 20
                calls, GB/s = bytes moved by the shapes (batch * RF * J * F * 4 read and as many written) over the time;
      `sweep`:  (a) + (b) mixed, pool_below in {128, 256, 512, 1024, 2048, everything} against the per-clip path.

Every side is a whole pass (upload, lift, finish, metrics, reduce) timed on the host clock with the device synchronised before it
starts and before it stops, the sides alternating in one process, one untimed round first, 5 repetitions each; mean, min, max and
standard deviation are kept, and with every ratio the run-to-run spread of both sides.  No speed threshold: the verdict says
whether the two ranges overlap.  The pooled clips' rows are checked against the per-clip rows at 2e-5 * max(1, |row|) on the
per-frame means (the pooled windows run the materialised-window kernels, the clips the clip kernels).
usage:  python tools/clips_windows_ab.py            every step in a fresh process of its own under its own time limit, stopping at
                                                    the first that fails, then profiles/clips_windows_ab.json is written
        python tools/clips_windows_ab.py --step S   one step (short | long | gather | sweep): writes measure_out/clips_windows_ab.S.json
        [--out FILE] [--clips N] [--reps R]         another result file; a smaller run (rehearsals; --clips scales both shards)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_ab_common as ab
from clips_ab_common import H36M_LEFT, H36M_RIGHT, alternate, make_set, ranges_overlap, verdict

TOOL = "clips_windows_ab"
STEPS = (("short", 420), ("long", 420), ("gather", 240), ("sweep", 900))      # (step, its time limit in seconds)
RF = 243
EVERYTHING = 10 ** 9
SWEEP = (128, 256, 512, 1024, 2048, EVERYTHING)


def shard(which, n_clips):
    """(a): 2000 / 240 of `n_clips` short clips; (b): `n_clips` long ones; mixed: both, the short ones first."""
    short = lambda: make_set(max(1, n_clips * 2000 // 240), seed=1, shortest=40, longest=400)      # noqa: E731
    if which == "short":
        return short()
    if which == "long":
        return make_set(n_clips)
    both = short() + make_set(n_clips)
    from ray3d_amd import evaluate
    return [evaluate.Clip(c.camera, c.rays, c.gt_norm, c.action, i) for i, c in enumerate(both)]


def close_rows(a, b):
    """The per-frame means of two row sets within 2e-5 * max(1, |row|): (agree, worst difference)."""
    import numpy as np
    ga, gb = (t[:, 3:].cpu().numpy() / t[:, 2:3].cpu().numpy() for t in (a, b))
    fin = np.isfinite(gb)
    worst = float(np.abs(ga[fin] - gb[fin]).max())
    return bool(np.isfinite(ga[fin]).all() and worst <= 2e-5 * max(1.0, float(np.abs(gb[fin]).max()))), worst


def spread(t):
    return round((t["max_ms"] - t["min_ms"]) / t["mean_ms"], 4)


def compare(a, b, frames, name="pooled"):
    for t in (a, b):
        t["poses_per_s"] = round(frames / t["mean_ms"] * 1e3, 1)
    return {"per_clip": a, name: b, "ratio_%s_over_per_clip" % name: round(b["mean_ms"] / a["mean_ms"], 4),
            "spread_per_clip": spread(a), "spread_%s" % name: spread(b), "ranges_overlap": ranges_overlap(a, b), "verdict": verdict(a, b, name)}


def step_pass(which, n_clips, reps):
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = shard(which, n_clips)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter = ab.make_lifter(clips, dev)
    kw = dict(flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    keep = {}

    def per_clip():
        keep["a"] = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, RF, dev, finish=True, **kw)

    def pooled():
        keep["b"] = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, RF, dev, pool_below=EVERYTHING, **kw)

    with torch.no_grad():
        a, b = alternate([per_clip, pooled], reps, dev, wall=True)
    lifter.check_status(dev)
    ok, worst = close_rows(keep["b"][2], keep["a"][2])
    res = compare(a, b, frames)
    res["what"] = "whole pass (upload, lift, finish, metrics, reduce), RF 243, flip on: %d clips, %d frames, no lanes" % (len(clips), frames)
    res["rows_agree"], res["worst_row_difference_m"] = ok, worst
    res["average_mm"] = {k: [float(v) for v in keep[k][1]] for k in sorted(keep)}
    if not ok:
        raise SystemExit("%s: the rows of the two paths differ by more than the bound: %s" % (which, json.dumps(res)))
    return res


def step_gather(n_clips, reps):
    import numpy as np
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = shard("short", n_clips)
    J, F, batch, calls = 17, 3, 4096, 20
    src = torch.from_numpy(np.concatenate([c.rays for c in clips], axis=0)).to(dev)
    perm = evaluate.mirror_permutation(J, H36M_LEFT, H36M_RIGHT)
    run_param = torch.from_numpy(np.stack([np.asarray(c.camera.param(), dtype=np.float32) for c in clips])).to(dev)
    x = torch.empty((batch, RF, J, F), device=dev)
    param = torch.empty((batch, 2), device=dev)
    status = torch.zeros((len(clips),), dtype=torch.int32, device=dev)
    out = {"what": "r3d_clips_windows alone, %d calls of %d windows between two device events: RF 243, J 17, F 3, %d runs" % (calls, batch, len(clips)),
           "bytes_per_call": 2 * batch * RF * J * F * 4}
    for flip in (False, True):
        table, _, total = evaluate.clip_window_table(clips, RF, False, flip, 4096)
        table_dev = evaluate._to_device_bytes(table, dev)
        starts = [(i * batch) % max(1, total - batch) for i in range(calls)]

        def run():
            for w0 in starts:
                evaluate.shard_windows_hip(src, table_dev, len(clips), run_param, w0, batch, RF, x=x, param=param, perm=perm, status=status)

        (t,) = alternate([run], reps, dev)
        assert not status.cpu().numpy().any()
        t["gb_per_s"] = round(out["bytes_per_call"] * calls / (t["mean_ms"] * 1e-3) / 1e9, 1)
        t["ms_per_call"] = round(t["mean_ms"] / calls, 4)
        out["flip%d" % flip] = t
    return out


def step_sweep(n_clips, reps):
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = shard("mixed", n_clips)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter = ab.make_lifter(clips, dev)
    kw = dict(flip=True, kps_left=H36M_LEFT, kps_right=H36M_RIGHT)
    keep = {}

    def side(below):
        def run():
            keep[below] = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, RF, dev, finish=True, pool_below=below, **kw)
        return run

    with torch.no_grad():
        times = alternate([side(None)] + [side(b) for b in SWEEP], reps, dev, wall=True)
    lifter.check_status(dev)
    out = {"what": "whole pass on shards (a) + (b) mixed, RF 243, flip on: %d clips, %d frames; pool_below against the per-clip path"
                   % (len(clips), frames), "per_clip": times[0]}
    for below, t in zip(SWEEP, times[1:]):
        ok, worst = close_rows(keep[below][2], keep[None][2])
        res = compare(dict(times[0]), t, frames)
        res.pop("per_clip")
        res["pooled_clips"] = sum(1 for c in clips if c.rays.shape[0] < below)
        res["rows_agree"], res["worst_row_difference_m"] = ok, worst
        if not ok:
            raise SystemExit("sweep %s: the rows differ by more than the bound: %s" % (below, json.dumps(res)))
        out["pool_below_%s" % ("everything" if below == EVERYTHING else below)] = res
    return out


def main():
    ap = ab.parser(__doc__, TOOL, STEPS)
    args = ap.parse_args()
    if args.step in ("short", "long"):
        return ab.run_step(TOOL, args, step_pass(args.step, args.clips, args.reps))
    if args.step:
        return ab.run_step(TOOL, args, (step_gather if args.step == "gather" else step_sweep)(args.clips, args.reps))
    head = ab.header(args)
    head["set"] = "(a) %d clips U(40, 400) seed 1; (b) %d clips U(1000, 6000) seed 0" % (max(1, args.clips * 2000 // 240), args.clips)
    head["timing"] = "host clock, device synchronised before start and stop, sides alternating, one untimed round first"
    return ab.run_steps(TOOL, STEPS, args, head)


if __name__ == "__main__":
    sys.exit(main())
