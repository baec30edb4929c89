#!/usr/bin/env python3
"""A/B of the measuring side of the clip evaluation: one r3d_clip_metrics call per clip against ONE r3d_clips_metrics call per
shard, on the H36M-shaped synthetic set (240 clips, lengths U(1000, 6000), seed 0; weights from ray3d_amd.synth).

  (a) `metrics`:     metrics only, on resident predictions - the per-clip loop as bench.py's evaluation pass issues it
                     (evaluate.clip_partials_hip with resident ground truth, rows written on the device) against
                     evaluate.shard_metrics_hip; the rows of both must be equal bit for bit.
  (b) `pass`:        the whole pass, evaluate.evaluate_clips against evaluate.evaluate_clips_batched (RF 243), without lanes;
      `pass-lanes2`: the same with R3D_OPT_LANES = 2 (the per-clip path lifts every clip on the next lane and joins before it
                     measures; the batched path joins once, before its one metrics call).

Device-event times, 5 repetitions of each side, the two sides alternating; mean, min, max and standard deviation are kept.
usage:  python tools/clips_metrics_ab.py            every step in a fresh process of its own under its own time limit, stopping
                                                    at the first that fails (as `timeout ... --step metrics && timeout ... --step
                                                    pass && ...` would), then profiles/clips_metrics_ab.json is written
        python tools/clips_metrics_ab.py --step S   one step (metrics | pass | pass-lanes2): writes measure_out/clips_metrics_ab.S.json
        [--out FILE] [--clips N] [--reps R] another result file; a smaller run (rehearsals) - tools/clips_ab_common.py."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_ab_common as ab
from clips_ab_common import alternate, make_set, verdict

TOOL = "clips_metrics_ab"
STEPS = (("metrics", 300), ("pass", 420), ("pass-lanes2", 420))      # (step, its time limit in seconds)


def step_metrics(n_clips, reps):
    import numpy as np
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = make_set(n_clips)
    aid = {a: i for i, a in enumerate(sorted(set(c.action for c in clips)))}
    table, first, total, longest = evaluate.clip_table(clips)
    table_dev = evaluate._to_device_bytes(table, dev)
    gt_all = torch.from_numpy(np.concatenate([c.gt_norm for c in clips], axis=0)).to(dev)
    noise = torch.from_numpy(np.random.default_rng(1).normal(0, 0.03, tuple(gt_all.shape)).astype(np.float32)).to(dev)
    pred_all = (gt_all + noise).reshape(total, 1, 17, 3).contiguous()
    preds = [pred_all[first[k]:first[k] + c.rays.shape[0]] for k, c in enumerate(clips)]
    gts = [gt_all[first[k]:first[k] + c.rays.shape[0]] for k, c in enumerate(clips)]
    headers = [(k, aid[c.action], c.rays.shape[0]) for k, c in enumerate(clips)]
    rows_a, rows_b = evaluate.partial_rows(headers, dev), evaluate.partial_rows(headers, dev)

    def per_clip():
        for k, c in enumerate(clips):
            evaluate.clip_partials_hip(preds[k], c, aid[c.action], gt_dev=gts[k], out=rows_a[k])

    def one_call():
        evaluate.shard_metrics_hip(pred_all, gt_all, table_dev, len(clips), total, longest, rows_b)

    a, b = alternate([per_clip, one_call], reps, dev)
    equal = bool(torch.equal(rows_a.view(torch.int64), rows_b.view(torch.int64)))
    res = {"what": "metrics only, predictions resident: %d clips, %d frames, J 17" % (len(clips), total),
           "per_clip": a, "batched": b, "rows_bit_equal": equal, "verdict": verdict(a, b),
           "launches": {"per_clip": "%d x (metrics + sum + row copy)" % len(clips), "batched": "2"}}
    if not equal:
        raise SystemExit("the rows of the two paths differ: %s" % json.dumps(res))
    return res


def step_pass(n_clips, reps, lanes):
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = make_set(n_clips)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter = ab.make_lifter(clips, dev)
    if lanes:
        lifter.set_lanes(lanes, dev)

    def lift_joined(padded, prow):
        # the per-clip path measures right behind the forward: the clip goes to the next lane and the caller's stream joins it
        with lifter.lane():
            out = lifter.forward_clip(padded, prow)
        lifter.join_lanes()
        return out

    keep = {}

    def per_clip():
        keep["a"] = evaluate.evaluate_clips(lift_joined if lanes else lifter.forward_clip, clips, 243, dev)

    def batched():
        keep["b"] = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 243, dev)

    with torch.no_grad():
        a, b = alternate([per_clip, batched], reps, dev)
    lifter.check_status(dev)
    equal = bool(torch.equal(keep["a"][2].view(torch.int64), keep["b"][2].view(torch.int64)))
    res = {"what": "whole pass (upload, lift, measure, reduce), RF 243: %d clips, %d frames, lanes %d" % (len(clips), frames, lanes),
           "per_clip": dict(a, poses_per_s=round(frames / a["mean_ms"] * 1e3, 1)),
           "batched": dict(b, poses_per_s=round(frames / b["mean_ms"] * 1e3, 1)),
           "rows_bit_equal": equal, "action_average_mm": {"per_clip": keep["a"][1], "batched": keep["b"][1]}, "verdict": verdict(a, b)}
    if lanes:
        lifter.set_lanes(0, dev)
    if not equal:
        raise SystemExit("the rows of the two paths differ: %s" % json.dumps(res))
    return res


def main():
    args = ab.parser(__doc__, TOOL, STEPS).parse_args()
    if args.step:
        return ab.run_step(TOOL, args, step_metrics(args.clips, args.reps) if args.step == "metrics" else
                           step_pass(args.clips, args.reps, 2 if args.step == "pass-lanes2" else 0))
    return ab.run_steps(TOOL, STEPS, args, ab.header(args))


if __name__ == "__main__":
    sys.exit(main())
