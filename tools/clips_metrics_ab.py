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
        [--clips N] [--reps R] shrink the run (rehearsals)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("metrics", 300), ("pass", 420), ("pass-lanes2", 420))      # (step, its time limit in seconds)
PART_DIR = os.path.join(ROOT, "measure_out")
OUT = os.path.join(ROOT, "profiles", "clips_metrics_ab.json")


def stats(ms):
    import numpy as np
    a = np.asarray(ms, dtype=np.float64)
    return {"mean_ms": round(float(a.mean()), 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
            "std_ms": round(float(a.std(ddof=1)) if a.size > 1 else 0.0, 4), "reps_ms": [round(float(v), 4) for v in a]}


def verdict(a, b):
    """b against a, beyond the spread of the repetitions: the ranges of the two sides must not overlap."""
    if b["max_ms"] < a["min_ms"]:
        return "batched faster (ranges do not overlap)"
    if b["min_ms"] > a["max_ms"]:
        return "batched SLOWER (ranges do not overlap)"
    return "no difference beyond the spread (ranges overlap)"


def make_set(n_clips, seed=0):
    """bench.py's evaluation stand-in: clip lengths ~ U(1000, 6000), four cameras, 15 actions."""
    import numpy as np
    import ray3d_amd
    from ray3d_amd import evaluate
    rng = np.random.default_rng(seed)
    lengths = [int(rng.integers(1000, 6001)) for _ in range(n_clips)]
    cams = [ray3d_amd.synthetic_camera(yaw, 4.5, -12.0, name="cam%d" % i) for i, yaw in enumerate((20, 110, 200, 290))]
    clips = []
    for i, n in enumerate(lengths):
        r = np.random.default_rng([seed, i])
        cam = cams[i % 4]
        world = r.normal(0, 0.3, (1, 17, 3)) + np.array([0, 0, 1.0]) + 0.02 * np.cumsum(r.normal(0, 1.0, (n, 1, 3)), axis=0) \
            + r.normal(0, 0.02, (n, 17, 3))
        rays = cam.rays_from_uv(cam.project(world)).astype(np.float32)
        clips.append(evaluate.Clip(cam, rays, cam.world2normalized(world).astype(np.float32), "A%d" % (i % 15), i))
    return clips


def alternate(run_a, run_b, reps, dev):
    """reps x (a, b), each timed by a pair of device events on the current stream; one untimed round first."""
    import torch
    run_a(), run_b()
    torch.cuda.synchronize(dev)
    ta, tb = [], []
    for _ in range(reps):
        for run, acc in ((run_a, ta), (run_b, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(dev))
            run()
            e1.record(torch.cuda.current_stream(dev))
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return stats(ta), stats(tb)


def step_metrics(n_clips, reps):
    import numpy as np
    import torch
    from ray3d_amd import evaluate
    dev = torch.device("cuda", 0)
    clips = make_set(n_clips)
    aid = {a: i for i, a in enumerate(sorted(set(c.action for c in clips)))}
    table, first, total, longest = evaluate.clip_table(clips)
    table_dev = torch.from_numpy(table.view(np.uint8)).to(dev)
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

    a, b = alternate(per_clip, one_call, reps, dev)
    equal = bool(torch.equal(rows_a.view(torch.int64), rows_b.view(torch.int64)))
    res = {"what": "metrics only, predictions resident: %d clips, %d frames, J 17" % (len(clips), total),
           "per_clip": a, "batched": b, "rows_bit_equal": equal, "verdict": verdict(a, b),
           "launches": {"per_clip": "%d x (metrics + sum + row copy)" % len(clips), "batched": "2"}}
    if not equal:
        raise SystemExit("the rows of the two paths differ: %s" % json.dumps(res))
    return res


def step_pass(n_clips, reps, lanes):
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import evaluate, synth
    from ray3d_amd.spec import config_from_dicts
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    for m, kind, seed in ((pos, "pos", 1), (trj, "trj", 2)):
        cfg = config_from_dicts(mc, kind)
        ray3d_amd.load_weight(m, {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(cfg, seed=seed).items()})
        m.eval()
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    clips = make_set(n_clips)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter.prepare(sorted(set(b for c in clips for b in lifter.clip_batch_sizes(c.rays.shape[0]))), dev)
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
        a, b = alternate(per_clip, batched, reps, dev)
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--clips", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    os.makedirs(PART_DIR, exist_ok=True)
    part = lambda s: os.path.join(PART_DIR, "clips_metrics_ab.%s.json" % s)
    if args.step:
        res = step_metrics(args.clips, args.reps) if args.step == "metrics" else \
            step_pass(args.clips, args.reps, 2 if args.step == "pass-lanes2" else 0)
        with open(part(args.step), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({args.step: res}))
        return 0
    merged = {"set": "%d clips, lengths U(1000, 6000), seed 0" % args.clips, "repetitions": args.reps,
              "timing": "device events around each side, sides alternating, one untimed round first"}
    for step, limit in STEPS:                     # a fresh process per step; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--clips", str(args.clips), "--reps", str(args.reps)]).returncode
        if rc != 0:
            print("step %s ended with status %d: stopping" % (step, rc), file=sys.stderr)
            return rc
        merged[step] = json.load(open(part(step)))
    with open(OUT, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print("wrote", OUT)
    return 0


if __name__ == "__main__":
    sys.exit(main())
