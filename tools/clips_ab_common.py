"""What the A/B tools of the calls over a whole shard of clips share (tools/clips_{metrics,encode,valid,poses,windows}_ab.py): the
240-clip stand-in sets, the RF-243 lifter on synthetic weights, the alternating timed loop, the statistics and the verdict, and
the runner - every step in a fresh process of its own under its own time limit, the first failure ending the run.
Common options: --step S (one step: writes measure_out/<tool>.S.json), --clips N and --reps R (a smaller run, rehearsals),
--out PATH (the merged result elsewhere than profiles/<tool>.json, so that a rerun does not overwrite the recorded file)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PART_DIR = os.path.join(ROOT, "measure_out")
H36M_LEFT, H36M_RIGHT = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
DIST = ((-0.2075, 0.2470, -0.0015, -0.0010, -0.0031), (-0.1942, 0.2404, -0.0027, -0.0016, 0.0068),
        (-0.2083, 0.2556, -0.0024, 0.0015, -0.0008), (-0.1983, 0.2183, -0.0009, -0.0029, -0.0089))    # k1 k2 p1 p2 k3, H36M-sized


def stats(ms):
    import numpy as np
    a = np.asarray(ms, dtype=np.float64)
    return {"mean_ms": round(float(a.mean()), 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
            "std_ms": round(float(a.std(ddof=1)) if a.size > 1 else 0.0, 4), "reps_ms": [round(float(v), 4) for v in a]}


def ranges_overlap(a, b):
    return not (b["max_ms"] < a["min_ms"] or b["min_ms"] > a["max_ms"])


def verdict(a, b, name="batched"):
    """b against a, beyond the spread of the repetitions: the ranges of the two sides must not overlap."""
    if b["max_ms"] < a["min_ms"]:
        return "%s faster (ranges do not overlap)" % name
    if b["min_ms"] > a["max_ms"]:
        return "%s SLOWER (ranges do not overlap)" % name
    return "no difference beyond the spread (ranges overlap)"


def baseline_entry(mine, runs):
    """This build's per-clip side against the per-clip side of another build's runs (their repetitions' range taken together)."""
    lo, hi = min(r["min_ms"] for r in runs), max(r["max_ms"] for r in runs)
    return {"what": "the per-clip path on a build of the parent commit, same session", "per_clip_runs": runs,
            "range_ms": [lo, hi], "per_clip_mean_within_baseline_range": lo <= mine["mean_ms"] <= hi,
            "per_clip_mean_not_above_baseline_range": mine["mean_ms"] <= hi,
            "per_clip_ranges_overlap": not (mine["max_ms"] < lo or mine["min_ms"] > hi)}


def make_set(n_clips, seed=0, pixels=False, shortest=1000, longest=6000):
    """bench.py's evaluation stand-in: clip lengths ~ U(1000, 6000) (or U(shortest, longest)), four cameras, 15 actions.  `pixels`:
    the same poses seen through distorted cameras (undistort=True), Clip.rays holding the RAW float32 pixels."""
    import numpy as np
    import ray3d_amd
    from ray3d_amd import evaluate
    rng = np.random.default_rng(seed)
    lengths = [int(rng.integers(shortest, longest + 1)) for _ in range(n_clips)]
    cams = []
    for i, yaw in enumerate((20, 110, 200, 290)):
        c = ray3d_amd.synthetic_camera(yaw, 4.5, -12.0, name="cam%d" % i)
        cams.append(ray3d_amd.Camera(c.K, c.Rw2c, c.Tw2c, dist_coeff=DIST[i], undistort=True, name="cam%d" % i, res_w=1024, res_h=1024)
                    if pixels else c)
    clips = []
    for i, n in enumerate(lengths):
        r = np.random.default_rng([seed, i])
        cam = cams[i % 4]
        world = r.normal(0, 0.3, (1, 17, 3)) + np.array([0, 0, 1.0]) + 0.02 * np.cumsum(r.normal(0, 1.0, (n, 1, 3)), axis=0) \
            + r.normal(0, 0.02, (n, 17, 3))
        uv = cam.project(world)
        rays = (cam.distort_points(uv) if pixels else cam.rays_from_uv(uv)).astype(np.float32)
        clips.append(evaluate.Clip(cam, rays, cam.world2normalized(world).astype(np.float32), "A%d" % (i % 15), i))
    return clips


def make_lifter(clips, dev):
    """The RF-243 pos + trj pair on synthetic weights, its schedules prepared for every batch size the clips are lifted in."""
    import numpy as np
    import torch
    import ray3d_amd
    from ray3d_amd import synth
    from ray3d_amd.spec import config_from_dicts
    torch.cuda.set_device(dev)
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    fac = ray3d_amd.Model(mc, {}, is_train=False)
    pos, trj = fac.get_pos_model(), fac.get_trj_model()
    for m, kind, seed in ((pos, "pos", 1), (trj, "trj", 2)):
        cfg = config_from_dicts(mc, kind)
        ray3d_amd.load_weight(m, {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(cfg, seed=seed).items()})
        m.eval()
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    lifter.prepare(sorted(set(b for c in clips for b in lifter.clip_batch_sizes(c.rays.shape[0]))), dev)
    return lifter


def alternate(sides, reps, dev, wall=False):
    """reps x (every side in turn), one untimed round first -> the statistics of each side.  Each run is timed by a pair of device
    events on the current stream - or, with `wall`, by a host clock with the device synchronised before it starts and stops."""
    import torch
    for run in sides:
        run()
    torch.cuda.synchronize(dev)
    times = [[] for _ in sides]
    for _ in range(reps):
        for run, acc in zip(sides, times):
            if wall:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize(dev)
                acc.append((time.perf_counter() - t0) * 1e3)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(dev))
            run()
            e1.record(torch.cuda.current_stream(dev))
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return [stats(t) for t in times]


def parser(doc, tool, steps):
    """The options every tool has; `tool` the tool's name (clips_*_ab), `steps` its ((step, time limit in seconds), ...)."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=[s for s, _ in steps])
    ap.add_argument("--clips", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", tool + ".json"))
    return ap


def header(args):
    return {"set": "%d clips, lengths U(1000, 6000), seed 0" % args.clips, "repetitions": args.reps,
            "timing": "device events around each side, sides alternating, one untimed round first"}


def run_step(tool, args, res):
    """What a --step process leaves: its result in measure_out/<tool>.<step>.json and on standard output."""
    os.makedirs(PART_DIR, exist_ok=True)
    with open(os.path.join(PART_DIR, "%s.%s.json" % (tool, args.step)), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({args.step: res}))
    return 0


def run_steps(tool, steps, args, merged, extra=(), after=None):
    """Every step of `steps` as a fresh process of tools/<tool>.py under its own time limit; the first that fails ends the run
    with its status.  The results go into `merged` by step name (`after(step, result)` may add to one), which is written to
    --out - or, with `merged` None, the only step's result itself is."""
    results = {}
    for step, limit in steps:
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "tools", tool + ".py"), "--step", step,
                             "--clips", str(args.clips), "--reps", str(args.reps)] + list(extra)).returncode
        if rc != 0:
            print("step %s ended with status %d: stopping, nothing written" % (step, rc), file=sys.stderr)
            return rc
        results[step] = json.load(open(os.path.join(PART_DIR, "%s.%s.json" % (tool, step))))
        if after is not None:
            after(step, results[step])
    return write_out(args.out, dict(merged, **results) if merged is not None else results[steps[0][0]])


def write_out(path, merged):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    print("wrote", path)
    return 0
