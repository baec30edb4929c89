#!/usr/bin/env python3
"""A/B of the input side of the clip evaluation FROM RAW PIXELS of distorted cameras, flip off, on the H36M-shaped synthetic set
(240 clips, lengths U(1000, 6000), seed 0, four cameras with H36M-sized Brown-Conrady coefficients, undistort=True; weights from
ray3d_amd.synth, RF 243):

  (a) per clip: evaluate.evaluate_clips with a lifter that calls forward_uv(padded, row16, prow) - every clip is edge-padded
      with NumPy, uploaded, and the pixel pre-pass runs in front of each of its forwards;
  (b) batched:  evaluate.evaluate_clips_batched(encode="ray") - the rank's pixels uploaded once, ONE r3d_clips_encode call,
      every clip lifted from its slice (forward_clip(n_windows=)), one r3d_clips_metrics call.

The rows of the two must be equal bit for bit.  Wall time per pass: a host clock around the whole pass, the device synchronised
before the clock starts and before it stops (the host steps - padding, pageable copies - are what differs); 5 repetitions of
each side, the two sides alternating, one untimed round first.  No threshold: the ratio is recorded.
usage:  python tools/clips_encode_ab.py            the pass in a fresh process of its own under a time limit (as `timeout ...
                                                   --step pass` would), then profiles/clips_encode_ab.json is written (--out: elsewhere)
        python tools/clips_encode_ab.py --step pass   the pass itself: writes measure_out/clips_encode_ab.pass.json
        [--clips N] [--reps R] shrink the run (rehearsals)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "clips_encode_ab.json")
PART = os.path.join(ROOT, "measure_out", "clips_encode_ab.pass.json")
LIMIT = 420          # seconds for the pass (12 passes of about 1.6 s, the schedules' preparation and the start of torch)
DIST = ((-0.2075, 0.2470, -0.0015, -0.0010, -0.0031), (-0.1942, 0.2404, -0.0027, -0.0016, 0.0068),
        (-0.2083, 0.2556, -0.0024, 0.0015, -0.0008), (-0.1983, 0.2183, -0.0009, -0.0029, -0.0089))    # k1 k2 p1 p2 k3, H36M-sized


def make_pixel_set(n_clips, seed=0):
    """clips_metrics_ab.make_set's poses seen through distorted cameras: Clip.rays holds the RAW float32 pixels."""
    import numpy as np
    import ray3d_amd
    from ray3d_amd import evaluate
    rng = np.random.default_rng(seed)
    lengths = [int(rng.integers(1000, 6001)) for _ in range(n_clips)]
    cams = []
    for i, yaw in enumerate((20, 110, 200, 290)):
        c = ray3d_amd.synthetic_camera(yaw, 4.5, -12.0)
        cams.append(ray3d_amd.Camera(c.K, c.Rw2c, c.Tw2c, dist_coeff=DIST[i], undistort=True, name="cam%d" % i, res_w=1024, res_h=1024))
    clips = []
    for i, n in enumerate(lengths):
        r = np.random.default_rng([seed, i])
        cam = cams[i % 4]
        world = r.normal(0, 0.3, (1, 17, 3)) + np.array([0, 0, 1.0]) + 0.02 * np.cumsum(r.normal(0, 1.0, (n, 1, 3)), axis=0) \
            + r.normal(0, 0.02, (n, 17, 3))
        px = cam.distort_points(cam.project(world)).astype(np.float32)
        clips.append(evaluate.Clip(cam, px, cam.world2normalized(world).astype(np.float32), "A%d" % (i % 15), i))
    return clips


def step_pass(args):
    import numpy as np
    import torch
    import ray3d_amd
    from clips_metrics_ab import stats, verdict
    from ray3d_amd import evaluate, synth
    from ray3d_amd.spec import config_from_dicts
    if not torch.cuda.is_available():
        raise SystemExit("clips_encode_ab measures on the GPU: none found")
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
    clips = make_pixel_set(args.clips)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter.prepare(sorted(set(b for c in clips for b in lifter.clip_batch_sizes(c.rays.shape[0]))), dev)
    rows16 = {id(c.camera): torch.from_numpy(c.camera.cam_row(distortion=True)).to(dev) for c in clips}
    current = {}

    class PerClip:
        """evaluate_clips hands the lifter (padded, param_row) only: the clips come in shard order, the camera row with them."""
        def __init__(self):
            order = evaluate.shard_clips([c.rays.shape[0] for c in clips], 1)[0]
            self.rows = [rows16[id(clips[i].camera)] for i in order]
            self.k = 0

        def __call__(self, padded, prow):
            row = self.rows[self.k]
            self.k += 1
            return lifter.forward_uv(padded, row, prow, window_stride=1)

    def per_clip():
        current["a"] = evaluate.evaluate_clips(PerClip(), clips, 243, dev)

    def batched():
        current["b"] = evaluate.evaluate_clips_batched(lifter.forward_clip, clips, 243, dev, encode="ray")

    ta, tb = [], []
    with torch.no_grad():
        per_clip(), batched()
        torch.cuda.synchronize(dev)
        for _ in range(args.reps):
            for run, acc in ((per_clip, ta), (batched, tb)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize(dev)
                acc.append((time.perf_counter() - t0) * 1e3)
    lifter.check_status(dev)
    a, b = stats(ta), stats(tb)
    equal = bool(torch.equal(current["a"][2].view(torch.int64), current["b"][2].view(torch.int64)))
    res = {"set": "%d clips, lengths U(1000, 6000), seed 0: %d frames, J 17, RF 243, four distorted cameras, flip off" % (len(clips), frames),
           "repetitions": args.reps,
           "timing": "host clock around the whole pass, device synchronised before start and stop; sides alternating, one untimed round first",
           "per_clip_forward_uv": dict(a, poses_per_s=round(frames / a["mean_ms"] * 1e3, 1)),
           "batched_encode": dict(b, poses_per_s=round(frames / b["mean_ms"] * 1e3, 1)),
           "ratio_batched_over_per_clip": round(b["mean_ms"] / a["mean_ms"], 4),
           "rows_bit_equal": equal, "action_average_mm": {"per_clip": current["a"][1], "batched": current["b"][1]},
           "verdict": verdict(a, b), "threshold": "none: the feature stands on the capability and on fewer host steps"}
    if not equal:
        raise SystemExit("the rows of the two paths differ: %s" % json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["pass"])
    ap.add_argument("--clips", type=int, default=240)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(PART), exist_ok=True)
    if args.step:
        res = step_pass(args)
        with open(PART, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0
    rc = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", "pass",
                         "--clips", str(args.clips), "--reps", str(args.reps)]).returncode     # a fresh process under its own time limit
    if rc != 0:
        print("the pass ended with status %d: nothing written" % rc, file=sys.stderr)
        return rc
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(json.load(open(PART)), f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
