"""R3D_INPUT_UV_DIST cost: ms per step of the pos + trj forward (bench.py's RF-243 model, J 17) fed
  rays     - ray-encoded keypoints (R3D_INPUT_RAYS),
  uv       - pixels + 8-double camera rows, rays encoded inside the first-level gather (R3D_INPUT_UV),
  uv_dist  - RAW pixels of distorted cameras + 16-double rows: the r3d_undistort_rays_f64 pre-pass, then the rays forward,
for (B, 243, 17, 2) batches with a camera per window (the four H36M coefficient sets of tests/golden/undistort.npz) and a
4096-window sliding clip with one camera.  Modes alternate inside every round (same clocks for all three); the median round
is reported, with the pre-pass's own time from the library's event-bracketed profile records.  Steps are host-timed around
a device synchronise (steps forwards back to back).

    python tools/undistort_time.py [--batches 256,1024] [--clip 4096] [--steps 20] [--rounds 7] [--json out.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/undistort_time.py --profile-only
      (the kernel's time from the trace: 60 UV_DIST steps per shape, nothing else - read the settled last ones)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def h36m_cameras():
    import ray3d_amd
    z = np.load(os.path.join(ROOT, "tests", "golden", "cameras.npz"))
    u = np.load(os.path.join(ROOT, "tests", "golden", "undistort.npz"))
    return [ray3d_amd.Camera(u["cam%d/K" % i], z["h36m_S9_%d/R" % i], z["h36m_S9_%d/t" % i], dist_coeff=u["cam%d/dist" % i],
                             undistort=True) for i in range(int(u["n"]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--clip", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default="")
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "undistort_time.py measures on an AMD GPU"
    import bench
    from ray3d_amd import synth
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lifter, states = bench.build(dev)
    cfg = states["pos"][0]
    rf, J = cfg.receptive_field, cfg.num_joints
    cams = h36m_cameras()

    shapes = []
    for B in [int(b) for b in args.batches.split(",") if b]:
        pick = [i % len(cams) for i in range(B)]
        uv = (1000.0 * synth.hash_uniform("undistort_time.%d" % B, (B, rf, J, 2), 1)).astype(np.float32)
        rays = np.stack([cams[c].rays_from_uv(uv[i]) for i, c in enumerate(pick)]).astype(np.float32)
        par = torch.from_numpy(np.stack([cams[c].param() for c in pick])).to(dev)
        r8 = torch.from_numpy(np.stack([cams[c].cam_row() for c in pick])).to(dev)
        r16 = torch.from_numpy(np.stack([cams[c].cam_row(distortion=True) for c in pick])).to(dev)
        uvd, raysd = torch.from_numpy(uv).to(dev), torch.from_numpy(rays).to(dev)
        shapes.append(("b%d" % B, B, {
            "rays": lambda raysd=raysd, par=par: lifter(raysd, par),
            "uv": lambda uvd=uvd, r8=r8, par=par: lifter.forward_uv(uvd, r8, par),
            "uv_dist": lambda uvd=uvd, r16=r16, par=par: lifter.forward_uv(uvd, r16, par)}))
    if args.clip > 0:
        n, cam = args.clip, cams[0]
        rng = np.random.default_rng(5)
        clip = (rng.uniform(200, 800, (1, J, 2)) + np.cumsum(rng.normal(0, 2.0, (n + rf - 1, J, 2)), axis=0)).astype(np.float32)
        rays = torch.from_numpy(cam.rays_from_uv(clip).astype(np.float32)).to(dev)
        clipd = torch.from_numpy(clip).to(dev)
        p1 = torch.from_numpy(cam.param()).to(dev)
        r8, r16 = torch.from_numpy(cam.cam_row()).to(dev), torch.from_numpy(cam.cam_row(distortion=True)).to(dev)
        shapes.append(("clip%d" % n, n, {
            "rays": lambda: lifter.forward_clip(rays, p1),
            "uv": lambda: lifter.forward_uv(clipd, r8, p1),
            "uv_dist": lambda: lifter.forward_uv(clipd, r16, p1)}))

    result = {"model": "RF %d, J %d, pos + trj (bench.py's)" % (rf, J), "steps": args.steps, "rounds": args.rounds, "shapes": {}}
    with torch.no_grad():
        for name, B, fns in shapes:
            lifter.prepare([B])
            if args.profile_only:                        # (enough back-to-back steps for the clock to settle: read the last ones)
                for _ in range(60):
                    fns["uv_dist"]()
                torch.cuda.synchronize()
                continue
            for fn in fns.values():                      # warm-up: schedules, binds, clocks
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) / args.steps * 1e3)
            ms = {k: float(np.median(v)) for k, v in times.items()}
            recs = lifter.profile_call(fns["uv_dist"], dev)
            pre = [r["ms"] for r in recs if r["kernel"] == "r3d_undistort_rays_f64"]
            pair = [r["ms"] for r in recs if r["kernel"] == "r3d_event_pair"]
            row = {"windows": B, "ms_per_step": {k: round(v, 4) for k, v in ms.items()},
                   "spread_ms": {k: round(float(max(v) - min(v)), 4) for k, v in times.items()},
                   "uv_dist_over_uv": round(ms["uv_dist"] / ms["uv"], 4),
                   "uv_dist_minus_uv_us": round((ms["uv_dist"] - ms["uv"]) * 1e3, 1),
                   "pre_pass_event_us": round(1e3 * (sum(pre) - len(pre) * (pair[0] if pair else 0.0)), 1),
                   "pre_pass_launches": len(pre)}
            result["shapes"][name] = row
            print(name, json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
