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
        [--clips N] [--reps R] shrink the run (rehearsals) - tools/clips_ab_common.py."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_ab_common as ab

TOOL = "clips_encode_ab"
STEPS = (("pass", 420),)     # seconds for the pass (12 passes of about 1.6 s, the schedules' preparation and the start of torch)


def step_pass(args):
    import torch
    from ray3d_amd import evaluate
    if not torch.cuda.is_available():
        raise SystemExit("clips_encode_ab measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    clips = ab.make_set(args.clips, pixels=True)
    frames = sum(c.rays.shape[0] for c in clips)
    lifter = ab.make_lifter(clips, dev)
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

    with torch.no_grad():
        a, b = ab.alternate([per_clip, batched], args.reps, dev, wall=True)
    lifter.check_status(dev)
    equal = bool(torch.equal(current["a"][2].view(torch.int64), current["b"][2].view(torch.int64)))
    res = {"set": "%d clips, lengths U(1000, 6000), seed 0: %d frames, J 17, RF 243, four distorted cameras, flip off" % (len(clips), frames),
           "repetitions": args.reps,
           "timing": "host clock around the whole pass, device synchronised before start and stop; sides alternating, one untimed round first",
           "per_clip_forward_uv": dict(a, poses_per_s=round(frames / a["mean_ms"] * 1e3, 1)),
           "batched_encode": dict(b, poses_per_s=round(frames / b["mean_ms"] * 1e3, 1)),
           "ratio_batched_over_per_clip": round(b["mean_ms"] / a["mean_ms"], 4),
           "rows_bit_equal": equal, "action_average_mm": {"per_clip": current["a"][1], "batched": current["b"][1]},
           "verdict": ab.verdict(a, b), "threshold": "none: the feature stands on the capability and on fewer host steps"}
    if not equal:
        raise SystemExit("the rows of the two paths differ: %s" % json.dumps(res))
    return res


def main():
    args = ab.parser(__doc__, TOOL, STEPS).parse_args()
    if args.step:
        return ab.run_step(TOOL, args, step_pass(args))
    return ab.run_steps(TOOL, STEPS, args, None)      # (the file holds the pass's result itself)


if __name__ == "__main__":
    sys.exit(main())
