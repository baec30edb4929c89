#!/usr/bin/env python3
"""A/B of one tick of a live caller with and without r3d_streams_repair - S cameras, one new frame of raw pixel keypoints each, the
newest pose back - on synthetic weights and distorted synthetic cameras (those of tools/online_ab.py), S in {1, 32, 256}, for the
RF-243 pair (ARCHITECTURE 3,3,3,3,3) and an RF-9 pair (3,3):

  `plain`:  OnlineLifter(repair=None).step(check=False) - r3d_streams_step and the forward: the tick as it was;
  `repair`: OnlineLifter(repair=K).step(check=False) - r3d_streams_repair in front of the same tick (one more launch of S
            workgroups of one wavefront), and the word of `synthetic` per stream copied out.

Both eager and captured into a hipGraph (OnlineLifter.capture()).  The frames carry gaps: every joint of every stream drops out
with probability --drop per frame (a NaN pixel), so holds, back-fills and closing gaps all occur while the ticks are timed; the
plain side is fed the same frames with the gaps left out (it would return NaN poses).  `repair_alone`: the one launch without the
step and the forward.  After RF + 2 gap-free ticks the two sides' poses are compared (expected equal bit for bit; recorded, not
asserted).

Timing: a side's run is TICKS ticks on a host clock with the device synchronised before it starts and before it stops; the sides
alternate, one untimed round first, REPS repetitions; the MEDIAN, min and max of ms per tick are kept.  The shader clock of the
last single-launch forward (r3d_last_clock) is recorded before and after each configuration.  No ratio is a pass condition.
usage:  python tools/online_repair_ab.py [--out FILE] [--streams 1,32,256] [--ticks N] [--reps R] [--configs rf243,rf9]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clips_ab_common import write_out                          # noqa: E402
from online_ab import CONFIGS, J, cameras, make_lifter, timed   # noqa: E402


def one(lifter, name, S, ticks, reps, drop, dev):
    import torch
    import ray3d_amd
    from ray3d_amd import _capi
    rf = lifter.receptive_field()
    K = min(5, rf - 1)
    rows, params = cameras(S, dev)
    gen = torch.Generator(device="cpu").manual_seed(S)
    frames = (1024.0 * torch.rand((rf + 4, S, J, 2), generator=gen)).to(dev)      # the ticks' new frames, device-resident
    gaps = torch.rand((rf + 4, S, J), generator=gen).to(dev) < drop
    gapped = torch.where(gaps.unsqueeze(-1), torch.full_like(frames, float("nan")), frames)
    at = [0]

    def nxt():
        at[0] = (at[0] + 1) % frames.shape[0]
        return at[0]

    lifter.prepare([S], dev)
    sides = {}
    for tag, repair in (("plain", None), ("repair", K)):
        for mode in ("eager", "captured"):
            ol = ray3d_amd.OnlineLifter(lifter, S, encoding="ray", device=dev, repair=repair)
            ol.set_cameras(rows, params)
            if mode == "captured":
                ol.capture()
            sides[tag, mode] = ol

    # ---- the same RF + 2 gap-free frames through all four: their poses
    with torch.no_grad():
        for t in range(rf + 2):
            outs = {k: ol.step(frames[t], check=False) for k, ol in sides.items()}
    torch.cuda.synchronize(dev)
    assert all(int(ol.status.abs().sum()) == 0 for ol in sides.values())
    ref = outs["plain", "eager"][0]
    same = {"%s_%s" % k: bool(torch.equal(ref, v[0])) for k, v in outs.items() if k != ("plain", "eager")}
    synthetic_zero = all(not bool(v[2]["synthetic"].any()) for k, v in outs.items() if k[0] == "repair")

    clock0 = lifter.last_clock_ghz(dev)
    with torch.no_grad():
        res = timed([lambda: sides["plain", "eager"].step(frames[nxt()], check=False),
                     lambda: sides["repair", "eager"].step(gapped[nxt()], check=False),
                     lambda: sides["plain", "captured"].step(frames[nxt()], check=False),
                     lambda: sides["repair", "captured"].step(gapped[nxt()], check=False)], ticks, reps, dev)
        # r3d_streams_repair alone: its one launch, no step, no forward (the heads stand still: every tick repairs the same slot)
        ol = sides["repair", "eager"]
        stream = torch.cuda.current_stream(dev).cuda_stream
        ol.action.fill_(_capi.R3D_STREAM_PUSH)
        ol.frame.copy_(gapped[0])

        def repair_alone():
            _capi.streams_repair(ol.state.data_ptr(), ol.repair_track.data_ptr(), S, rf, ol.lag, J, 3, ol.encoding, ol.frame.data_ptr(), None, 0.0,
                                 ol.cam.data_ptr(), ol.action.data_ptr(), K, ol.frame_out.data_ptr(), ol.synthetic.data_ptr(), stream)
        (alone,) = timed([repair_alone], ticks, reps, dev)
    lifter.check_status(dev)
    for ol in sides.values():
        ol.release()
    torch.cuda.synchronize(dev)
    lifter.release_prepared()
    pe, re_, pc, rcap = res
    return {"config": name, "receptive_field": rf, "streams": S, "max_gap": K, "drop_probability": drop,
            "plain": pe, "repair": re_, "plain_captured": pc, "repair_captured": rcap, "repair_alone": alone,
            "added_ms_eager": round(re_["median_ms"] - pe["median_ms"], 4), "added_ms_captured": round(rcap["median_ms"] - pc["median_ms"], 4),
            "ratio_repair_over_plain": round(re_["median_ms"] / pe["median_ms"], 4),
            "ratio_repair_over_plain_captured": round(rcap["median_ms"] / pc["median_ms"], 4),
            "gap_free_poses_equal_to_plain_eager": same, "gap_free_synthetic_all_zero": synthetic_zero,
            "shader_clock_ghz_before_after": [clock0, lifter.last_clock_ghz(dev)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_repair_ab.json"))
    ap.add_argument("--streams", default="1,32,256")
    ap.add_argument("--configs", default="rf243,rf9")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--drop", type=float, default=0.02)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("online_repair_ab.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    for name in args.configs.split(","):
        lifter = make_lifter(CONFIGS[name], dev)
        for S in (int(v) for v in args.streams.split(",")):
            rows.append(one(lifter, name, S, args.ticks, args.reps, args.drop, dev))
            print(json.dumps(rows[-1]), flush=True)
    head = {"what": "ms per tick of a live caller: OnlineLifter.step with r3d_streams_repair in front of the tick against the same build's "
                    "tick without it; eager and captured; the repair side's frames carry gaps",
            "timing": "host clock around %d ticks, device synchronised before start and stop, the sides alternating, one untimed round first, "
                      "%d repetitions: median / min / max of ms per tick" % (args.ticks, args.reps),
            "device": torch.cuda.get_device_name(dev), "rows": rows}
    return write_out(args.out, head)


if __name__ == "__main__":
    sys.exit(main())
