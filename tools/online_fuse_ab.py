#!/usr/bin/env python3
"""A/B of the multi-camera end of one live tick - S streams of the RF-243 pair (ARCHITECTURE 3,3,3,3,3, synthetic weights), flip on, one
new frame of rays per stream, world poses and residuals from r3d_streams_poses, and per GROUP of streams (cameras that watch the
same person; groups of 2, 4 and 8) one fused world skeleton with its spread, contributor count and used masks:

  A `torch`:  what a caller writes without r3d_streams_fuse - OnlineLifter(world=True, quality=True).step, then torch ops on the
              device that restate the rule of include/ray3d_hip.h over the padded (G, M) member table: a gather, the candidate
              masks, the weights, the pairwise distances and the weighted medoid gate, the masked weighted mean, the spread, the
              count and the used words (vectorised: the sums run in torch's order, so the last bits may differ);
  B `call`:   OnlineLifter(world=True, quality=True, groups=...).step - the same tick, then ONE r3d_streams_fuse launch.

Both eager and captured (A: OnlineLifter.capture() for the tick and a second torch.cuda.graph around the torch tail; B:
OnlineLifter.capture()).  The new frame is a device tensor on all sides.  After lag + 3 ticks on the same frames the sides' fused
outputs are compared (recorded, not asserted).  `fuse_alone`: the one launch without the tick.

Timing: the clocks are settled by WARM seconds of ticks first; a side's run is TICKS ticks between two device events on the current
stream, read after a synchronise; the four sides alternate, REPS repetitions; the MEDIAN, min and max of ms per tick are kept.  The
shader clock of the last single-launch forward (r3d_last_clock) is recorded around every configuration.  No ratio is a pass condition.
usage:  python tools/online_fuse_ab.py [--out FILE] [--streams 1,32,256] [--sizes 2,4,8] [--ticks N] [--reps R] [--warm SECONDS]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clips_ab_common import write_out                              # noqa: E402
from online_ab import J, make_lifter                               # noqa: E402
from online_finish_ab import LEFT, RIGHT, cameras, timed           # noqa: E402

SOFT_PX, MAX_PX, MAX_DIST = 2.0, 0.0, 0.3


def torch_fuse(world, reproj, emit, status, member):
    """The rule with torch ops: (S, J, 3) world, (S, J) residuals, the step's words and the (G, M) member table ->
    (fused (G, J, 3), spread (G, J), count (G, J), used (G, M))."""
    import torch
    S = world.shape[0]
    valid = (member >= 0) & (member < S)
    idx = member.clamp(0, S - 1).long()
    finished = (status == 0) & (emit >= 0)
    x, r = world[idx], reproj[idx]                                  # (G, M, J, 3), (G, M, J)
    cand = (valid & finished[idx])[..., None] & torch.isfinite(x).all(-1) & torch.isfinite(r)
    if MAX_PX > 0:
        cand = cand & (r <= MAX_PX)
    w = torch.where(cand, 1.0 / (SOFT_PX * SOFT_PX + r * r), torch.zeros_like(r))
    x = torch.where(cand[..., None], x, torch.zeros_like(x))
    inl = cand
    if MAX_DIST > 0:
        xt, wt, ct = x.permute(0, 2, 1, 3), w.permute(0, 2, 1), cand.permute(0, 2, 1)      # (G, J, M, ...)
        d = torch.cdist(xt, xt)                                     # (G, J, M, M)
        cost = (d * wt[..., None, :]).sum(-1)
        cost = torch.where(ct, cost, torch.full_like(cost, float("inf")))
        best = cost.argmin(-1)
        dm = d.gather(-2, best[..., None, None].expand(-1, -1, 1, d.shape[-1])).squeeze(-2)
        gated = ct & (dm <= MAX_DIST)
        inl = torch.where((ct.sum(-1) >= 2)[..., None], gated, ct).permute(0, 2, 1)
    wi = w * inl
    den = wi.sum(1)
    fused = (wi[..., None] * x).sum(1) / den[..., None]
    spread = torch.sqrt((wi * ((x - fused[:, None]) ** 2).sum(-1)).sum(1) / den)
    used = (inl.long() << torch.arange(world.shape[1], device=world.device)).sum(-1)
    return fused, spread, inl.sum(1), used


def one(lifter, S, size, ticks, reps, warm, dev):
    import torch
    import ray3d_amd
    from ray3d_amd import _capi
    rf = lifter.receptive_field()
    rows, params, trans = cameras(S, dev)
    size = min(size, S)
    groups = [list(range(g, min(g + size, S))) for g in range(0, S, size)]
    gen = torch.Generator(device="cpu").manual_seed(S)
    person = torch.rand((rf + 4, len(groups), J, 3), generator=gen) - 0.5
    frames = torch.stack([person[:, s // size] for s in range(S)], 1) + 0.01 * torch.randn((rf + 4, S, J, 3), generator=gen)
    frames[..., 2] = 1.0
    frames = frames.to(dev)                    # the ticks' new frames (rays), device-resident: a group's cameras see alike
    at = [0]

    def new_frame():
        at[0] = (at[0] + 1) % frames.shape[0]
        return frames[at[0]]

    def lifters(**options):
        pair = [ray3d_amd.OnlineLifter(lifter, S, flip=True, kps_left=LEFT, kps_right=RIGHT, device=dev, world=True, quality=True, **options)
                for _ in range(2)]
        for ol in pair:
            ol.set_cameras(rows, params, trans)
        pair[1].capture()
        return pair

    a_eager, a_cap = lifters()
    b_eager, b_cap = lifters(groups=groups, fuse_soft_px=SOFT_PX, fuse_max_px=MAX_PX, fuse_max_dist=MAX_DIST)
    member = b_eager.member.clone()

    def torch_eager():
        _, _, extras = a_eager.step(new_frame(), check=False)
        return torch_fuse(extras["world"], extras["reproj"], a_eager.emit, a_eager.status, member)

    # A captured: the tick's own graph, then a graph around the tail that reads the buffers r3d_streams_poses writes
    with torch.no_grad():
        f = a_cap._finish
        torch_fuse(f["world"], f["reproj"], a_cap.emit, a_cap.status, member)
        torch.cuda.synchronize(dev)
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                tail_c = torch_fuse(f["world"], f["reproj"], a_cap.emit, a_cap.status, member)
    torch.cuda.synchronize(dev)

    def torch_captured():
        a_cap.step(new_frame(), check=False)
        g.replay()
        return tail_c

    def call(ol):
        _, _, extras = ol.step(new_frame(), check=False)
        return extras["fused"], extras["fused_spread"], extras["fused_count"], extras["fused_used"]

    sides = [torch_eager, torch_captured, lambda: call(b_eager), lambda: call(b_cap)]
    with torch.no_grad():
        for t in range(b_eager.lag + 3):       # the same frames through all four (every stream emits from tick `lag` on)
            outs = []
            for run in sides:
                at[0] = t - 1
                outs.append([v.clone() for v in run()])
        torch.cuda.synchronize(dev)
        ref = outs[2]
        same = {"worst_fused_difference_m": [float((o[0] - ref[0]).abs().nan_to_num(0.0).max()) for o in outs],
                "worst_spread_difference_m": [float((o[1] - ref[1]).abs().nan_to_num(0.0).max()) for o in outs],
                "count_equal": [bool(torch.equal(o[2].long(), ref[2].long())) for o in outs],
                "used_equal": [bool(torch.equal(o[3].long(), ref[3].long())) for o in outs],
                "mean_count": float(ref[2].double().mean()), "median_spread_m": float(ref[1].nan_to_num(0.0).median())}
        clock0 = lifter.last_clock_ghz(dev)
        res = timed(sides, ticks, reps, warm, dev)
        ol, z, stream = b_eager, b_eager._fuse, torch.cuda.current_stream(dev).cuda_stream

        def fuse_alone():
            _capi.streams_fuse(ol._finish["world"].data_ptr(), ol._finish["reproj"].data_ptr(), ol.emit.data_ptr(), ol.status.data_ptr(), None,
                               S, J, ol.member.data_ptr(), ol.G, _capi.FUSE_MAX_MEMBERS, SOFT_PX, MAX_PX, MAX_DIST, z["fused"].data_ptr(),
                               z["fused_spread"].data_ptr(), z["fused_count"].data_ptr(), z["fused_used"].data_ptr(), stream)
        (alone,) = timed([fuse_alone], ticks, reps, 0.2, dev)
    lifter.check_status(dev)
    a_cap.release(), b_cap.release()
    del g
    torch.cuda.synchronize(dev)
    lifter.release_prepared()
    te, tc, ce, cc = res
    return {"receptive_field": rf, "streams": S, "group_size": size, "groups": len(groups), "torch_eager": te, "torch_captured": tc,
            "call_eager": ce, "call_captured": cc, "fuse_alone": alone,
            "ratio_call_over_torch_eager": round(ce["median_ms"] / te["median_ms"], 4),
            "ratio_call_over_torch_captured": round(cc["median_ms"] / tc["median_ms"], 4),
            "saved_us_per_tick_eager": round(1e3 * (te["median_ms"] - ce["median_ms"]), 1),
            "saved_us_per_tick_captured": round(1e3 * (tc["median_ms"] - cc["median_ms"]), 1),
            "outputs_against_call_eager (torch_eager, torch_captured, call_eager, call_captured)": same,
            "shader_clock_ghz_before_after": [clock0, lifter.last_clock_ghz(dev)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_fuse_ab.json"))
    ap.add_argument("--streams", default="1,32,256")
    ap.add_argument("--sizes", default="2,4,8")
    ap.add_argument("--arch", default="3,3,3,3,3")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("online_fuse_ab.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lifter = make_lifter(args.arch, dev)
    rows = []
    for S in (int(v) for v in args.streams.split(",")):
        for size in (int(v) for v in args.sizes.split(",")):
            if size > S and rows and rows[-1]["streams"] == S:
                continue                       # (one stream: a single group of one, measured once)
            rows.append(one(lifter, S, size, args.ticks, args.reps, args.warm, dev))
            print(json.dumps(rows[-1]), flush=True)
    head = {"what": "ms per tick of a live multi-camera caller that wants one fused world skeleton per group of streams: "
                    "OnlineLifter(world, quality).step + a torch restatement of the fusion rule, against OnlineLifter(groups=).step (one "
                    "r3d_streams_fuse launch); eager and captured; soft_px %g, max_px %g, max_dist %g" % (SOFT_PX, MAX_PX, MAX_DIST),
            "timing": "%g s of ticks first, then device events around %d ticks, four sides alternating, %d repetitions: median / min / max "
                      "of ms per tick" % (args.warm, args.ticks, args.reps),
            "device": torch.cuda.get_device_name(dev), "rows": rows}
    return write_out(args.out, head)


if __name__ == "__main__":
    sys.exit(main())
