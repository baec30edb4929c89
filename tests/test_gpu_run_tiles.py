"""Two-source tiles on the GPU (r3d_schedule.cpp pack_runs, r3d_tiles.hpp gemm_tile_nb with n0 < NB): one-tile-deep M = B levels cut
into equal runs of column blocks that cross the end of a row - into the next unit of the problem, or into the next problem.
The shapes are the ones that can go wrong: ragged last units (130 = 4 units + 2 rows, 250 = 7 units + 26 rows), 192 and 224 windows
(six and seven units) and the full 256."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, check_parity, dev_switch, load_model_fixture
from run_tiles_util import forward_lists
from test_gpu_parity import build_modules

pytestmark = pytest.mark.gpu

BATCHES = (130, 192, 224, 250, 256)
# two-source tiles of the RF 27 pair's call, by the host's own tile lists (tests/test_run_tiles_host.py sweeps every size): eight
# units are cut into runs, fewer keep the row-by-row cut - those sizes hold the one-source path of the changed tile to the oracle
TWO_SOURCE = {130: 0, 192: 0, 224: 0, 250: 160, 256: 160}
_REF = {}


def _reference(mc, B):
    """The torch port's poses for the call of B windows (computed once per size, never modified)."""
    from ray3d_amd import synth
    from oracle import torch_port
    if B not in _REF:
        _, _, (cp, sp), (ct, st) = build_modules(mc)
        x = synth.synth_rays(B, cp, seed=77)
        p = synth.synth_param(B, seed=78)
        sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
        with torch.no_grad():
            ref = (torch_port.forward(cp, sds[0], torch.from_numpy(x), torch.from_numpy(p)) +
                   torch_port.forward(ct, sds[1], torch.from_numpy(x), torch.from_numpy(p))).numpy()
        ref.setflags(write=False)
        _REF[B] = (x, p, ref)
    return _REF[B]


@pytest.mark.parametrize("B", BATCHES)
def test_run_tiles_against_the_oracle(B, monkeypatch, tmp_path):
    """Every window against the torch port at the literal 1e-4 bound; the level-by-level form bit-identical (the same tiles); two
    consecutive calls bit-identical; the whole-tile packing (R3D_NO_NB, hooks build) within 2e-5 * max(1, max|ref|) - the bound the
    project holds that pair to (which block sits on wavefronts 0-3 or is added up through LDS changes, nothing else)."""
    import ray3d_amd
    if os.environ.get("R3D_BF16X3") == "1":
        pytest.skip("bf16x3 handles keep their packing")
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3")
    x, p, ref = _reference(mc, B)

    def lift(staged=False, calls=1):
        pos, trj, _, _ = build_modules(mc)
        lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
        lifter.set_staged(staged)
        xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
        with torch.no_grad():
            outs = [lifter(xd, pd).clone() for _ in range(calls)]
        lifter.check_status()
        return outs
    out, again = lift(calls=2)
    check_parity(out, ref, "run tiles vs torch port")
    assert torch.equal(out, again)
    if os.environ.get("R3D_STAGED") != "1":
        assert torch.equal(lift(staged=True)[0], out)
    # what the call ran (the host's own tile lists)
    two = sum(1 for t in forward_lists(mc, B, tmp_path)[1] if t["src2"] >= 0)
    print("B=%d: %d two-source tiles" % (B, two))
    assert two == TWO_SOURCE[B]
    dev_switch(monkeypatch, "R3D_NO_NB", "1")
    whole = lift()[0]
    check_parity(whole, ref, "whole tiles vs torch port")
    diff = (whole - out).abs().max().item()
    print("B=%d: max |whole tiles - run tiles| = %.3e (bound %.3e)" % (B, diff, 2e-5 * max(1.0, float(np.abs(ref).max()))))
    assert diff <= 2e-5 * max(1.0, float(np.abs(ref).max()))


def test_run_tiles_inside_concatenated_operands_at_192_windows(tmp_path):
    """The RF 243 pair at 192 windows: its FuseBlocks w2 launch is cut into runs that cross into the next unit of the same problem
    (six units, 6-block runs), beside launches that keep the row-by-row cut - against the torch port, both forms, twice."""
    import ray3d_amd
    from ray3d_amd import synth
    from oracle import torch_port
    if os.environ.get("R3D_BF16X3") == "1":
        pytest.skip("bf16x3 handles keep their packing")
    mc = ray3d_amd.default_model_config(ARCHITECTURE="3,3,3,3,3")
    B = 192
    probs, tiles, rc = forward_lists(mc, B, tmp_path)
    two = [t for t in tiles if t["src2"] >= 0]
    assert rc == 0 and two and all(t["src2"] == t["prob"] for t in two)
    pos, trj, (cp, sp), (ct, st) = build_modules(mc)
    x, p = synth.synth_rays(B, cp, seed=77), synth.synth_param(B, seed=78)
    sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s_.items()} for s_ in (sp, st)]
    with torch.no_grad():
        ref = (torch_port.forward(cp, sds[0], torch.from_numpy(x), torch.from_numpy(p)) +
               torch_port.forward(ct, sds[1], torch.from_numpy(x), torch.from_numpy(p))).numpy()
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    with torch.no_grad():
        out, again = lifter(xd, pd).clone(), lifter(xd, pd).clone()
        lifter.set_staged(True)
        staged = lifter(xd, pd).clone()
    lifter.check_status()
    check_parity(out, ref, "RF 243 at 192 windows vs torch port")
    assert torch.equal(out, again)
    if os.environ.get("R3D_STAGED") != "1":
        assert torch.equal(staged, out)


def test_run_tiles_on_the_bench_fixture_at_256_windows():
    """The headline call: the RF 243 pair of bench.py on tests/golden/model_j17_rf243_s3.npz, the fixture's windows tiled to 256."""
    import ray3d_amd
    if os.environ.get("R3D_BF16X3") == "1":
        pytest.skip("bf16x3 handles keep their packing")
    z, mc = load_model_fixture("j17_rf243_s3")
    assert os.path.exists(os.path.join(GOLDEN, "model_j17_rf243_s3.npz"))
    pos, trj, _, _ = build_modules(mc)
    lifter = ray3d_amd.Ray3DLifter(pos, trj).eval()
    n = z["x"].shape[0]
    idx = np.arange(256) % n
    x, p = torch.from_numpy(z["x"][idx]).cuda(), torch.from_numpy(z["param"][idx]).cuda()
    with torch.no_grad():
        out = lifter(x, p)
        again = lifter(x, p)
    lifter.check_status()
    check_parity(out.cpu().numpy(), (z["out_pos"] + z["out_trj"])[idx], "RF 243 at 256 windows vs reference fixture")
    assert torch.equal(out, again)
