"""What tests/test_streams_poses_host.py and tests/test_gpu_streams_poses.py share: the NumPy restatement of r3d_streams_poses's stated
arithmetic (include/ray3d_hip.h), a rig that keeps every buffer of the call inside guard bands (tests/buffers_util.py) and runs it on
the host hook or on the device, and the inputs both run."""
import functools
import os

import numpy as np
import torch

import buffers_util as bu
from conftest import GOLDEN, hooks_library
from ray3d_amd import _capi, evaluate

FILL32, FILL64 = np.float32(-7.0), np.float64(-7.0)      # what the outputs hold before a call: rows nobody finished must keep it
QNAN32, QNAN64 = np.uint32(0x7FC00000), np.uint64(0x7FF8000000000000)
OUTPUTS = ("pred", "world", "reproj", "quality")
H36M_LEFT, H36M_RIGHT = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
J14_LEFT, J14_RIGHT = [4, 5, 6, 10, 11], [1, 2, 3, 12, 13]


def perm_of(J):
    return evaluate.mirror_permutation(J, *((H36M_LEFT, H36M_RIGHT) if J == 17 else (J14_LEFT, J14_RIGHT)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def _canon(a):
    """A NaN the arithmetic produced leaves as the canonical quiet NaN."""
    a = np.array(a)
    bits(a)[np.isnan(a)] = QNAN32 if a.dtype == np.float32 else QNAN64
    return a


@functools.lru_cache(maxsize=None)
def golden_cameras():
    """The first three H36M cameras of cameras.npz (those of streams_poses.npz), undistort=False."""
    import ray3d_amd
    z = np.load(os.path.join(GOLDEN, "cameras.npz"))
    return tuple(ray3d_amd.Camera(z["h36m_S9_%d/K" % i], z["h36m_S9_%d/R" % i], z["h36m_S9_%d/t" % i], res_w=1000, res_h=1002,
                                  name="h36m_S9_%d" % i) for i in range(3))


# ------------------------------------------------------------------ the stated arithmetic, in NumPy

def finish(raw, raw_m, perm):
    """p: the raw bits, or fl32(fl32(raw + m) * 0.5f) with m = joint perm[j] of raw_m, component 0 negated."""
    if raw_m is None:
        return raw.copy()
    m = raw_m[:, perm].copy()
    m[..., 0] = -m[..., 0]
    with np.errstate(all="ignore"):
        return _canon(((raw + m).astype(np.float32) * np.float32(0.5)).astype(np.float32))


def world_of(desc, p):
    """component r = ((R[3r] x + R[3r+1] y) + R[3r+2] z) + T[r] in float64, every product and sum rounded once."""
    x, y, z = (p[..., k].astype(np.float64) for k in range(3))
    R, T = desc[:, None, 0:9], desc[:, None, 9:12]
    with np.errstate(all="ignore"):
        return _canon(np.stack([((R[..., 3 * r] * x + R[..., 3 * r + 1] * y) + R[..., 3 * r + 2] * z) + T[..., r] for r in range(3)], -1))


def reproj_of(desc, cam, p, ray):
    fx, fy, c, sn, h = cam[:, None, 0], cam[:, None, 1], cam[:, None, 4], cam[:, None, 5], desc[:, None, 12]
    with np.errstate(all="ignore"):
        yy = p[..., 1].astype(np.float64) + h
        z = p[..., 2].astype(np.float64)
        Xc = p[..., 0].astype(np.float64)
        Yc = c * yy - sn * z
        Zc = sn * yy + c * z
        a, b = Xc / Zc, Yc / Zc
        xo = ray[..., 0].astype(np.float64)
        yo = c * ray[..., 1].astype(np.float64) - sn * ray[..., 2].astype(np.float64)
        du, dv = fx * (a - xo), fy * (b - yo)
        return _canon(np.sqrt(du * du + dv * dv))


def quality_of(res):
    out = np.empty((res.shape[0], 2), np.float64)
    with np.errstate(all="ignore"):
        for s, row in enumerate(res):
            total = np.float64(0.0)
            for v in row:                     # joint order, from zero
                total = total + v
            out[s] = (total / np.float64(len(row)), row.max())
            if np.isnan(row).any():
                bits(out)[s] = QNAN64
    return _canon(out)


def restate(inp, flip, which=OUTPUTS):
    """What the call leaves in FILL-ed outputs: rows of finished streams from the stated arithmetic, every other row the fill."""
    S, J = inp["raw"].shape[:2]
    done = (inp["status"] == 0) & (inp["emit"] >= 0)
    p = finish(inp["raw"], inp["raw_m"] if flip else None, inp["perm"])
    ray = inp["x"][:, inp["rf"] - 1 - inp["lag"]]
    full = dict(pred=p, world=world_of(inp["desc"], p), reproj=reproj_of(inp["desc"], inp["cam"], p, ray))
    full["quality"] = quality_of(full["reproj"])
    out = {}
    for k in which:
        o = np.full(full[k].shape, FILL32 if k == "pred" else FILL64, full[k].dtype)
        o[done] = full[k][done]
        out[k] = o
    return out


# ------------------------------------------------------------------ inputs

def make_inputs(S, J, rf, lag, seed, emit=None, status=None):
    """S streams on the H36M cameras: poses near 5 m in front of the camera in the normalised frame, the rays of a keypoint a few
    pixels off, windows whose other rows hold NaNs nothing may read."""
    rng = np.random.RandomState(seed)
    cams = [golden_cameras()[s % 3] for s in range(S)]
    desc = np.stack([c.stream_pose_row() for c in cams])
    cam = np.stack([c.cam_row(distortion=True) for c in cams])
    Xw = 0.3 * rng.standard_normal((S, J, 3)) + np.array([0.0, 0.0, 1.0])
    pn = np.stack([c.world2normalized(Xw[s]) for s, c in enumerate(cams)])
    raw = (pn + 0.02 * rng.standard_normal(pn.shape)).astype(np.float32)
    raw_m = (pn * np.array([-1.0, 1.0, 1.0]) + 0.02 * rng.standard_normal(pn.shape)).astype(np.float32)[:, np.argsort(perm_of(J))]
    x = np.empty((S, rf, J, 3), np.float32)
    x.view(np.uint32)[:] = 0x7FC00BAD
    for s, c in enumerate(cams):
        x[s, rf - 1 - lag] = c.rays_from_uv(c.project(Xw[s])).astype(np.float32)
    return dict(raw=raw, raw_m=raw_m, perm=perm_of(J), desc=desc, cam=cam, x=x, rf=rf, lag=lag,
                emit=np.arange(S, dtype=np.int64) if emit is None else np.asarray(emit, np.int64),
                status=np.zeros(S, np.int32) if status is None else np.asarray(status, np.int32))


class Rig:
    """The buffers of one r3d_streams_poses caller, carved exact-sized out of one pattern-filled arena on `device` ("cpu": the host
    hook runs on them; a cuda device: the kernel).  The outputs are filled with FILL* before every call; the guards are checked
    after it."""

    def __init__(self, device, inp, pattern=bu.NANS):
        self.device, self.inp = torch.device(device), inp
        S, J = inp["raw"].shape[:2]
        self.S, self.J = S, J
        arrays = [("raw", inp["raw"]), ("raw_m", inp["raw_m"]), ("emit", inp["emit"]), ("status", inp["status"]), ("desc", inp["desc"]),
                  ("cam", inp["cam"]), ("x", inp["x"]), ("pred", np.full((S, J, 3), FILL32)), ("world", np.full((S, J, 3), FILL64)),
                  ("reproj", np.full((S, J), FILL64)), ("quality", np.full((S, 2), FILL64))]
        self.arena = bu.Arena(self.device, pattern, bu.Arena.capacity_for([a.nbytes for _, a in arrays]))
        self.t = {n: self.arena.put(a, 256, 4 if n in ("raw", "raw_m", "x", "pred") else 0, n)() for n, a in arrays}

    def write(self, **arrays):
        for n, a in arrays.items():
            self.t[n].copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def args(self, flip, which=OUTPUTS, **over):
        t = self.t
        a = dict(raw=t["raw"].data_ptr(), raw_m=t["raw_m"].data_ptr() if flip else None, S=self.S, J=self.J,
                 perm=self.inp["perm"] if flip else None, emit=t["emit"].data_ptr(), status=t["status"].data_ptr(),
                 desc=t["desc"].data_ptr(), cam=t["cam"].data_ptr(), x=t["x"].data_ptr(), rf=self.inp["rf"], lag=self.inp["lag"])
        a.update({k: (t[k].data_ptr() if k in which else None) for k in OUTPUTS})
        a.update(over)
        return tuple(a[k] for k in ("raw", "raw_m", "S", "J", "perm", "emit", "status", "desc", "cam", "x", "rf", "lag") + OUTPUTS)

    def read(self):
        return {k: self.t[k].cpu().numpy().copy() for k in OUTPUTS}

    def call(self, flip, which=OUTPUTS, **over):
        """One call.  -> dict(rc, pred, world, reproj, quality) as NumPy copies (rc: the hook's; 0 on a device, where a failure raises)."""
        t = self.t
        t["pred"].fill_(float(FILL32))
        for k in OUTPUTS[1:]:
            t[k].fill_(float(FILL64))
        args = self.args(flip, which, **over)
        if self.device.type == "cpu":
            hooks_library()
            rc = _capi.debug_streams_poses_host(*args)
        else:
            _capi.use_hooks(False)
            _capi.streams_poses(*args, torch.cuda.current_stream(self.device).cuda_stream)
            rc = 0
        self.arena.check()
        return dict(self.read(), rc=rc)


def untouched(got):
    """Every output still holds its fill."""
    return all((got[k] == (FILL32 if k == "pred" else FILL64)).all() for k in OUTPUTS)
