"""What the call-history tests share (tests/test_call_history_host.py, tests/test_gpu_call_history.py).

A handle pair carries state from one call to the next - the bound problem table and the counter bank of every schedule
(Schedule::Fwd::bound), the two activation banks of calls of a few windows, the schedule cache, the per-handle status word and
last stream, the Python mirror's workspaces.  The tests run MANY calls on one long-lived pair and hold every forward to the bits
of the same call on a fresh pair that has done nothing else (the cold reference), which is itself held to the oracle.

Host part (no device, no torch): the closed set of operations as hashable descriptors, the r3d_input a forward amounts to
(`call_of`), what it reads of the pool (`extents`), the BoundKey the library derives from it (`bound_key`), the seeded sequence
generator and the directed list of key-field pairs.  GPU part: `Rig` - the pool, fresh pairs, the cold cache, the oracle."""
import collections
import random

import numpy as np

ARCH = "3,3,3"
RF, J, F, E = 27, 17, 3, 2
BMAX = 150
# straddle the gemv (4 | 5), poll (16 | 17) and latency (32) limits and the plan-kind edges the hooks library reports (48 | 49, 96 | 97)
WINDOW_COUNTS = (1, 4, 5, 16, 17, 32, 48, 49, 96, 97, 150)
NAN_AT = (3, 13, 5, 1)               # (window, frame, joint, component) of the one NaN of buffer 'xn'
PREPARE_SIZES = (4, 17, 97)          # what the `prepare` mutator pins

# ---- the pool: every buffer is allocated once and is large enough for every view taken of it -------------------------------------
POOL = collections.OrderedDict([
    ("x0", ((BMAX, RF, J, F), "float32")), ("x1", ((BMAX, RF, J, F), "float32")), ("xn", ((BMAX, RF, J, F), "float32")),
    ("p0", ((BMAX, E), "float32")), ("p1", ((BMAX, E), "float32")), ("pb", ((1, E), "float32")),
    ("c0", ((BMAX, 8), "float64")), ("c1", ((BMAX, 8), "float64")),        # camera tables of R3D_INPUT_UV
    ("d0", ((BMAX, 16), "float64")), ("d1", ((BMAX, 16), "float64")),      # ... and of R3D_INPUT_UV_DIST
])

# ---- descriptors -----------------------------------------------------------------------------------------------------------------
# a forward through one of the Python entry points: `xbuf` / `side` pick the x buffer and the (parameter, camera) buffers, `lane`
# the lane it is issued on while lanes are on
Forward = collections.namedtuple("Forward", "form B xbuf side lane")
Mutator = collections.namedtuple("Mutator", "name arg")
# the r3d_input a forward amounts to (buffers by their pool names; `ws`: whose workspace the call runs in)
Call = collections.namedtuple("Call", "mode x window_stride B param param_stride cam cam_stride ws")
Config = collections.namedtuple("Config", "staged lanes weights device_weights")
# where every pair starts.  Weights packed on the device (r3d_finalize_dev): the host path's r3d_finalize costs 0.16 s per model
# - 0.45 s per fresh pair, measured - and every cold reference builds two fresh pairs; set_device_weights(False) is the option
# that is switched "on" for a while here, and the eviction test runs on the host path throughout
COLD = Config(False, 0, 0, True)

FORMS = ("forward", "forward_trj", "split", "uv_rows", "uv_bcast", "uv_dist", "clip", "pos_alone", "trj_alone", "graph", "forward_nan")
# which of (pos + trj, pos alone, trj alone) a form returns, in order
OUTPUTS = {"forward": ("sum",), "forward_trj": ("sum", "trj"), "split": ("pos", "trj"), "uv_rows": ("sum",), "uv_bcast": ("sum",),
           "uv_dist": ("sum",), "clip": ("sum",), "pos_alone": ("pos",), "trj_alone": ("trj",), "graph": ("sum",), "forward_nan": ("sum",)}
MUTATORS = (Mutator("set_staged", True), Mutator("set_staged", False), Mutator("refresh_weights", None),
            Mutator("load_state_dict", 1), Mutator("load_state_dict", 0), Mutator("set_device_weights", True),
            Mutator("set_device_weights", False), Mutator("prepare", PREPARE_SIZES), Mutator("release_prepared", None),
            Mutator("set_lanes", 2), Mutator("set_lanes", 0))
# what leaves the starting configuration, and what comes back to it
_OFF = {MUTATORS[0]: MUTATORS[1], MUTATORS[3]: MUTATORS[4], MUTATORS[6]: MUTATORS[5], MUTATORS[7]: MUTATORS[8], MUTATORS[9]: MUTATORS[10]}


def accepts(form, B):
    """Every form takes every window count (a clip of B + RF - 1 frames gives B windows; CLIP_ROUND = 0 lifts exact sizes)."""
    return form in FORMS and B in WINDOW_COUNTS


def after(cfg, mut):
    """The configuration a mutator leaves behind (prepare / release_prepared / refresh_weights change no cold result)."""
    if mut.name == "set_staged":
        return cfg._replace(staged=bool(mut.arg))
    if mut.name == "set_lanes":
        return cfg._replace(lanes=int(mut.arg))
    if mut.name == "load_state_dict":
        return cfg._replace(weights=int(mut.arg))
    if mut.name == "set_device_weights":
        return cfg._replace(device_weights=bool(mut.arg))
    assert mut.name in ("refresh_weights", "prepare", "release_prepared"), mut
    return cfg


def call_of(fwd):
    """The r3d_input of a Forward."""
    x, p, B = "x%d" % fwd.xbuf, "p%d" % fwd.side, fwd.B
    f = fwd.form
    if f in ("forward", "forward_trj", "split", "graph"):
        return Call("rays", x, RF, B, p, E, None, 0, "pair")
    if f == "forward_nan":
        return Call("rays", "xn", RF, B, p, E, None, 0, "pair")
    if f == "pos_alone" or f == "trj_alone":
        return Call("rays", x, RF, B, p, E, None, 0, f[:3])
    if f == "uv_rows":
        return Call("uv", x, RF, B, p, E, "c%d" % fwd.side, 8, "pair")
    if f == "uv_bcast":
        return Call("uv", x, RF, B, "pb", 0, "c%d" % fwd.side, 0, "pair")
    if f == "uv_dist":
        return Call("uv_dist", x, RF, B, p, E, "d%d" % fwd.side, 16, "pair")
    assert f == "clip", f
    return Call("rays", x, 1, B, "pb", 0, None, 0, "pair")


def frame_floats(call):
    return J * (F if call.mode == "rays" else 2)


def extents(call):
    """{pool name: (elements the call reads from the start of the buffer, elements the buffer has)}: window i covers frames
    [i * stride, i * stride + RF), so the largest index read is (B - 1) * stride + RF frames; B parameter / camera rows, or one."""
    def size(name):
        return int(np.prod(POOL[name][0]))
    frames = (call.B - 1) * call.window_stride + RF
    out = {call.x: (frames * frame_floats(call), size(call.x))}
    if call.param is not None:
        out[call.param] = ((call.B if call.param_stride else 1) * E, size(call.param))
    if call.cam is not None:
        width = POOL[call.cam][0][1]
        out[call.cam] = ((call.B if call.cam_stride else 1) * width, size(call.cam))
    return out


KEY_FIELDS = ("variant", "x", "param", "cam", "workspace", "enc_ws", "cam_stride", "enc_bytes", "param_stride")


def bound_key(call):
    """BoundKey (r3d_internal.hpp) as resolve_single builds it, pointers by pool name.  The weight arenas are the handles' and do
    not change between two calls.  `variant` restates pick_schedule: UV input + 2 * (the first levels read the per-frame buffer,
    call_shares_first_layers: stride one frame, one camera, (frames - 2) * 4 <= B * (RF / 3)); the GPU test checks that restatement
    against the kernel the call's launch record names."""
    assert call.mode in ("rays", "uv"), "the pixel pre-pass modes forward rays out of the workspace: not in the directed list"
    uv = call.mode == "uv"
    jf = frame_floats(call)
    frames = (call.B - 1) * call.window_stride + RF
    shared = call.window_stride == 1 and not (uv and call.cam_stride) and (frames - 2) * 4 <= call.B * (RF // 3)
    return {"variant": int(uv) + 2 * int(shared), "x": call.x, "param": call.param, "cam": call.cam, "workspace": call.ws,
            "enc_ws": call.window_stride * jf, "cam_stride": call.cam_stride, "enc_bytes": frames * jf * 4,
            "param_stride": call.param_stride}


def key_diff(a, b):
    ka, kb = bound_key(a), bound_key(b)
    return {f for f in KEY_FIELDS if ka[f] != kb[f]}


# ---- the directed list: pairs of eager single-launch calls at one window count that differ in ONE BoundKey field ----------------
DIRECTED_B = 150
_BASE = Call("rays", "x0", RF, DIRECTED_B, "p0", E, None, 0, "pair")
_UV = Call("uv", "x0", RF, DIRECTED_B, "p0", E, "c0", 8, "pair")
# (name, call A, call B, the key fields that differ).  At a fixed window count enc_ws and enc_bytes are functions of one
# another - frames = (B - 1) * stride + RF - so no two calls of one schedule differ in the window stride or in the frame count
# alone: the stride pair changes exactly those two.  The input kind changes the floats per frame (3 | 2) with the variant: the rays
# call slides by 18 frames and the pixel call by 27 so that enc_ws (918 floats) stays, and enc_bytes moves with the variant; a clip
# call differs from a batch call in variant, stride and frame count by what a clip call is.  Every other pair is one field.
DIRECTED = (
    ("x", _BASE, _BASE._replace(x="x1"), {"x"}),
    ("param", _BASE, _BASE._replace(param="p1"), {"param"}),
    ("param_stride", _BASE._replace(param_stride=0), _BASE, {"param_stride"}),
    ("cam", _UV, _UV._replace(cam="c1"), {"cam"}),
    ("cam_stride", _UV._replace(cam_stride=0), _UV, {"cam_stride"}),
    ("window_stride", _BASE, _BASE._replace(window_stride=13), {"enc_ws", "enc_bytes"}),
    ("variant-rays-uv", _UV._replace(mode="rays", window_stride=18), _UV, {"variant", "enc_bytes"}),
    ("variant-batch-clip", _BASE._replace(param_stride=0), _BASE._replace(param_stride=0, window_stride=1), {"variant", "enc_ws", "enc_bytes"}),
    ("workspace", _BASE, _BASE._replace(ws="other"), {"workspace"}),
)


# ---- seeded sequences -------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)


def sequence(seed):
    """The operations of one seed, a pure function of it.  The ordered pairs (form -> form) and (mutator -> form) are dealt out to
    the seeds round robin, so the shipped seeds together hold every one by construction; a seed's generator only shuffles its
    share, draws buffers and lanes, repeats a call at once now and then (the path that skips the bind) and comes back to an
    earlier call of its own (the state a schedule kept across what ran in between).  A switched-on option is switched off again
    one item later - the host weight path at once: a fresh pair on it costs twenty times one on the device path.  Occurrence k of a form in seed number i runs WINDOW_COUNTS[(len(SEEDS) * k + i) % 11] windows: two
    occurrences per seed give every form every count."""
    idx, n = SEEDS.index(seed), len(SEEDS)
    rng = random.Random(7919 * (seed + 1))
    pairs = [(f, g) for f in FORMS for g in FORMS]
    follows = [(m, f) for m in MUTATORS for f in FORMS]
    items = [("pair", p) for i, p in enumerate(pairs) if i % n == idx] + [("mut", q) for i, q in enumerate(follows) if i % n == idx]
    rng.shuffle(items)
    steps, seen, occ = [], [], collections.Counter()
    pending = []                                       # [items left before the option goes off again, the mutator that does it]

    def forward(form):
        k = occ[form]
        occ[form] += 1
        B = WINDOW_COUNTS[(n * k + idx) % len(WINDOW_COUNTS)]
        fwd = Forward(form, B, 0 if form == "forward_nan" else rng.randrange(2), rng.randrange(2), rng.randrange(2))
        steps.append(fwd)
        seen.append(fwd)
        if rng.random() < 0.25:
            steps.append(fwd)                          # the same call again, at once

    while items or pending:
        if pending and (pending[0][0] <= 0 or not items):
            _, off = pending.pop(0)
            at = next((i for i, it in enumerate(items) if it[0] == "mut" and it[1][0] == off), None)
            if at is None:
                steps.append(off)
                continue
            kind, what = items.pop(at)
        else:
            kind, what = items.pop(0)
        for p in pending:
            p[0] -= 1
        if seen and rng.random() < 0.3:
            steps.append(rng.choice(seen))             # an earlier call of this sequence, as it was
        if kind == "pair":
            if not (steps and isinstance(steps[-1], Forward) and steps[-1].form == what[0]):
                forward(what[0])
            forward(what[1])
        else:
            steps.append(what[0])
            forward(what[1])
            if what[0] in _OFF:
                pending.append([0 if what[0].name == "set_device_weights" else 1, _OFF[what[0]]])
    return steps


def describe(op):
    if isinstance(op, Forward):
        return "%s(B=%d, x%d, side %d, lane %d)" % op
    if isinstance(op, Mutator):
        return "%s(%r)" % op
    return "_run(%s)" % ", ".join("%s=%r" % kv for kv in op._asdict().items())


# ---- camera rows and the float64 ray encoding of the pixel modes (camera.py:423-471 restated for a bare row) ---------------------
def camera_table(seed, width):
    """(BMAX, width) float64 rows {fx, fy, cx, cy, cos(pitch), sin(pitch), 0, 0 [, k1, k2, p1, p2, k3, 0, 0, 0]} of cameras with unit-sized
    intrinsics: the pool's x buffers hold ray components of order one, and the SAME storage read as pixel pairs must encode to
    rays of order one too."""
    from ray3d_amd import synth
    u = synth.hash_uniform("call_history.cam%d" % width, (BMAX, 8), seed)
    rows = np.zeros((BMAX, width), dtype=np.float64)
    rows[:, 0], rows[:, 1] = 1.0 + 0.2 * u[:, 0], 1.0 + 0.2 * u[:, 1]
    rows[:, 2], rows[:, 3] = 0.1 * (u[:, 2] - 0.5), 0.1 * (u[:, 3] - 0.5)
    pitch = -0.1 + 0.4 * u[:, 4]
    rows[:, 4], rows[:, 5] = np.cos(pitch), np.sin(pitch)
    if width == 16:
        rows[:, 8] = -0.05 + 0.02 * u[:, 5]
        rows[:, 9], rows[:, 10], rows[:, 11], rows[:, 12] = 0.01, 0.001 * (u[:, 6] - 0.5), -0.0005, 0.002 * u[:, 7]
    return rows


def rays_of_pixels(uv, row):
    """float64 rays (..., 3) of pixel keypoints (..., 2) under one camera row (8 or 16 doubles; the 16-wide row undistorts first:
    five fixed-point iterations on normalised coordinates, lib/camera/camera.py:412-441 as ray3d_amd.Camera restates it)."""
    uv = np.asarray(uv, dtype=np.float64)
    fx, fy, cx, cy, c, s = (float(v) for v in row[:6])
    x0, y0 = (uv[..., 0] - cx) / fx, (uv[..., 1] - cy) / fy
    x, y = x0, y0
    if len(row) == 16 and np.any(row[8:13] != 0.0):
        k1, k2, p1, p2, k3 = (float(v) for v in row[8:13])
        x, y = x0.copy(), y0.copy()
        for _ in range(5):
            r2 = x * x + y * y
            icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return np.stack([x, c * y + s, -s * y + c], axis=-1)


def bits_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Rig:
    """The GPU side: the pool, fresh pairs in a given configuration, one call of any descriptor on a pair, the cold cache, the oracle.
    One per test session (module-level `rig()`): cold results and oracle outputs are computed once and shared."""

    def __init__(self):
        import torch
        import ray3d_amd
        from ray3d_amd import synth
        from conftest import synth_states
        self.dev = torch.device("cuda:0")
        self.mc = ray3d_amd.default_model_config(ARCHITECTURE=ARCH)
        (cp, sp), (ct, st) = synth_states(self.mc)
        assert (cp.receptive_field, cp.num_joints, cp.in_features, cp.extrinsic_dim) == (RF, J, F, E)
        self.cp, self.ct = cp, ct
        # weight set 0: what every other test loads; set 1: the same generator under other seeds
        self.states = [(sp, st), (synth.synth_state(cp, seed=11), synth.synth_state(ct, seed=12))]
        x0 = synth.synth_rays(BMAX, cp, seed=301)
        xn = x0.copy()
        xn[NAN_AT] = np.nan
        self.np = {"x0": x0, "x1": synth.synth_rays(BMAX, cp, seed=302), "xn": xn,
                   "p0": synth.synth_param(BMAX, seed=311), "p1": synth.synth_param(BMAX, seed=312),
                   "pb": synth.synth_param(1, seed=313),
                   "c0": camera_table(1, 8), "c1": camera_table(2, 8), "d0": camera_table(3, 16), "d1": camera_table(4, 16)}
        for name, (shape, dtype) in POOL.items():
            assert self.np[name].shape == shape and str(self.np[name].dtype) == dtype, name
        self.t = {k: torch.from_numpy(v).to(self.dev) for k, v in self.np.items()}
        self.side_stream = torch.cuda.Stream(self.dev)
        self._cold, self._oracle, self._templates = {}, {}, {}
        self.unstable = set()            # forms (or directed calls) whose two fresh pairs disagreed: compared with the oracle instead

    # ---- pairs
    def new_lifter(self, cfg=COLD):
        """A pair that has done nothing: new modules (copies of a template that never made a handle), new handles."""
        import copy
        import ray3d_amd
        if cfg.weights not in self._templates:
            fac = ray3d_amd.Model(self.mc, {}, is_train=False)
            pos, trj = fac.get_pos_model(), fac.get_trj_model()
            self.load(pos, trj, cfg.weights)
            pos.eval(), trj.eval()
            # (parameters on the device: set_device_weights packs them there)
            self._templates[cfg.weights] = ray3d_amd.Ray3DLifter(pos, trj).eval().to(self.dev)
        template = self._templates[cfg.weights]
        assert template.pos._handle is None and template.trj._handle is None
        lifter = copy.deepcopy(template)
        lifter.CLIP_ROUND = 0                                           # a clip of B windows is ONE call of B windows
        lifter.set_device_weights(cfg.device_weights)
        if cfg.staged:
            lifter.set_staged(True)
        if cfg.lanes:
            lifter.set_lanes(cfg.lanes, self.dev)
        return lifter

    def load(self, pos, trj, which):
        import torch
        import ray3d_amd
        sp, st = self.states[which]
        ray3d_amd.load_weight(pos, {k: torch.from_numpy(np.asarray(v)) for k, v in sp.items()})
        ray3d_amd.load_weight(trj, {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})

    def mutate(self, lifter, mut):
        import torch
        if mut.name == "set_staged":
            lifter.set_staged(mut.arg)
        elif mut.name == "refresh_weights":
            lifter.pos.refresh_weights()
            lifter.trj.refresh_weights()
        elif mut.name == "load_state_dict":
            self.load(lifter.pos, lifter.trj, mut.arg)
        elif mut.name == "set_device_weights":
            lifter.set_device_weights(mut.arg)
        elif mut.name == "prepare":
            lifter.prepare(list(mut.arg), self.dev)
        elif mut.name == "release_prepared":
            lifter.release_prepared()
        else:
            assert mut.name == "set_lanes", mut
            torch.cuda.synchronize(self.dev)
            lifter.set_lanes(mut.arg, self.dev)

    # ---- one call
    def _views(self, call):
        x = self.t[call.x]
        jf = frame_floats(call)
        frames = (call.B - 1) * call.window_stride + RF
        return x, x.view(-1)[:frames * jf].view(frames, J, jf // J)

    def run(self, lifter, fwd, cfg):
        """One Forward on `lifter` (which is in configuration `cfg`): the tuple of its outputs, finished."""
        import torch
        call, B, f = call_of(fwd), fwd.B, fwd.form
        x, seq = self._views(call)
        p = self.t[call.param]
        pv = p[:B] if call.param_stride else p[0]
        cam = None if call.cam is None else (self.t[call.cam][:B] if call.cam_stride else self.t[call.cam][0])

        def go():
            if f in ("forward", "forward_nan"):
                return lifter(x[:B], pv)
            if f == "forward_trj":
                return lifter(x[:B], pv, return_trj=True)
            if f == "split":
                return lifter.forward_split(x[:B], pv)
            if f in ("uv_rows", "uv_bcast", "uv_dist"):
                return lifter.forward_uv(seq.view(B, RF, J, 2), cam, pv)
            if f == "clip":
                return lifter.forward_clip(seq, pv)
            if f == "pos_alone":
                return lifter.pos(x[:B], pv)
            assert f == "trj_alone", f
            return lifter.trj(x[:B], pv)

        with torch.no_grad():
            if f == "graph":
                res = self._graph(lifter, x[:B], pv, B, cfg, fwd.lane)
            elif not cfg.lanes:
                res = go()
            elif f in ("pos_alone", "trj_alone"):
                # a module alone: the lanes are its own handle's, and a forward on any other stream would be relayed round robin
                h = (lifter.pos if f == "pos_alone" else lifter.trj).handle(self.dev)
                st = torch.cuda.ExternalStream(h.lane_stream(fwd.lane), device=self.dev)
                torch.cuda.synchronize(self.dev)
                with torch.cuda.stream(st):
                    res = go()
            else:
                with lifter.lane(fwd.lane):
                    res = go()
                lifter.join_lanes()
        torch.cuda.synchronize(self.dev)
        return tuple(t.clone() for t in (res if isinstance(res, tuple) else (res,)))

    def _graph(self, lifter, xv, pv, B, cfg, lane):
        """prepare, capture one forward of B windows (on the lane's own stream while lanes are on), replay it once, drop the graph."""
        import torch
        from ray3d_amd import _capi
        if (self.dev, B) not in lifter._prepared:
            lifter.prepare([B], self.dev)
        hp, ht = lifter.pos.handle(self.dev), lifter.trj.handle(self.dev)          # (a pending weight refresh happens here, not under capture)
        stream = lifter.lane_stream(lane) if cfg.lanes else self.side_stream
        (lifter._lane_ws[lane] if cfg.lanes else lifter._ws).get(_capi.workspace_bytes(hp, ht, B), self.dev)
        out = torch.empty((B, 1, J, 3), dtype=torch.float32, device=self.dev)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(stream):
            with torch.cuda.graph(g, stream=stream):
                lifter._run(_capi.R3D_INPUT_RAYS, xv, RF, B, pv, E, out=out)
        out.zero_()
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(stream):
            g.replay()
        torch.cuda.synchronize(self.dev)
        g.reset()
        return out

    def run_call(self, lifter, call, other_ws=None):
        """One directed Call through Ray3DLifter._run (the arguments the entry points hide): (poses,), finished."""
        import torch
        from ray3d_amd import _capi
        assert call.mode in ("rays", "uv") and call.ws in ("pair", "other")
        with torch.no_grad():
            out = lifter._run(_capi.R3D_INPUT_RAYS if call.mode == "rays" else _capi.R3D_INPUT_UV, self.t[call.x], call.window_stride,
                              call.B, self.t[call.param], call.param_stride, None if call.cam is None else self.t[call.cam], call.cam_stride,
                              workspace=other_ws if call.ws == "other" else None)
        torch.cuda.synchronize(self.dev)
        return (out.clone(),)

    # ---- the oracle: float64 encoding, oracle/torch_port.py per network (what test_gpu_parity._oracle_lift runs), windows are
    # independent, so every call is evaluated once at BMAX windows and a call of B windows is held to the first B rows
    def oracle(self, call, weights):
        import torch
        from oracle import torch_port
        key = (call._replace(B=BMAX, ws="pair"), weights)
        if key not in self._oracle:
            c = key[0]
            for name, (need, have) in extents(c).items():
                assert need <= have, (name, need, have)
            jf = frame_floats(c)
            frames = (BMAX - 1) * c.window_stride + RF
            seq = self.np[c.x].reshape(-1)[:frames * jf].reshape(frames, J, jf // J)
            wins = np.stack([seq[i * c.window_stride:i * c.window_stride + RF] for i in range(BMAX)])
            if c.mode != "rays":
                rows = self.np[c.cam]
                wins = np.stack([rays_of_pixels(wins[i], rows[i if c.cam_stride else 0]) for i in range(BMAX)]).astype(np.float32)
            prm = self.np[c.param]
            prm = prm[:BMAX] if c.param_stride else np.repeat(prm[:1], BMAX, axis=0)
            sds = [{k: torch.from_numpy(np.asarray(v)) for k, v in s.items()} for s in self.states[weights]]
            with torch.no_grad():
                xw, pw = torch.from_numpy(np.ascontiguousarray(wins)), torch.from_numpy(np.ascontiguousarray(prm))
                pos, trj = torch_port.forward(self.cp, sds[0], xw, pw), torch_port.forward(self.ct, sds[1], xw, pw)
                self._oracle[key] = {"pos": pos.numpy(), "trj": trj.numpy(), "sum": (pos + trj).numpy()}
        return self._oracle[key]

    def hold_to_oracle(self, outs, kinds, call, weights, what):
        """check_parity of every output (the literal 1e-4) - for the NaN variant on the windows that hold no NaN, and the NaN window is NaN."""
        from conftest import check_parity
        ref = self.oracle(call, weights)
        rows = np.arange(call.B)
        if call.x == "xn" and call.B > NAN_AT[0]:
            rows = rows[rows != NAN_AT[0]]
            assert bool(outs[0][NAN_AT[0]].isnan().any()), what + ": the window that holds the NaN must not come out finite"
        for t, kind in zip(outs, kinds):
            assert t.shape[0] == call.B, (what, t.shape)
            check_parity(t.cpu().numpy()[rows], ref[kind][:call.B][rows], "%s %s" % (what, kind))

    # ---- the cold reference
    def cold(self, op, cfg=COLD):
        """The outputs of `op` (a Forward, or a directed Call) as the ONLY call of a fresh pair in configuration `cfg`.  Once per key:
        two fresh pairs must agree bit for bit (else the key's form is noted in `unstable`), and the result is held to the oracle."""
        import warnings
        directed = isinstance(op, Call)
        key = (op, cfg) if directed else (op._replace(lane=op.lane if cfg.lanes else 0), cfg)     # (the lane matters only with lanes)
        if key not in self._cold:
            got = []
            for _ in range(2):
                lifter = self.new_lifter(cfg)
                if directed:
                    from ray3d_amd.modules import _Workspace
                    got.append(self.run_call(lifter, op, _Workspace()))
                else:
                    got.append(self.run(lifter, op, cfg))
                lifter.check_status(self.dev)
                del lifter
            call = op if directed else call_of(op)
            kinds = ("sum",) if directed else OUTPUTS[op.form]
            self.hold_to_oracle(got[0], kinds, call, cfg.weights, "cold " + describe(op))
            if not all(bits_equal(a, b) for a, b in zip(got[0], got[1])):
                self.unstable.add(op if directed else op.form)
                warnings.warn("call history: two fresh pairs disagree on %s in %s - its results are held to the oracle instead" % (describe(op), cfg))
            self._cold[key] = got[0]
        return self._cold[key]

    def compare(self, outs, op, cfg, what):
        """`outs` of a call with a history against the cold reference: bit for bit (NaN windows: NaN where the reference is)."""
        directed = isinstance(op, Call)
        want = self.cold(op, cfg)
        call = op if directed else call_of(op)
        if (op if directed else op.form) in self.unstable:
            self.hold_to_oracle(outs, ("sum",) if directed else OUTPUTS[op.form], call, cfg.weights, what)
            return
        assert len(outs) == len(want), what
        for i, (a, b) in enumerate(zip(outs, want)):
            if call.x == "xn":
                nan = b.isnan()
                assert bool((a.isnan() == nan).all()), "%s: output %d is NaN elsewhere than the fresh pair's" % (what, i)
                a, b = a.masked_fill(nan, 0.0), b.masked_fill(nan, 0.0)
            if not bits_equal(a, b):
                bad = (a.contiguous().view(-1, a.shape[-2] * 3) != b.contiguous().view(-1, b.shape[-2] * 3)).any(dim=1).nonzero().flatten().tolist()
                err = float((a.double() - b.double()).abs().max())
                raise AssertionError("%s: output %d differs from the same call on fresh handles in windows %s%s (max abs diff %.3e)"
                                     % (what, i, bad[:8], " ..." if len(bad) > 8 else "", err))


_RIG = []


def rig():
    if not _RIG:
        _RIG.append(Rig())
    return _RIG[0]
