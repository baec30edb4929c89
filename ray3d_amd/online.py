"""Live streams lifted a frame at a time (r3d_streams_step, include/ray3d_hip.h): several cameras each deliver one new frame of 2D
keypoints per tick and each wants its newest pose back.  :class:`OnlineLifter` keeps a head and a ring of the last RF frames per
stream in device memory; a tick is one r3d_streams_step call - the new frames go into the rings, the windows of the frames that
are now complete are written into a fixed (S, RF, J, F) batch - followed by the plain forward of that batch.  Nothing is rebuilt
from a history with torch ops, nothing is encoded twice, and the whole tick can be captured into one hipGraph.
"""
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _capi, evaluate

IDLE, PUSH, RESTART, DRAIN = _capi.R3D_STREAM_IDLE, _capi.R3D_STREAM_PUSH, _capi.R3D_STREAM_RESTART, _capi.R3D_STREAM_DRAIN


class OnlineLifter:
    """`num_streams` live streams through `lifter` (a :class:`Ray3DLifter`), one frame per stream and tick.

    `encoding`: None - :meth:`step` takes model-input rows (S, J, F), copied bit for bit - or "ray" / "intrinsic" / "screen": it
    takes raw pixels (S, J, 2), encoded on the device through the streams' camera rows (:meth:`set_cameras`) by the routine
    r3d_clips_encode writes with.  The window of a CAUSAL model ends at the newest frame (lag 0: a pose per pushed frame); a
    centred model's pose of frame n needs the `pad` frames behind it (lag = pad): it is emitted `pad` ticks later, and the last
    `pad` frames of a stream that ends come out of :meth:`drain`.  `flip`: the reference's test-time flip (trainer.py:299-353) -
    the mirrored windows are gathered by the same call (`kps_left` / `kps_right`), lifted by a second forward, and the two passes
    averaged through :func:`evaluate.mirror_output` (`joints_left` / `joints_right`, default the keypoint lists).
    `world` / `quality`: the tick's finished poses come from ONE r3d_streams_poses call instead of the torch flip finish - the same
    float32 poses, and beside them (:meth:`step`'s third value) the poses in world coordinates (cam.normalized2world, float64) and
    / or the re-projection residual of every joint against the keypoints that were fed in, in undistorted pixels, with its mean
    and maximum per stream: the quality signal of a stream without ground truth.  Both read the streams' transform rows
    (:meth:`set_cameras` ``transforms=``, :meth:`Camera.stream_pose_row`); `quality` needs a 3-feature (ray) model and the camera
    rows - with ``encoding=None`` they are then passed to :meth:`set_cameras` as well.  Off by default: the tick is then exactly
    what it was.
    `repair` (an int K in 0 .. RF - 1, None: off): the streams survive dropped keypoints - r3d_streams_repair runs in front of the
    step of every tick.  Frames may then hold non-finite entries (a joint the detector did not deliver), and :meth:`step` takes
    detector confidences (`min_conf`: a joint below it counts as not delivered).  A missing joint is held at its last observed
    value; when it comes back after a gap of at most K frames, the frames of the gap that are still to be emitted are interpolated
    (K = 0: hold only); a joint missing from a stream's start is back-filled from its first observation.  :meth:`step` then
    returns ``extras["synthetic"]``: per stream the bit mask of the joints of the emitted frame that were not observed.
    `previews` (a strictly increasing sequence of 1 .. 8 looks, each in 0 .. lag - 1; None: off; centred models only): early
    poses.  A centred model's pose of a frame comes `lag` ticks after the frame; with previews every tick also enqueues
    r3d_streams_peek behind its final forward - for every look L the window the reference builds when the clip ENDS at this tick's
    frame, for the frame L ticks old - and lifts the K * S preview windows with ONE more forward (and the mirrored one with `flip`),
    finished the way the final poses are.  :meth:`step` then returns ``extras["previews"]``.  A small look is early and has seen
    little of the future (look 0: the newest frame, no future at all); look lag - 1 lacks one frame only.  A preview is superseded
    by the final pose of its frame `lag - L` ticks later and never revised; the final poses are bit for bit what they are without
    previews.  With `repair` the previews are lifted from the repaired ring.
    `groups` (a list of lists of stream indices, e.g. ``[[0, 3], [1, 2, 4]]``; None: off; needs `world`): several cameras watch the
    same person - every tick also enqueues ONE r3d_streams_fuse call behind r3d_streams_poses, and :meth:`step` returns one world
    skeleton per group: per joint the weighted mean of the world poses of the group's streams that finished a frame this tick.
    With `quality` the weight of a joint is 1 / (`fuse_soft_px`^2 + residual^2) and a residual above `fuse_max_px` (> 0) drops
    the joint of that stream; without it every weight is 1.  With `repair` a held or interpolated keypoint does not vote against
    an observed one.  `fuse_max_dist` (metres, > 0): of cameras that disagree, only those within that distance of the weighted
    medoid are kept - of two, the one with the smaller residual.  A group has 1 .. 16 members (or none: its rows are NaN); the
    table lives on the device, has room for 16 members per group and is rewritten by :meth:`set_groups`.  The final poses, world
    poses and quality outputs are bit for bit what they are without groups.  Previews are NOT fused: extras["previews"] stay
    per stream.
    `cameras` (an int C; None: off; with `max_detections` D): the streams are C cameras x P = `num_streams` / C slots (stream
    s = c * P + p, P <= 32) and :meth:`track` takes what a 2D detector delivers - per camera and tick an unordered list of up to
    D <= 32 skeletons with joints missing - instead of :meth:`step`'s per-stream rows: ONE r3d_streams_assign call in front of the
    tick associates each camera's detections with its slots (greedy, by the mean joint distance to the slot's last observation
    over the detection's size, at most `assign_max_cost`), starts a track on a free slot for a detection nobody claims (at least
    `assign_min_joints` observed joints, default min(4, J); a match needs `assign_min_common` joints in common, default
    min(3, J)), keeps a track alive through `assign_max_missed` unmatched ticks and then ends it (the slot drains and is free
    again), and writes the tick's actions, frame rows and confidences on the device.  `assign_fill`: what an unmatched live slot
    pushes - "nan" (needs `repair`, which then holds or interpolates the joints) or "hold" (the per-joint last observation).
    Identities are per camera: (camera, extras["track_id"]) names a track.  Which camera's track is which person is decided on the
    device with `people=` (below); without it a caller maps the tracks to people and drives :meth:`set_groups`.
    :meth:`set_cameras` is unchanged: a camera's row is repeated over its P slots.  Without `cameras` nothing of the class changes.
    `people` (an int G in 1..32; None: off; needs `cameras` and `world`, excludes `groups`): the cameras are `scenes` rooms of
    `cameras` / `scenes` <= 16 cameras each that see the same people, and every :meth:`track` tick also enqueues ONE
    r3d_streams_link call between r3d_streams_poses and r3d_streams_fuse: it keeps G people per scene in device memory, links each
    camera's finished tracks to the person whose reference pose is nearest (the mean joint distance of the world poses, at most
    `link_max_dist` metres, over at least `link_min_common` common joints, default min(3, J)), starts a person for a track nobody
    claims (at least `link_min_joints` finite joints, default min(4, J)), unlinks a track whose identity changed or ended - with
    `link_break_dist` (metres, > 0, >= `link_max_dist`) also one that moved that far from its person -, frees a person that had
    no link for more than `link_max_missed` ticks, and writes the member table the fuse call of the same tick reads: the fuse
    buffers have `scenes` * G rows, person n * G + g in row n * G + g, and :meth:`set_groups` raises.  Nothing comes back to the
    host in between, so :meth:`capture` records the whole tick from detections to one fused skeleton per person.  Such a lifter
    takes :meth:`track` only: :meth:`step` and :meth:`lift_clips` refuse it.  Without `people` nothing of the class changes.
    The lifter is prepared for batches of `num_streams` windows (and of K * `num_streams` with previews) here, once."""

    def __init__(self, lifter, num_streams: int, encoding: Optional[str] = None, flip: bool = False,
                 kps_left: Sequence[int] = (), kps_right: Sequence[int] = (), joints_left: Optional[Sequence[int]] = None,
                 joints_right: Optional[Sequence[int]] = None, device=None, world: bool = False, quality: bool = False,
                 repair: Optional[int] = None, min_conf: float = 0.0, previews: Optional[Sequence[int]] = None,
                 groups: Optional[Sequence[Sequence[int]]] = None, fuse_soft_px: float = 2.0, fuse_max_px: float = 0.0,
                 fuse_max_dist: float = 0.0, cameras: Optional[int] = None, max_detections: Optional[int] = None,
                 assign_max_cost: float = 0.5, assign_max_missed: int = 5, assign_min_joints: Optional[int] = None,
                 assign_min_common: Optional[int] = None, assign_fill: str = "nan", people: Optional[int] = None, scenes: int = 1,
                 link_max_dist: float = 0.5, link_break_dist: float = 0.0, link_max_missed: int = 25,
                 link_min_joints: Optional[int] = None, link_min_common: Optional[int] = None):
        pos = lifter.pos
        if lifter.num_lanes():
            raise ValueError("OnlineLifter: a lifter with lanes is not supported (set_lanes(0) first)")
        self.lifter = lifter
        self.S, self.rf, self.J, self.F = int(num_streams), lifter.receptive_field(), pos.num_joints_in, pos.in_features
        self.lag = 0 if pos.cfg.causal else pos.pad
        if encoding is None:
            self.encoding, self.width = _capi.R3D_ENCODE_NONE, self.F
        else:
            self.encoding, self.width = evaluate._encoding_id(encoding, "encoding"), 2
            if _capi.ENCODE_FLOATS[self.encoding] != self.F:
                raise ValueError("encoding=%r writes %d floats per keypoint; this pair takes %d" % (encoding, _capi.ENCODE_FLOATS[self.encoding], self.F))
        nbytes = _capi.streams_state_bytes(self.S, self.rf, self.J, self.F)
        if nbytes == 0:
            raise ValueError("OnlineLifter: num_streams must be in 1..%d (got %d)" % (_capi.CLIPS_MAX, self.S))
        self.flip = bool(flip)
        self.world, self.quality = bool(world), bool(quality)
        if self.quality and self.F != 3:
            raise ValueError("OnlineLifter: quality=True is defined for 3-feature (ray) inputs only; this pair takes %d" % self.F)
        self.looks = self._check_looks(previews, self.lag) if previews is not None else None
        self.G, table = 0, None
        if people is not None:          # the member table is r3d_streams_link's output: scenes * people rows, empty until the first tick
            if groups is not None:
                raise ValueError("OnlineLifter: people= writes the member table itself; it excludes groups=")
            if cameras is None or not self.world:
                raise ValueError("OnlineLifter: people= needs cameras= (the tracks it links) and world=True (the poses it compares)")
            self.G = self._link_shape(people, scenes, cameras)
            table = np.full((self.G, _capi.FUSE_MAX_MEMBERS), -1, np.int32)
        if groups is not None:
            if not self.world:
                raise ValueError("OnlineLifter: groups need world=True (the streams' world poses are what is fused)")
            table = self._member_table(groups, None, self.S)
            self.G = table.shape[0]
        if self.G:
            self.fuse_soft_px, self.fuse_max_px, self.fuse_max_dist = float(fuse_soft_px), float(fuse_max_px), float(fuse_max_dist)
            if not np.isfinite(self.fuse_soft_px) or self.fuse_soft_px <= 0:
                raise ValueError("OnlineLifter: fuse_soft_px must be finite and > 0 (got %r)" % (fuse_soft_px,))
            if np.isnan(self.fuse_max_px) or np.isnan(self.fuse_max_dist):
                raise ValueError("OnlineLifter: fuse_max_px and fuse_max_dist must not be NaN (<= 0 switches them off)")
        if self.looks and _capi.streams_state_bytes(len(self.looks) * self.S, self.rf, self.J, self.F) == 0:
            raise ValueError("OnlineLifter: len(previews) * num_streams must be in 1..%d (got %d)" % (_capi.CLIPS_MAX, len(self.looks) * self.S))
        self.perm = evaluate.mirror_permutation(self.J, kps_left, kps_right) if self.flip else None
        self.joints = (list(kps_left if joints_left is None else joints_left), list(kps_right if joints_right is None else joints_right))
        dev = self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        S, rf, J, F = self.S, self.rf, self.J, self.F
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)                 # all zero: S freshly reset streams
        self.x = torch.zeros((S, rf, J, F), dtype=torch.float32, device=dev)
        self.x_mirror = torch.zeros((S, rf, J, F), dtype=torch.float32, device=dev) if self.flip else None
        self.emit = torch.full((S,), -1, dtype=torch.int64, device=dev)
        self.status = torch.zeros((S,), dtype=torch.int32, device=dev)
        self.frame = torch.zeros((S, J, self.width), dtype=torch.float32, device=dev)
        self.action = torch.zeros((S,), dtype=torch.int32, device=dev)
        self.cam = torch.zeros((S, 16), dtype=torch.float64, device=dev) if encoding is not None or self.quality else None
        self.param = torch.zeros((S, pos.extrinsic_dim), dtype=torch.float32, device=dev) if pos.camera_embedding else None
        self.transforms = self._finish = None
        if self.world or self.quality:  # r3d_streams_poses: the descriptors, the forwards' raw outputs and what the call writes
            self.transforms = torch.zeros((S, 14), dtype=torch.float64, device=dev)
            self._finish = dict(raw=torch.zeros((S, 1, J, 3), dtype=torch.float32, device=dev),
                                raw_m=torch.zeros((S, 1, J, 3), dtype=torch.float32, device=dev) if self.flip else None,
                                pred=torch.zeros((S, 1, J, 3), dtype=torch.float32, device=dev),
                                world=torch.zeros((S, J, 3), dtype=torch.float64, device=dev) if self.world else None,
                                reproj=torch.zeros((S, J), dtype=torch.float64, device=dev) if self.quality else None,
                                quality=torch.zeros((S, 2), dtype=torch.float64, device=dev) if self.quality else None)
        self.repair, self.min_conf = None, float(min_conf)
        if repair is not None:          # r3d_streams_repair: the track, the confidences, the repaired frame and the mask words
            if isinstance(repair, bool) or int(repair) != repair or not 0 <= int(repair) <= rf - 1:
                raise ValueError("OnlineLifter: repair must be an int in 0..%d (got %r)" % (rf - 1, repair))
            if not np.isfinite(self.min_conf):
                raise ValueError("OnlineLifter: min_conf must be finite (got %r)" % (min_conf,))
            self.repair = int(repair)
            self.repair_track = torch.zeros(_capi.streams_track_bytes(S, rf, J, self.width), dtype=torch.uint8, device=dev)   # all zero: fresh
            self.frame_out = torch.zeros((S, J, self.width), dtype=torch.float32, device=dev)
            self.conf = torch.zeros((S, J), dtype=torch.float32, device=dev)
            self.synthetic = torch.zeros((S,), dtype=torch.int32, device=dev)      # (uint32 words: 17 bits are used)
            self._use_conf = False
        self._fuse = None
        if self.G:                      # r3d_streams_fuse: the member table and what the call writes
            M = _capi.FUSE_MAX_MEMBERS
            self.member = torch.from_numpy(table).to(dev)
            self._fuse = dict(fused=torch.zeros((self.G, J, 3), dtype=torch.float64, device=dev),
                              fused_spread=torch.zeros((self.G, J), dtype=torch.float64, device=dev),
                              fused_count=torch.zeros((self.G, J), dtype=torch.int32, device=dev),
                              fused_used=torch.zeros((self.G, M), dtype=torch.int32, device=dev))      # (uint32 words: 17 bits are used)
        self._assign, self._tracking, self._use_det_conf = None, False, False
        if cameras is not None:         # r3d_streams_assign: its state, the detections and what the call writes beside action / frame / conf
            self._assign = self._assign_setup(cameras, max_detections, assign_max_cost, assign_max_missed, assign_min_joints,
                                              assign_min_common, assign_fill)
        elif max_detections is not None:
            raise ValueError("OnlineLifter: max_detections needs cameras=")
        self._link = None
        if people is not None:          # r3d_streams_link: its state and what the call writes beside the member table
            self._link = self._link_setup(people, scenes, link_max_dist, link_break_dist, link_max_missed, link_min_joints, link_min_common)
        self._pfinish = self._pv = None
        if self.looks:                  # r3d_streams_peek: K * S preview windows, their words, and the K-fold copies of the streams' rows
            K = len(self.looks)
            self.px = torch.zeros((K, S, rf, J, F), dtype=torch.float32, device=dev)
            self.px_mirror = torch.zeros((K, S, rf, J, F), dtype=torch.float32, device=dev) if self.flip else None
            self.pemit = torch.full((K, S), -1, dtype=torch.int64, device=dev)
            self.pstatus = torch.zeros((K, S), dtype=torch.int32, device=dev)
            self._ptiled = {name: torch.zeros((K * S,) + tuple(buf.shape[1:]), dtype=buf.dtype, device=dev) if buf is not None else None
                            for name, buf in (("cam_rows", self.cam), ("params", self.param), ("transforms", self.transforms))}
            if self._finish is not None:
                self._pfinish = dict(raw=torch.zeros((K * S, 1, J, 3), dtype=torch.float32, device=dev),
                                     raw_m=torch.zeros((K * S, 1, J, 3), dtype=torch.float32, device=dev) if self.flip else None,
                                     pred=torch.zeros((K * S, 1, J, 3), dtype=torch.float32, device=dev),
                                     world=torch.zeros((K * S, J, 3), dtype=torch.float64, device=dev) if self.world else None,
                                     reproj=torch.zeros((K * S, J), dtype=torch.float64, device=dev) if self.quality else None,
                                     quality=torch.zeros((K * S, 2), dtype=torch.float64, device=dev) if self.quality else None)
        self._cameras_set = self.cam is None and self.param is None and self.transforms is None
        self._graph = None
        self._captured = None       # the captured tick's (poses, out, out_mirror) buffers
        if self.flip:               # the flip finish without host-built index tensors: what a captured tick runs
            out_perm = evaluate.mirror_permutation(J, *self.joints)
            self._out_perm_host = [int(v) for v in out_perm]
            self._out_perm = torch.tensor(out_perm, dtype=torch.int64, device=dev)
            self._out_sign = torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float32, device=dev)
        lifter.prepare([S] + ([len(self.looks) * S] if self.looks else []), dev)

    def _assign_setup(self, cameras, max_detections, max_cost, max_missed, min_joints, min_common, fill):
        """The arguments of `cameras=` checked -> dict of r3d_streams_assign's parameter block and buffers."""
        S, J, dev = self.S, self.J, self.device

        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        if not integer(cameras) or cameras < 1 or S % int(cameras) or not 1 <= S // int(cameras) <= _capi.ASSIGN_MAX_SLOTS:
            raise ValueError("OnlineLifter: num_streams must be cameras * P with P in 1..%d slots per camera (got num_streams=%d, "
                             "cameras=%r)" % (_capi.ASSIGN_MAX_SLOTS, S, cameras))
        if not integer(max_detections) or not 1 <= max_detections <= _capi.ASSIGN_MAX_DETECTIONS:
            raise ValueError("OnlineLifter: cameras= needs max_detections in 1..%d (got %r)" % (_capi.ASSIGN_MAX_DETECTIONS, max_detections))
        C, D = int(cameras), int(max_detections)
        min_joints = min(4, J) if min_joints is None else min_joints
        min_common = min(3, J) if min_common is None else min_common
        if not integer(min_joints) or not integer(min_common) or not 1 <= min_joints <= J or not 1 <= min_common <= J:
            raise ValueError("OnlineLifter: assign_min_joints and assign_min_common must be in 1..%d (got %r, %r)" % (J, min_joints, min_common))
        if not integer(max_missed) or max_missed < 0:
            raise ValueError("OnlineLifter: assign_max_missed must be an int >= 0 (got %r)" % (max_missed,))
        if not np.isfinite(float(max_cost)) or float(max_cost) <= 0:
            raise ValueError("OnlineLifter: assign_max_cost must be finite and > 0 (got %r)" % (max_cost,))
        if fill not in ("nan", "hold"):
            raise ValueError("OnlineLifter: assign_fill must be 'nan' or 'hold' (got %r)" % (fill,))
        if fill == "nan" and self.repair is None:
            raise ValueError("OnlineLifter: assign_fill='nan' needs repair= (r3d_streams_repair holds or interpolates the missing "
                             "frames); assign_fill='hold' pushes the last observation instead")
        if not np.isfinite(self.min_conf):
            raise ValueError("OnlineLifter: min_conf must be finite (got %r)" % (self.min_conf,))
        prm = _capi.assign_params(C, S // C, D, J, self.width, self.lag, int(min_joints), int(min_common), int(max_missed),
                                  _capi.R3D_ASSIGN_FILL_NAN if fill == "nan" else _capi.R3D_ASSIGN_FILL_HOLD, self.min_conf, float(max_cost))
        return dict(prm=prm, C=C, D=D,
                    state=torch.zeros(_capi.streams_assign_bytes(C, S // C, J, self.width), dtype=torch.uint8, device=dev),   # all zero: no tracks
                    det=torch.zeros((C, D, J, self.width), dtype=torch.float32, device=dev),
                    det_conf=torch.zeros((C, D, J), dtype=torch.float32, device=dev),
                    det_count=torch.zeros((C,), dtype=torch.int32, device=dev),
                    track_id=torch.full((S,), -1, dtype=torch.int64, device=dev),
                    match=torch.full((S,), -1, dtype=torch.int32, device=dev),
                    assign_stats=torch.zeros((C, 4), dtype=torch.int32, device=dev))

    def _link_shape(self, people, scenes, cameras) -> int:
        """`people=`, `scenes=` and the cameras checked -> the number of people, scenes * people."""
        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        if not integer(people) or not 1 <= people <= _capi.LINK_MAX_PEOPLE:
            raise ValueError("OnlineLifter: people must be an int in 1..%d (got %r)" % (_capi.LINK_MAX_PEOPLE, people))
        if not integer(scenes) or scenes < 1 or not integer(cameras) or cameras < 1 or cameras % int(scenes) \
                or cameras // int(scenes) > _capi.FUSE_MAX_MEMBERS:
            raise ValueError("OnlineLifter: cameras must be scenes * C with C in 1..%d cameras per scene (got cameras=%r, scenes=%r)"
                             % (_capi.FUSE_MAX_MEMBERS, cameras, scenes))
        if int(scenes) * int(people) > _capi.CLIPS_MAX:
            raise ValueError("OnlineLifter: scenes * people must be in 1..%d (got %d)" % (_capi.CLIPS_MAX, int(scenes) * int(people)))
        return int(scenes) * int(people)

    def _link_setup(self, people, scenes, max_dist, break_dist, max_missed, min_joints, min_common):
        """The arguments of `people=` checked -> dict of r3d_streams_link's parameter block and buffers."""
        S, J, dev, z = self.S, self.J, self.device, self._assign
        N, G = int(scenes), int(people)

        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        min_joints = min(4, J) if min_joints is None else min_joints
        min_common = min(3, J) if min_common is None else min_common
        if not integer(min_joints) or not integer(min_common) or not 1 <= min_joints <= J or not 1 <= min_common <= J:
            raise ValueError("OnlineLifter: link_min_joints and link_min_common must be in 1..%d (got %r, %r)" % (J, min_joints, min_common))
        if not integer(max_missed) or max_missed < 0:
            raise ValueError("OnlineLifter: link_max_missed must be an int >= 0 (got %r)" % (max_missed,))
        max_dist, break_dist = float(max_dist), float(break_dist)
        if not np.isfinite(max_dist) or max_dist <= 0:
            raise ValueError("OnlineLifter: link_max_dist must be finite and > 0 (got %r)" % (max_dist,))
        if np.isnan(break_dist) or (break_dist > 0 and (not np.isfinite(break_dist) or break_dist < max_dist)):
            raise ValueError("OnlineLifter: link_break_dist must be <= 0 (off) or finite and >= link_max_dist (got %r)" % (break_dist,))
        C = z["C"] // N
        prm = _capi.link_params(N, C, S // z["C"], G, _capi.FUSE_MAX_MEMBERS, J, int(min_joints), int(min_common), int(max_missed),
                                max_dist, break_dist)
        return dict(prm=prm, N=N, G=G,
                    state=torch.zeros(_capi.streams_link_bytes(N, C, G, J), dtype=torch.uint8, device=dev),      # all zero: no people
                    person_id=torch.full((N * G,), -1, dtype=torch.int64, device=dev),
                    stream_person=torch.full((S,), -1, dtype=torch.int32, device=dev),
                    link_stats=torch.zeros((N, 4), dtype=torch.int32, device=dev))

    @staticmethod
    def _check_looks(previews, lag: int):
        if lag == 0:
            raise ValueError("OnlineLifter: previews need a centred model - this pair is causal (lag 0): a look lies in 0..lag - 1")
        try:
            looks = tuple(previews)
            ok = all(not isinstance(v, bool) and int(v) == v for v in looks)
        except (TypeError, ValueError):
            looks, ok = (), False
        if not ok or not 1 <= len(looks) <= _capi.STREAMS_PEEK_MAX:
            raise ValueError("OnlineLifter: previews must be a sequence of 1..%d ints (got %r)" % (_capi.STREAMS_PEEK_MAX, previews))
        looks = tuple(int(v) for v in looks)
        if min(looks) < 0 or max(looks) > lag - 1:
            raise ValueError("OnlineLifter: every look of previews must be in 0..%d = lag - 1 (got %r)" % (lag - 1, looks))
        if any(b <= a for a, b in zip(looks, looks[1:])):
            raise ValueError("OnlineLifter: previews must be strictly increasing (got %r)" % (looks,))
        return looks

    @staticmethod
    def _member_table(groups, num_groups, num_streams):
        """The (G, FUSE_MAX_MEMBERS) int32 member table of `groups`, empty slots -1; `num_groups`: the number it must have."""
        M = _capi.FUSE_MAX_MEMBERS
        try:
            rows = [[v for v in g] for g in groups]
            ok = all(not isinstance(v, bool) and int(v) == v for g in rows for v in g)
        except (TypeError, ValueError):
            rows, ok = [], False
        if not ok or not 1 <= len(rows) <= _capi.CLIPS_MAX:
            raise ValueError("OnlineLifter: groups must be a list of 1..%d lists of stream indices (got %r)" % (_capi.CLIPS_MAX, groups))
        if num_groups is not None and len(rows) != num_groups:
            raise ValueError("set_groups: the lifter was built for %d groups (got %d)" % (num_groups, len(rows)))
        table = np.full((len(rows), M), -1, np.int32)
        for g, row in enumerate(rows):
            if len(row) > M:
                raise ValueError("OnlineLifter: group %d has %d members; r3d_streams_fuse takes at most %d" % (g, len(row), M))
            if any(not 0 <= int(v) < num_streams for v in row):
                raise ValueError("OnlineLifter: group %d names a stream outside 0..%d (got %r)" % (g, num_streams - 1, row))
            table[g, :len(row)] = [int(v) for v in row]
        return table

    # ---- setup -----------------------------------------------------------------------------------------------------------
    def set_groups(self, groups):
        """Who watches whom has changed: rewrites the member table on the device - the buffer the ticks read, also the captured
        one - so that the NEXT tick fuses the new groups.  The number of groups stays what the lifter was built with; a group may
        be empty."""
        if self._link is not None:
            raise ValueError("set_groups: a lifter built with people= writes its member table on the device (r3d_streams_link)")
        if not self.G:
            raise ValueError("set_groups: needs an OnlineLifter built with groups=")
        self.member.copy_(torch.from_numpy(self._member_table(groups, self.G, self.S)))

    def set_cameras(self, cam_rows=None, params=None, transforms=None):
        """The streams' cameras: `cam_rows` (S, 16) float64 - :meth:`Camera.cam_row` with distortion=True, what the pixel encodings
        and `quality` read -, `params` (S, E) float32, the forward's camera-parameter rows (models with a camera embedding), and
        `transforms` (S, 14) float64 - :meth:`Camera.stream_pose_row`, needed with `world` or `quality`.  Copied into the buffers
        the ticks read (also the captured one's): it may be called between ticks."""
        for given, buf, name, dtype in ((cam_rows, self.cam, "cam_rows", torch.float64), (params, self.param, "params", torch.float32),
                                        (transforms, self.transforms, "transforms", torch.float64)):
            if buf is None:
                continue
            if given is None:
                raise ValueError("set_cameras: %s %s are needed" % (name, tuple(buf.shape)))
            t = torch.as_tensor(given).to(dtype)
            if tuple(t.shape) != tuple(buf.shape):
                raise ValueError("set_cameras: %s must be %s (got %s)" % (name, tuple(buf.shape), tuple(t.shape)))
            buf.copy_(t)
            if self.looks:              # the preview batch's rows: look k, stream s at row k * S + s
                self._ptiled[name].copy_(buf.repeat((len(self.looks),) + (1,) * (buf.dim() - 1)))
        self._cameras_set = True

    # ---- one tick --------------------------------------------------------------------------------------------------------
    def _mirror_finish(self, pred, pred_m):
        """0.5 * (pred + mirror_output(pred_m)) with device-resident indices (the values of evaluate.mirror_output exactly: a
        negation and a permutation)."""
        return 0.5 * (pred + pred_m.index_select(2, self._out_perm) * self._out_sign)

    def _tick(self, out=None, out_m=None, pout=None, pout_m=None):
        """r3d_streams_step, the forward(s), the flip finish - on the current stream -> poses (S, 1, J, 3).  With previews the tick
        goes on behind them: r3d_streams_peek, the preview batch's forward(s) and finish (:meth:`_preview_tick`)."""
        poses = self._final_tick(out, out_m)
        if self.looks:
            self._pv = self._preview_tick(pout, pout_m)
        return poses

    def _preview_tick(self, out=None, out_m=None):
        """r3d_streams_peek behind the tick's final forward, ONE forward over the K * S preview windows (and the mirrored one), and
        the finish in use - the torch flip average, or one r3d_streams_poses call over K * S pseudo-streams that reads the peek's
        emit and status words -> preview poses (K * S, 1, J, 3), look k, stream s at row k * S + s."""
        dev, lifter, KS = self.device, self.lifter, len(self.looks) * self.S
        with torch.cuda.device(dev):
            _capi.streams_peek(self.state.data_ptr(), self.S, self.rf, self.lag, self.J, self.F, self.looks, self.action.data_ptr(),
                               self.status.data_ptr(), self.px.data_ptr(), self.px_mirror.data_ptr() if self.flip else None, self.perm,
                               self.pemit.data_ptr(), self.pstatus.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        x = self.px.view(KS, self.rf, self.J, self.F)
        xm = self.px_mirror.view(KS, self.rf, self.J, self.F) if self.flip else None
        param, E = self._ptiled["params"], lifter.pos.extrinsic_dim
        f = self._pfinish
        if f is not None:
            lifter._run(_capi.R3D_INPUT_RAYS, x, self.rf, KS, param, E, out=f["raw"])
            if self.flip:
                lifter._run(_capi.R3D_INPUT_RAYS, xm, self.rf, KS, param, E, out=f["raw_m"])

            def ptr(t):
                return t.data_ptr() if t is not None else None
            with torch.cuda.device(dev):
                _capi.streams_poses(ptr(f["raw"]), ptr(f["raw_m"]), KS, self.J, self._out_perm_host if self.flip else None,
                                    self.pemit.data_ptr(), self.pstatus.data_ptr(), self._ptiled["transforms"].data_ptr(),
                                    ptr(self._ptiled["cam_rows"]), x.data_ptr(), self.rf, self.lag, ptr(f["pred"]), ptr(f["world"]),
                                    ptr(f["reproj"]), ptr(f["quality"]), torch.cuda.current_stream(dev).cuda_stream, in_features=self.F)
            return f["pred"]
        if out is None:             # eager: the public forward, the reference's flip finish
            pred = lifter.forward(x, param)
            if self.flip:
                pred = 0.5 * (pred + evaluate.mirror_output(lifter.forward(xm, param), *self.joints))
            return pred
        pred = lifter._run(_capi.R3D_INPUT_RAYS, x, self.rf, KS, param, E, out=out)
        if self.flip:
            pred = self._mirror_finish(pred, lifter._run(_capi.R3D_INPUT_RAYS, xm, self.rf, KS, param, E, out=out_m))
        return pred

    def _final_tick(self, out=None, out_m=None):
        dev, lifter = self.device, self.lifter
        if self._tracking:              # the tick's actions, frame rows and confidences come from the detections
            z = self._assign
            with torch.cuda.device(dev):
                _capi.streams_assign(z["state"].data_ptr(), z["prm"], z["det"].data_ptr(),
                                     z["det_conf"].data_ptr() if self._use_det_conf else None, z["det_count"].data_ptr(),
                                     self.action.data_ptr(), self.frame.data_ptr(), self.conf.data_ptr() if self.repair is not None else None,
                                     z["match"].data_ptr(), z["track_id"].data_ptr(), z["assign_stats"].data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream)
        frame = self.frame
        if self.repair is not None:     # the repaired frame is what the step pushes
            with torch.cuda.device(dev):
                _capi.streams_repair(self.state.data_ptr(), self.repair_track.data_ptr(), self.S, self.rf, self.lag, self.J, self.F, self.encoding,
                                     self.frame.data_ptr(), self.conf.data_ptr() if self._use_conf else None, self.min_conf,
                                     self.cam.data_ptr() if self.cam is not None and self.encoding != _capi.R3D_ENCODE_NONE else None,
                                     self.action.data_ptr(), self.repair, self.frame_out.data_ptr(), self.synthetic.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream)
            frame = self.frame_out
        with torch.cuda.device(dev):
            _capi.streams_step(self.state.data_ptr(), self.S, self.rf, self.lag, self.J, self.F, self.encoding, frame.data_ptr(),
                               self.cam.data_ptr() if self.cam is not None else None, self.action.data_ptr(), self.x.data_ptr(),
                               self.x_mirror.data_ptr() if self.flip else None, self.perm, self.emit.data_ptr(), self.status.data_ptr(),
                               torch.cuda.current_stream(dev).cuda_stream)
        if self._finish is not None:
            return self._finish_tick()
        if out is None:             # eager: the public forward, the reference's flip finish
            pred = lifter.forward(self.x, self.param)
            if self.flip:
                pred = 0.5 * (pred + evaluate.mirror_output(lifter.forward(self.x_mirror, self.param), *self.joints))
            return pred
        E = lifter.pos.extrinsic_dim
        pred = lifter._run(_capi.R3D_INPUT_RAYS, self.x, self.rf, self.S, self.param, E, out=out)
        if self.flip:
            pred = self._mirror_finish(pred, lifter._run(_capi.R3D_INPUT_RAYS, self.x_mirror, self.rf, self.S, self.param, E, out=out_m))
        return pred

    def _finish_tick(self):
        """The forward(s) into the (S, 1, J, 3) buffers, then ONE r3d_streams_poses call: the flip average, the world transform and
        the residuals of the streams that finished a frame this tick - eagerly and under capture alike -> poses (S, 1, J, 3)."""
        dev, lifter, f = self.device, self.lifter, self._finish
        E = lifter.pos.extrinsic_dim
        lifter._run(_capi.R3D_INPUT_RAYS, self.x, self.rf, self.S, self.param, E, out=f["raw"])
        if self.flip:
            lifter._run(_capi.R3D_INPUT_RAYS, self.x_mirror, self.rf, self.S, self.param, E, out=f["raw_m"])

        def ptr(t):
            return t.data_ptr() if t is not None else None
        with torch.cuda.device(dev):
            _capi.streams_poses(ptr(f["raw"]), ptr(f["raw_m"]), self.S, self.J, self._out_perm_host if self.flip else None,
                                self.emit.data_ptr(), self.status.data_ptr(), self.transforms.data_ptr(), ptr(self.cam), self.x.data_ptr(),
                                self.rf, self.lag, ptr(f["pred"]), ptr(f["world"]), ptr(f["reproj"]), ptr(f["quality"]),
                                torch.cuda.current_stream(dev).cuda_stream, in_features=self.F)
            if self._link is not None:      # the member table of this tick: the cameras' tracks linked to people
                k, t = self._link, self._assign
                _capi.streams_link(k["state"].data_ptr(), k["prm"], ptr(f["world"]), self.emit.data_ptr(), self.status.data_ptr(),
                                   t["track_id"].data_ptr(), self.member.data_ptr(), k["person_id"].data_ptr(),
                                   k["stream_person"].data_ptr(), k["link_stats"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            if self._fuse is not None:      # one more launch: the groups' skeletons from what the call above just wrote
                z = self._fuse
                _capi.streams_fuse(ptr(f["world"]), ptr(f["reproj"]), self.emit.data_ptr(), self.status.data_ptr(),
                                   self.synthetic.data_ptr() if self.repair is not None else None, self.S, self.J, self.member.data_ptr(),
                                   self.G, _capi.FUSE_MAX_MEMBERS, self.fuse_soft_px, self.fuse_max_px, self.fuse_max_dist,
                                   ptr(z["fused"]), ptr(z["fused_spread"]), ptr(z["fused_count"]), ptr(z["fused_used"]),
                                   torch.cuda.current_stream(dev).cuda_stream)
        return f["pred"]

    def _extras(self):
        f = self._finish
        out = {k: f[k].clone() for k in ("world", "reproj", "quality") if f[k] is not None} if f is not None else {}
        if self.repair is not None:
            out["synthetic"] = self.synthetic.clone()
        if self._fuse is not None:
            out.update({k: v.clone() for k, v in self._fuse.items()})
        if self._tracking:
            out.update({k: self._assign[k].clone() for k in ("track_id", "match", "assign_stats")})
        if self._link is not None:
            out.update({k: self._link[k].clone() for k in ("person_id", "stream_person", "link_stats")})
        if self.looks:
            K, S, p = len(self.looks), self.S, self._pfinish
            poses, frames = self._pv.clone().view(K, S, self.J, 3), self.pemit.clone()
            more = {k: p[k].clone().view((K, S) + tuple(p[k].shape[1:])) for k in ("world", "reproj", "quality") if p[k] is not None} if p else {}
            out["previews"] = [dict({k: v[i] for k, v in more.items()}, look=L, poses=poses[i], frames=frames[i]) for i, L in enumerate(self.looks)]
        return out

    def step(self, frame=None, actions=None, check: bool = True, conf=None):
        """One tick.  `frame` (S, J, 2) pixels or (S, J, F) model-input rows, a tensor or an array (None: no stream delivers one -
        a tick of DRAIN / IDLE actions); `actions` (S,) R3D_STREAM_* words (None: every stream PUSHes).
        -> (poses (S, J, 3), frames (S,) int64): frames[s] is the index of the frame poses[s] belongs to - the newest one for a causal
        model, `pad` frames back for a centred one - or -1: stream s has no pose this tick and poses[s] is not meaningful.
        With `world` / `quality` -> (poses, frames, extras): a dict with "world" (S, J, 3) float64, "reproj" (S, J) float64 pixels
        and "quality" (S, 2) float64 (mean, max of the stream's residuals) - the keys that were asked for; rows of streams without
        a pose this tick are not meaningful (they keep what an earlier tick left).
        With `repair` -> (poses, frames, extras) as well: extras["synthetic"] (S,) int32, bit j set = joint j of the frame the pose
        belongs to was not observed (held, interpolated or back-filled); the "reproj" of such a joint compares the prediction with
        a made-up keypoint.  `frame` may then hold non-finite entries, and `conf` (S, J) detector confidences may be given: a joint
        below `min_conf` (or with a NaN confidence) counts as not delivered.  A lifter that was captured takes `conf` on every tick
        or on none.
        With `previews` -> (poses, frames, extras) as well: extras["previews"] is a list with one dict per look L, in the order
        given: "look" L, "poses" (S, J, 3), "frames" (S,) int64 - frames[s] the frame the early pose of stream s belongs to (the
        newest one less L), or -1: stream s has no preview this tick (it did not PUSH, or holds no more than L frames) and its
        rows are not meaningful - and, with `world` / `quality`, "world" (S, J, 3), "reproj" (S, J) and "quality" (S, 2) of the
        preview poses.  A preview is never revised: the final pose of that frame arrives `lag - L` ticks later in `poses`.
        With `groups` -> extras["fused"] (G, J, 3) float64, one world skeleton per group; extras["fused_spread"] (G, J) float64,
        the weighted RMS distance in metres of the contributing cameras from the fused joint; extras["fused_count"] (G, J) int32,
        how many cameras contributed (0: no member of the group delivered the joint this tick - "fused" and "fused_spread" are
        NaN there); extras["fused_used"] (G, 16) int32, bit j of word (g, m) set = the m-th member of group g contributed to
        joint j.  Previews are not fused.
        Raises on a refused stream (an unknown action, a PUSH after a drain began: RESTART starts the next clip) unless `check`
        is off - the check reads the status words back, the tick's one synchronisation."""
        if not self._cameras_set:
            raise RuntimeError("OnlineLifter: call set_cameras first (this configuration reads camera rows / parameter rows)")
        if self._link is not None:
            raise ValueError("step: a lifter built with people= links the tracks r3d_streams_assign keeps: it takes track() only")
        if self._assign is not None and self._graph is not None:
            raise ValueError("step: the captured tick of a lifter built with cameras= starts with r3d_streams_assign: use track()")
        self._tracking = False
        if frame is not None:
            t = torch.as_tensor(frame)
            if tuple(t.shape) != tuple(self.frame.shape):
                raise ValueError("step: frame must be %s (got %s)" % (tuple(self.frame.shape), tuple(t.shape)))
            self.frame.copy_(t.to(torch.float32))
        elif actions is None:
            raise ValueError("step: without a frame the actions must be given")
        if conf is not None:
            if self.repair is None:
                raise ValueError("step: conf needs an OnlineLifter built with repair=")
            c = torch.as_tensor(conf)
            if tuple(c.shape) != (self.S, self.J):
                raise ValueError("step: conf must be %s (got %s)" % ((self.S, self.J), tuple(c.shape)))
            if self._graph is not None and not self._use_conf:
                raise ValueError("step: the captured tick was recorded without confidences")
            self.conf.copy_(c.to(torch.float32))
            self._use_conf = True
        elif self.repair is not None:
            if self._graph is not None and self._use_conf:
                raise ValueError("step: the captured tick was recorded with confidences")
            self._use_conf = False
        if actions is None:
            self.action.fill_(PUSH)
        else:
            a = torch.as_tensor(actions)
            if tuple(a.shape) != (self.S,):
                raise ValueError("step: actions must be (%d,) (got %s)" % (self.S, tuple(a.shape)))
            self.action.copy_(a.to(torch.int32))
        return self._run_tick(check)

    def track(self, detections, counts, conf=None, check: bool = True):
        """One tick from a detector's output (a lifter built with `cameras=`): `detections` (C, D, J, 2) pixels or (C, D, J, F)
        model-input rows, a tensor or an array - per camera up to D skeletons in any order, a joint that was not detected
        non-finite; `counts` (C,) how many of each camera's rows are filled (read clamped into 0..D; the rows behind it are not
        looked at); `conf` (C, D, J) detector confidences (a joint below `min_conf`, or with a NaN confidence, counts as not
        detected).  The inputs are copied into persistent device buffers, then r3d_streams_assign, r3d_streams_repair (with
        `repair`), r3d_streams_step and the rest of the tick are enqueued exactly as :meth:`step` does with the actions, frame
        rows and confidences the assign call wrote - nothing comes back to the host in between, and a captured lifter replays
        all of it.  -> (poses, frames, extras) as :meth:`step` returns them, and extras["track_id"] (S,) int64 - the identity of
        the track in slot s this tick, counted per camera from 0, -1 for a free slot; a track keeps its identity and its slot
        from its first tick to the last pose of its drain -, extras["match"] (S,) int32 - the detection row the slot took this
        tick (matched or born from), -1 for none: the slot pushed a synthetic frame, drains or is free - and
        extras["assign_stats"] (C, 4) int32: the camera's valid detections, the matched ones, the births and the valid
        detections that found no free slot.  A track's last `assign_max_missed` frames before its end are synthetic (nobody was
        matched): with `repair` extras["synthetic"] marks their joints.  Cross-camera grouping: with `people=` the tick links
        the cameras' tracks to people itself - extras["person_id"] (scenes * G,) int64, the identity of the person in row g of the
        fused outputs, counted per scene from 0, -1 for a free row; extras["stream_person"] (S,) int32, the row of the person
        that holds stream s, or -1; extras["link_stats"] (scenes, 4) int32: the scene's live people, the links made by matching,
        the births and the tracks that found no free person; the extras["fused*"] rows are those people's skeletons -; without
        it a caller maps (camera, track_id) to people and calls :meth:`set_groups`.  A lifter that was captured takes `conf` on
        every tick or on none."""
        z = self._assign
        if z is None:
            raise ValueError("track: needs an OnlineLifter built with cameras=")
        if not self._cameras_set:
            raise RuntimeError("OnlineLifter: call set_cameras first (this configuration reads camera rows / parameter rows)")
        t = torch.as_tensor(detections)
        if tuple(t.shape) != tuple(z["det"].shape):
            raise ValueError("track: detections must be %s (got %s)" % (tuple(z["det"].shape), tuple(t.shape)))
        n = torch.as_tensor(counts)
        if tuple(n.shape) != (z["C"],):
            raise ValueError("track: counts must be (%d,) (got %s)" % (z["C"], tuple(n.shape)))
        if conf is not None:
            c = torch.as_tensor(conf)
            if tuple(c.shape) != tuple(z["det_conf"].shape):
                raise ValueError("track: conf must be %s (got %s)" % (tuple(z["det_conf"].shape), tuple(c.shape)))
        if self._graph is not None and self._use_det_conf != (conf is not None):
            raise ValueError("track: the captured tick was recorded %s confidences" % ("with" if self._use_det_conf else "without"))
        z["det"].copy_(t.to(torch.float32))
        z["det_count"].copy_(n.to(torch.int32))
        if conf is not None:
            z["det_conf"].copy_(c.to(torch.float32))
        self._use_det_conf = conf is not None
        self._tracking = True
        if self.repair is not None:     # the repair reads the confidences the assign call writes (1.0 without a detector's)
            self._use_conf = True
        return self._run_tick(check)

    def _run_tick(self, check: bool):
        """The tick on the buffers as they stand - replayed when captured - and what :meth:`step` returns."""
        with torch.no_grad():
            if self._graph is not None:
                self._graph.replay()
                poses = self._captured[0].clone()
            else:
                poses = self._tick()
                if self._finish is not None:
                    poses = poses.clone()
        frames = self.emit.clone()
        extras = self._extras() if self._finish is not None or self.repair is not None or self.looks or self._tracking else None
        if check:
            bad = torch.nonzero(self.status).flatten().tolist()
            if bad:
                raise RuntimeError("r3d_streams_step refused streams %s (an unknown action, a PUSH after a drain began, or a "
                                   "corrupted head): RESTART them" % bad)
        return (poses[:, 0], frames) if extras is None else (poses[:, 0], frames, extras)

    def drain(self, check: bool = True) -> List[tuple]:
        """The streams have ended: `lag` ticks of DRAIN for every stream -> the list of their (poses, frames) - with `world` /
        `quality` (poses, frames, extras), as :meth:`step` returns them.  Nothing for a
        causal model.  Afterwards a stream takes RESTART (its next clip), not PUSH."""
        act = torch.full((self.S,), DRAIN, dtype=torch.int32)
        return [self.step(None, act, check) for _ in range(self.lag)]

    def lift_clips(self, clips: Sequence, cam_rows=None, params=None, transforms=None, world: bool = False, previews: bool = False) -> list:
        """Clips of unequal length - at most S arrays (N_k, J, 2 or F) - fed side by side, one stream each: RESTART, PUSH ..., the
        drain when a clip ends, then IDLE.  -> per clip its poses (N_k, J, 3) in frame order: what the reference's evaluation
        computes for the clip (edge padding, eval_data_prepare, the forward, the flip average).
        `world` (a lifter built with `world` and / or `quality`): -> per clip (poses, extras), `extras` the frames' rows of what
        :meth:`step` returns third - "world" (N_k, J, 3) float64, "reproj" (N_k, J) and "quality" (N_k, 2), the keys asked for, and
        with `repair` "synthetic" (N_k,) int32.  With `repair` the clips may hold non-finite entries (joints that were not detected).
        `previews` (a lifter built with `previews`): -> per clip (poses, extras) as well, and extras["previews"] is a list with one
        dict per look L: "look" L, "poses" (max(N_k - L, 0), J, 3) - the early poses of the frames 0 .. N_k - 1 - L in frame order,
        each lifted when the stream held L more frames than it; the clip's last L frames never get that preview, so a clip of no
        more than L frames has none - and the frames' "world" / "reproj" / "quality" rows where the lifter was built with them.
        Comparing these poses and `poses[:N_k - L]` with ground truth (:mod:`ray3d_amd.metrics`) is what a look costs in accuracy.
        With `groups` and `world`: -> (the per-clip list, fused): `fused` has one dict per group - "fused" (T_g, J, 3), "fused_spread"
        (T_g, J), "fused_count" (T_g, J) and "fused_used" (T_g, 16), row n the group's skeleton of frame n.  The clips start together,
        so frame n of every clip is emitted by the same tick; T_g is the length of the longest clip among the group's members
        (0 when no member carries a clip)."""
        if self._link is not None:
            raise ValueError("lift_clips: a lifter built with people= links the tracks r3d_streams_assign keeps: it takes track() only")
        if len(clips) > self.S:
            raise ValueError("lift_clips: %d clips on %d streams" % (len(clips), self.S))
        if world and self._finish is None and self.repair is None:
            raise ValueError("lift_clips: world=True needs an OnlineLifter built with world=True, quality=True or repair=")
        if previews and not self.looks:
            raise ValueError("lift_clips: previews=True needs an OnlineLifter built with previews=")
        if cam_rows is not None or params is not None or transforms is not None:
            self.set_cameras(cam_rows, params, transforms)
        clips = [np.ascontiguousarray(torch.as_tensor(c).cpu().numpy(), dtype=np.float32) for c in clips]
        lengths = [c.shape[0] for c in clips]
        if min(lengths) < 1:
            raise ValueError("lift_clips: a clip needs at least one frame")
        outs = [torch.empty((n, self.J, 3), dtype=torch.float32, device=self.device) for n in lengths]
        seen = [0] * len(clips)
        rows = {k: v for k, v in (self._finish or {}).items() if k in ("world", "reproj", "quality") and v is not None}
        if self.repair is not None:
            rows["synthetic"] = self.synthetic
        more = [{k: torch.empty((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=self.device) for k, v in rows.items()} for n in lengths]
        early = None
        if previews:                # per clip and look: the rows of the frames 0 .. N - 1 - L
            prow = dict({k: v for k, v in (self._pfinish or {}).items() if k in ("world", "reproj", "quality") and v is not None}, poses=torch.empty((0, self.J, 3), dtype=torch.float32))
            early = [[dict({k: torch.empty((max(n - L, 0),) + tuple(v.shape[1:]), dtype=v.dtype, device=self.device) for k, v in prow.items()},
                           look=L) for L in self.looks] for n in lengths]
            early_seen = [[0] * len(self.looks) for _ in lengths]
        fused = None
        if world and self._fuse is not None:
            spans = [max([lengths[s] for s in row if 0 <= s < len(clips)], default=0) for row in self.member.cpu().tolist()]
            fused = [{k: torch.empty((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=self.device) for k, v in self._fuse.items()} for n in spans]
        frame = np.zeros(tuple(self.frame.shape), np.float32)
        for t in range(max(lengths) + self.lag):
            act = np.full(self.S, IDLE, np.int32)
            for s, (c, n) in enumerate(zip(clips, lengths)):
                if t < n:
                    act[s], frame[s] = (RESTART if t == 0 else PUSH), c[t]
                elif t < n + self.lag:
                    act[s] = DRAIN
            poses, frames, *extras = self.step(frame, act)
            for s, n in enumerate(frames.tolist()[:len(clips)]):
                if n >= 0:
                    outs[s][n] = poses[s]
                    for k, v in (extras[0].items() if extras else ()):
                        if k != "previews" and not k.startswith("fused"):
                            more[s][k][n] = v[s]
                    seen[s] += 1
            for g, rows_g in enumerate(fused or ()):       # (every clip began at tick 0: this tick emits frame t - lag)
                if 0 <= t - self.lag < rows_g["fused"].shape[0]:
                    for k, dst in rows_g.items():
                        dst[t - self.lag] = extras[0][k][g]
            for i, pv in enumerate(extras[0]["previews"] if previews else ()):
                for s, n in enumerate(pv["frames"].tolist()[:len(clips)]):
                    if n >= 0:
                        for k, dst in early[s][i].items():
                            if k != "look":
                                dst[n] = pv[k][s]
                        early_seen[s][i] += 1
        assert seen == lengths, (seen, lengths)
        if previews:
            assert early_seen == [[max(n - L, 0) for L in self.looks] for n in lengths], (early_seen, lengths)
            for s in range(len(clips)):
                more[s]["previews"] = early[s]
        per_clip = list(zip(outs, more)) if world or previews else outs
        return (per_clip, fused) if fused is not None else per_clip

    # ---- capture ---------------------------------------------------------------------------------------------------------
    def capture(self):
        """Record one tick - r3d_streams_assign (with `cameras`: the captured lifter then takes :meth:`track`, not :meth:`step`),
        r3d_streams_repair (with `repair`), r3d_streams_step, the forward or forwards, the flip finish
        (with `people` r3d_streams_link and with `groups` or `people` r3d_streams_fuse behind it), and with
        `previews` r3d_streams_peek, the preview batch's forward or forwards and their finish - into
        a hipGraph on a side stream; from then on :meth:`step` copies its inputs into the captured buffers and replays it.  The streams' state is not touched:
        capture may come between two ticks."""
        if self._graph is not None:
            return
        if not self._cameras_set:
            raise RuntimeError("OnlineLifter: call set_cameras before capture")
        dev, S, J = self.device, self.S, self.J
        out = torch.empty((S, 1, J, 3), dtype=torch.float32, device=dev)
        out_m = torch.empty((S, 1, J, 3), dtype=torch.float32, device=dev) if self.flip else None
        E = self.lifter.pos.extrinsic_dim
        pout = pout_m = None
        with torch.no_grad():       # the workspace and the schedules exist before the capture: nothing allocates inside it
            if self.looks:          # (the larger batch first: the grow-only workspace is then final)
                KS = len(self.looks) * S
                pout = torch.empty((KS, 1, J, 3), dtype=torch.float32, device=dev)
                pout_m = torch.empty((KS, 1, J, 3), dtype=torch.float32, device=dev) if self.flip else None
                self.lifter._run(_capi.R3D_INPUT_RAYS, self.px.view(KS, self.rf, J, self.F), self.rf, KS, self._ptiled["params"], E, out=pout)
            self.lifter._run(_capi.R3D_INPUT_RAYS, self.x, self.rf, S, self.param, E, out=out)
        torch.cuda.synchronize(dev)
        self.lifter.check_status(dev)
        if self._assign is not None:    # the recorded tick starts with r3d_streams_assign; its repair reads the confidences it writes
            self._tracking = True
            if self.repair is not None:
                self._use_conf = True
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
        with torch.no_grad(), torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                poses = self._tick(out, out_m, pout, pout_m)
        torch.cuda.synchronize(dev)
        self._graph, self._captured = g, (poses, out, out_m, pout, pout_m)

    def release(self):
        """Drop the captured graph (before the lifter's prepared schedules are released or its options change)."""
        if self._graph is not None:
            torch.cuda.synchronize(self.device)
            self._graph = self._captured = None
