"""Batched evaluation over clips: the caller side of the lifting path.

Reproduces the behaviour of ``Trainer.evaluate_core`` / ``Trainer.evaluate``
(lib/train_val/trainer.py:283-405, :407-483) around the HIP forward:

* a clip is edge-padded by (RF-1)//2 frames per side (lib/dataloader/generators.py:213-216) and
  window i covers padded frames [i, i+RF) (trainer.py:47-58) - the windows are gathered inside
  the first-layer tiles (`Ray3DLifter.forward_clip`), not materialised;
* the camera row [height, pitch] is shared by all windows of the clip (trainer.py:297,324);
* prediction = pos + trj, optionally averaged with the mirrored pass (trainer.py:299-302,338-353);
* prediction and ground truth go to world coordinates in float64 (trainer.py:355-364) and the five
  per-clip errors are accumulated weighted by the number of frames (trainer.py:386-403);
* the 2-feature baselines (RAY_ENCODING False): a clip whose ground truth is in the camera frame (``Clip.frame ==
  "camera"``) goes to the world through camera2world (trainer.py:361-362); without a trajectory model
  (``root_relative=True``) the ground truth is made root-relative and nothing is transformed (trainer.py:319-320, :382-384).

Multi-GPU: whole clips are partitioned over ranks (one process per GPU), each rank evaluates its
share with resident weights, and ONE all_gather of the fixed-size per-clip partial rows
(RCCL over xGMI with the nccl backend, gloo on CPU) brings them together.  There is no other
collective on the path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import metrics as M
from .camera import Camera
from .skeleton import H36M_17_PARENTS, validate_parents

PARTIAL_COLS = 8   # clip_id, action_id, n_frames, sum_mpjpe, sum_pmpjpe, sum_nmpjpe, sum_vel, sum_root


@dataclass
class Clip:
    camera: Camera
    rays: np.ndarray          # (N, J, F) float32 ray-encoded keypoints (model input space; F = 2: the 2-feature encodings)
    gt_norm: np.ndarray       # (N, J, 3) float32 ground truth in the normalised frame (`frame` "camera": the camera frame)
    action: str = ""
    clip_id: int = 0
    frame: str = "normalized"   # the frame of gt_norm and of the predictions: "normalized" | "camera"
    conf: Optional[np.ndarray] = None   # (N, J) float32 keypoint confidences, read by ``repair=`` only (None: every keypoint +inf)


_IDENTITY_R, _IDENTITY_T = np.eye(3, dtype=np.float64), np.zeros((3, 1), dtype=np.float64)


def clip_world_transform(clip: Clip, root_relative: bool = False):
    """(R (3,3), T (3,1)) float64 taking the clip's predictions and ground truth to the frame the errors are measured in:
    Rn2w / Tn2w (normalised frame), Rc2w / Tc2w (camera frame, trainer.py:361-362), identity for root-relative evaluation."""
    if root_relative:
        return _IDENTITY_R, _IDENTITY_T
    if clip.frame == "camera":
        return clip.camera.Rc2w, clip.camera.Tc2w
    if clip.frame != "normalized":
        raise ValueError("Clip.frame must be 'normalized' or 'camera' (got %r)" % (clip.frame,))
    return clip.camera.Rn2w, clip.camera.Tn2w


def root_relative_gt(gt: np.ndarray) -> np.ndarray:
    """trainer.py:319-320 on (N, J, 3): every joint relative to the root, the root itself at the origin."""
    gt = np.array(gt, dtype=np.float32, copy=True)
    gt[:, 1:] -= gt[:, :1]
    gt[:, 0] = 0
    return gt


def pad_clip(rays: np.ndarray, pad: int, causal_shift: int = 0) -> np.ndarray:
    """np.pad(seq, ((pad + shift, pad - shift), (0,0), (0,0)), 'edge') - generators.py:213-216;
    shift = pad for CAUSAL models (main.py:85-89: the window then ends at the frame it predicts)."""
    return np.concatenate([np.repeat(rays[:1], pad + causal_shift, axis=0), rays,
                           np.repeat(rays[-1:], pad - causal_shift, axis=0)], axis=0)


def mirror_input(clip: torch.Tensor, kps_left: Sequence[int], kps_right: Sequence[int]) -> torch.Tensor:
    """trainer.py:299-302: negate x, swap left/right keypoints."""
    out = clip.clone()
    out[..., 0] *= -1
    out[:, list(kps_left) + list(kps_right)] = out[:, list(kps_right) + list(kps_left)]
    return out


def mirror_output(pred: torch.Tensor, joints_left: Sequence[int], joints_right: Sequence[int]) -> torch.Tensor:
    """trainer.py:340-342 on (N,1,J,3) predictions."""
    out = pred.clone()
    out[..., 0] *= -1
    out[:, :, list(joints_left) + list(joints_right)] = out[:, :, list(joints_right) + list(joints_left)]
    return out


def mirror_pixels(camera: Camera, encoding: str, kps_left: Sequence[int], kps_right: Sequence[int]) -> Callable:
    """`mirror` of :func:`predict_clip` for clips that hold RAW PIXELS (lifted through ``forward_uv(..., encoding=)``): the
    reference mirrors the ENCODED input (trainer.py:299-302, x -> -x), and the pixels whose encoding that is are
    u -> res_w - u ("screen": -(u/w*2 - 1) = (w - u)/w*2 - 1) or u -> 2 cx - u ("intrinsic"), computed in float64 and
    rounded once to float32 - equal to the negated encoding up to that rounding of the pixel (<= 2^-24 of it).  Not for an
    undistort=True camera: the tangential terms are not symmetric about the principal point."""
    if encoding == "screen":
        if camera.res_w is None:
            raise ValueError("the screen encoding needs the camera's resolution (res_w, res_h)")
        axis = camera.res_w
    elif encoding == "intrinsic":
        if camera.undistort:
            raise ValueError("mirror_pixels: the pixels of an undistort=True camera have no exact mirror image; undistort on the host first")
        axis = 2.0 * camera.cx
    else:
        raise ValueError("encoding must be 'intrinsic' or 'screen' (got %r)" % (encoding,))

    def mirror(clip: torch.Tensor) -> torch.Tensor:
        out = clip.clone()
        out[..., 0] = (axis - clip[..., 0].to(torch.float64)).to(clip.dtype)
        out[:, list(kps_left) + list(kps_right)] = out[:, list(kps_right) + list(kps_left)]
        return out
    return mirror


def predict_clip(lift_clip: Callable, clip: Clip, rf: int, device, flip: bool = False,
                 kps_left: Sequence[int] = (), kps_right: Sequence[int] = (), causal: bool = False,
                 joints_left: Optional[Sequence[int]] = None, joints_right: Optional[Sequence[int]] = None,
                 mirror: Optional[Callable] = None) -> torch.Tensor:
    """(N,1,J,3) absolute poses in the normalised frame for one clip.
    `lift_clip(padded (N+RF-1,J,F) tensor, param_row (E,) tensor) -> (N,1,J,3)`.
    `mirror`: what makes the mirrored input of the flip pass from the padded one, when the clip does not hold the encoded
    input itself (:func:`mirror_pixels`); default :func:`mirror_input`."""
    pad = (rf - 1) // 2
    padded = torch.from_numpy(pad_clip(np.asarray(clip.rays, dtype=np.float32), pad, pad if causal else 0)).to(device)
    prow = torch.from_numpy(clip.camera.param()).to(device)
    pred = lift_clip(padded, prow)
    if flip:
        pred_m = lift_clip(mirror(padded) if mirror is not None else mirror_input(padded, kps_left, kps_right), prow)
        pred = 0.5 * (pred + mirror_output(pred_m, kps_left if joints_left is None else joints_left,
                                           kps_right if joints_right is None else joints_right))
    return pred


def _header_rows(headers: Sequence[tuple], cols: int, device) -> torch.Tensor:
    """A (k, cols) float64 matrix of per-clip rows with the host-known columns - clip id, action id, frame count - filled in
    and the rest zero, made on the host and moved in ONE host-to-device copy."""
    rows = torch.zeros((len(headers), cols), dtype=torch.float64)
    if headers:
        rows[:, :3] = torch.tensor([[float(v) for v in h] for h in headers], dtype=torch.float64)
    return rows.to(device)


def partial_rows(headers: Sequence[tuple], device) -> torch.Tensor:
    """The (k, PARTIAL_COLS) float64 matrix of a rank's per-clip rows with the host-known columns - clip id, action id,
    frame count - filled in: ONE host-to-device copy per evaluation instead of one per clip (the error columns are written
    on the device by :func:`clip_partials_hip`)."""
    return _header_rows(headers, PARTIAL_COLS, device)


def clip_partials_hip(pred_norm: torch.Tensor, clip: Clip, action_id: int = 0,
                      gt_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      root_relative: bool = False) -> torch.Tensor:
    """clip_partials on the GPU through r3d_clip_metrics: world transform, the five error sums and the per-frame
    Procrustes fits in one float64 kernel on the current stream - no D2H copy of the predictions.
    `gt_dev`: the clip's ground truth already on the device (callers that keep a data set resident in HBM).
    `out`: a row of :func:`partial_rows` (header columns already on the device): only the five sums are written, by a
    device copy - no host tensor, no host synchronisation per clip, whatever the number of ranks.
    The rigid transform is the clip's (:func:`clip_world_transform`); `root_relative`: the clip's ground truth is already
    root-relative (the caller's job, :func:`root_relative_gt`) and the transform is the identity."""
    from . import _capi
    dev = pred_norm.device
    n = pred_norm.shape[0]
    pred = pred_norm.reshape(n, -1, 3).contiguous().float()
    if gt_dev is not None:
        gt = gt_dev.to(dev, torch.float32).reshape(n, -1, 3).contiguous()
    else:
        gt = torch.from_numpy(np.ascontiguousarray(clip.gt_norm, dtype=np.float32)).to(dev, non_blocking=True).reshape(n, -1, 3)
    assert gt.shape == pred.shape, "ground truth %s vs prediction %s" % (tuple(gt.shape), tuple(pred.shape))
    sums = torch.empty(_capi.METRIC_OUT_DOUBLES, dtype=torch.float64, device=dev)
    R, T = clip_world_transform(clip, root_relative)
    _capi.clip_metrics(pred.data_ptr(), gt.data_ptr(), n, pred.shape[1], np.asarray(R, dtype=np.float64),
                       np.asarray(T, dtype=np.float64).reshape(3), sums.data_ptr(),
                       torch.cuda.current_stream(dev).cuda_stream)
    if out is not None:
        assert out.shape == (PARTIAL_COLS,) and out.dtype == torch.float64 and out.device == dev
        out[3:8] = sums[:5]           # R3D_METRIC_* order == columns 3..7 (mpjpe, p-mpjpe, n-mpjpe, velocity, root)
        return out
    row = torch.empty(PARTIAL_COLS, dtype=torch.float64, device=dev)
    for c, v in enumerate((clip.clip_id, action_id, n)):
        row[c].fill_(float(v))        # (scalars travel as kernel arguments: no pageable host tensor, no blocking copy)
    row[3:8] = sums[:5]
    return row


def clip_partials(pred_norm: torch.Tensor, clip: Clip, action_id: int = 0, root_relative: bool = False) -> torch.Tensor:
    """One PARTIAL_COLS row (float64, on pred's device): N-weighted error sums in metres.  Predictions on a GPU
    go through the HIP kernel; CPU tensors (host-logic tests with a stand-in lifter) through torch."""
    if pred_norm.is_cuda:
        return clip_partials_hip(pred_norm, clip, action_id, root_relative=root_relative)
    dev = pred_norm.device
    n = pred_norm.shape[0]
    Rm, Tm = clip_world_transform(clip, root_relative)
    R = torch.from_numpy(Rm.T.copy()).to(dev)
    T = torch.from_numpy(Tm.T.copy()).to(dev)
    pw = pred_norm.to(torch.float64).reshape(n, 1, -1, 3) @ R + T             # trainer.py:358
    gw = torch.from_numpy(np.asarray(clip.gt_norm, dtype=np.float32)).to(dev).to(torch.float64)
    gw = gw.reshape(n, 1, -1, 3) @ R + T                                        # trainer.py:359
    row = torch.zeros(PARTIAL_COLS, dtype=torch.float64, device=dev)
    row[0], row[1], row[2] = clip.clip_id, action_id, n
    row[3] = n * M.mpjpe(pw, gw)                                                # trainer.py:386
    row[4] = n * M.p_mpjpe(pw.reshape(n, -1, 3), gw.reshape(n, -1, 3))          # :393
    row[5] = n * M.n_mpjpe(pw, gw)                                              # :388
    row[6] = n * M.mean_velocity_error(pw.reshape(n, -1, 3), gw.reshape(n, -1, 3))   # :395
    row[7] = n * M.mpjpe(pw[:, :, 0:1], gw[:, :, 0:1])                          # :387
    return row


def reduce_partials(rows: torch.Tensor) -> Dict[int, tuple]:
    """{action_id: (e1, e2, e3, ev, er)} in millimetres - trainer.py:399-403 per action."""
    rows = rows.detach().to("cpu", torch.float64)
    out = {}
    for a in sorted(set(int(v) for v in rows[:, 1].tolist())):
        sel = rows[rows[:, 1] == a]
        n = sel[:, 2].sum()
        out[a] = tuple(float(sel[:, c].sum() / n * 1000.0) for c in (3, 4, 5, 6, 7))
    return out


def reduce_camera_wise(rows: torch.Tensor, camera_index: Sequence[int], camera_ids: Sequence[str]) -> List[tuple]:
    """``CAMERA_WISE_PERFORMANCE`` (lib/train_val/trainer.py:425-446) from the gathered per-clip rows: for every camera
    of the list (file order) and every action, the frame-weighted errors of THAT camera's clips (what
    ``fetch_via_action(..., camera_idx=cam_idx)`` + ``evaluate_core`` produce); after each camera the reference logs
    the mean over all (camera, action) errors collected SO FAR - its lists are not reset between cameras - rounded to
    0.1 mm.  ``camera_index[clip_id]`` is the clip's camera position (``PoseData.camera_index``).
    Returns ``[(camera id, (p1, p2, p3, vel, root))]`` in that cumulative form; :func:`format_camera_report` prints it."""
    rows = rows.detach().to("cpu", torch.float64)
    cam_of = torch.tensor([int(camera_index[int(c)]) for c in rows[:, 0].tolist()], dtype=torch.int64)
    collected: List[List[float]] = []
    out = []
    for ci, cid in enumerate(camera_ids):
        sel_c = rows[cam_of == ci]
        for a in sorted(set(int(v) for v in sel_c[:, 1].tolist())):
            sel = sel_c[sel_c[:, 1] == a]
            n = sel[:, 2].sum()
            collected.append([float(sel[:, c].sum() / n * 1000.0) for c in (3, 4, 5, 6, 7)])
        if collected:
            out.append((str(cid), tuple(round(float(v), 1) for v in np.mean(np.array(collected), axis=0))))
    return out


def format_camera_report(per_camera: Sequence[tuple]) -> List[str]:
    """'CAM ID <id>, p1 p2 p3 vel root' lines (trainer.py:446)."""
    return ["CAM ID %s, %s %s %s %s %s" % ((cid,) + tuple(v)) for cid, v in per_camera]


def action_average(per_action: Dict[int, tuple]) -> tuple:
    """Unweighted mean over actions, rounded to 0.1 mm like trainer.py:473-477."""
    arr = np.array(list(per_action.values()), dtype=np.float64)
    return tuple(round(float(v), 1) for v in arr.mean(axis=0))


# ------------------------------------------------------------------------------------ sharding

def shard_clips(lengths: Sequence[int], world_size: int) -> List[List[int]]:
    """Greedy longest-first bin packing of whole clips by frame count; deterministic, so every rank
    derives the same assignment without communicating."""
    bins: List[List[int]] = [[] for _ in range(world_size)]
    load = [0] * world_size
    for idx in sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i)):
        r = min(range(world_size), key=lambda k: (load[k], k))
        bins[r].append(idx)
        load[r] += int(lengths[idx])
    return bins


def gather_partials(local_rows: torch.Tensor, counts: Sequence[int], group=None, cols: int = PARTIAL_COLS) -> torch.Tensor:
    """The single exchange step: all_gather of per-clip rows (`cols` wide), padded to the largest shard."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    kmax = max(max(counts), 1)
    pad = torch.zeros((kmax, cols), dtype=torch.float64, device=local_rows.device)
    pad[: local_rows.shape[0]] = local_rows
    bucket = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(bucket, pad, group=group)
    return torch.cat([bucket[r][: counts[r]] for r in range(world)], dim=0)


def _shard_plan(clips: Sequence[Clip], rank: int, world_size: int):
    """(actions, aid, shards, mine): the sorted action names, their ids, every rank's clip indices (:func:`shard_clips`) and
    this rank's clips in the order of its shard."""
    actions = sorted(set(c.action for c in clips))
    aid = {a: i for i, a in enumerate(actions)}
    shards = shard_clips([c.rays.shape[0] for c in clips], world_size)
    return actions, aid, shards, [clips[idx] for idx in shards[rank]]


def _shard_rows(clips: Sequence[Clip], aid: Dict[str, int], shard: Sequence[int], cols: int, device) -> torch.Tensor:
    """The `cols`-wide rows of the clips of `shard` (indices into `clips`) with their headers in place (:func:`_header_rows`)."""
    return _header_rows([(idx, aid[clips[idx].action], clips[idx].rays.shape[0]) for idx in shard], cols, device)


def _gather(local: torch.Tensor, shards: Sequence[Sequence[int]], group, cols: int) -> torch.Tensor:
    """The rows of all ranks (:func:`gather_partials`); with one rank they are `local` itself and nothing is exchanged."""
    return gather_partials(local, [len(s) for s in shards], group, cols=cols) if len(shards) > 1 else local


def _report(allrows: torch.Tensor, alldetail: Optional[torch.Tensor], actions: Sequence[str], clips: Sequence[Clip],
            include_root: bool = False):
    """What the evaluations return from the gathered rows: (per_action, action-wise average, rows as gathered) - or, with the
    gathered detail rows, both sorted by clip id and (per_action, average, rows, detail) as :func:`evaluate_clips_detail` describes."""
    if alldetail is not None:
        order = torch.argsort(allrows[:, 0], stable=True)
        allrows, alldetail = allrows[order], alldetail[order]
    per = reduce_partials(allrows)
    named = {actions[a]: v for a, v in per.items()}
    if alldetail is None:
        return named, action_average(per), allrows
    tables = reduce_detail(allrows, alldetail, clips[0].gt_norm.shape[1] if len(clips) else 0, include_root)
    detail = {(actions[a] if a != "overall" else a): t for a, t in tables.items()}
    detail["rows"] = alldetail
    return named, action_average(per), allrows, detail


def evaluate_clips(lift_clip: Callable, clips: Sequence[Clip], rf: int, device, flip: bool = False,
                   kps_left: Sequence[int] = (), kps_right: Sequence[int] = (),
                   rank: int = 0, world_size: int = 1, group=None, causal: bool = False,
                   joints_left: Optional[Sequence[int]] = None, joints_right: Optional[Sequence[int]] = None,
                   root_relative: bool = False, mirror: Optional[Callable] = None):
    """Evaluate `clips` (sharded over `world_size` ranks when > 1; `causal`: pad as main.py:85-89 does for
    CAUSAL models).  Every rank returns
    (per_action {name: (e1,e2,e3,ev,er) mm}, action-wise average, gathered partial rows).
    Each clip is measured in the world frame through the transform of ITS frame (`Clip.frame`); `root_relative` (models
    without a trajectory network, RAY_ENCODING False: trainer.py:315-320, :382-384): the ground truth is made
    root-relative and compared with the predictions as they are.  `mirror`: see :func:`predict_clip` (clips of raw pixels)."""
    actions, aid, shards, _ = _shard_plan(clips, rank, world_size)
    on_gpu = torch.device(device).type == "cuda"
    local = _shard_rows(clips, aid, shards[rank], PARTIAL_COLS, device)
    for k, idx in enumerate(shards[rank]):
        c = clips[idx]
        pred = predict_clip(lift_clip, c, rf, device, flip, kps_left, kps_right, causal, joints_left, joints_right, mirror)
        cc = Clip(c.camera, c.rays, root_relative_gt(c.gt_norm) if root_relative else c.gt_norm, c.action, idx, c.frame)
        if on_gpu and pred.is_cuda:
            clip_partials_hip(pred, cc, aid[c.action], out=local[k], root_relative=root_relative)
        else:
            local[k] = clip_partials(pred, cc, aid[c.action], root_relative)
    return _report(_gather(local, shards, group, PARTIAL_COLS), None, actions, clips)


# ------------------------------------------------------------------------------------ per-joint / per-frame / PCK detail

DETAIL_COLS = M.DETAIL_DOUBLES   # 3 rows of 17 per-joint sums (raw, Procrustes-fitted, root-relative), then 31 PCK counts
PCK_THRESHOLDS_MM = tuple(5.0 * k for k in range(M.DETAIL_THRESHOLDS))


def _clip_detail_hip(pred_norm: torch.Tensor, clip: Clip, gt_dev: Optional[torch.Tensor], frames: bool,
                     root_relative: bool = False):
    """(five sums, detail row, per-frame tensor or None) of one clip through r3d_clip_metrics_detail on the current stream."""
    from . import _capi
    dev = pred_norm.device
    n = pred_norm.shape[0]
    pred = pred_norm.reshape(n, -1, 3).contiguous().float()
    if gt_dev is not None:
        gt = gt_dev.to(dev, torch.float32).reshape(n, -1, 3).contiguous()
    else:
        gt = torch.from_numpy(np.ascontiguousarray(clip.gt_norm, dtype=np.float32)).to(dev, non_blocking=True).reshape(n, -1, 3)
    assert gt.shape == pred.shape, "ground truth %s vs prediction %s" % (tuple(gt.shape), tuple(pred.shape))
    sums = torch.empty(_capi.METRIC_OUT_DOUBLES, dtype=torch.float64, device=dev)
    detail = torch.empty(_capi.DETAIL_OUT_DOUBLES, dtype=torch.float64, device=dev)
    per_frame = torch.empty((n, 5), dtype=torch.float64, device=dev) if frames else None
    R, T = clip_world_transform(clip, root_relative)
    _capi.clip_metrics_detail(pred.data_ptr(), gt.data_ptr(), n, pred.shape[1], np.asarray(R, dtype=np.float64),
                              np.asarray(T, dtype=np.float64).reshape(3), sums.data_ptr(),
                              per_frame.data_ptr() if frames else None, detail.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    return sums[:5], detail[:_capi.DETAIL_DOUBLES], per_frame


def clip_detail(pred_norm: torch.Tensor, clip: Clip, gt_dev: Optional[torch.Tensor] = None, frames: bool = False,
                root_relative: bool = False):
    """The DETAIL_COLS-wide detail row of one clip (float64, on pred's device, metres / counts; layout:
    :func:`ray3d_amd.metrics.clip_detail`), and with `frames` also the (N, 5) per-frame errors in R3D_METRIC_* order.
    Predictions on a GPU go through the HIP kernel; CPU tensors (host-logic tests, a stand-in lifter) through torch."""
    if pred_norm.is_cuda:
        _, detail, per_frame = _clip_detail_hip(pred_norm, clip, gt_dev, frames, root_relative)
        return (detail, per_frame) if frames else detail
    dev = pred_norm.device
    n = pred_norm.shape[0]
    Rm, Tm = clip_world_transform(clip, root_relative)
    R = torch.from_numpy(Rm.T.copy()).to(dev)
    T = torch.from_numpy(Tm.T.copy()).to(dev)
    gt = clip.gt_norm if gt_dev is None else gt_dev.detach().cpu().numpy()
    pw = pred_norm.to(torch.float64).reshape(n, -1, 3) @ R + T
    gw = torch.from_numpy(np.asarray(gt, dtype=np.float32)).to(dev).to(torch.float64).reshape(n, -1, 3) @ R + T
    detail, per_frame = M.clip_detail(pw, gw)
    return (detail, per_frame) if frames else detail


def reduce_detail(rows: torch.Tensor, detail_rows: torch.Tensor, num_joints: int, include_root: bool = False) -> Dict:
    """{action_id: table, "overall": table} from the per-clip partial rows and their detail rows (same row order), frame
    weighted: table = {"mpjpe", "p_mpjpe", "root_rel": per-joint errors in mm (num_joints long), "pck": PCK in percent at
    each of PCK_THRESHOLDS_MM, "pck150": its last entry, "auc": the mean over the thresholds}.  PCK counts the joints whose
    root-relative distance is strictly below the threshold; `include_root` adds the root joint (distance 0 by construction)
    to the count of every threshold above 0 and to the total.  Clips are added up in clip-id order, so the result does
    not depend on how they were sharded."""
    rows = rows.detach().to("cpu", torch.float64)
    detail_rows = detail_rows.detach().to("cpu", torch.float64)
    order = torch.argsort(rows[:, 0], stable=True)
    rows, detail_rows = rows[order], detail_rows[order]
    W, nj = M.DETAIL_MAX_JOINTS, M.DETAIL_JOINT_ROWS * M.DETAIL_MAX_JOINTS

    def table(sel):
        n = rows[sel, 2].sum()
        d = detail_rows[sel].sum(dim=0)
        counts, total = d[nj:].clone(), n * (num_joints - 1)
        if include_root:
            counts[1:] += n
            total = n * num_joints
        pck = (counts / total * 100.0).tolist()
        out = {name: (d[r * W: r * W + num_joints] / n * 1000.0).tolist() for r, name in enumerate(("mpjpe", "p_mpjpe", "root_rel"))}
        out.update(pck=pck, pck150=pck[-1], auc=float(np.mean(pck)))
        return out

    out = {a: table(rows[:, 1] == a) for a in sorted(set(int(v) for v in rows[:, 1].tolist()))}
    out["overall"] = table(torch.ones(rows.shape[0], dtype=torch.bool))
    return out


def evaluate_clips_detail(lift_clip: Callable, clips: Sequence[Clip], rf: int, device, flip: bool = False,
                          kps_left: Sequence[int] = (), kps_right: Sequence[int] = (),
                          rank: int = 0, world_size: int = 1, group=None, causal: bool = False,
                          joints_left: Optional[Sequence[int]] = None, joints_right: Optional[Sequence[int]] = None,
                          include_root: bool = False, root_relative: bool = False, mirror: Optional[Callable] = None):
    """:func:`evaluate_clips` with the per-joint tables and PCK / AUC on top.  Every rank returns
    (per_action, action-wise average, partial rows, detail) - the first three as evaluate_clips does, the rows in clip-id
    order - with detail = {action name: table, "overall": table, "rows": the gathered detail rows} (tables:
    :func:`reduce_detail`).  On a GPU one r3d_clip_metrics_detail call per clip yields both rows; with `world_size` > 1 the
    detail rows travel in ONE additional all_gather.  `Clip.frame`, `root_relative` and `mirror` as in :func:`evaluate_clips`."""
    actions, aid, shards, _ = _shard_plan(clips, rank, world_size)
    on_gpu = torch.device(device).type == "cuda"
    local = _shard_rows(clips, aid, shards[rank], PARTIAL_COLS, device)
    dlocal = torch.zeros((len(shards[rank]), DETAIL_COLS), dtype=torch.float64, device=device)
    for k, idx in enumerate(shards[rank]):
        c = clips[idx]
        pred = predict_clip(lift_clip, c, rf, device, flip, kps_left, kps_right, causal, joints_left, joints_right, mirror)
        cc = Clip(c.camera, c.rays, root_relative_gt(c.gt_norm) if root_relative else c.gt_norm, c.action, idx, c.frame)
        if on_gpu and pred.is_cuda:
            local[k, 3:8], dlocal[k], _ = _clip_detail_hip(pred, cc, None, False, root_relative)
        else:
            local[k] = clip_partials(pred, cc, aid[c.action], root_relative)
            dlocal[k] = clip_detail(pred, cc, root_relative=root_relative)
    return _report(_gather(local, shards, group, PARTIAL_COLS), _gather(dlocal, shards, group, DETAIL_COLS), actions, clips, include_root)


# ------------------------------------------------------------------------------------ the pieces of the calls over a whole shard

def _need(t: torch.Tensor, name: str, dtype, dev, shape=None, rows=None, numel=None, last=None):
    """ValueError unless `t` is a contiguous `dtype` tensor on `dev` of exactly `shape` - or, where two layouts are taken
    ((N, J, 3) and (N, 1, J, 3)), of `rows` leading rows, `numel` elements and a last dimension of `last`, whichever are given."""
    if t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.dim() < 1 \
            or (shape is not None and tuple(t.shape) != tuple(shape)) or (rows is not None and t.shape[0] != rows) \
            or (numel is not None and t.numel() != numel) or (last is not None and t.shape[-1] != last):
        size = "shape %s" % (tuple(shape),) if shape is not None else \
            ", ".join("%s %d" % (k, v) for k, v in (("rows", rows), ("elements", numel), ("last dimension", last)) if v is not None)
        raise ValueError("%s: a contiguous %s tensor (%s) on %s is needed" % (name, dtype, size, dev))


def _need_table(table_dev: torch.Tensor, num_clips: int, desc_bytes: int, dev):
    """ValueError unless `table_dev` holds `num_clips` descriptors of `desc_bytes` bytes (``_capi.CLIP_DESC_BYTES`` /
    ``_capi.CLIP_INPUT_DESC_BYTES``), contiguous, on `dev`."""
    if table_dev.device != dev or not table_dev.is_contiguous() or table_dev.numel() * table_dev.element_size() < num_clips * desc_bytes:
        raise ValueError("table_dev: %d descriptors of %d bytes on %s are needed" % (num_clips, desc_bytes, dev))


_scratch_of: Dict = {}    # device -> the scratch of the shard calls


def _shard_scratch(dev, nbytes: int) -> torch.Tensor:
    """The cached per-device scratch of the shard calls, grown (never shrunk) to `nbytes`."""
    scratch = _scratch_of.get(dev)
    if scratch is None or scratch.numel() < nbytes:
        scratch = _scratch_of[dev] = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    return scratch


def _out_buffer(t: Optional[torch.Tensor], name: str, want: bool, dtype, dev, shape: tuple, exact: bool = True):
    """The caller's output buffer `t` if given - of exactly `shape`, or without `exact` of shape[0] rows and as many elements -
    else a new (not zeroed) one of `shape` if `want`, else None."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev) if want else None
    if exact:
        _need(t, name, dtype, dev, shape=shape)
    else:
        _need(t, name, dtype, dev, rows=shape[0], numel=int(np.prod(shape)))
    return t


def _status_buffer(status: Optional[torch.Tensor], num_clips: int, dev) -> torch.Tensor:
    """The caller's int32 (num_clips,) status buffer, or a new one."""
    return _out_buffer(status, "status", True, torch.int32, dev, (num_clips,))


def _raise_if_refused(status: torch.Tensor, call: str):
    """Reads the status of a shard call (a device-to-host copy: the one synchronisation of the input / finishing side)."""
    bad = torch.nonzero(status).flatten().tolist()
    if bad:
        raise RuntimeError("%s refused the descriptors of clips %s of this rank's shard" % (call, bad))


def _to_device_bytes(table: np.ndarray, dev) -> torch.Tensor:
    """A descriptor table's bytes on `dev`: the one upload of the table."""
    return torch.from_numpy(table.view(np.uint8)).to(dev)


def _ground_truth(mine: Sequence[Clip], dev, root_relative: bool = False) -> torch.Tensor:
    """The shard's ground truth back to back, (total_frames, J, 3) float32 on `dev` in one upload (`root_relative`: made so first)."""
    return torch.from_numpy(np.concatenate(
        [np.ascontiguousarray(root_relative_gt(c.gt_norm) if root_relative else c.gt_norm, dtype=np.float32) for c in mine], axis=0)).to(dev)


def _desc_table(lengths: Sequence[int], transforms: Sequence[tuple]):
    """(table of r3d_clip_desc rows, first_frames, total_frames, max_frames) of clips of these frame counts and (R, T) laid out
    back to back."""
    from . import _capi
    table = np.zeros(len(lengths), dtype=_capi.clip_desc_dtype())
    first_frames, at, longest = [], 0, 0
    for k, (n, (R, T)) in enumerate(zip(lengths, transforms)):
        table[k]["first_frame"], table[k]["n_frames"] = at, n
        table[k]["rn2w"] = np.asarray(R, dtype=np.float64).reshape(9)
        table[k]["tn2w"] = np.asarray(T, dtype=np.float64).reshape(3)
        first_frames.append(at)
        at += n
        longest = max(longest, n)
    return table, first_frames, at, longest


def _lifter_of(lift_clip: Callable, partial_ok: bool = False, need: Optional[str] = None, by_name: bool = False):
    """The object whose bound method `lift_clip` is - with `partial_ok` also through a ``functools.partial`` of one - or None.
    `need` (the option that needs a Ray3DLifter, named in the message): a ValueError unless it has ``clip_batch_sizes`` and, with
    `by_name`, `lift_clip` is its ``forward_clip`` itself (``raw_out=`` is used).  Decided before any shard is cut."""
    lifter = getattr(lift_clip, "__self__", None) or (getattr(getattr(lift_clip, "func", None), "__self__", None) if partial_ok else None)
    if need is not None and (lifter is None or not hasattr(lifter, "clip_batch_sizes")
                             or (by_name and getattr(lift_clip, "__name__", "") != "forward_clip")):
        raise ValueError("%s: lift_clip must be %sthe bound forward_clip of a Ray3DLifter (its clip_batch_sizes%s are used)"
                         % (need, "(a functools.partial of) " if partial_ok else "", " and raw_out=" if by_name else ""))
    return lifter


def _encoding_id(encoding, arg: str = "encode") -> int:
    """R3D_ENCODE_* of the encoding's name; a ValueError names the argument `arg`."""
    if encoding not in ENCODINGS:
        raise ValueError("%s must be one of %s (got %r)" % (arg, sorted(ENCODINGS), encoding))
    return ENCODINGS[encoding]


def _repair_needs_encode(repair, encode):
    """``repair=`` works on the encode call's buffer: a ValueError without ``encode=``, or for a K outside 0..REPAIR_MAX_ROWS."""
    if repair is None:
        return
    from . import _capi
    if encode is None:
        raise ValueError("repair=: the repair works on the encode call's buffer (r3d_clips_encode's output); give encode= and raw pixels")
    if isinstance(repair, bool) or int(repair) != repair or not 0 <= int(repair) <= _capi.REPAIR_MAX_ROWS:
        raise ValueError("repair= must be an integer in 0..%d, the longest gap that is interpolated (got %r)" % (_capi.REPAIR_MAX_ROWS, repair))


class _ShardInputs:
    """What the clips `mine` of a shard are lifted from.  ``inputs(k)`` -> (input of clip k, its mirrored input or None without
    `flip`, the clip's camera parameter row on `dev`, extra keywords of ``lift_clip``):

    * `encode` None: ``Clip.rays`` is the model input - the clip is edge-padded (:func:`pad_clip`) and uploaded when asked for,
      the mirrored input is `mirror`'s or :func:`mirror_input`'s;
    * `encode` given: ``Clip.rays`` holds raw pixels - here, once, the shard's pixels and its :func:`clip_input_table` are
      uploaded, ONE :func:`shard_encode_hip` call on the current stream pads, encodes and - with `flip` - mirrors every clip and
      its status is read (a refused descriptor raises); a clip's inputs are its slices of the two buffers, lifted with
      ``n_windows=``.  `lifter`'s ``clip_batch_sizes`` size the slices.  Clips of fewer than `pool_below` frames (0: none) are
      encoded without padding: they are not lifted from slices but gathered from the buffer (:class:`_Pool`).
      `repair` (None: off - no code path, buffer or launch differs): ONE :func:`shard_repair_hip` call right behind the encode call,
      on its two buffers and its table (with `pool_below` the re-laid-out one), with ``max_gap=repair``; keypoints of confidence
      (``Clip.conf``; clips without one count as +inf) below `min_conf` are not observed; `repair_out` (a dict) receives "state",
      "stats" and "status"; a refused descriptor raises."""

    def __init__(self, mine: Sequence[Clip], rf: int, dev, causal: bool, encode: Optional[str], lifter, flip: bool = False,
                 kps_left: Sequence[int] = (), kps_right: Sequence[int] = (), mirror: Optional[Callable] = None, pool_below: int = 0,
                 repair: Optional[int] = None, min_conf: float = 0.0, repair_out: Optional[dict] = None):
        self.mine, self.dev, self.flip, self.encode = mine, dev, flip, encode
        self.lengths = [int(c.rays.shape[0]) for c in mine]
        self.pad, self.shift = (rf - 1) // 2, ((rf - 1) // 2 if causal else 0)
        self.mirror = mirror if mirror is not None else (lambda x: mirror_input(x, kps_left, kps_right))
        if encode is None:
            return
        sizes_of = lifter.clip_batch_sizes
        itable, self.first, out_rows, max_rows = clip_input_table(mine, rf, causal, lambda n: sum(sizes_of(n)) - n)
        if pool_below and any(n < pool_below for n in self.lengths):
            # a pooled clip (``pool_below=``) is gathered by r3d_clips_windows, whose clamp is the padding: pads 0 for it
            self.first, out_rows, max_rows = [], 0, 0
            for d in itable:
                if int(d["n_frames"]) < pool_below:
                    d["pad_front"] = d["pad_back"] = 0
                d["out_first"] = out_rows
                self.first.append(out_rows)
                rows = int(d["pad_front"]) + int(d["n_frames"]) + int(d["pad_back"])
                out_rows, max_rows = out_rows + rows, max(max_rows, rows)
        self.rows = [int(d["pad_front"]) + int(d["n_frames"]) + int(d["pad_back"]) for d in itable]
        px_all = torch.from_numpy(np.concatenate([np.ascontiguousarray(c.rays, dtype=np.float32) for c in mine], axis=0)).to(dev)
        perm = mirror_permutation(px_all.shape[1], kps_left, kps_right) if flip else None
        if repair is not None:
            from . import _capi
            for k, rows in enumerate(self.rows):
                if rows > _capi.REPAIR_MAX_ROWS:
                    raise ValueError("repair=: clip %d of this rank's shard (clip_id %s, %d frames) has %d padded rows; r3d_clips_repair takes "
                                     "at most %d" % (k, mine[k].clip_id, self.lengths[k], rows, _capi.REPAIR_MAX_ROWS))
        table_dev = _to_device_bytes(itable, dev)
        self.x_all, self.xm_all, status = shard_encode_hip(px_all, table_dev, len(mine), out_rows, max_rows, encode, perm)
        if repair is not None:
            conf_all = None
            if any(c.conf is not None for c in mine):
                J = px_all.shape[1]
                conf_all = torch.from_numpy(np.concatenate(
                    [np.ascontiguousarray(c.conf, dtype=np.float32).reshape(n, J) if c.conf is not None else np.full((n, J), np.inf, np.float32)
                     for c, n in zip(mine, self.lengths)], axis=0)).to(dev)
            rstate, rstats, rstatus = shard_repair_hip(self.x_all, table_dev, len(mine), out_rows, max_rows, int(repair), self.xm_all, perm,
                                                       conf_all, min_conf)
        _raise_if_refused(status, "r3d_clips_encode")
        if repair is not None:
            _raise_if_refused(rstatus, "r3d_clips_repair")
            if repair_out is not None:
                repair_out.update(state=rstate, stats=rstats, status=rstatus)

    def __call__(self, k: int):
        c = self.mine[k]
        if self.encode is None:
            x = torch.from_numpy(pad_clip(np.asarray(c.rays, dtype=np.float32), self.pad, self.shift)).to(self.dev)
            xm, kw = (self.mirror(x) if self.flip else None), {}
        else:
            rows = slice(self.first[k], self.first[k] + self.rows[k])
            x, xm, kw = self.x_all[rows], (self.xm_all[rows] if self.flip else None), {"n_windows": c.rays.shape[0]}
        return x, xm, torch.from_numpy(c.camera.param()).to(self.dev), kw


def _deal(lifter, count: int, lift: Callable[[int], object]) -> list:
    """``lift(k)`` for k in 0..count-1 - when `lifter` has lanes (``set_lanes``), each on the next lane's stream, and the ONE
    join of the pass after the last.  -> what the calls returned."""
    lanes = lifter is not None and getattr(lifter, "num_lanes", lambda: 0)() > 0
    out = []
    for k in range(count):
        if lanes:
            with lifter.lane():          # the clip's upload, its forwards and what follows them on the next lane's stream
                out.append(lift(k))
        else:
            out.append(lift(k))
    if lanes:
        lifter.join_lanes()
    return out


# ------------------------------------------------------------------------------------ a whole shard in one metrics call

def clip_table(clips: Sequence[Clip], root_relative: bool = False):
    """(table, first_frames, total_frames, max_frames) of `clips` laid out back to back in the given order: `table` a NumPy
    structured array of r3d_clip_desc rows (``_capi.clip_desc_dtype()``) - clip k's frames are rows [first_frames[k],
    first_frames[k] + N_k) of the shard's prediction / ground-truth buffers, its transform is :func:`clip_world_transform`'s -
    to be uploaded once per data set (``torch.from_numpy(table.view(np.uint8))``) and handed to :func:`shard_metrics_hip`."""
    return _desc_table([int(np.asarray(c.rays).shape[0]) for c in clips], [clip_world_transform(c, root_relative) for c in clips])


def shard_metrics_hip(pred_all: torch.Tensor, gt_all: torch.Tensor, table_dev: torch.Tensor, num_clips: int, total_frames: int,
                      max_frames: int, rows: torch.Tensor, detail_rows: Optional[torch.Tensor] = None,
                      frames: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE r3d_clips_metrics call on the current stream for every clip of a shard: `pred_all` / `gt_all` (total_frames, J, 3)
    (or (total_frames, 1, J, 3)) float32, `table_dev` the uploaded bytes of :func:`clip_table`, `rows` the (num_clips,
    PARTIAL_COLS) float64 matrix of :func:`partial_rows` whose columns 3..7 are written in place - with the bits
    :func:`clip_partials_hip` gives clip by clip; optional `detail_rows` (num_clips, DETAIL_COLS) and `frames` (total_frames, 5).
    No copy, no allocation (the scratch is a cached tensor per device), no synchronisation."""
    from . import _capi
    dev = pred_all.device
    _need(pred_all, "pred_all", torch.float32, dev, rows=total_frames, last=3)
    _need(gt_all, "gt_all", torch.float32, dev, rows=total_frames, last=3)
    J = pred_all.numel() // (3 * total_frames)
    if pred_all.numel() != gt_all.numel():
        raise ValueError("ground truth %s vs prediction %s" % (tuple(gt_all.shape), tuple(pred_all.shape)))
    _need_table(table_dev, num_clips, _capi.CLIP_DESC_BYTES, dev)
    _need(rows, "rows (the matrix of partial_rows)", torch.float64, dev, shape=(num_clips, PARTIAL_COLS))
    if detail_rows is not None:
        _need(detail_rows, "detail_rows", torch.float64, dev, shape=(num_clips, DETAIL_COLS))
    if frames is not None:
        _need(frames, "frames", torch.float64, dev, shape=(total_frames, 5))
    scratch = _shard_scratch(dev, _capi.clips_metrics_scratch_bytes(num_clips, max_frames, detail_rows is not None))
    with torch.cuda.device(dev):
        _capi.clips_metrics(pred_all.data_ptr(), gt_all.data_ptr(), total_frames, J, table_dev.data_ptr(), num_clips, max_frames,
                            rows.data_ptr() + 3 * 8, PARTIAL_COLS,
                            detail_rows.data_ptr() if detail_rows is not None else None, DETAIL_COLS,
                            frames.data_ptr() if frames is not None else None,
                            scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream)
    return rows


# ------------------------------------------------------------------------------------ a whole shard's inputs in one encode call

ENCODINGS = {"ray": 0, "intrinsic": 1, "screen": 2}     # R3D_ENCODE_*: what `encode=` / shard_encode_hip name


def mirror_permutation(num_joints: int, kps_left: Sequence[int], kps_right: Sequence[int]) -> List[int]:
    """`perm` with mirror_input(x)[:, j] == x[:, perm[j]] (component 0 negated): left and right keypoints trade places."""
    perm = list(range(num_joints))
    for a, b in zip(list(kps_left) + list(kps_right), list(kps_right) + list(kps_left)):
        perm[a] = b
    if sorted(perm) != list(range(num_joints)):
        raise ValueError("kps_left / kps_right do not make a permutation of the %d keypoints" % num_joints)
    return perm


def clip_input_table(clips: Sequence[Clip], rf: int, causal: bool = False, surplus: Optional[Callable[[int], int]] = None):
    """(table, out_first, out_rows, max_rows) for `clips` whose ``rays`` hold RAW PIXELS (N, J, 2), laid out back to back in the
    given order in one pixel buffer: `table` a NumPy structured array of r3d_clip_input_desc rows
    (``_capi.clip_input_desc_dtype()``) - clip k's frames are rows [first_frame, first_frame + N_k) of the pixel buffer, its
    padded, encoded input rows [out_first[k], out_first[k] + pad_front + N_k + pad_back) of the output buffer of `out_rows`
    rows, back to back as well.  pad_front = pad + shift and pad_back = pad - shift + surplus(N_k), with pad = (RF-1)//2 and
    shift = pad for `causal` models - :func:`pad_clip`'s padding - and `surplus(n)` the rows the rounded-up batch sizes of an
    n-window clip read past it (``sum(lifter.clip_batch_sizes(n)) - n``; None: 0), so that a clip's slice is what
    ``Ray3DLifter.forward_clip(..., n_windows=N_k)`` takes.  Camera rows: ``Camera.cam_row(distortion=True)``.  `max_rows` is
    the longest clip's output row count.  Uploaded once (``torch.from_numpy(table.view(np.uint8))``) and handed to
    :func:`shard_encode_hip`."""
    from . import _capi
    pad = (rf - 1) // 2
    shift = pad if causal else 0
    table = np.zeros(len(clips), dtype=_capi.clip_input_desc_dtype())
    out_first, src, at, longest = [], 0, 0, 0
    for k, c in enumerate(clips):
        n = int(np.asarray(c.rays).shape[0])
        extra = int(surplus(n)) if surplus is not None else 0
        if extra < 0:
            raise ValueError("surplus(%d) is negative" % n)
        table[k]["first_frame"], table[k]["n_frames"], table[k]["out_first"] = src, n, at
        table[k]["pad_front"], table[k]["pad_back"] = pad + shift, pad - shift + extra
        table[k]["cam"] = c.camera.cam_row(distortion=True)
        out_first.append(at)
        rows = 2 * pad + n + extra
        src += n
        at += rows
        longest = max(longest, rows)
    return table, out_first, at, longest


def shard_encode_hip(px_all: torch.Tensor, table_dev: torch.Tensor, num_clips: int, out_rows: int, max_rows: int,
                     encoding: str = "ray", mirror_perm: Optional[Sequence[int]] = None, x_all: Optional[torch.Tensor] = None,
                     x_mirror_all: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """ONE r3d_clips_encode call on the current stream for every clip of a shard: `px_all` (total_frames, J, 2) float32 raw
    pixels, `table_dev` the uploaded bytes of :func:`clip_input_table`, `encoding` "ray" | "intrinsic" | "screen"; with
    `mirror_perm` (:func:`mirror_permutation`) the same launch writes the flip pass's inputs as well.  Returns
    (x_all (out_rows, J, F) float32, x_mirror_all or None, status (num_clips,) int32: 0 = followed, 1 = invalid descriptor).
    `x_all` / `x_mirror_all` / `status`: tensors to write into (contiguous, of exactly these shapes) instead of new ones -
    needed under hipGraph capture; new buffers are NOT zeroed: rows no clip covers keep what they held.  No copy and no
    synchronisation: the caller reads `status` when it wants to."""
    from . import _capi
    dev = px_all.device
    enc = _encoding_id(encoding, "encoding")
    F = _capi.ENCODE_FLOATS[enc]
    if not px_all.is_cuda or px_all.dim() != 3 or px_all.shape[0] < 1:
        raise ValueError("px_all: a contiguous float32 (total_frames, J, 2) tensor on a GPU is needed")
    _need(px_all, "px_all", torch.float32, dev, last=2)
    total, J = int(px_all.shape[0]), int(px_all.shape[1])
    _need_table(table_dev, num_clips, _capi.CLIP_INPUT_DESC_BYTES, dev)
    if (x_mirror_all is not None) and mirror_perm is None:
        raise ValueError("x_mirror_all without mirror_perm")
    x_all = _out_buffer(x_all, "x_all", True, torch.float32, dev, (out_rows, J, F))
    x_mirror_all = _out_buffer(x_mirror_all, "x_mirror_all", mirror_perm is not None, torch.float32, dev, (out_rows, J, F))
    status = _status_buffer(status, num_clips, dev)
    with torch.cuda.device(dev):
        _capi.clips_encode(px_all.data_ptr(), total, J, enc, table_dev.data_ptr(), num_clips, max_rows, x_all.data_ptr(), out_rows,
                           x_mirror_all.data_ptr() if x_mirror_all is not None else None,
                           [int(v) for v in mirror_perm] if mirror_perm is not None else None,
                           status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return x_all, x_mirror_all, status


def shard_repair_hip(x_all: torch.Tensor, table_dev: torch.Tensor, num_clips: int, out_rows: int, max_rows: int, max_gap: int,
                     x_mirror_all: Optional[torch.Tensor] = None, mirror_perm: Optional[Sequence[int]] = None,
                     conf_all: Optional[torch.Tensor] = None, min_conf: float = 0.0, state: Optional[torch.Tensor] = None,
                     stats: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """ONE r3d_clips_repair call on the current stream, right behind the :func:`shard_encode_hip` call whose `x_all` (out_rows, J,
    F) / `x_mirror_all`, `table_dev`, `out_rows` and `max_rows` it is given: every keypoint that is not observed - a non-finite
    component, or with `conf_all` ((total_frames, J) float32 over the SOURCE frames) a confidence below `min_conf` - is repaired IN
    PLACE in both buffers: gaps of at most `max_gap` rows interpolated from both sides, longer ones held, a late first observation
    back-filled, a joint never observed the canonical NaN (include/ray3d_hip.h has the rule).  Returns (state (out_rows, J) uint8:
    0 observed, 1 interpolated, 2 held, 3 back-filled, 4 never observed; stats (num_clips, J, 4) int32: those four counts over each
    clip's own frames; status (num_clips,) int32: 0 = followed, 1 = invalid descriptor).  `state` / `stats` / `status`: tensors to
    write into (contiguous, of exactly these shapes) instead of new ones - needed under hipGraph capture; a new `state` is NOT
    zeroed: rows no clip covers keep what they held.  No copy and no synchronisation: the caller reads `status` when it wants to."""
    from . import _capi
    dev = x_all.device
    if not x_all.is_cuda or x_all.dim() != 3 or x_all.shape[-1] not in (2, 3):
        raise ValueError("x_all: a contiguous float32 (out_rows, J, 2 | 3) tensor on a GPU is needed")
    J, F = int(x_all.shape[1]), int(x_all.shape[2])
    _need(x_all, "x_all", torch.float32, dev, shape=(out_rows, J, F))
    _need_table(table_dev, num_clips, _capi.CLIP_INPUT_DESC_BYTES, dev)
    if (x_mirror_all is None) != (mirror_perm is None):
        raise ValueError("x_mirror_all and mirror_perm go together (both or neither)")
    if x_mirror_all is not None:
        _need(x_mirror_all, "x_mirror_all", torch.float32, dev, shape=(out_rows, J, F))
    if max_rows > _capi.REPAIR_MAX_ROWS:
        raise ValueError("max_rows is %d: r3d_clips_repair takes clips of at most %d rows" % (max_rows, _capi.REPAIR_MAX_ROWS))
    total = 0
    if conf_all is not None:
        if conf_all.dim() != 2 or conf_all.shape[0] < 1:
            raise ValueError("conf_all: a contiguous float32 (total_frames, J) tensor is needed")
        _need(conf_all, "conf_all", torch.float32, dev, last=J)
        total = int(conf_all.shape[0])
    state = _out_buffer(state, "state", True, torch.uint8, dev, (out_rows, J))
    stats = _out_buffer(stats, "stats", True, torch.int32, dev, (num_clips, J, 4))
    status = _status_buffer(status, num_clips, dev)
    with torch.cuda.device(dev):
        _capi.clips_repair(x_all.data_ptr(), out_rows, J, F, x_mirror_all.data_ptr() if x_mirror_all is not None else None,
                           [int(v) for v in mirror_perm] if mirror_perm is not None else None, table_dev.data_ptr(), num_clips, max_rows,
                           conf_all.data_ptr() if conf_all is not None else None, total, float(min_conf), int(max_gap),
                           state.data_ptr(), stats.data_ptr(), status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return state, stats, status


# ------------------------------------------------------------------------------------ a whole shard's finished poses in one call

def clip_raw_table(lengths: Sequence[int], sizes_of: Callable[[int], Sequence[int]]):
    """(raw_first, raw_rows) for clips of these frame counts whose forwards write into ONE raw buffer back to back: clip k owns rows
    [raw_first[k], raw_first[k] + sum(sizes_of(N_k))) - what ``Ray3DLifter.forward_clip(..., raw_out=)`` takes, `sizes_of` the
    lifter's ``clip_batch_sizes`` - of which the first N_k are its poses and the rest the surplus windows' that
    r3d_clips_poses never reads.  `raw_first` goes to the device as int64 (:func:`shard_poses_hip`)."""
    raw_first, at = [], 0
    for n in lengths:
        raw_first.append(at)
        at += int(sum(sizes_of(int(n))))
    return raw_first, at


def shard_poses_hip(raw_all: torch.Tensor, table_dev: torch.Tensor, raw_first_dev: torch.Tensor, num_clips: int, total_frames: int,
                    max_frames: int, raw_mirror_all: Optional[torch.Tensor] = None, mirror_perm: Optional[Sequence[int]] = None,
                    pred: bool = True, world: bool = False, pred_all: Optional[torch.Tensor] = None,
                    world_all: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """ONE r3d_clips_poses call on the current stream for every clip of a shard: `raw_all` (raw_rows, J, 3) (or (raw_rows, 1, J, 3))
    float32, what the forwards wrote (``forward_clip(raw_out=)``); `raw_mirror_all` the same from the pass over the mirrored
    input, with `mirror_perm` (:func:`mirror_permutation` of the OUTPUT joints); `table_dev` the uploaded bytes of
    :func:`clip_table` (the one :func:`shard_metrics_hip` reads), `raw_first_dev` (num_clips,) int64 (:func:`clip_raw_table`).
    Returns (pred_all (total_frames, J, 3) float32 or None, world_all (total_frames, J, 3) float64 or None, status (num_clips,)
    int32: 0 = followed, 1 = invalid descriptor) - `pred` / `world` say which outputs are wanted.  `pred_all` / `world_all` /
    `status`: tensors to write into (contiguous, total_frames rows of J * 3 elements; (num_clips,)) instead of new ones - needed
    under hipGraph capture; new buffers are NOT zeroed: rows no clip covers keep what they held.  No copy and no
    synchronisation: the caller reads `status` when it wants to."""
    from . import _capi
    dev = raw_all.device
    if not raw_all.is_cuda or raw_all.dim() not in (3, 4) or raw_all.shape[0] < 1 or (raw_all.dim() == 4 and raw_all.shape[1] != 1):
        raise ValueError("raw_all: a contiguous float32 (raw_rows, J, 3) tensor on a GPU is needed")
    _need(raw_all, "raw_all", torch.float32, dev, last=3)
    raw_rows, J = int(raw_all.shape[0]), int(raw_all.shape[-2])
    if (raw_mirror_all is None) != (mirror_perm is None):
        raise ValueError("raw_mirror_all and mirror_perm go together")
    if raw_mirror_all is not None:
        _need(raw_mirror_all, "raw_mirror_all", torch.float32, dev, rows=raw_rows, numel=raw_all.numel())
    _need_table(table_dev, num_clips, _capi.CLIP_DESC_BYTES, dev)
    _need(raw_first_dev, "raw_first_dev", torch.int64, dev, shape=(num_clips,))
    pred = pred or pred_all is not None
    world = world or world_all is not None
    if not pred and not world:
        raise ValueError("neither pred nor world is wanted: nothing to write")
    pred_all = _out_buffer(pred_all, "pred_all", pred, torch.float32, dev, (total_frames, J, 3), exact=False)
    world_all = _out_buffer(world_all, "world_all", world, torch.float64, dev, (total_frames, J, 3), exact=False)
    status = _status_buffer(status, num_clips, dev)
    with torch.cuda.device(dev):
        _capi.clips_poses(raw_all.data_ptr(), raw_mirror_all.data_ptr() if raw_mirror_all is not None else None, raw_rows, J,
                          [int(v) for v in mirror_perm] if mirror_perm is not None else None, table_dev.data_ptr(),
                          raw_first_dev.data_ptr(), num_clips, max_frames, pred_all.data_ptr() if pred_all is not None else None,
                          world_all.data_ptr() if world_all is not None else None, total_frames, status.data_ptr(),
                          torch.cuda.current_stream(dev).cuda_stream)
    return pred_all, world_all, status


# ------------------------------------------------------------------------------------ a shard of short clips lifted in full batches

def clip_window_table(clips: Sequence, rf: int, causal: bool = False, flip: bool = False, surplus: int = 0,
                      first_frames: Optional[Sequence[int]] = None):
    """(table, win_first, total_windows) for the POOLED windows of `clips` (:class:`Clip` objects, or plain frame counts): `table`
    a NumPy structured array of r3d_window_run_desc rows (``_capi.window_run_dtype()``), one run per clip in the given order -
    clip k's N_k windows are [win_first[k], win_first[k] + N_k) of the pooled list of `total_windows` = sum N_k windows, window i
    of it the frames [i - pad - shift, i - pad - shift + RF) of the clip clamped to the clip (``start = -(pad + shift)``,
    ``step = 1``): :func:`pad_clip` plus the sliding windows of eval_data_prepare, with pad = (RF-1)//2 and shift = pad for
    `causal` models.  The clips' frames are rows [first_frames[k], first_frames[k] + N_k) of the source buffer (None: back to
    back).  `flip`: every run carries ``flip = 1`` - the table of the flip pass, a second table over the same windows.
    `surplus` extra windows go to the LAST run (not counted in `total_windows`): they slide over the clamped last frame, as the
    surplus windows of ``forward_clip`` do, so that ``sum(lifter.clip_batch_sizes(total_windows)) - total_windows`` of them make
    every batch of ``Ray3DLifter.forward_windows`` full.  Uploaded once (``torch.from_numpy(table.view(np.uint8))``)."""
    from . import _capi
    pad = (rf - 1) // 2
    shift = pad if causal else 0
    if surplus < 0:
        raise ValueError("surplus is negative")
    table = np.zeros(len(clips), dtype=_capi.window_run_dtype())
    win_first, src, at = [], 0, 0
    for k, c in enumerate(clips):
        n = int(c) if isinstance(c, (int, np.integer)) else int(np.asarray(c.rays).shape[0])
        if n < 1:
            raise ValueError("clip %d has no frame" % k)
        table[k]["first_frame"] = src if first_frames is None else int(first_frames[k])
        table[k]["n_frames"], table[k]["win_first"], table[k]["n_windows"] = n, at, n
        table[k]["start"], table[k]["step"], table[k]["flip"] = -(pad + shift), 1, 1 if flip else 0
        win_first.append(at)
        src += n
        at += n
    if len(clips):
        table[-1]["n_windows"] += int(surplus)
    return table, win_first, at


def shard_windows_hip(src_all: torch.Tensor, table_dev: torch.Tensor, num_runs: int, run_param: Optional[torch.Tensor],
                      window0: int, batch: int, rf: int, x: Optional[torch.Tensor] = None, param: Optional[torch.Tensor] = None,
                      perm: Optional[Sequence[int]] = None, status: Optional[torch.Tensor] = None):
    """ONE r3d_clips_windows call on the current stream: the pooled windows [window0, window0 + batch) of the run table
    `table_dev` (the uploaded bytes of :func:`clip_window_table`, or any r3d_window_run_desc rows) gathered from `src_all`
    (total_frames, J, F) float32 model-input rows into `x` (batch, RF, J, F), with `run_param` (num_runs, E) float32 - or None -
    each window's parameter row into `param` (batch, E).  `perm` (:func:`mirror_permutation` of the input keypoints): needed when
    a run may flip.  Returns (x, param or None, status (num_runs,) int32: written for the runs with a window in the range, 0 =
    followed, 1 = invalid descriptor).  `x` / `param` / `status`: tensors to write into (contiguous, of exactly these shapes)
    instead of new ones - needed under hipGraph capture; new buffers are NOT zeroed, a new status is.  No copy and no
    synchronisation: the caller reads `status` when it wants to."""
    from . import _capi
    dev = src_all.device
    if not src_all.is_cuda or src_all.dim() != 3 or src_all.shape[0] < 1 or src_all.shape[2] not in (2, 3):
        raise ValueError("src_all: a contiguous float32 (total_frames, J, 2 | 3) tensor on a GPU is needed")
    _need(src_all, "src_all", torch.float32, dev)
    total, J, F = (int(v) for v in src_all.shape)
    _need_table(table_dev, num_runs, _capi.WINDOW_RUN_DESC_BYTES, dev)
    if (param is not None) and run_param is None:
        raise ValueError("param without run_param")
    E = 0
    if run_param is not None:
        if run_param.dim() != 2:
            raise ValueError("run_param: a (num_runs, E) tensor is needed")
        E = int(run_param.shape[1])
        _need(run_param, "run_param", torch.float32, dev, shape=(num_runs, E))
    x = _out_buffer(x, "x", True, torch.float32, dev, (batch, rf, J, F))
    param = _out_buffer(param, "param", run_param is not None, torch.float32, dev, (batch, E))
    if status is None:
        status = torch.zeros((num_runs,), dtype=torch.int32, device=dev)
    else:
        _need(status, "status", torch.int32, dev, shape=(num_runs,))
    with torch.cuda.device(dev):
        _capi.clips_windows(src_all.data_ptr(), total, J, F, rf, table_dev.data_ptr(), num_runs,
                            run_param.data_ptr() if run_param is not None else None, E, int(window0), int(batch), x.data_ptr(),
                            param.data_ptr() if param is not None else None, [int(v) for v in perm] if perm is not None else None,
                            status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return x, param, status


class _Pool:
    """The clips of a shard that are lifted as pooled windows (``pool_below=``): `index` their positions in the shard,
    `win_first` {position: first pooled window = the clip's compact row in the raw buffers}, the run tables of the straight and
    the flip pass on the device, the source buffer the runs name, the runs' parameter rows."""

    def __init__(self, mine: Sequence[Clip], inputs: "_ShardInputs", rf: int, causal: bool, flip: bool, lifter, below: int,
                 kps_left: Sequence[int], kps_right: Sequence[int]):
        dev = inputs.dev
        self.index = [k for k, n in enumerate(inputs.lengths) if n < below]
        sub = [mine[k] for k in self.index]
        self.windows = sum(inputs.lengths[k] for k in self.index)
        if not self.index:
            return
        surplus = sum(lifter.clip_batch_sizes(self.windows)) - self.windows
        if inputs.encode is not None:     # the encode call's output: the pooled clips lie in it without padding
            self.src, firsts = inputs.x_all, [inputs.first[k] for k in self.index]
        else:                             # the pooled clips' rays, uploaded once
            self.src, firsts = torch.from_numpy(np.concatenate([np.ascontiguousarray(c.rays, dtype=np.float32) for c in sub], axis=0)).to(dev), None
        table, win_first, _ = clip_window_table(sub, rf, causal, False, surplus, firsts)
        self.win_first = dict(zip(self.index, win_first))
        self.table_dev = _to_device_bytes(table, dev)
        self.table_m_dev = _to_device_bytes(clip_window_table(sub, rf, causal, True, surplus, firsts)[0], dev) if flip else None
        self.perm = mirror_permutation(int(self.src.shape[1]), kps_left, kps_right) if flip else None
        self.run_param = torch.from_numpy(np.stack([np.asarray(c.camera.param(), dtype=np.float32) for c in sub])).to(dev) \
            if lifter.pos.camera_embedding else None


def _lift_finished(lift_clip: Callable, lifter, inputs, mirror_joints: Optional[tuple], table_dev: torch.Tensor,
                   total: int, longest: int, pred_all: Optional[torch.Tensor], world: bool, raw_first_dev: Optional[torch.Tensor] = None,
                   pool: Optional[_Pool] = None):
    """The raw destination of the forwards - ``evaluate_clips_batched(finish=True)``, :func:`predict_clips_batched` and
    :func:`evaluate_camera_sweep`: every clip of `inputs` (:class:`_ShardInputs` / :class:`_SliceInputs`) lifted with ``raw_out=``
    into its rows of ONE raw buffer (with a flip pass - `mirror_joints` (left, right) of the OUTPUT, else None - the mirrored
    input into a second one), dealt to the lanes and joined once (:func:`_deal`), then ONE :func:`shard_poses_hip` call over
    `table_dev` (:func:`clip_table` of the shard) whose status is read: a refused descriptor raises.  `raw_first_dev`: the
    :func:`clip_raw_table` of ``inputs.lengths`` already on the device (a caller that uploads the tables of many passes at once).
    `pool` (``pool_below=``): its clips are not lifted one by one - the first ``sum(clip_batch_sizes(pool.windows))`` rows of the raw
    buffers are the pooled windows, written by ``lifter.forward_windows`` in full batches, and a pooled clip's raw_first is its
    compact position among them; the other clips follow behind, lifted as without a pool.
    -> (pred_all, world_all or None)."""
    lengths, dev, flip = inputs.lengths, inputs.dev, mirror_joints is not None
    J = lifter.pos.num_joints_in
    sizes_of = lifter.clip_batch_sizes
    if pool is not None and pool.index:
        if raw_first_dev is not None:
            raise ValueError("a pool lays the raw buffers out itself: raw_first_dev must be None")
        pool_rows = sum(sizes_of(pool.windows))
        raw_first, raw_rows = [], pool_rows
        for k, n in enumerate(lengths):
            raw_first.append(pool.win_first[k] if k in pool.win_first else raw_rows)
            raw_rows += 0 if k in pool.win_first else sum(sizes_of(n))
    else:
        pool = None
        raw_first, raw_rows = clip_raw_table(lengths, sizes_of)
    raw_all = torch.empty((raw_rows, 1, J, 3), dtype=torch.float32, device=dev)
    raw_m_all = torch.empty((raw_rows, 1, J, 3), dtype=torch.float32, device=dev) if flip else None
    if raw_first_dev is None:
        raw_first_dev = torch.tensor(raw_first, dtype=torch.int64).to(dev)

    def lift(k):
        rows = slice(raw_first[k], raw_first[k] + sum(sizes_of(lengths[k])))
        x, xm, prow, kw = inputs(k)
        lift_clip(x, prow, raw_out=raw_all[rows], **kw)
        if flip:
            lift_clip(xm, prow, raw_out=raw_m_all[rows], **kw)

    if pool is None:
        _deal(lifter, len(lengths), lift)
    else:
        lifter.forward_windows(pool.src, pool.table_dev, len(pool.index), pool.run_param, pool.windows, raw_all[:pool_rows])
        if flip:
            lifter.forward_windows(pool.src, pool.table_m_dev, len(pool.index), pool.run_param, pool.windows, raw_m_all[:pool_rows],
                                   perm=pool.perm)
        rest = [k for k in range(len(lengths)) if k not in pool.win_first]
        _deal(lifter, len(rest), lambda i: lift(rest[i]))
    perm = mirror_permutation(J, *mirror_joints) if flip else None
    pred_all, world_all, status = shard_poses_hip(raw_all, table_dev, raw_first_dev, len(lengths), total, longest, raw_m_all, perm,
                                                  pred=True, world=world, pred_all=pred_all)
    _raise_if_refused(status, "r3d_clips_poses")
    return pred_all, world_all


def predict_clips_batched(lift_clip: Callable, clips: Sequence[Clip], rf: int, device, flip: bool = False,
                          kps_left: Sequence[int] = (), kps_right: Sequence[int] = (),
                          joints_left: Optional[Sequence[int]] = None, joints_right: Optional[Sequence[int]] = None,
                          causal: bool = False, encode: Optional[str] = None, world: bool = True, root_relative: bool = False,
                          pool_below: Optional[int] = None, repair: Optional[int] = None, min_conf: float = 0.0,
                          repair_out: Optional[dict] = None):
    """:func:`predict_clip` for many clips, with the poses in world coordinates on top - the numerical core of the reference's
    Trainer.render (lib/train_val/trainer.py:505-526: cam.normalized2world / cam.camera2world on the flip-averaged poses) without
    its height rebase and its animation.  Every clip is lifted with ``raw_out=`` into one raw buffer and ONE r3d_clips_poses call
    finishes them all (the lifting code of ``evaluate_clips_batched(finish=True)``).  Returns, per clip in the given order,
    (poses (N, J, 3) float32 - the bits of :func:`predict_clip` - , world (N, J, 3) float64 or None without `world`): views of the
    two shard buffers.  The transform is :func:`clip_world_transform`'s: a ``frame="camera"`` clip goes through Rc2w / Tc2w,
    `root_relative` is the identity.  `lift_clip` must be the bound ``forward_clip`` of a lifter; `encode` as in
    :func:`evaluate_clips_batched`, and so are `pool_below` and `repair` / `min_conf` / `repair_out`.  Single rank, GPU only.  No ground truth is needed: ``Clip.gt_norm``
    may be an empty array."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("predict_clips_batched finishes the poses on the GPU (r3d_clips_poses); on CPU tensors use predict_clip")
    lifter = _lifter_of(lift_clip, need="predict_clips_batched", by_name=True)
    if encode is not None:
        _encoding_id(encode)
    _repair_needs_encode(repair, encode)
    if not clips:
        return []
    table, first, total, longest = clip_table(clips, root_relative)
    table_dev = _to_device_bytes(table, dev)
    below = int(pool_below or 0)
    inputs = _ShardInputs(clips, rf, dev, causal, encode, lifter, flip, kps_left, kps_right, pool_below=below, repair=repair,
                          min_conf=min_conf, repair_out=repair_out)
    jl = kps_left if joints_left is None else joints_left
    jr = kps_right if joints_right is None else joints_right
    pool = _Pool(clips, inputs, rf, causal, flip, lifter, below, kps_left, kps_right) if below else None
    pred_all, world_all = _lift_finished(lift_clip, lifter, inputs, (jl, jr) if flip else None, table_dev, total, longest, None, world,
                                         pool=pool)
    return [(pred_all[first[k]:first[k] + c.rays.shape[0]],
             world_all[first[k]:first[k] + c.rays.shape[0]] if world_all is not None else None) for k, c in enumerate(clips)]


def evaluate_clips_batched(lift_clip: Callable, clips: Sequence[Clip], rf: int, device, flip: bool = False,
                           kps_left: Sequence[int] = (), kps_right: Sequence[int] = (),
                           rank: int = 0, world_size: int = 1, group=None, causal: bool = False,
                           joints_left: Optional[Sequence[int]] = None, joints_right: Optional[Sequence[int]] = None,
                           root_relative: bool = False, mirror: Optional[Callable] = None, detail: bool = False,
                           include_root: bool = False, encode: Optional[str] = None, finish: bool = False,
                           pool_below: Optional[int] = None, repair: Optional[int] = None, min_conf: float = 0.0,
                           repair_out: Optional[dict] = None):
    """:func:`evaluate_clips` (with `detail`: :func:`evaluate_clips_detail`, `include_root` as there) with the measuring side in
    ONE call per shard: the rank's clip table and ground truth are uploaded once, every clip is lifted into its slice of one
    prediction buffer (``lift_clip(padded, param_row, out=slice)``: ``Ray3DLifter.forward_clip``; the flip average is written
    into the slice), and one :func:`shard_metrics_hip` call fills the error columns of all rows - then the same gather and
    reduction.  Same arguments, same return values, the same bits in every row.  GPU only.  When `lift_clip` is the bound
    ``forward_clip`` of a lifter with lanes (``set_lanes``), the clips are dealt to the lanes and joined once, before the
    metrics call.

    `encode` ("ray" | "intrinsic" | "screen"): ``Clip.rays`` holds RAW PIXELS (N, J, 2) and the input side is one call per
    shard as well - the rank's pixels are uploaded once as one buffer and ONE r3d_clips_encode call (:func:`shard_encode_hip`,
    on the caller's stream, before the first forward) pads, encodes and - with `flip` - mirrors every clip; each clip is
    then lifted from its slice, ``lift_clip(x_all[slice], param_row, out=dst, n_windows=N)``: no per-clip upload, pad or
    concatenation.  `lift_clip` must be the bound ``forward_clip`` of a lifter (its ``clip_batch_sizes`` size the slices).
    The flip pass mirrors the ENCODED input, as the reference does - also right for undistort=True cameras, which
    :func:`mirror_pixels` refuses; `kps_left` / `kps_right` give the permutation and `mirror` must be None.

    `finish`: the step between the forwards and the measurement is one call per shard as well - every clip is lifted with
    ``raw_out=`` into one raw buffer (with `flip` the mirrored pass into a second one; with lanes ONE join in all, also for clips
    with tails), ONE r3d_clips_poses call (:func:`shard_poses_hip`) writes the prediction buffer - flip average included - and the
    one metrics call runs as before.  `lift_clip` must be the bound ``forward_clip`` of a lifter.  Same return values, the same
    bits in every row.

    `pool_below` (None or 0: off, exactly the path and the bits above): the clips of a shard with FEWER than this many frames are
    not lifted clip by clip.  Their windows form one pool that ``Ray3DLifter.forward_windows`` lifts in full batches of the plain
    (B, RF, J, F) forward - per batch one r3d_clips_windows gather (:func:`shard_windows_hip`; the clamp of its index is the edge
    padding, a flip run mirrors on the way) and one forward written straight into the raw buffers, where a pooled clip's rows are
    its compact position in the pool; the longer clips go through ``forward_clip(raw_out=)`` as before, and the same single
    r3d_clips_poses and r3d_clips_metrics calls finish and measure all of them.  Implies `finish`.  With `encode` the pooled
    clips are encoded without padding and gathered from the encode call's output; without it their rays are uploaded once.  Not
    with lanes (the pooled batches fill the chip by themselves) and not with a `mirror` callable.  A pooled clip's poses come
    from the materialised-window kernels instead of the clip kernels: they agree with the per-clip path within the bound the
    clip forwards are held to against materialised windows, not bit for bit; the rows of the other clips keep their bits.
    Recommended: ``pool_below=1024``.  Measured at RF 243, flip on (profiles/clips_windows_ab.json): pooling 2 000
    clips of 40 - 400 frames takes 0.62 of the per-clip path's time (run-to-run spread 3.6 % / 0.3 %); thresholds of 512, 1 024
    and 2 048 on a mixed shard cannot be told apart; pooling clips of 1 000 - 6 000 frames is 5 % SLOWER than lifting them per
    clip (the clip kernels' per-frame first level), so the crossover lies between 400 and about 2 000 frames.

    `repair` (None: off - no code path, buffer or launch differs; needs `encode`): pixel archives with dropped keypoints.  A NaN
    keypoint makes the encode call write a non-finite input row, and every window that reads it comes out NaN.  With ``repair=K``
    ONE r3d_clips_repair call (:func:`shard_repair_hip`) runs right behind the shard's encode call, on its buffers and its table
    (with `pool_below` the re-laid-out one): per clip and joint, gaps of at most K frames are interpolated from both sides, longer
    ones held, a late first observation back-filled over the clip's start; a joint never observed stays NaN.  With ``Clip.conf``
    ((N, J) confidences; a clip without one counts as +inf) a keypoint below `min_conf` is not observed either.  `repair_out` (a
    dict) receives this rank's "state" (out_rows, J) uint8, "stats" (clips, J, 4) int32 and "status"; a refused descriptor raises,
    and so does a clip of more than ``_capi.REPAIR_MAX_ROWS`` padded rows.  A clip without a missing keypoint keeps its bits."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("evaluate_clips_batched measures on the GPU (r3d_clips_metrics); on CPU tensors use evaluate_clips")
    lifter = _lifter_of(lift_clip)
    if encode is not None:        # (decided before the shards are cut: every rank raises alike, also one with an empty shard)
        _encoding_id(encode)
        if mirror is not None:
            raise ValueError("encode=: the flip pass mirrors the encoded input on the device; `mirror` must be None")
        _lifter_of(lift_clip, need="encode=")
    _repair_needs_encode(repair, encode)
    below = int(pool_below or 0)
    if below:
        if mirror is not None:
            raise ValueError("pool_below=: the flip pass is mirrored by the gather on the device; `mirror` must be None")
        finish = True
    if finish:
        _lifter_of(lift_clip, need="pool_below=" if below else "finish=True", by_name=True)
    actions, aid, shards, mine = _shard_plan(clips, rank, world_size)
    local = _shard_rows(clips, aid, shards[rank], PARTIAL_COLS, dev)
    dlocal = torch.zeros((len(mine), DETAIL_COLS), dtype=torch.float64, device=dev) if detail else None
    if mine:
        table, first, total, longest = clip_table(mine, root_relative)
        table_dev = _to_device_bytes(table, dev)
        gt_all = _ground_truth(mine, dev, root_relative)
        pred_all = torch.empty((total, 1, gt_all.shape[1], 3), dtype=torch.float32, device=dev)
        inputs = _ShardInputs(mine, rf, dev, causal, encode, lifter, flip, kps_left, kps_right, mirror, pool_below=below, repair=repair,
                              min_conf=min_conf, repair_out=repair_out)
        jl = kps_left if joints_left is None else joints_left
        jr = kps_right if joints_right is None else joints_right
        if finish:
            pool = _Pool(mine, inputs, rf, causal, flip, lifter, below, kps_left, kps_right) if below else None
            _lift_finished(lift_clip, lifter, inputs, (jl, jr) if flip else None, table_dev, total, longest, pred_all, False, pool=pool)
        else:
            def lift(k):
                dst = pred_all[first[k]:first[k] + mine[k].rays.shape[0]]
                x, xm, prow, kw = inputs(k)
                lift_clip(x, prow, out=dst, **kw)
                if flip:
                    pred_m = lift_clip(xm, prow, **kw)
                    torch.add(dst, mirror_output(pred_m, jl, jr), out=dst)     # 0.5 * (pred + mirrored), as predict_clip rounds it
                    dst.mul_(0.5)

            _deal(lifter, len(mine), lift)
        shard_metrics_hip(pred_all, gt_all, table_dev, len(mine), total, longest, local, dlocal)
    return _report(_gather(local, shards, group, PARTIAL_COLS), _gather(dlocal, shards, group, DETAIL_COLS) if detail else None,
                   actions, clips, include_root)


# ------------------------------------------------------------------------------------ a virtual-camera sweep from world poses

SWEEP_COLS = PARTIAL_COLS + 2   # a partial row, then the camera's index in the sweep and the clip's keypoints outside its frame


@dataclass
class WorldClip:
    world: np.ndarray         # (N, J, 3) float32 poses in WORLD coordinates, metres (the 3D archive's)
    action: str = ""
    clip_id: int = 0


def _ground_truth_transform(camera: Camera, frame: str):
    """((R, T) world -> the frame of the ground truth, (R, T) back to the world) of `camera`: the normalised frame, or the
    camera frame of the 2-feature baselines (trainer.py:361-362)."""
    if frame == "normalized":
        return (camera.Rw2n, camera.Tw2n), (camera.Rn2w, camera.Tn2w)
    if frame == "camera":
        return (camera.Rw2c, camera.Tw2c), (camera.Rc2w, camera.Tc2w)
    raise ValueError("frame must be 'normalized' or 'camera' (got %r)" % (frame,))


def clip_project_table(world_clips: Sequence[WorldClip], pairs: Sequence[tuple], cameras: Sequence[Camera], rf: int,
                       causal: bool = False, surplus: Optional[Callable[[int], int]] = None, frame: str = "normalized"):
    """(table, out_first, out_rows, max_rows, gt_first, gt_rows) for the (clip index, camera index) `pairs` of a camera sweep:
    `table` a NumPy structured array of r3d_clip_project_desc rows (``_capi.clip_project_desc_dtype()``), one per pair.  The
    SOURCE buffer holds `world_clips` back to back in the given order, each once: every camera's descriptors name the same
    frames.  Pair k's padded, encoded input is rows [out_first[k], out_first[k] + pad_front + N + pad_back) of an output buffer
    of `out_rows` rows and its ground truth rows [gt_first[k], gt_first[k] + N) of a buffer of `gt_rows` rows, both back to back
    in the order of `pairs`; padding and `surplus` as in :func:`clip_input_table`.  Per pair the camera's ``proj_row()``,
    ``cam_row(distortion=True)`` (the frame size in slots 6 / 7: the cameras need res_w / res_h) and the world -> `frame`
    transform ("normalized": Rw2n / Tw2n, "camera": Rw2c / Tw2c).  Uploaded once and handed to :func:`shard_project_hip`."""
    from . import _capi
    pad = (rf - 1) // 2
    shift = pad if causal else 0
    src_first = np.concatenate([[0], np.cumsum([int(np.asarray(c.world).shape[0]) for c in world_clips])]).astype(np.int64)
    table = np.zeros(len(pairs), dtype=_capi.clip_project_desc_dtype())
    out_first, gt_first, at, gat, longest = [], [], 0, 0, 0
    for k, (ci, cam_i) in enumerate(pairs):
        cam = cameras[cam_i]
        if cam.res_w is None or cam.res_h is None:
            raise ValueError("camera %r has no res_w / res_h: the in-frame count and the screen encoding need the frame size" % (cam.name,))
        n = int(np.asarray(world_clips[ci].world).shape[0])
        extra = int(surplus(n)) if surplus is not None else 0
        if extra < 0:
            raise ValueError("surplus(%d) is negative" % n)
        (R, T), _ = _ground_truth_transform(cam, frame)
        d = table[k]
        d["first_frame"], d["n_frames"], d["out_first"], d["gt_first"] = src_first[ci], n, at, gat
        d["pad_front"], d["pad_back"] = pad + shift, pad - shift + extra
        d["proj"], d["cam"] = cam.proj_row(), cam.cam_row(distortion=True)
        d["rw2g"], d["tw2g"] = np.asarray(R, dtype=np.float64).reshape(9), np.asarray(T, dtype=np.float64).reshape(3)
        out_first.append(at)
        gt_first.append(gat)
        rows = 2 * pad + n + extra
        at += rows
        gat += n
        longest = max(longest, rows)
    return table, out_first, at, longest, gt_first, gat


def shard_project_hip(world_all: torch.Tensor, table_dev: torch.Tensor, num_clips: int, out_rows: int, max_rows: int, gt_rows: int,
                      encoding: str = "ray", mirror_perm: Optional[Sequence[int]] = None, x_all: Optional[torch.Tensor] = None,
                      x_mirror_all: Optional[torch.Tensor] = None, gt_all: Optional[torch.Tensor] = None,
                      px_all: Optional[torch.Tensor] = None, outside: Optional[torch.Tensor] = None,
                      status: Optional[torch.Tensor] = None, gt: bool = True, px: bool = False, count: bool = True):
    """ONE r3d_clips_project call on the current stream for every (clip, camera) pair of a pass: `world_all` (total_frames, J, 3)
    float32 world poses, `table_dev` the uploaded bytes of :func:`clip_project_table` (or a slice of them: a pass's descriptors),
    `encoding` "ray" | "intrinsic" | "screen"; with `mirror_perm` (:func:`mirror_permutation`) the same launch writes the flip
    pass's inputs as well.  Returns (x_all (out_rows, J, F) float32, x_mirror_all or None, gt_all (gt_rows, J, 3) float32 or None,
    px_all (gt_rows, J, 2) float64 or None, outside (num_clips,) int32 or None: the pair's keypoints outside its camera's frame,
    status (num_clips,) int32: 0 = followed, 1 = invalid descriptor) - `gt` / `px` / `count` say which optional outputs are wanted.
    `x_all` / ... / `status`: tensors to write into (contiguous, of exactly these shapes) instead of new ones - needed under
    hipGraph capture; new buffers are NOT zeroed: rows no pair covers keep what they held.  `outside` IS zeroed here, on the
    current stream (the call adds to it).  No copy and no synchronisation: the caller reads `status` when it wants to."""
    from . import _capi
    dev = world_all.device
    enc = _encoding_id(encoding, "encoding")
    F = _capi.ENCODE_FLOATS[enc]
    if not world_all.is_cuda or world_all.dim() != 3 or world_all.shape[0] < 1:
        raise ValueError("world_all: a contiguous float32 (total_frames, J, 3) tensor on a GPU is needed")
    _need(world_all, "world_all", torch.float32, dev, last=3)
    total, J = int(world_all.shape[0]), int(world_all.shape[1])
    _need_table(table_dev, num_clips, _capi.CLIP_PROJECT_DESC_BYTES, dev)
    if (x_mirror_all is not None) and mirror_perm is None:
        raise ValueError("x_mirror_all without mirror_perm")
    x_all = _out_buffer(x_all, "x_all", True, torch.float32, dev, (out_rows, J, F))
    x_mirror_all = _out_buffer(x_mirror_all, "x_mirror_all", mirror_perm is not None, torch.float32, dev, (out_rows, J, F))
    gt_all = _out_buffer(gt_all, "gt_all", gt, torch.float32, dev, (gt_rows, J, 3))
    px_all = _out_buffer(px_all, "px_all", px, torch.float64, dev, (gt_rows, J, 2))
    outside = _out_buffer(outside, "outside", count, torch.int32, dev, (num_clips,))
    status = _status_buffer(status, num_clips, dev)
    with torch.cuda.device(dev):
        if outside is not None:
            outside.zero_()
        _capi.clips_project(world_all.data_ptr(), total, J, enc, table_dev.data_ptr(), num_clips, max_rows, x_all.data_ptr(), out_rows,
                            x_mirror_all.data_ptr() if x_mirror_all is not None else None,
                            [int(v) for v in mirror_perm] if mirror_perm is not None else None,
                            gt_all.data_ptr() if gt_all is not None else None, px_all.data_ptr() if px_all is not None else None,
                            gt_rows, outside.data_ptr() if outside is not None else None, status.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream)
    return x_all, x_mirror_all, gt_all, px_all, outside, status


class _SliceInputs:
    """``inputs(k)`` (as :class:`_ShardInputs`) of clips whose padded inputs already lie in buffers on the device: clip k is rows
    [first[k], first[k] + rows[k]) of `x_all` (and of `xm_all`, the mirrored inputs, or None), lifted with ``n_windows=lengths[k]``
    and the parameter row ``params[k]`` (a device tensor)."""

    def __init__(self, dev, lengths: Sequence[int], first: Sequence[int], rows: Sequence[int], x_all: torch.Tensor,
                 xm_all: Optional[torch.Tensor], params: Sequence[torch.Tensor]):
        self.dev, self.lengths, self.first, self.rows, self.x_all, self.xm_all, self.params = dev, lengths, first, rows, x_all, xm_all, params

    def __call__(self, k: int):
        rows = slice(self.first[k], self.first[k] + self.rows[k])
        return self.x_all[rows], (self.xm_all[rows] if self.xm_all is not None else None), self.params[k], {"n_windows": self.lengths[k]}


def reduce_camera_sweep(rows: torch.Tensor, actions: Sequence[str], camera_names: Sequence[str]) -> List[tuple]:
    """[(camera name, per_action {name: (e1, e2, e3, ev, er) mm}, action-wise average, keypoints outside the frame)] in the order
    of `camera_names` from the gathered SWEEP_COLS-wide rows of :func:`evaluate_camera_sweep` - per camera what one
    ``main.py --evaluate`` run of scripts/synthetic/test_aug.py logs; a camera without rows (an empty sweep) is left out."""
    rows = rows.detach().to("cpu", torch.float64)
    out = []
    for ci, name in enumerate(camera_names):
        sel = rows[rows[:, PARTIAL_COLS] == ci]
        if sel.shape[0] == 0:
            continue
        sel = sel[torch.argsort(sel[:, 0], stable=True)]            # clip-id order: the sums do not depend on the sharding
        per = reduce_partials(sel[:, :PARTIAL_COLS])
        out.append((str(name), {actions[a]: v for a, v in per.items()}, action_average(per), int(sel[:, PARTIAL_COLS + 1].sum().item())))
    return out


def evaluate_camera_sweep(lift_clip: Callable, world_clips: Sequence[WorldClip], cameras: Sequence[Camera], rf: int, device,
                          flip: bool = False, kps_left: Sequence[int] = (), kps_right: Sequence[int] = (),
                          joints_left: Optional[Sequence[int]] = None, joints_right: Optional[Sequence[int]] = None,
                          causal: bool = False, encode: str = "ray", frame: str = "normalized", finish: bool = True,
                          cameras_per_pass: Optional[int] = None, rank: int = 0, world_size: int = 1, group=None):
    """The reference's synthetic camera sweep (data/camera_augmentation.py:626-846 + scripts/synthetic/test_aug.py: the world-frame
    ground truth projected through every virtual camera, one whole evaluation per camera) from WORLD poses, on the device: every
    clip of `world_clips` is seen through every camera of `cameras` (:func:`ray3d_amd.camera.camera_grid`; each needs res_w /
    res_h) and evaluated as :func:`evaluate_clips_batched` evaluates a clip of that camera.  The world poses, the descriptor
    tables of ALL (clip, camera) pairs and the cameras' parameter rows are uploaded ONCE; then, per pass of `cameras_per_pass`
    cameras (None: all in one pass; the buffers of a pass are reused by the next), ONE :func:`shard_project_hip` call makes the
    padded, encoded - with `flip` also the mirrored - inputs, the ground truth in `frame` and the in-frame counts, the clips are
    lifted from their slices with ``raw_out=`` (dealt to the lanes, one join), ONE :func:`shard_poses_hip` call finishes the
    poses and ONE :func:`shard_metrics_hip` call measures them through the camera's Rn2w / Tn2w (`frame` "camera": Rc2w / Tc2w).
    No per-camera upload, no per-clip host arithmetic.  `lift_clip` must be the bound ``forward_clip`` of a lifter; `finish`
    must be True (the poses are finished on the device); `encode` "ray" | "intrinsic" | "screen".  `rank` / `world_size`: the
    (clip, camera) pairs are dealt to the ranks as :func:`evaluate_clips` deals clips, the rows travel in ONE all_gather.
    Every rank returns (:func:`reduce_camera_sweep` of all rows - per camera, in order, (camera name, per_action, action-wise
    average, keypoints outside the frame) -, the gathered (pairs, SWEEP_COLS) float64 rows: a partial row with the clip's index
    in column 0, then the camera's index and the pair's outside count).  A camera that loses keypoints is still evaluated: the
    reference drops it when it builds its sets (check_in_frame), here the count says so and the caller decides."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("evaluate_camera_sweep runs on the GPU (r3d_clips_project)")
    if not finish:
        raise ValueError("evaluate_camera_sweep finishes the poses on the device: finish must be True")
    lifter = _lifter_of(lift_clip, need="evaluate_camera_sweep", by_name=True)
    enc_name = encode
    _encoding_id(encode)
    if frame not in ("normalized", "camera"):
        raise ValueError("frame must be 'normalized' or 'camera' (got %r)" % (frame,))
    if cameras_per_pass is not None and cameras_per_pass < 1:
        raise ValueError("cameras_per_pass must be >= 1 (got %r)" % (cameras_per_pass,))
    actions = sorted(set(c.action for c in world_clips))
    aid = {a: i for i, a in enumerate(actions)}
    lengths = [int(np.asarray(c.world).shape[0]) for c in world_clips]
    pairs = [(k, ci) for ci in range(len(cameras)) for k in range(len(world_clips))]
    shards = shard_clips([lengths[k] for k, _ in pairs], world_size)
    per_pass = len(cameras) if cameras_per_pass is None else int(cameras_per_pass)
    mine = sorted(shards[rank], key=lambda i: pairs[i][1] // per_pass)     # stable: pass by pass, the shard's order within
    local = _header_rows([(pairs[i][0], aid[world_clips[pairs[i][0]].action], lengths[pairs[i][0]]) for i in mine], PARTIAL_COLS, dev)
    extra = torch.zeros((len(mine), 2), dtype=torch.float64)
    if mine:
        extra[:, 0] = torch.tensor([float(pairs[i][1]) for i in mine], dtype=torch.float64)
    extra = extra.to(dev)
    if mine:
        sizes_of = lifter.clip_batch_sizes
        J = int(np.asarray(world_clips[0].world).shape[1])
        jl = kps_left if joints_left is None else joints_left
        jr = kps_right if joints_right is None else joints_right
        in_perm = mirror_permutation(J, kps_left, kps_right) if flip else None
        # the passes' tables, host side: descriptors, metric descriptors and raw rows, each pass laid out from row 0 of its buffers
        passes, at = [], 0
        while at < len(mine):
            end = at
            while end < len(mine) and pairs[mine[end]][1] // per_pass == pairs[mine[at]][1] // per_pass:
                end += 1
            pp = [pairs[i] for i in mine[at:end]]
            ptable, out_first, out_rows, max_rows, gt_first, gt_rows = clip_project_table(
                world_clips, pp, cameras, rf, causal, lambda n: sum(sizes_of(n)) - n, frame)
            ns = [lengths[k] for k, _ in pp]
            mtable, _, total, longest = _desc_table(ns, [_ground_truth_transform(cameras[ci], frame)[1] for _, ci in pp])
            assert total == gt_rows and list(mtable["first_frame"]) == gt_first
            raw_first, _ = clip_raw_table(ns, sizes_of)
            rows_of = [int(d["pad_front"]) + int(d["n_frames"]) + int(d["pad_back"]) for d in ptable]
            passes.append(dict(at=at, end=end, pairs=pp, ptable=ptable, mtable=mtable, raw_first=raw_first, out_first=out_first,
                               rows=rows_of, out_rows=out_rows, max_rows=max_rows, gt_rows=gt_rows, longest=longest, lengths=ns))
            at = end
        # the uploads of the whole sweep: the world poses, the three tables of every pass, the cameras' parameter rows
        world_all = torch.from_numpy(np.concatenate([np.ascontiguousarray(c.world, dtype=np.float32) for c in world_clips], axis=0)).to(dev)
        ptable_dev = _to_device_bytes(np.concatenate([p["ptable"] for p in passes]), dev)
        mtable_dev = _to_device_bytes(np.concatenate([p["mtable"] for p in passes]), dev)
        raw_first_dev = torch.tensor([v for p in passes for v in p["raw_first"]], dtype=torch.int64).to(dev)
        params_dev = torch.from_numpy(np.stack([c.param() for c in cameras])).to(dev)
        from . import _capi
        F = _capi.ENCODE_FLOATS[ENCODINGS[enc_name]]
        most_out, most_gt = max(p["out_rows"] for p in passes), max(p["gt_rows"] for p in passes)
        x_buf = torch.empty((most_out, J, F), dtype=torch.float32, device=dev)
        xm_buf = torch.empty((most_out, J, F), dtype=torch.float32, device=dev) if flip else None
        gt_buf = torch.empty((most_gt, J, 3), dtype=torch.float32, device=dev)
        pred_buf = torch.empty((most_gt, 1, J, 3), dtype=torch.float32, device=dev)
        outside = torch.empty(len(mine), dtype=torch.int32, device=dev)
        status = torch.empty(len(mine), dtype=torch.int32, device=dev)
        for p in passes:
            a, b, k = p["at"], p["end"], p["end"] - p["at"]
            x_all, xm_all, gt_all, _, _, _ = shard_project_hip(
                world_all, ptable_dev[a * _capi.CLIP_PROJECT_DESC_BYTES:b * _capi.CLIP_PROJECT_DESC_BYTES], k, p["out_rows"],
                p["max_rows"], p["gt_rows"], enc_name, in_perm, x_all=x_buf[:p["out_rows"]],
                x_mirror_all=xm_buf[:p["out_rows"]] if flip else None, gt_all=gt_buf[:p["gt_rows"]], outside=outside[a:b],
                status=status[a:b])
            _raise_if_refused(status[a:b], "r3d_clips_project")
            inputs = _SliceInputs(dev, p["lengths"], p["out_first"], p["rows"], x_all, xm_all, [params_dev[ci] for _, ci in p["pairs"]])
            mtab = mtable_dev[a * _capi.CLIP_DESC_BYTES:b * _capi.CLIP_DESC_BYTES]
            pred_all = pred_buf[:p["gt_rows"]]
            _lift_finished(lift_clip, lifter, inputs, (jl, jr) if flip else None, mtab, p["gt_rows"], p["longest"], pred_all, False,
                           raw_first_dev=raw_first_dev[a:b])
            shard_metrics_hip(pred_all, gt_all, mtab, k, p["gt_rows"], p["longest"], local[a:b])
        extra[:, 1] = outside.to(torch.float64)
    allrows = _gather(torch.cat([local, extra], dim=1), shards, group, SWEEP_COLS)
    return reduce_camera_sweep(allrows, actions, [c.name for c in cameras]), allrows


def format_detail_report(table: Dict, joint_names: Optional[Sequence[str]] = None) -> List[str]:
    """Plain text for one table of :func:`reduce_detail`: one line per joint, then the PCK / AUC line."""
    nj = len(table["mpjpe"])
    names = list(joint_names) if joint_names is not None else ["joint %2d" % j for j in range(nj)]
    assert len(names) == nj
    lines = ["%s: MPJPE %.1f mm, P-MPJPE %.1f mm, root-relative %.1f mm"
             % (names[j], table["mpjpe"][j], table["p_mpjpe"][j], table["root_rel"][j]) for j in range(nj)]
    lines.append("PCK@150mm: %.1f %%, AUC: %.1f %%" % (table["pck150"], table["auc"]))
    return lines


# ------------------------------------------------------------------------------------ validation losses (Trainer.test)

VALID_COLS = 3 + M.VALID_DOUBLES   # clip_id, action_id, n_frames, then the R3D_VALID_DOUBLES sums of r3d_clip_valid_losses


def clip_valid(pos_or_sum: torch.Tensor, trj: Optional[torch.Tensor], clip: Clip, parents=H36M_17_PARENTS,
               pos_is_sum: bool = False, gt_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               gt_root_relative: bool = False, action_id: int = 0) -> torch.Tensor:
    """One VALID_COLS row (float64, on the predictions' device) of the clip's validation-loss sums - what one batch adds to
    the accumulators of Trainer.test (lib/train_val/trainer.py:187-223), in the normalised frame, metres; layout and rounding
    contract: r3d_clip_valid_losses in include/ray3d_hip.h.
    `pos_or_sum` (N,1,J,3) or (N,J,3): the pos network's output - or, with `pos_is_sum`, pos + trj as Ray3DLifter writes it;
    `trj` (N,1,1,3) or (N,3), None for configurations without a trajectory model (then `gt_root_relative` makes the ground
    truth root-relative first: the models that are not fed rays, :195-197).  `clip.gt_norm` (or `gt_dev`, already on the
    device) is the ABSOLUTE ground truth.  `parents`: the joint tree of the bone terms (:mod:`ray3d_amd.skeleton`), None for
    none.  `out`: a row of ``partial_rows(..., cols=VALID_COLS)`` whose header is already in place - only the sums are written.
    GPU tensors go through the HIP kernel on the current stream (no copy to the host, no synchronisation); CPU tensors
    (host-logic tests, a stand-in lifter) through the torch restatement in :mod:`ray3d_amd.metrics`.  Nothing is modified."""
    dev = pos_or_sum.device
    n = pos_or_sum.shape[0]
    pos = pos_or_sum.detach().reshape(n, -1, 3).contiguous().float()
    J = pos.shape[1]
    t = trj.detach().to(dev).reshape(n, 3).contiguous().float() if trj is not None else None
    tree = validate_parents(parents, J) if parents is not None else None
    if pos_is_sum and t is None:
        raise ValueError("pos_is_sum needs the trajectory")
    if gt_root_relative and t is not None:
        raise ValueError("gt_root_relative is for models without a trajectory: with one the ground truth must be absolute")
    if gt_dev is not None:
        gt = gt_dev.to(dev, torch.float32).reshape(n, -1, 3).contiguous()
    else:
        gt = torch.from_numpy(np.ascontiguousarray(clip.gt_norm, dtype=np.float32)).to(dev, non_blocking=True).reshape(n, -1, 3)
    assert gt.shape == pos.shape, "ground truth %s vs prediction %s" % (tuple(gt.shape), tuple(pos.shape))
    if pos.is_cuda:
        from . import _capi
        sums = torch.empty(_capi.VALID_OUT_DOUBLES, dtype=torch.float64, device=dev)
        flags = (_capi.R3D_VALID_POS_IS_SUM if pos_is_sum else 0) | (_capi.R3D_VALID_GT_ROOT_RELATIVE if gt_root_relative else 0)
        with torch.cuda.device(dev):
            _capi.clip_valid_losses(pos.data_ptr(), t.data_ptr() if t is not None else None, gt.data_ptr(), n, J, tree, flags,
                                    sums.data_ptr(), None, torch.cuda.current_stream(dev).cuda_stream)
        sums = sums[:M.VALID_DOUBLES]
    else:
        sums, _ = M.clip_valid(pos, t, gt, tree, pos_is_sum, gt_root_relative)
    if out is not None:
        assert out.shape == (VALID_COLS,) and out.dtype == torch.float64 and out.device == dev
        out[3:] = sums
        return out
    row = torch.empty(VALID_COLS, dtype=torch.float64, device=dev)
    for c, v in enumerate((clip.clip_id, action_id, n)):
        row[c].fill_(float(v))
    row[3:] = sums
    return row


def _valid_plan(clips: Sequence[Clip], group, device):
    """(shards, this rank's clips, its VALID_COLS rows with the headers in place): whole clips sharded over the ranks of `group`
    when torch.distributed is initialised, else one shard."""
    import torch.distributed as dist
    distributed = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if distributed else (0, 1)
    _, aid, shards, mine = _shard_plan(clips, rank, world)
    return shards, mine, _shard_rows(clips, aid, shards[rank], VALID_COLS, device)


def _valid_report(local: torch.Tensor, shards, group, clips: Sequence[Clip], parents, bone_pairs):
    """(:func:`reduce_valid` of all ranks' rows, the rows in clip-id order)."""
    allrows = _gather(local, shards, group, VALID_COLS)
    allrows = allrows[torch.argsort(allrows[:, 0], stable=True)]
    num_joints = int(clips[0].gt_norm.shape[1]) if len(clips) else 1
    return reduce_valid(allrows, num_joints if parents is not None else 1, bone_pairs), allrows


def validate_clips(lift_clip: Callable, clips: Sequence[Clip], rf: int, device, parents=H36M_17_PARENTS, group=None,
                   pos_is_sum: bool = True, gt_root_relative: bool = False, causal: bool = False,
                   bone_pairs: Optional[Sequence[tuple]] = None):
    """Trainer.test's pass over `clips` (trainer.py:174-225; no flip, no world transform): every clip is lifted and
    :func:`clip_valid` fills its row.  `lift_clip(padded (N+RF-1,J,F), param_row)` returns (poses, trj) - with `pos_is_sum`
    the poses are pos + trj, ``Ray3DLifter.forward_clip(..., return_trj=True)`` - or, for a configuration without a
    trajectory model, the poses alone.  With torch.distributed initialised (`group`: the process group, None the default one)
    whole clips are sharded over the ranks as in :func:`evaluate_clips` and the rows travel in ONE all_gather.
    Every rank returns (:func:`reduce_valid` of all rows, the rows in clip-id order)."""
    shards, mine, local = _valid_plan(clips, group, device)
    pad = (rf - 1) // 2
    for k, c in enumerate(mine):
        padded = torch.from_numpy(pad_clip(np.asarray(c.rays, dtype=np.float32), pad, pad if causal else 0)).to(device)
        res = lift_clip(padded, torch.from_numpy(c.camera.param()).to(device))
        poses, trj = res if isinstance(res, tuple) else (res, None)
        clip_valid(poses, trj, c, parents, pos_is_sum and trj is not None, out=local[k], gt_root_relative=gt_root_relative)
    return _valid_report(local, shards, group, clips, parents, bone_pairs)


def shard_valid_hip(pos_all: torch.Tensor, trj_all: Optional[torch.Tensor], gt_all: torch.Tensor, table_dev: torch.Tensor,
                    num_clips: int, total_frames: int, max_frames: int, rows: torch.Tensor, parents=H36M_17_PARENTS, flags: int = 0,
                    frames: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE r3d_clips_valid_losses call on the current stream for every clip of a shard: `pos_all` / `gt_all` (total_frames, J, 3)
    (or (total_frames, 1, J, 3)) float32, `trj_all` (total_frames, 3) (or (total_frames, 1, 1, 3)) float32 or None, `table_dev` the
    uploaded bytes of a table of r3d_clip_desc rows (:func:`clip_table`, or :func:`clip_frame_table`: the transforms are not
    read), `rows` the (num_clips, VALID_COLS) float64 matrix of row headers whose columns 3.. are written in place - with the
    bits :func:`clip_valid` gives clip by clip; `parents` the joint tree (None: no bone terms), `flags` R3D_VALID_*; optional
    `frames` (total_frames, VALID_COUNT).  No copy, no allocation (the scratch is a cached tensor per device), no
    synchronisation."""
    from . import _capi
    dev = pos_all.device
    _need(pos_all, "pos_all", torch.float32, dev, rows=total_frames, last=3)
    _need(gt_all, "gt_all", torch.float32, dev, rows=total_frames, last=3)
    J = pos_all.numel() // (3 * total_frames)
    if pos_all.numel() != gt_all.numel():
        raise ValueError("ground truth %s vs prediction %s" % (tuple(gt_all.shape), tuple(pos_all.shape)))
    if trj_all is not None:
        _need(trj_all, "trj_all", torch.float32, dev, rows=total_frames, numel=3 * total_frames)
    _need_table(table_dev, num_clips, _capi.CLIP_DESC_BYTES, dev)
    _need(rows, "rows (the matrix of row headers)", torch.float64, dev, shape=(num_clips, VALID_COLS))
    if frames is not None:
        _need(frames, "frames", torch.float64, dev, shape=(total_frames, M.VALID_COUNT))
    tree = validate_parents(parents, J) if parents is not None else None
    scratch = _shard_scratch(dev, _capi.clips_valid_scratch_bytes(num_clips, max_frames))
    with torch.cuda.device(dev):
        _capi.clips_valid_losses(pos_all.data_ptr(), trj_all.data_ptr() if trj_all is not None else None, gt_all.data_ptr(), total_frames,
                                 J, tree, flags, table_dev.data_ptr(), num_clips, max_frames, rows.data_ptr() + 3 * 8, VALID_COLS,
                                 frames.data_ptr() if frames is not None else None,
                                 scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream)
    return rows


def clip_frame_table(lengths: Sequence[int]):
    """(table, first_frame, total_frames, longest) for clips of these frame counts laid out back to back: r3d_clip_desc rows
    with the identity for a transform - what r3d_clips_valid_losses needs of a table (it reads first_frame / n_frames only; a
    caller that also evaluates hands it :func:`clip_table`'s)."""
    return _desc_table([int(n) for n in lengths], [(_IDENTITY_R, _IDENTITY_T)] * len(lengths))


def validate_clips_batched(lift_clip: Callable, clips: Sequence[Clip], rf: int, device, parents=H36M_17_PARENTS, group=None,
                           pos_is_sum: bool = True, gt_root_relative: bool = False, causal: bool = False,
                           bone_pairs: Optional[Sequence[tuple]] = None, encode: Optional[str] = None, repair: Optional[int] = None,
                           min_conf: float = 0.0, repair_out: Optional[dict] = None):
    """:func:`validate_clips` with the measuring side in ONE call per shard: the rank's clip table and ground truth are uploaded
    once, every clip is lifted into its slice of one pose buffer and one trajectory buffer
    (``lift_clip(padded, param_row, out=pose_slice, trj_out=trj_slice)``), and one :func:`shard_valid_hip` call fills the sums
    of all rows - then the same gather and :func:`reduce_valid`.  Same return values, the same bits in every row.  GPU only.

    `lift_clip` takes the two keywords and returns (poses, trj) - ``functools.partial(lifter.forward_clip, return_trj=True)``
    - or, for a configuration without a trajectory model, ignores ``trj_out`` and returns the poses alone; every clip of a
    pass must answer alike.  When it is (a partial of) the bound ``forward_clip`` of a lifter with lanes (``set_lanes``), the
    clips are dealt to the lanes and joined once, before the metrics call.

    `encode` ("ray" | "intrinsic" | "screen"): ``Clip.rays`` holds RAW PIXELS (N, J, 2) and the input side is one call per
    shard as well, exactly as in :func:`evaluate_clips_batched` (no mirror): the rank's pixels are uploaded once, ONE
    r3d_clips_encode call pads and encodes every clip, each clip is lifted from its slice with ``n_windows=``; a descriptor
    the encode call refuses raises.  `repair` / `min_conf` / `repair_out`: as in :func:`evaluate_clips_batched`."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("validate_clips_batched measures on the GPU (r3d_clips_valid_losses); on CPU tensors use validate_clips")
    lifter = _lifter_of(lift_clip, partial_ok=True)
    if encode is not None:        # (decided before the shards are cut: every rank raises alike, also one with an empty shard)
        _encoding_id(encode)
        _lifter_of(lift_clip, partial_ok=True, need="encode=")
    _repair_needs_encode(repair, encode)
    shards, mine, local = _valid_plan(clips, group, dev)
    if mine:
        table, first, total, longest = clip_frame_table([c.rays.shape[0] for c in mine])
        table_dev = _to_device_bytes(table, dev)
        gt_all = _ground_truth(mine, dev)
        pos_all = torch.empty((total, 1, gt_all.shape[1], 3), dtype=torch.float32, device=dev)
        trj_all = torch.empty((total, 1, 1, 3), dtype=torch.float32, device=dev)
        inputs = _ShardInputs(mine, rf, dev, causal, encode, lifter, repair=repair, min_conf=min_conf, repair_out=repair_out)

        def lift(k):
            rows = slice(first[k], first[k] + mine[k].rays.shape[0])
            x, _, prow, kw = inputs(k)
            return isinstance(lift_clip(x, prow, out=pos_all[rows], trj_out=trj_all[rows], **kw), tuple)

        with_trj = set(_deal(lifter, len(mine), lift))
        if len(with_trj) != 1:
            raise RuntimeError("lift_clip returned a trajectory for some clips of the pass and none for others")
        has_trj = with_trj.pop()
        if gt_root_relative and has_trj:
            raise ValueError("gt_root_relative is for models without a trajectory: with one the ground truth must be absolute")
        from . import _capi
        flags = (_capi.R3D_VALID_POS_IS_SUM if pos_is_sum and has_trj else 0) | (_capi.R3D_VALID_GT_ROOT_RELATIVE if gt_root_relative else 0)
        shard_valid_hip(pos_all, trj_all if has_trj else None, gt_all, table_dev, len(mine), total, longest, local, parents, flags)
    return _valid_report(local, shards, group, clips, parents, bone_pairs)


def reduce_valid(rows: torch.Tensor, num_joints: int = 17, bone_pairs: Optional[Sequence[tuple]] = None) -> Dict:
    """The figures of Trainer.test from the per-clip rows (:func:`clip_valid`), in the reference's units (its logs multiply
    every figure by 1000), frame-weighted over all clips as trainer.py:222-225 does:

    * ``valid_mm``: losses_3d_valid * 1000 - what a checkpoint stores as ``best_performance``; ``pos_mm``: test_pos;
    * ``trj_mm``: the depth-weighted root error by the elementwise definition of Trainer.train (:119-120);
      ``trj_mm_as_logged``: the figure Trainer.test logs as test_trj, mean(w) * mean(d) per clip (:217-218 broadcast the
      weights to an outer product);
    * ``bone_mm``: test_bone, length plus direction term; ``bone_len_mm`` and ``bone_dir`` (x 1000) its two parts;
    * ``bones``: one dict per bone (bone b = joint b+1 and its parent) from the same per-bone sums: ``len_err_mm`` mean
      |predicted - true length|, ``len_pred_mm`` / ``len_gt_mm`` the mean lengths, ``len_pred_std_mm`` the deviation of the
      predicted length over all frames, sqrt(E[l^2] - E[l]^2);
    * ``symmetry``: for every pair (a, b) of `bone_pairs` (mirror-image bones, e.g. skeleton.H36M_17_BONE_PAIRS) the
      differences of the two mean lengths, ``(a, b, pred_diff_mm, gt_diff_mm)``.
    Clips are added up in clip-id order: the result does not depend on how they were sharded."""
    rows = rows.detach().to("cpu", torch.float64)
    rows = rows[torch.argsort(rows[:, 0], stable=True)]
    n = rows[:, 2].sum()
    s = rows[:, 3:].sum(dim=0)
    C, W = M.VALID_COUNT, M.VALID_MAX_BONES
    logged = (rows[:, 3 + 3] * rows[:, 3 + 4] / rows[:, 2]).sum()
    out = {"frames": int(n), "valid_mm": float(s[0] / n * 1000.0), "pos_mm": float(s[1] / n * 1000.0),
           "trj_mm": float(s[2] / n * 1000.0), "trj_mm_as_logged": float(logged / n * 1000.0),
           "bone_len_mm": float(s[5] / n * 1000.0), "bone_dir": float(s[6] / n * 1000.0),
           "bone_mm": float((s[5] + s[6]) / n * 1000.0)}
    per = s[C:].reshape(M.VALID_BONE_ROWS, W) / n
    bones = []
    for b in range(max(num_joints - 1, 0)):
        var = float(per[2, b] - per[1, b] * per[1, b])
        bones.append({"len_err_mm": float(per[0, b] * 1000.0), "len_pred_mm": float(per[1, b] * 1000.0),
                      "len_gt_mm": float(per[3, b] * 1000.0), "len_pred_std_mm": float(np.sqrt(max(var, 0.0)) * 1000.0)})
    out["bones"] = bones
    out["symmetry"] = [(int(a), int(b), bones[a]["len_pred_mm"] - bones[b]["len_pred_mm"], bones[a]["len_gt_mm"] - bones[b]["len_gt_mm"])
                       for a, b in (bone_pairs or ())]
    return out


def format_valid_report(table: Dict, bone_names: Optional[Sequence[str]] = None) -> List[str]:
    """Plain text for the table of :func:`reduce_valid`: the four figures Trainer.test logs (trainer.py:275-278), the
    elementwise trajectory figure, then one line per bone and per mirror-image pair."""
    nb = len(table["bones"])
    names = list(bone_names) if bone_names is not None else ["bone %2d" % b for b in range(nb)]
    assert len(names) == nb
    lines = ["test      (losses_3d_valid): %.3f mm over %d frames" % (table["valid_mm"], table["frames"]),
             "test_pos  (root-relative):   %.3f mm" % table["pos_mm"],
             "test_trj  (as logged):       %.3f   [elementwise, as in training: %.3f]" % (table["trj_mm_as_logged"], table["trj_mm"]),
             "test_bone (length + direction): %.3f   [length %.3f mm]" % (table["bone_mm"], table["bone_len_mm"])]
    lines += ["%s: length error %.1f mm, length %.1f mm (true %.1f mm), deviation over time %.1f mm"
              % (names[b], t["len_err_mm"], t["len_pred_mm"], t["len_gt_mm"], t["len_pred_std_mm"]) for b, t in enumerate(table["bones"])]
    lines += ["%s vs %s: predicted lengths differ by %.1f mm (true: %.1f mm)" % (names[a], names[b], dp, dg)
              for a, b, dp, dg in table["symmetry"]]
    return lines


def format_report(named: Dict[str, tuple], average: tuple) -> List[str]:
    """The lines Trainer.evaluate logs (lib/train_val/trainer.py:459-477): per action, then the action-wise
    averages rounded to 0.1 mm."""
    labels = ("Protocol #1 Error (MPJPE):  ", "Protocol #2 Error (P-MPJPE):", "Protocol #3 Error (N-MPJPE):",
              "Velocity    Error (MPJVE):  ", "Root        Error (MRPE):  ")
    lines = []
    for action, vals in named.items():
        lines.append("----" + action + "----")
        lines += ["%s %s mm" % (lab, v) for lab, v in zip(labels, vals)]
        lines.append("----------")
    heads = ("Protocol #1   (MPJPE)", "Protocol #2 (P-MPJPE)", "Protocol #3 (N-MPJPE)", "Velocity      (MPJVE)",
             "Root           (MRPE)")
    lines += ["%s action-wise average: %s mm" % (h, round(float(v), 1)) for h, v in zip(heads, average)]
    return lines
