"""Pose evaluation on the GPU: ADD / ADD-S and their AUCs, the numbers every FFB6D result is reported in.

Host-side mirror of the reference's evaluation
    Basic_Utils.cal_add_cuda / cal_adds_cuda / cal_auc, VOCap   ffb6d/utils/basic_utils.py:34-46,642-669
    eval_metric / eval_metric_lm                                ffb6d/utils/pvn3d_eval_utils_kpls.py:162-196,287-305
    TorchEval (cal_auc, cal_lm_add, eval_pose_parallel)         ffb6d/utils/pvn3d_eval_utils_kpls.py:326-506
over the C ABI of include/ffb6d_eval.h.  The reference scores one object at a time (two [N,N,3] tensors and a host
sync per distance); here every object of a frame or of a batch goes through one `add_adds` launch.

The model clouds the reference reads from dataset files (`get_pointxyz_cuda`) and the LineMOD diameters
(`models_info.yml`) are arguments.  There is no CPU fallback: distances are computed by the HIP library on a GPU;
only the AUC arithmetic (`VOCap`, `cal_auc`) is plain numpy.
"""
import os
import pickle

import numpy as np
import torch

from . import _lib
from . import pose as _pose
from .ops import _need_gpu, _stream

YCB_SYM_CLS_IDS = [13, 16, 19, 20, 21]     # common.py:96
LM_SYM_CLS_IDS = [10, 11]                  # common.py:103


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _default_device():
    return torch.device("cuda", torch.cuda.current_device())


class ModelPoints:
    """Model clouds of every class, uploaded once: `points` is a list (index = class id) or a dict {class id: [N_c,3]};
    classes missing from a dict, or given as None, have 0 points.  Holds pts f32 [total,3] and begin i64 [n_cls+1] on
    `device` and the per-class sizes on the host."""

    def __init__(self, points, device=None):
        if isinstance(points, dict):
            n_cls = max(int(k) for k in points) + 1 if points else 0
            points = [points.get(c) for c in range(n_cls)]
        arrs = [np.zeros((0, 3), np.float32) if p is None else np.ascontiguousarray(_np(p), np.float32).reshape(-1, 3)
                for p in points]
        self.n_cls = len(arrs)
        if self.n_cls == 0:
            raise ValueError("ModelPoints needs at least one class")
        self.counts = np.array([len(a) for a in arrs], np.int64)
        self.max_points = int(self.counts.max())
        self.device = torch.device(device) if device is not None else _default_device()
        begin = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.pts = torch.from_numpy(np.concatenate(arrs)).to(self.device)
        self.begin = torch.from_numpy(begin).to(self.device)

    @classmethod
    def of_tensor(cls, p3ds):
        """One class made of an [N,3] float32 device tensor, used in place (no copy when already contiguous)."""
        self = cls.__new__(cls)
        self.pts = p3ds.detach().contiguous().float()
        self.n_cls, self.counts = 1, np.array([p3ds.shape[0]], np.int64)
        self.max_points, self.device = int(p3ds.shape[0]), p3ds.device
        self.begin = torch.tensor([0, int(p3ds.shape[0])], dtype=torch.int64, device=p3ds.device)
        return self


def _launch(models, pred, gt, class_of):
    """pred, gt f32 [Q,3,4] and class_of i32 [Q] already on models.device -> add, adds f32 [Q]."""
    _need_gpu(pred, gt, class_of, models.pts)
    Q = int(class_of.shape[0])
    dev = models.device
    add = torch.empty((Q,), dtype=torch.float32, device=dev)
    adds = torch.empty((Q,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    wbytes = lib.ffb6d_pose_add_adds_workspace_bytes(Q, models.max_points)
    ws = torch.empty((max(wbytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _lib.traced("add_adds", 0, (Q, models.max_points)):
        rc = lib.ffb6d_pose_add_adds_f32(models.pts.data_ptr(), models.begin.data_ptr(), models.n_cls, class_of.data_ptr(),
                                         pred.data_ptr(), gt.data_ptr(), Q, add.data_ptr(), adds.data_ptr(), ws.data_ptr(),
                                         wbytes, _stream(models.pts))
    _lib.check(rc, "ffb6d_pose_add_adds_f32")
    return add, adds


def _poses(x, dev):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, np.float32))
    return t.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3, 4).contiguous()


def add_adds(pred_RT, gt_RT, class_of, models):
    """ADD and ADD-S of Q objects in one launch: pred_RT, gt_RT [Q,3,4] (numpy or tensors; cast to float32 first, like
    eval_metric's `pred_RT.astype(np.float32)`, :183), class_of [Q] class ids into `models` (a ModelPoints).
    Returns device tensors add [Q], adds [Q] (metres), not read back.  The library reads the Q class ids and the class
    table back to validate them and size its grid (include/ffb6d_eval.h): the call waits for the work queued before it."""
    dev = models.device
    pred, gt = _poses(pred_RT, dev), _poses(gt_RT, dev)
    cls = class_of if torch.is_tensor(class_of) else torch.from_numpy(np.asarray(class_of, np.int64).reshape(-1))
    cls = cls.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if pred.shape[0] != cls.shape[0] or gt.shape[0] != cls.shape[0]:
        raise ValueError(f"{pred.shape[0]} predicted / {gt.shape[0]} ground-truth poses for {cls.shape[0]} class ids")
    return _launch(models, pred, gt, cls)


def cal_add_cuda(pred_RT, gt_RT, p3ds):
    """basic_utils.py:651-657: mean distance between the model points p3ds [N,3] (device) under both poses; 0-d tensor."""
    return add_adds(pred_RT, gt_RT, [0], ModelPoints.of_tensor(p3ds))[0][0]


def cal_adds_cuda(pred_RT, gt_RT, p3ds):
    """basic_utils.py:659-669: mean over the ground-truth points of the distance to the nearest predicted point; 0-d tensor."""
    return add_adds(pred_RT, gt_RT, [0], ModelPoints.of_tensor(p3ds))[1][0]


def VOCap(rec, prec):
    """Area under the accuracy-threshold curve up to 0.1 (basic_utils.py:34-46), same arithmetic: rec sorted distances
    (inf = beyond the threshold, dropped), prec the cumulative accuracy; the curve is closed at (0.1, last accuracy)."""
    keep = rec != np.inf
    if not keep.any():
        return 0
    r, p = rec[keep], prec[keep]
    mrec = np.concatenate(([0.0], r, [0.1])).astype(np.float64)
    mpre = np.concatenate(([0.0], p, [p[-1]])).astype(np.float64)
    m = len(p)
    mpre[:m] = np.maximum.accumulate(mpre[:m])      # the reference's running max stops short of the last two entries
    step = np.flatnonzero(mrec[1:] != mrec[:-1]) + 1
    return np.sum((mrec[step] - mrec[step - 1]) * mpre[step]) * 10


def cal_auc(add_dis, max_dis=0.1):
    """basic_utils.py:642-649: AUC (in percent) of a list of distances; distances above max_dis count as misses
    (inf), an empty list gives 0."""
    d = np.array(add_dis)
    d[d > max_dis] = np.inf
    d = np.sort(d)
    n = len(add_dis)
    acc = np.arange(1, n + 1, dtype=np.float32) / n
    return VOCap(d, acc) * 100


def _frame_rows(cls_ids, pred_cls_ids, pred_pose_lst, pred_kpc_lst, gt_kps):
    """YCB matching of eval_metric (:170-184): gt objects in order up to the first id 0; each takes the first prediction
    of its class, else a zero pose and zero keypoints.  -> list of (class id, icls, pred RT f32 [3,4], kp_err or None)."""
    ids = _np(cls_ids).reshape(len(cls_ids), -1)[:, 0] if len(cls_ids) else np.zeros(0, np.int64)
    pred_ids = _np(pred_cls_ids).reshape(-1)
    rows = []
    for icls, cid in enumerate(ids):
        cid = int(cid)
        if cid == 0:
            break
        match = np.where(pred_ids == cid)[0]
        gt_kp = _np(gt_kps[icls]) if gt_kps is not None else None
        if len(match) == 0:
            pred_RT = np.zeros((3, 4), np.float32)
            pred_kp = np.zeros(gt_kp.shape) if gt_kp is not None else None
        else:
            pred_RT = np.asarray(pred_pose_lst[match[0]]).astype(np.float32)
            pred_kp = np.asarray(pred_kpc_lst[match[0]])[:-1, :] if gt_kp is not None else None
        kp_err = np.linalg.norm(gt_kp - pred_kp, axis=1).mean() if gt_kp is not None else None
        rows.append((cid, icls, pred_RT, kp_err))
    return rows


def eval_metric(cls_ids, pred_pose_lst, pred_cls_ids, RTs, mask, label, gt_kps, gt_ctrs, pred_kpc_lst, models=None,
                n_cls=None):
    """pvn3d_eval_utils_kpls.py:162-196 with the model clouds as `models` (a ModelPoints indexed by class id; the
    reference reads them with get_pointxyz_cuda).  n_cls: length of the per-class lists (default models.n_cls; the
    reference uses config.n_classes).  Every object of the frame is scored by one add_adds launch.
    Returns (cls_add_dis, cls_adds_dis, cls_kp_err): distances go to their class and to class 0, kp errors
    (float32 mean of the keypoint norms, centre row excluded) to their class only."""
    if models is None:
        raise ValueError("models (ModelPoints) is required")
    n_cls = n_cls or models.n_cls
    cls_add_dis, cls_adds_dis, cls_kp_err = ([[] for _ in range(n_cls)] for _ in range(3))
    rows = _frame_rows(cls_ids, pred_cls_ids, pred_pose_lst, pred_kpc_lst, gt_kps)
    if not rows:
        return cls_add_dis, cls_adds_dis, cls_kp_err
    gts = np.stack([_np(RTs[icls]) for _, icls, _, _ in rows])
    add, adds = add_adds(np.stack([r[2] for r in rows]), gts, [r[0] for r in rows], models)
    add, adds = add.tolist(), adds.tolist()
    for k, (cid, _, _, kp_err) in enumerate(rows):
        cls_kp_err[cid].append(kp_err)
        for lst, v in ((cls_add_dis, add[k]), (cls_adds_dis, adds[k])):
            lst[cid].append(v)
            lst[0].append(v)
    return cls_add_dis, cls_adds_dis, cls_kp_err


def eval_metric_lm(cls_ids, pred_pose_lst, RTs, mask, label, obj_id, models=None, n_cls=None):
    """pvn3d_eval_utils_kpls.py:287-305: the one predicted pose against RTs[0], model cloud of class obj_id in `models`.
    Returns (cls_add_dis, cls_adds_dis)."""
    if models is None:
        raise ValueError("models (ModelPoints) is required")
    n_cls = n_cls or models.n_cls
    cls_add_dis, cls_adds_dis = [[] for _ in range(n_cls)], [[] for _ in range(n_cls)]
    add, adds = add_adds(np.asarray(pred_pose_lst[0]).astype(np.float32)[None], _np(RTs[0])[None], [obj_id], models)
    add, adds = add.item(), adds.item()
    for lst, v in ((cls_add_dis, add), (cls_adds_dis, adds)):
        lst[obj_id].append(v)
        lst[0].append(v)
    return cls_add_dis, cls_adds_dis


class TorchEval:
    """Accumulates the distances of a test run and summarises them, like the reference's TorchEval (:326-506).
    models: ModelPoints indexed by class id; sym_cls_ids: classes whose ADD(-S) is ADD-S (YCB_SYM_CLS_IDS /
    LM_SYM_CLS_IDS).  Distances stay on the device, one pair of tensors per scored batch, until a summary is asked for;
    the reference-named lists (cls_add_dis, cls_adds_dis, pred_kp_errs, pred_id2pose_lst) are filled then."""

    def __init__(self, n_cls=22, models=None, sym_cls_ids=YCB_SYM_CLS_IDS):
        self.n_cls = n_cls
        self.models = models
        self.sym_cls_ids = list(sym_cls_ids)
        self.cls_add_dis = [[] for _ in range(n_cls)]
        self.cls_adds_dis = [[] for _ in range(n_cls)]
        self.pred_kp_errs = [[] for _ in range(n_cls)]
        self.pred_id2pose_lst = []
        self._pending = []              # (class id per row, add [Q] device tensor, adds [Q] device tensor)

    # ---- scoring ----------------------------------------------------------------------------------------------
    def _score(self, cls, pred, gt):
        """One upload (poses and class ids in one buffer) and one launch for the rows of a batch."""
        Q = len(cls)
        if Q == 0:
            return
        if self.models is None:
            raise ValueError("TorchEval needs models (ModelPoints) to score poses")
        buf = np.empty(24 * Q + Q, np.float32)
        buf[:12 * Q] = np.asarray(pred, np.float32).reshape(-1)
        buf[12 * Q:24 * Q] = np.asarray(gt, np.float32).reshape(-1)
        buf[24 * Q:].view(np.int32)[:] = cls
        dev = torch.from_numpy(buf).to(self.models.device, non_blocking=False)
        add, adds = _launch(self.models, dev[:12 * Q].view(Q, 3, 4), dev[12 * Q:24 * Q].view(Q, 3, 4),
                            dev[24 * Q:].view(torch.int32))
        self._pending.append((np.asarray(cls, np.int64), add, adds))

    def eval_poses(self, results, cls_ids, RTs, gt_kps=None, obj_id=None):
        """Score what pose.solve_poses (or one batch of pipeline.SensorToPose.run) returned, without solving again.
          results: list over frames of (class ids, poses [n,3,4], keypoints [n,n_kps+1,3]);
          cls_ids [B,n_obj(,1)], RTs [B,n_obj,3,4]: ground truth per frame (YCB flow, matched as eval_metric does);
          gt_kps [B,n_obj,n_kps,3]: optional, adds the keypoint errors;
          obj_id: LineMOD flow instead -- each frame's first pose against RTs[b][0], scored with the model of obj_id."""
        cls, pred, gt = [], [], []
        if obj_id is not None:
            for b, (_, poses, _) in enumerate(results):
                cls.append(int(obj_id))
                pred.append(np.asarray(poses[0]).astype(np.float32))
                gt.append(_np(RTs[b][0]))
        else:
            for b, (ids, poses, kps) in enumerate(results):
                rows = _frame_rows(cls_ids[b], ids, poses, kps, gt_kps[b] if gt_kps is not None else None)
                for cid, icls, pred_RT, kp_err in rows:
                    cls.append(cid)
                    pred.append(pred_RT)
                    gt.append(_np(RTs[b][icls]))
                    if kp_err is not None:
                        self.pred_kp_errs[cid].append(kp_err)
                self.pred_id2pose_lst.append({cid: p for cid, p in zip(ids, poses)})
        self._score(cls, pred, gt)

    def eval_pose_parallel(self, pclds, rgbs, masks, pred_ctr_ofs, gt_ctr_ofs, labels, cnt, cls_ids, RTs, pred_kp_ofs,
                           gt_kps, gt_ctrs, min_cnt=20, merge_clus=False, use_ctr_clus_flter=True, use_ctr=True, obj_id=0,
                           kp_type='farthest', ds='ycb', mesh_kps=None, mesh_ctr=None, r_lst=None):
        """The reference's signature (:448-500) plus the mesh keypoints / centres / radii pose.cal_frame_poses takes
        (ds='ycb': mesh_kps [n_cls,n_kps,3], mesh_ctr [n_cls,3] by class id, r_lst; otherwise the object's own
        mesh_kps [n_kps,3], mesh_ctr [3]).  One pose.solve_poses call for the whole batch, then one scoring launch."""
        if mesh_kps is None or (use_ctr and mesh_ctr is None):
            raise ValueError("mesh_kps / mesh_ctr are required")
        masks = masks.long()
        if ds == "ycb":
            res = _pose.solve_poses(pclds, masks, pred_ctr_ofs, pred_kp_ofs, mesh_kps, mesh_ctr, r_lst=r_lst, use_ctr=use_ctr,
                                    use_ctr_clus_flter=use_ctr_clus_flter)
            self.eval_poses(res, cls_ids, RTs, gt_kps=gt_kps)
        else:
            n_kps = pred_kp_ofs.shape[1]
            kps = np.zeros((2, n_kps, 3), np.float32)
            kps[1] = np.asarray(mesh_kps, np.float32).reshape(n_kps, 3)
            ctr = np.zeros((2, 3), np.float32)
            if mesh_ctr is not None:
                ctr[1] = np.asarray(mesh_ctr, np.float32).reshape(3)
            res = _pose.solve_poses(pclds, masks, pred_ctr_ofs, pred_kp_ofs, kps, ctr, use_ctr=use_ctr,
                                    use_ctr_clus_flter=use_ctr_clus_flter, refine_mask=False, classes=[1])
            self.eval_poses(res, cls_ids, RTs, obj_id=obj_id)

    # ---- summaries --------------------------------------------------------------------------------------------
    def _flush(self):
        """Moves the distances of the scored batches into the per-class lists (reads them back)."""
        for cls, add, adds in self._pending:
            for lst, vals in ((self.cls_add_dis, add.tolist()), (self.cls_adds_dis, adds.tolist())):
                for cid, v in zip(cls, vals):
                    lst[cid].append(v)
                    lst[0].append(v)
        self._pending = []

    def _add_s(self, cls_id, sym):
        return self.cls_adds_dis[cls_id] if cls_id in sym else self.cls_add_dis[cls_id]

    def cal_auc(self, save_dir=None):
        """Summary of a YCB run (:340-399): per-class AUCs of ADD, ADD-S and ADD(-S) (ADD-S for sym_cls_ids), index 0 =
        all objects; the 'average of all objects' means over classes 1..n_cls-1 (classes without samples count as 0);
        the mean keypoint error.  Pickles the reference's two files into save_dir if given.
        Unlike the reference, calling it twice gives the same answer: the reference's `self.cls_add_s_dis[0] +=`
        appends every class's ADD(-S) list to class 0 again on each call; here the class-0 ADD(-S) list is built anew."""
        self._flush()
        add_s = [[] for _ in range(self.n_cls)]
        for c in range(1, self.n_cls):
            add_s[c] = self._add_s(c, self.sym_cls_ids)
            add_s[0] = add_s[0] + add_s[c]
        add_auc = [cal_auc(self.cls_add_dis[i]) for i in range(self.n_cls)]
        adds_auc = [cal_auc(self.cls_adds_dis[i]) for i in range(self.n_cls)]
        add_s_auc = [cal_auc(add_s[i]) for i in range(self.n_cls)]
        n_objs = sum(len(lst) for lst in self.pred_kp_errs)
        kp_sum = 0.0
        for c in range(1, self.n_cls):
            kp_sum += sum(self.pred_kp_errs[c])
        sv_info = dict(add_dis_lst=self.cls_add_dis, adds_dis_lst=self.cls_adds_dis, add_auc_lst=add_auc,
                       adds_auc_lst=adds_auc, add_s_auc_lst=add_s_auc, pred_kp_errs=self.pred_kp_errs)
        if save_dir is not None:
            tag = "{}_{}_{}".format(adds_auc[0], add_auc[0], add_s_auc[0])
            with open(os.path.join(save_dir, "pvn3d_eval_cuda_{}.pkl".format(tag)), "wb") as fh:
                pickle.dump(sv_info, fh)
            with open(os.path.join(save_dir, "pvn3d_eval_cuda_{}_id2pose.pkl".format(tag)), "wb") as fh:
                pickle.dump(self.pred_id2pose_lst, fh)
        out = dict(sv_info)
        out.update(mean_add_auc=np.mean(add_auc[1:]), mean_adds_auc=np.mean(adds_auc[1:]),
                   mean_add_s_auc=np.mean(add_s_auc[1:]), mean_kp_err=kp_sum / n_objs if n_objs else float("nan"))
        return out

    def cal_lm_add(self, obj_id, diameter, test_occ=False, save_dir=None):
        """Summary of a LineMOD run for one object (:401-446): AUCs of ADD, ADD-S, ADD(-S) (ADD-S for LM_SYM_CLS_IDS) and
        `add` / `adds`, the percentage of samples closer than 0.1 * diameter; diameter in mm as models_info.yml gives it.
        The reference's own cal_lm_add needs its LineMOD config, which is not loadable everywhere: the 0.1-diameter rule
        is pinned against a numpy restatement of :420-422, the AUCs against the reference's cal_auc."""
        self._flush()
        add_lst, adds_lst = self.cls_add_dis[obj_id], self.cls_adds_dis[obj_id]
        add_s_lst = self._add_s(obj_id, LM_SYM_CLS_IDS)
        d = diameter / 1000.0 * 0.1
        add = np.mean(np.array(add_lst) < d) * 100
        adds = np.mean(np.array(adds_lst) < d) * 100
        sv_info = dict(add_dis_lst=self.cls_add_dis, adds_dis_lst=self.cls_adds_dis, add_auc_lst=[cal_auc(add_lst)],
                       adds_auc_lst=[cal_auc(adds_lst)], add_s_auc_lst=[cal_auc(add_s_lst)], add=add, adds=adds)
        if save_dir is not None:
            occ = "occlusion" if test_occ else ""
            with open(os.path.join(save_dir, "pvn3d_eval_cuda_{}_{}_{}_{}.pkl".format(obj_id, occ, add, adds)), "wb") as fh:
                pickle.dump(sv_info, fh)
        return sv_info
