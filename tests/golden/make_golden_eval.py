"""tests/golden/make_golden_eval.py -- pose-evaluation goldens produced by RUNNING THE REFERENCE
(build container only; needs /root/reference):  python tests/golden/make_golden_eval.py

eval_small.npz holds, for the seeded inputs below (the tests regenerate them; only outputs are stored):
  add{i} / adds{i}                      Basic_Utils.cal_add_cuda / cal_adds_cuda of ADD_CASES[i] (RING_CASE last)
  auc{i}                                Basic_Utils.cal_auc of auc_lists()[i]
  ycb{i}_add / ycb{i}_adds / ycb{i}_kp (+ _len)
                                        eval_metric on pose_small.npz's YCB case i (its recorded reference poses, ids and
                                        keypoints against the true poses of synth.make_pose_case, plus one ground-truth
                                        object no prediction has); the 22 per-class lists
                                        concatenated, with their lengths in *_len
  te_{key}, te_means, te_mean_kp_err    TorchEval.cal_auc over te_lists() (symmetric ids included): AUC lists, the printed
                                        'average of all objects' add / adds / add(-s) and mean keypoint error
"""
import contextlib
import io
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from ffb6d_amd import synth  # noqa: E402

# (seed, n model points, pose pair kind)
ADD_CASES = [(501, 1, "near"), (502, 63, "near"), (503, 63, "far"), (504, 2000, "near"), (505, 2000, "zero"),
             (506, 2620, "near"), (507, 2620, "same"), (508, 2620, "far")]
RING_CASE = (509, 1200, 6)              # ring-symmetric model, prediction = ground truth turned by the symmetry angle
YCB_CASES = [(201, 2500, 3, True), (202, 1800, 2, False), (203, 1500, 4, True)]     # = make_golden_pose.YCB_CASES
YCB_MODEL_SIZES = [0, 300, 513, 64, 1000, 257]      # model cloud size per class id (row 0 unused)
N_CLS = 22                                          # config.n_classes of the YCB flow


def add_inputs(i):
    """(p3ds f32 [N,3], pred f32 [3,4], gt f32 [3,4]) of case i (ADD_CASES, then RING_CASE)."""
    if i < len(ADD_CASES):
        seed, n, kind = ADD_CASES[i]
        return (synth.model_cloud(seed, n),) + synth.eval_pose_pair(seed, kind)
    seed, n, k = RING_CASE
    _, gt = synth.eval_pose_pair(seed, "near")
    pred = gt.copy()
    pred[:, :3] = (gt[:, :3].astype(np.float64) @ synth.rot_z(synth.ring_angle(k))).astype(np.float32)
    return synth.ring_model(seed, n, k), pred, gt


def n_add_cases():
    return len(ADD_CASES) + 1


def auc_lists():
    rng = np.random.RandomState(601)
    return [[],                                                     # empty
            [0.11, 0.5, 0.1000001],                                 # all above the threshold
            [0.1, 0.05, 0.1, 0.02],                                 # exactly at the threshold (kept)
            [0.03, 0.03, 0.01, 0.03, 0.01, 0.2],                    # duplicates
            [0.042],                                                # a single value
            list(np.float32(0.15 * rng.rand(500)).astype(np.float64))]    # f32 distances as .item() gives them


def ycb_models():
    return {c: synth.model_cloud(700 + c, n) for c, n in enumerate(YCB_MODEL_SIZES) if c > 0}


def ycb_inputs(i, pose_golden):
    """The arguments of eval_metric for YCB case i (numpy; the caller turns them into tensors)."""
    seed, n, n_obj, _ = YCB_CASES[i]
    case = synth.make_pose_case(seed, n_pts=n, n_obj=n_obj)
    cls_ids, RTs, gt_kps = synth.pose_case_ground_truth(case, extra_seed=800 + i)
    return dict(cls_ids=cls_ids, RTs=RTs, gt_kps=gt_kps, pred_cls_ids=pose_golden[f"ycb{i}_ids"],
                pred_pose_lst=list(pose_golden[f"ycb{i}_pose"]), pred_kpc_lst=list(pose_golden[f"ycb{i}_kps"]))


def te_lists():
    """Per-class distance and kp-error lists for TorchEval.cal_auc (22 classes; some empty, symmetric ids 13, 16, 21 among
    the filled ones); class 0 holds every distance in sample order, as eval_pose_parallel leaves it."""
    rng = np.random.RandomState(602)
    add, adds, kp = ([[] for _ in range(N_CLS)] for _ in range(3))
    for c in (1, 2, 5, 13, 16, 21):
        for _ in range(rng.randint(3, 40)):
            a = float(np.float32(0.12 * rng.rand()))
            s = float(np.float32(a * rng.rand()))
            add[c].append(a)
            adds[c].append(s)
            add[0].append(a)
            adds[0].append(s)
            kp[c].append(np.float32(0.01 * rng.rand()))
    return add, adds, kp


TE_KEYS = ("add_auc_lst", "adds_auc_lst", "add_s_auc_lst")


def main():
    import torch

    from oracle import ref_harness as rh
    out = {}
    _, pose_mod = rh.reference_pose_modules()
    bs = pose_mod.bs_utils                              # the reference's Basic_Utils (no mesh override installed yet)
    assert hasattr(bs, "cal_adds_cuda"), "reference_pose_modules() was called with mesh overrides earlier in this process"
    for i in range(n_add_cases()):
        p3ds, pred, gt = (torch.from_numpy(a) for a in add_inputs(i))
        out[f"add{i}"] = np.float64(bs.cal_add_cuda(pred, gt, p3ds).item())
        out[f"adds{i}"] = np.float64(bs.cal_adds_cuda(pred, gt, p3ds).item())
    for i, lst in enumerate(auc_lists()):
        out[f"auc{i}"] = np.float64(bs.cal_auc(lst))

    pose_golden = np.load(os.path.join(HERE, "pose_small.npz"))
    models = ycb_models()
    names = list(pose_mod.cls_lst)
    bs.get_pointxyz_cuda = lambda cls, ds_type="ycb": torch.from_numpy(models[names.index(cls) + 1].copy())
    pose_mod.config.n_classes = N_CLS
    for i in range(len(YCB_CASES)):
        a = ycb_inputs(i, pose_golden)
        add, adds, kp = pose_mod.eval_metric(torch.from_numpy(a["cls_ids"]), a["pred_pose_lst"], a["pred_cls_ids"],
                                             torch.from_numpy(a["RTs"]), None, None, torch.from_numpy(a["gt_kps"]), None,
                                             a["pred_kpc_lst"])
        for name, lists, dt in (("add", add, np.float64), ("adds", adds, np.float64), ("kp", kp, np.float64)):
            out[f"ycb{i}_{name}"] = np.asarray([v for lst in lists for v in lst], dt)
            out[f"ycb{i}_{name}_len"] = np.asarray([len(lst) for lst in lists], np.int64)

    te = pose_mod.TorchEval()
    te.cls_add_dis, te.cls_adds_dis, te.pred_kp_errs = te_lists()
    printed = io.StringIO()
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(printed):
        pose_mod.config.log_eval_dir = tmp
        te.cal_auc()
        pk = [f for f in os.listdir(tmp) if not f.endswith("_id2pose.pkl")]
        with open(os.path.join(tmp, pk[0]), "rb") as fh:
            sv = pickle.load(fh)
    for k in TE_KEYS:
        out[f"te_{k}"] = np.asarray(sv[k], np.float64)
    # the means are only printed by the reference: "mean kps errs: x", then add / adds / add(-s) under "Average of all object:"
    lines = printed.getvalue().splitlines()
    out["te_mean_kp_err"] = np.float64(float(next(ln for ln in lines if ln.startswith("mean kps errs:")).split(":")[1]))
    avg = lines.index("Average of all object:")
    out["te_means"] = np.array([float(lines[avg + 1 + j].split("\t")[1]) for j in range(3)], np.float64)

    path = os.path.join(HERE, "eval_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
