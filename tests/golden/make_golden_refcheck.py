"""tests/golden/make_golden_refcheck.py -- regenerates refcheck.json and loss_ref.npz by RUNNING THE REFERENCE ITSELF (needs the
reference tree and oracle/_ref, like make_golden.py):

    python tests/golden/make_golden_refcheck.py

The tests that pin the restatements (oracle/knn, oracle/ops_ref, oracle/inputs_ref, ffb6d_amd.loss, the KNN on the emulator) to the
reference's own code compare against these files, so they run wherever the repository is checked out:

  refcheck.json   sha256 of the reference's outputs on the seeded inputs built below: KNN indices, gathers and back-projection are
                  compared bit for bit, so a digest pins them as tightly as the arrays would
  loss_ref.npz    the reference's loss terms and gradients (compared to a tolerance: float sums)

The input builders live here so that the tests and this generator cannot drift apart.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFCHECK = os.path.join(HERE, "refcheck.json")
LOSS_REF = os.path.join(HERE, "loss_ref.npz")

PICK_SEEDS = (1, 99991)
KNN_CASES = [(1, 3000, 3000, 16), (2, 777, 1500, 1), (1, 4800, 48, 16), (1, 48, 4800, 1)]
LOSS_SEEDS = (0, 1)


def sha(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_refcheck():
    with open(REFCHECK) as fh:
        return json.load(fh)


def pick_points():
    """oracle distance pick vs cpp_knn_batch_distance_pick: 300 queries, K = 16, clock pinned to PICK_SEEDS"""
    return np.random.RandomState(5).rand(2, 700, 3).astype(np.float32)


def knn_case(B, S, Q, K):
    rng = np.random.RandomState(S + Q + K)
    return rng.rand(B, S, 3).astype(np.float32), rng.rand(B, Q, 3).astype(np.float32)


def ops_case():
    g = torch.Generator().manual_seed(3)
    feat = torch.randn(2, 7, 120, 1, generator=g)
    pool = torch.randint(0, 120, (2, 33, 16), generator=g)
    up = torch.randint(0, 120, (2, 500, 1), generator=g)
    xyz = torch.rand(2, 120, 3, generator=g)
    nei = torch.randint(0, 120, (2, 120, 16), generator=g)
    pc = torch.randn(2, 120, 9, generator=g)
    return feat, pool, up, xyz, nei, pc


def dpt_case():
    """a 480x640 depth image (mm) with invalid, NaN and Inf pixels, and the two (intrinsics, cam_scale) of LineMOD and YCB"""
    from ffb6d_amd import synth
    rng = np.random.RandomState(3)
    dpt = (1000.0 * (0.5 + rng.rand(480, 640))).astype(np.float32)
    dpt[rng.rand(480, 640) < 0.1] = 0.0
    dpt[7, 9], dpt[8, 10] = np.nan, np.inf
    return dpt, ((synth.LINEMOD_K, 1000.0), (np.array([[1066.778, 0., 312.9869], [0., 1067.487, 241.3109], [0., 0., 1.]]), 10000.0))


def emu_knn_case():
    g = np.random.default_rng(3)
    return g.standard_normal((2, 3500, 3)).astype(np.float32), g.standard_normal((2, 900, 3)).astype(np.float32)


def loss_case(seed, B=2, C=5, N=64, K=8):
    g = torch.Generator().manual_seed(seed)
    ep = {"pred_rgbd_segs": torch.randn(B, C, N, generator=g), "pred_kp_ofs": torch.randn(B, K, N, 3, generator=g),
          "pred_ctr_ofs": torch.randn(B, 1, N, 3, generator=g)}
    labels = torch.randint(0, C, (B, N), generator=g)
    labels[0, : N // 2] = 0                                  # background points carry no offset loss
    return ep, labels, torch.randn(B, N, K, 3, generator=g), torch.randn(B, N, 1, 3, generator=g)


def main():
    sys.path.insert(0, ROOT)
    import importlib.util
    import types
    import warnings
    from oracle import knn as oknn
    from oracle import ref_harness as rh

    out = {"distance_pick": {}, "knn_batch": {}, "ops": {}, "dpt_2_pcld": [], "emu_knn": {}}
    pts = pick_points()
    for seed in PICK_SEEDS:
        idx, q = rh.ref_knn_batch_distance_pick(pts, 300, 16, seed)
        out["distance_pick"][str(seed)] = {"idx": sha(idx), "queries": sha(q)}
    for case in KNN_CASES:
        sup, qry = knn_case(*case)
        out["knn_batch"]["%d,%d,%d,%d" % case] = sha(rh.ref_knn_batch(sup, qry, case[3], omp=True))

    m_ffb6d, m_randla, _ = rh.reference_modules()
    feat, pool, up, xyz, nei, pc = ops_case()
    out["ops"] = {"random_sample": sha(m_ffb6d.FFB6D.random_sample(feat, pool)),
                  "nearest_interpolation": sha(m_ffb6d.FFB6D.nearest_interpolation(feat, up)),
                  "gather_neighbour": sha(m_randla.Building_block.gather_neighbour(pc, nei)),
                  "relative_pos_encoding": sha(m_randla.Building_block(16).relative_pos_encoding(xyz, nei))}

    # Dataset.dpt_2_pcld (linemod_dataset.py:188-199) called unbound on an object carrying the two index maps of its __init__
    # (:31-32), then get_item's NaN / Inf clean-up (:258-259)
    Dataset = rh.reference_dataset_class()
    me = types.SimpleNamespace(xmap=np.array([[j for i in range(640)] for j in range(480)]),
                               ymap=np.array([[i for i in range(640)] for j in range(480)]))
    dpt, cams = dpt_case()
    for K, cam_scale in cams:
        want = Dataset.dpt_2_pcld(me, dpt.copy(), cam_scale, K)
        want[np.isnan(want)] = 0.0
        want[np.isinf(want)] = 0.0
        out["dpt_2_pcld"].append({"dtype": str(want.dtype), "shape": list(want.shape), "sha256": sha(want)})

    sup, qry = emu_knn_case()
    for K in (1, 16):
        want = rh.ref_knn_batch(sup, qry, K, omp=True)
        out["emu_knn"][str(K)] = [sha(oknn.canonical_ties(want[b], sup[b], qry[b])[0]) for b in range(sup.shape[0])]

    # the reference's loss module (ffb6d/models/loss.py), assembled as train_lm.py:245-259 with FocalLoss(gamma=2), OFLoss()
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(rh.REF_FFB6D, "models", "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    loss = {}
    for seed in LOSS_SEEDS:
        ep, labels, kp_t, ctr_t = loss_case(seed)
        leaves = {k: v.clone().requires_grad_(True) for k, v in ep.items()}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # F.log_softmax without dim (loss.py:31)
            seg = ref.FocalLoss(gamma=2)(leaves["pred_rgbd_segs"], labels.view(-1)).sum()
        kp = ref.OFLoss()(leaves["pred_kp_ofs"], kp_t, labels).sum()
        ctr = ref.OFLoss()(leaves["pred_ctr_ofs"], ctr_t, labels).sum()
        total = 2.0 * seg + kp + ctr
        total.backward()
        loss[f"s{seed}/terms"] = np.array([float(t) for t in (seg, kp, ctr, total)], np.float64)
        for k in sorted(leaves):
            loss[f"s{seed}/grad/{k}"] = leaves[k].grad.numpy()
    np.savez_compressed(LOSS_REF, **loss)
    with open(REFCHECK, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", REFCHECK, LOSS_REF)


if __name__ == "__main__":
    main()
