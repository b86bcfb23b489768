"""tests/golden/make_golden_taps.py -- regenerates the stage-boundary fixtures by RUNNING THE REFERENCE ITSELF with forward
hooks on its stage modules (build container only: needs /root/reference and oracle/_ref).  The reference is not edited: the
hooks sit on `rndla_ds_stages[i]`, `rndla_up_stages[i]`, `cnn_ds_stages[i]`, `cnn_up_stages[i]` and the eight
`{ds,up}_fuse_{p2r,r2p}_{pre,fuse}_layers[i]` lists and record what passes the stage boundaries of FFB6D.forward
(ffb6d/models/ffb6d.py:231-298).

    python tests/golden/make_golden_taps.py

Same batch, weights and index pyramid as make_golden.make_forward()'s small case (config 7, 2 frames, 1024 points, 120 x 160,
5 classes, seed-0 weights, the reference's own KNN); this run's end_points are checked against forward_small.npz, FRAME 0 is
kept.  All float32, reference layout ([C,H,W] / [C,N]).

  stage_taps_sample.npz   strided sample + `/absmax` + `/stride` of every stage output: the 14 post-fusion embeddings
                          (`rgb_emb_ds{i}`, `p_emb_ds{i}`, `rgb_emb_up{i}`, `p_emb_up{i}` -- the `taps` of oracle/forward_ref.py and
                          forward_pm.forward), and the stage outputs between them: `f_encoder_{i}` (rndla_ds_stages),
                          `f_decoder_{i}` (rndla_up_stages), `rgb_emb0_ds{i}` (cnn_ds_stages), `rgb_emb0_up{i}` (cnn_up_stages)
  stage_point_io.npz      point branch, whole tensors: `enc_in_{i}` (feature input of rndla_ds_stages[i]), `f_encoder_{i}`,
                          `p_emb0_ds{i}` (its sub-sampling = the input of ds_fuse_p2r_pre_layers[i]), and for the decoder
                          `dec_skip_{i}` / `dec_p_{i}` (the two tensors the reference concatenates, the second BEFORE the
                          interpolation) / `f_decoder_{i}`, i = 0..2.  `idx/<key>`: an index tensor of the pyramid wherever the
                          reference's kd-tree orders an exact distance tie differently from oracle.knn (none today)
  stage_fusion_io.npz     both fusion directions of encoder stage 1 (whole: `enc1/rgb_emb0`, `enc1/p_emb0`, `enc1/rgb_emb`,
                          `enc1/p_emb`) and of decoder stage 1 on the pixel rows U = (pixels named by r2p_up_nei_idx1) + (every
                          16th pixel): `dec1/U` (int32, sorted), `dec1/rgb_emb0_U`, `dec1/rgb_emb_U` ([C,|U|]), `dec1/p2r_idx_U`,
                          `dec1/r2p_idx_U` (r2p_up_nei_idx1 as positions in U), `dec1/p_emb0`, `dec1/p_emb`
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from ffb6d_amd import synth  # noqa: E402
from oracle import knn as oknn  # noqa: E402
from oracle import pyramid as opyr  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

GEOMETRY = dict(config=7, frames=2, n_points=1024, height=120, width=160, n_classes=5)
FILES = ("stage_taps_sample.npz", "stage_point_io.npz", "stage_fusion_io.npz")
STRIDES = (1, 7, 17, 37, 97, 197, 397, 797)     # primes: coprime to every channel count and map width
SAMPLE_MAX = 4096
# Agreement of this run's end_points with forward_small.npz (written by another process): oneDNN is bit-reproducible run to
# run on one machine and thread count (measured: equal bits); between thread counts end points move by ~1e-4 absolute, which is
# what this bar allows for, relative to each tensor's range.
END_POINT_BAR = 1e-5

STAGE_LISTS = ["rndla_ds_stages", "rndla_up_stages", "cnn_ds_stages", "cnn_up_stages"] + \
    ["%s_fuse_%s_%s_layers" % (a, b, c) for a in ("ds", "up") for b in ("p2r", "r2p") for c in ("pre", "fuse")]


def sample_stride(n):
    return next(s for s in STRIDES if n <= SAMPLE_MAX * s)


def frames_and_pyramid(knn_search):
    g = GEOMETRY
    frames = synth.make_batch(g["config"], g["frames"], n_points=g["n_points"], height=g["height"], width=g["width"])
    return frames, opyr.build_batch(frames, knn_search)


def hooked_reference_forward(frames, pyr):
    """({(list name, i): (input tensors, output)}, end_points) of the unmodified reference on CPU."""
    import torch
    model = rh.build_reference_model(n_classes=GEOMETRY["n_classes"], n_pts=GEOMETRY["n_points"])
    model.load_state_dict(synth.synth_state_dict(model, 0))
    model.eval()
    seen, handles = {}, []

    def recorder(key):
        def hook(mod, args, out):
            assert key not in seen, key
            seen[key] = ([a.detach().clone() for a in args if torch.is_tensor(a)], out.detach().clone())
        return hook
    for name in STAGE_LISTS:
        for i, mod in enumerate(getattr(model, name)):
            handles.append(mod.register_forward_hook(recorder((name, i))))
    inputs = {"rgb": torch.from_numpy(frames["rgb"].astype(np.float32)),
              "cld_rgb_nrm": torch.from_numpy(frames["cld_rgb_nrm"]),
              "choose": torch.from_numpy(frames["choose"].astype(np.int64))}
    for k, v in pyr.items():
        inputs[k] = torch.from_numpy(v.astype(np.int64) if v.dtype == np.int32 else v)
    with torch.no_grad():
        ep = model(inputs)
    for h in handles:
        h.remove()
    return seen, {k: v.numpy() for k, v in ep.items()}


def generate(verbose=True):
    """{file name: {key: array}} of the three fixtures, from a fresh run of the reference."""
    frames, pyr = frames_and_pyramid(mg.ref_knn_search)
    seen, ep = hooked_reference_forward(frames, pyr)
    gold = np.load(os.path.join(HERE, "forward_small.npz"))
    for k in gold.files:
        err = float(np.abs(ep[k] - gold[k]).max()) / float(np.abs(gold[k]).max())
        if verbose:
            print("end point %-16s vs forward_small.npz: max err / range %.3e%s" % (k, err, " (equal bits)" if np.array_equal(ep[k], gold[k]) else ""))
        assert err <= END_POINT_BAR, (k, err)

    def f0(t):
        """frame 0: [C,H,W], or [C,N] for the point branch's [B,C,N,1]"""
        a = t[0].numpy()
        return np.ascontiguousarray(a[..., 0] if a.ndim == 3 and a.shape[-1] == 1 else a)

    def out(name, i):
        return f0(seen[(name, i)][1])

    def arg(name, i):
        return f0(seen[(name, i)][0][0])

    # ---- every stage output by name ----
    stage = {}
    for i in range(4):
        stage["rgb_emb_ds%d" % i], stage["p_emb_ds%d" % i] = out("ds_fuse_p2r_fuse_layers", i), out("ds_fuse_r2p_fuse_layers", i)
        stage["f_encoder_%d" % i], stage["f_decoder_%d" % i] = out("rndla_ds_stages", i), out("rndla_up_stages", i)
        stage["rgb_emb0_ds%d" % i], stage["rgb_emb0_up%d" % i] = out("cnn_ds_stages", i), out("cnn_up_stages", i)
    for i in range(3):
        stage["rgb_emb_up%d" % i], stage["p_emb_up%d" % i] = out("up_fuse_p2r_fuse_layers", i), out("up_fuse_r2p_fuse_layers", i)

    # a. strided samples
    samples = {}
    for k, v in stage.items():
        s = sample_stride(v.size)
        samples[k] = np.ascontiguousarray(v.reshape(-1)[::s])
        samples[k + "/absmax"] = np.float32(np.abs(v).max())
        samples[k + "/stride"] = np.int32(s)

    # b. point branch, whole tensors
    point = {}
    ours = opyr.build_batch(frames, oknn.knn_search)         # what the tests rebuild
    for k in sorted(pyr):
        if not np.array_equal(pyr[k], ours[k]):
            assert pyr[k].dtype == np.int32, k               # only an index tensor may differ (exact-distance ties)
            if verbose:
                print("index tensor %s differs from oracle.knn (tie order): stored" % k)
            point["idx/" + k] = np.ascontiguousarray(pyr[k][0])
    for i in range(4):
        point["enc_in_%d" % i] = arg("rndla_ds_stages", i)
        point["f_encoder_%d" % i] = stage["f_encoder_%d" % i]
        point["p_emb0_ds%d" % i] = arg("ds_fuse_p2r_pre_layers", i)
        if i:
            assert np.array_equal(point["enc_in_%d" % i], stage["p_emb_ds%d" % (i - 1)])
    prev = stage["p_emb_ds3"]
    for i in range(3):
        cat, skip = arg("rndla_up_stages", i), stage["p_emb_ds%d" % (2 - i)]
        c = skip.shape[0]
        assert np.array_equal(cat[:c], skip)
        assert np.array_equal(cat[c:], prev[:, pyr["cld_interp_idx%d" % (3 - i)][0, :, 0]])     # ffb6d.py:273-278
        point["dec_skip_%d" % i], point["dec_p_%d" % i], point["f_decoder_%d" % i] = skip, prev, stage["f_decoder_%d" % i]
        prev = stage["p_emb_up%d" % i]

    # c. fusion stages
    fusion = {"enc1/rgb_emb0": stage["rgb_emb0_ds1"], "enc1/p_emb0": point["p_emb0_ds1"],
              "enc1/rgb_emb": stage["rgb_emb_ds1"], "enc1/p_emb": stage["p_emb_ds1"]}
    rgb0, rgb = stage["rgb_emb0_up1"], stage["rgb_emb_up1"]
    C, h, w = rgb0.shape
    r2p, p2r = pyr["r2p_up_nei_idx1"][0], pyr["p2r_up_nei_idx1"][0]                              # [n,16], [h*w,1]
    U = np.union1d(r2p.reshape(-1), np.arange(0, h * w, 16)).astype(np.int32)
    fusion.update({"dec1/U": U, "dec1/rgb_emb0_U": np.ascontiguousarray(rgb0.reshape(C, -1)[:, U]),
                   "dec1/rgb_emb_U": np.ascontiguousarray(rgb.reshape(C, -1)[:, U]),
                   "dec1/p2r_idx_U": np.ascontiguousarray(p2r[U].astype(np.int32)),
                   "dec1/r2p_idx_U": np.searchsorted(U, r2p).astype(np.int32),
                   "dec1/p_emb0": stage["f_decoder_1"], "dec1/p_emb": stage["p_emb_up1"]})
    assert np.array_equal(U[fusion["dec1/r2p_idx_U"]], r2p)
    res = dict(zip(FILES, (samples, point, fusion)))
    for d in res.values():
        for k, v in d.items():
            assert v.dtype in (np.float32, np.int32), (k, v.dtype)
    return res


def main():
    total = 0
    for name, arrays in generate().items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        total += size
        print("%s: %d arrays, %d bytes" % (name, len(arrays), size))
        assert size <= 834 * 1024, name                      # no new fixture larger than the largest one there was (f4_vectors.npz)
    assert total <= 2 * 1024 * 1024
    print("stage goldens written, %d bytes in all" % total)


if __name__ == "__main__":
    main()
