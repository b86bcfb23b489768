"""Point-to-plane against point-to-point ICP on the GPU box (ffb6d_amd.refine, metric="plane" | "point"): writes
profiles/icp_plane_bench.json and prints it.  Scene: the one of scripts/bench_icp_instances.py (scripts/icp_bench_scene.py), normals
estimated from the model clouds (refine.PreparedModels(normals="estimate")), gate 0.02 m.

For the class call (one problem per (frame, class), under the pose of the class's first instance) and both instance modes, at
1, 2, 3, 5 and 10 iterations: the time per call of the two metrics and the mean ADD of the poses they return.  With --parent-lib
(a libffb6d_amd.so built from the parent commit) the parent's point calls are timed in the same run, alternating with the others,
through the same Python wrappers: that is the comparison.  The cost of an iteration is the slope between 1 and 10 iterations.

The calls of a group alternate in one process; every sample times --inner calls in a row and ends in a device synchronise (host
clock); median / min / max of --reps samples after two warm-up rounds of every shape.  --profile runs the 10-iteration class call of
both metrics a few times and nothing else, for a kernel trace taken in a run of its own."""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import icp_inst_ref as iref  # noqa: E402
from ffb6d_amd import _lib, evaluate, refine  # noqa: E402
from icp_bench_scene import scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--n-points", type=int, default=12288)
ap.add_argument("--classes", type=int, default=5)
ap.add_argument("--model-points", type=int, default=2048)
ap.add_argument("--view-points", type=int, default=1000)
ap.add_argument("--free", type=float, default=0.4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--parent-lib", default=None, help="libffb6d_amd.so built from the parent commit: its point calls are timed too")
ap.add_argument("--profile", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_plane_bench.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
ITERS, MAX_DIST = (1, 2, 3, 5, 10), 0.02

s = scene(args.batch, args.n_points, args.classes, args.model_points, args.view_points, args.free)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
pcld, mask, inst = (up(s[k]) for k in ("pcld", "mask", "inst"))
frame_of, class_of, inst_of, T0 = (up(s[k]) for k in ("frame_of", "class_of", "inst_of", "T0"))
prepared = refine.PreparedModels(evaluate.ModelPoints(iref.models_of(s["models"]), device=dev), normals="estimate")
first = torch.arange(0, len(s["frame_of"]), 2, device=dev)              # the class problems: one per (frame, class)
first_np = np.arange(0, len(s["frame_of"]), 2)

parent = None
if args.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        if hasattr(parent, name):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = res, argtypes
    # the parent's calls read the model set prepared by this build: the same size here, and below the same bits from its point
    # calls as from this build's ("same_bits_as_point"); a parent with another layout fails one of the two
    sizes = [lib.ffb6d_icp_prepared_bytes(prepared.total, prepared.n_cls) for lib in (parent, _lib.load())]
    assert sizes[0] == sizes[1] == prepared.buf.numel(), f"prepared model set: {sizes} bytes, buffer {prepared.buf.numel()}"


@contextlib.contextmanager
def bound_to(lib):
    """The package's wrappers on another build of the library, so both builds are timed through the same Python.  It swaps the
    handle ffb6d_amd._lib.load() caches (`_lib._LIB`, what tests/simt/bind.py swaps for the emulator); that the prepared model
    set serves both builds is checked where the parent is loaded."""
    mine = _lib.load()
    _lib._LIB = lib
    try:
        yield
    finally:
        _lib._LIB = mine


def call(kind, metric, iters):
    kw = dict(max_iter=iters, max_dist=MAX_DIST, metric=metric)
    if kind == "class":
        return refine.icp_refine(pcld, mask, T0[first], frame_of[first], class_of[first], prepared, **kw)
    return refine.icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, prepared, mode=kind, **kw)


def parent_call(kind, iters):
    with bound_to(parent):
        kw = dict(max_iter=iters, max_dist=MAX_DIST)
        if kind == "class":
            return refine.icp_refine(pcld, mask, T0[first], frame_of[first], class_of[first], prepared, **kw)
        return refine.icp_refine_instances(pcld, mask, inst, T0, frame_of, class_of, inst_of, prepared, mode=kind, **kw)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.inner):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.inner


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=len(ms))


def alternate(fns, reps):
    for _ in range(2):                                                   # warm-up: every shape of the timed window
        for fn in fns.values():
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: summary(v) for k, v in times.items()}


def mean_add(kind, T):
    T = T.cpu().numpy()
    rows = first_np if kind == "class" else np.arange(len(s["class_of"]))
    return float(np.mean([iref.add(s["models"][s["class_of"][p]], T[k], s["gt"][p]) for k, p in enumerate(rows)]))


if args.profile:
    for _ in range(5):
        for metric in ("point", "plane"):
            call("class", metric, 10)
    torch.cuda.synchronize()
    sys.exit(0)

out = dict(batch=args.batch, n_points=args.n_points, classes=args.classes, model_points=args.model_points, reps=args.reps, inner=args.inner,
           free_share=args.free, max_dist=MAX_DIST, iterations=list(ITERS), problems_class=int(first.numel()),
           problems_instance=int(frame_of.numel()), parent_timed=parent is not None,
           add_before_mm=dict(class_call=1e3 * mean_add("class", T0[first]), instance_calls=1e3 * mean_add("map", T0)))
for kind in ("class", "map", "nearest"):
    fns = {}
    for it in ITERS:
        for metric in ("point", "plane"):
            fns[f"{metric}_{it}"] = lambda it=it, metric=metric: call(kind, metric, it)
        if parent is not None:
            fns[f"parent_point_{it}"] = lambda it=it: parent_call(kind, it)
    res = alternate(fns, args.reps)
    for it in ITERS:
        for metric in ("point", "plane"):
            T, st = call(kind, metric, it)
            res[f"{metric}_{it}"]["mean_add_mm"] = 1e3 * mean_add(kind, T)
        if parent is not None:                                           # the parent's point call computes what this one does
            same = bool(torch.equal(parent_call(kind, it)[0], call(kind, "point", it)[0]))
            assert same, f"{kind}, {it} iterations: the parent's point call and this build's give different poses"
            res[f"parent_point_{it}"]["same_bits_as_point"] = same
    per_iter = lambda name: (res[f"{name}_10"]["median_ms"] - res[f"{name}_1"]["median_ms"]) / 9      # noqa: E731
    res["ms_per_iteration"] = {m: per_iter(m) for m in ("point", "plane") + (("parent_point",) if parent is not None else ())}
    res["plane_over_point_per_iteration"] = res["ms_per_iteration"]["plane"] / res["ms_per_iteration"]["point"]
    if parent is not None:
        res["plane_over_parent_point_per_iteration"] = res["ms_per_iteration"]["plane"] / res["ms_per_iteration"]["parent_point"]
        res["point_over_parent_point_10"] = res["point_10"]["median_ms"] / res["parent_point_10"]["median_ms"]
    out[kind] = res

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(out, sort_keys=True))
