"""Writes tests/golden/color_jitter.npz: small images, ColorJitter parameter sets and PILLOW's outputs for them, with the operation
sequence that torchvision's PIL backend performs (tests/color_jitter_ref.pil_color_jitter), plus the SHA-256 digests of Pillow's
output on the 4096 x 4096 image of all 2^24 colours for the hue at shifts 244 and 12 and the saturation at 0.8 and 1.2.

    python tests/golden/make_golden_jitter.py          (needs PIL; about a minute, most of it the colour cube)

Nothing of the project's arithmetic goes into the file: the restatement (tests/color_jitter_ref.py) and the kernels are held TO it.
npz keys: img_<i> uint8 [3,H,W]; out_<k> uint8 [3,H,W] of case k; meta: one JSON string {"pillow": version,
"cases": [{"img": i, "params": {...} or null, "what": ...}], "cube": [{"params": {...}, "sha256": ...}]}."""
import hashlib
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import color_jitter_ref as ref  # noqa: E402

OUT = os.path.join(HERE, "color_jitter.npz")
CUBE = [dict(order=[3], hue=-0.05), dict(order=[3], hue=0.05), dict(order=[2], saturation=0.8), dict(order=[2], saturation=1.2)]


def images():
    rng = np.random.RandomState(20240607)
    yy, xx = np.mgrid[0:64, 0:64]
    smooth = np.stack([(yy * 4) % 256, (xx * 3 + yy) % 256, 255 - (xx * 2 + yy * 2) % 256]).astype(np.uint8)
    imgs = dict(
        px1=rng.randint(0, 256, (3, 1, 1)), px2=rng.randint(0, 256, (3, 1, 2)), small=rng.randint(0, 256, (3, 3, 5)),
        odd=rng.randint(0, 256, (3, 37, 53)), aligned=smooth,
        constant=np.broadcast_to(np.array([40, 120, 200]).reshape(3, 1, 1), (3, 3, 5)),
        white=rng.randint(236, 256, (3, 3, 5)),
        half=np.array([10, 11] * 3).reshape(3, 1, 2),                   # grey 10 and 11: L = 10 and 11, mean 10.5, m = 11
        coarse=rng.randint(0, 4, (3, 5, 7)) * 85)
    return {k: np.ascontiguousarray(v, dtype=np.uint8) for k, v in imgs.items()}


def cases():
    """(image name, params, what)"""
    rng = np.random.RandomState(7)
    out = []
    factors = [0.0, 1.0, 0.37, 0.8, 1.2, 1.9, 2.5]
    hues = [-0.05, 0.05, -0.5, 0.5, 0.0, 0.31]
    for k, order in enumerate(itertools.permutations(range(4))):        # every order once, contrast in every position
        p = dict(order=list(order), brightness=factors[(k + 2) % 7], contrast=factors[(k + 4) % 7], saturation=factors[(k + 5) % 7],
                 hue=hues[k % 6])
        out.append(("small", p, "order"))
    for name in ("px1", "px2", "odd", "aligned", "constant", "white", "half", "coarse"):
        order = rng.permutation(4).tolist()
        out.append((name, dict(order=order, brightness=float(rng.uniform(0.8, 1.2)), contrast=float(rng.uniform(0.8, 1.2)),
                               saturation=float(rng.uniform(0.8, 1.2)), hue=float(rng.uniform(-0.05, 0.05))), "reference ranges"))
    out.append(("odd", dict(order=[2, 0, 3, 1], brightness=1.6, contrast=0.45, saturation=1.9, hue=-0.5), "wide factors"))
    out.append(("aligned", dict(order=[1, 3, 2, 0], brightness=0.6, contrast=1.7, saturation=0.3, hue=0.5), "wide factors"))
    out.append(("white", dict(order=[0, 1, 2, 3], brightness=1.5, contrast=2.0, saturation=2.5, hue=0.05), "clip"))
    out.append(("half", dict(order=[1], contrast=0.5), "mean 10.5"))
    out.append(("half", dict(order=[1], contrast=0.0), "mean 10.5"))
    out.append(("small", None, "0 operations"))
    out.append(("small", dict(order=[3, 2, 1, 0]), "0 operations"))
    for op, key in enumerate(ref.KEYS):                                 # single operations at every kind of factor
        for v in (hues[:4] if key == "hue" else [0.0, 1.0, 0.37, 1.9]):
            out.append(("coarse" if op % 2 else "small", {"order": [op], key: v}, "1 operation"))
    out.append(("small", dict(order=[0, 1, 2, 3], contrast=1.3, hue=-0.05), "2 operations"))
    out.append(("small", dict(order=[3, 2, 1, 0], brightness=0.9, saturation=1.1), "2 operations"))
    out.append(("small", dict(order=[2, 1, 0, 3], brightness=1.1, contrast=0.9, saturation=0.0), "3 operations"))
    out.append(("coarse", dict(order=[3, 0, 1], brightness=1.0, contrast=1.2, hue=0.5), "3 operations"))
    return out


def main():
    import PIL
    imgs = images()
    names = list(imgs)
    arrays = {f"img_{i}": imgs[n] for i, n in enumerate(names)}
    meta = dict(pillow=PIL.__version__, images=names, cases=[], cube=[])
    for k, (name, params, what) in enumerate(cases()):
        arrays[f"out_{k}"] = ref.pil_color_jitter(imgs[name], params)
        meta["cases"].append(dict(img=names.index(name), params=params, what=what))
    cube = ref.colour_cube()
    for params in CUBE:
        meta["cube"].append(dict(params=params, sha256=hashlib.sha256(ref.pil_color_jitter(cube, params).tobytes()).hexdigest()))
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(meta["cases"]), "cases")


if __name__ == "__main__":
    main()
