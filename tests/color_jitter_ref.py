"""numpy restatement of the ColorJitter rule of include/ffb6d_train.h (ffb6d_color_jitter_u8): torchvision's PIL backend,
that is Pillow's ImageEnhance.Brightness / Contrast / Color and an HSV round trip with a uint8 hue shift, byte for byte.
Images are uint8 [3,H,W] (or [B,3,H,W] for the batch helper), plane 0 = R.  tests/test_color_jitter_cpu.py holds this file to
Pillow itself (the committed goldens, and the live library where it imports)."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
KEYS = ("brightness", "contrast", "saturation", "hue")


def luminance(img):
    """L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16 (Pillow's RGB -> L)"""
    r, g, b = (img[c].astype(np.int64) for c in range(3))
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16


def blend(d, x, factor):
    """(float)d + alpha ((float)x - (float)d) in float32, product and sum rounded separately; clip, then truncate"""
    a = np.float32(factor)
    d = np.asarray(d).astype(np.float32)
    x = np.asarray(x).astype(np.float32)
    t = d + a * (x - d)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.minimum(t, np.float32(255)))).astype(np.uint8)


def contrast_mean(img):
    lum = luminance(img)
    return int(float(lum.sum()) / float(lum.size) + 0.5)


def hue_shift(hue):
    """(int)(hue 255.0) truncated toward zero, modulo 256: what np.uint8(hue_factor * 255) wraps to in torchvision"""
    return int(float(hue) * 255.0) % 256                               # int() truncates toward zero; -12 % 256 = 244


def rgb_to_hsv(img):
    r, g, b = (img[c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(np.float32)
        s = cr / mx.astype(np.float32)
        rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (r, g, b))
        rc, gc, bc = (np.where(grey, 0, q).astype(np.float64) for q in (rc, gc, bc))
        h = np.where(r == mx, bc - gc, np.where(g == mx, 2.0 + rc - bc, 4.0 + gc - rc)).astype(np.float32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
        H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip((np.where(grey, 0, s).astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H, S = np.where(grey, 0, H), np.where(grey, 0, S)
    return H.astype(np.uint8), S.astype(np.uint8), mx.astype(np.uint8)


def _c_round(x):
    """C round() of non-negative float32 values (half away from zero)"""
    fl = np.floor(x)
    return (fl + (x - fl >= np.float32(0.5))).astype(np.int64)


def hsv_to_rgb(H, S, V):
    f32 = np.float32
    hh = H.astype(f32) * f32(6) / f32(255)
    fl = np.floor(hh)
    i = fl.astype(np.int64) % 6
    f = hh - fl
    fs = S.astype(f32) / f32(255)
    v = V.astype(f32)
    one = f32(1)
    p = np.clip(_c_round(v * (one - fs)), 0, 255)
    q = np.clip(_c_round(v * (one - fs * f)), 0, 255)
    t = np.clip(_c_round(v * (one - fs * (one - f))), 0, 255)
    vv = V.astype(np.int64)
    table = [(vv, t, p), (q, vv, p), (p, vv, t), (p, q, vv), (t, p, vv), (vv, p, q)]
    out = np.empty((3,) + H.shape, np.uint8)
    for c in range(3):
        out[c] = np.where(S == 0, vv, np.choose(i, [row[c] for row in table]))
    return out


def op_brightness(img, f):
    return blend(0, img, f)


def op_contrast(img, f):
    return blend(contrast_mean(img), img, f)


def op_saturation(img, f):
    return blend(luminance(img)[None], img, f)


def op_hue_shift(img, shift):
    H, S, V = rgb_to_hsv(img)
    return hsv_to_rgb(((H.astype(np.int64) + shift) & 255).astype(np.uint8), S, V)


def chain(params):
    """The (op, value) list of one frame's params dict, in its order; ops whose key is missing are skipped."""
    if params is None:
        return []
    out = []
    for op in params.get("order", (0, 1, 2, 3)):
        if params.get(KEYS[op]) is not None:
            out.append((op, params[KEYS[op]]))
    return out


def color_jitter(img, params):
    """One frame uint8 [3,H,W] through its chain."""
    x = np.ascontiguousarray(img)
    for op, val in chain(params):
        if op == BRIGHTNESS:
            x = op_brightness(x, val)
        elif op == CONTRAST:
            x = op_contrast(x, val)
        elif op == SATURATION:
            x = op_saturation(x, val)
        else:
            x = op_hue_shift(x, hue_shift(val))
    return x.copy() if x is img else x


def color_jitter_batch(rgb, params):
    return np.stack([color_jitter(rgb[b], params[b]) for b in range(len(rgb))])


def colour_cube():
    """All 2^24 colours as one uint8 [3,4096,4096] image: pixel n = y 4096 + x holds R = n >> 16, G = (n >> 8) & 255, B = n & 255"""
    n = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([(n >> 16).astype(np.uint8), ((n >> 8) & 255).astype(np.uint8), (n & 255).astype(np.uint8)])


def pil_color_jitter(img, params):
    """The same frame through Pillow itself, with the operation sequence of torchvision's PIL backend (needs PIL):
    ImageEnhance.Brightness / Contrast / Color(...).enhance(f); for hue convert("HSV"), a wrapping uint8 add on the H band,
    merge, convert("RGB").  Not part of the restatement: the yardstick it is held to."""
    from PIL import Image, ImageEnhance
    im = Image.fromarray(np.ascontiguousarray(np.transpose(img, (1, 2, 0))), "RGB")
    for op, val in chain(params):
        if op == BRIGHTNESS:
            im = ImageEnhance.Brightness(im).enhance(val)
        elif op == CONTRAST:
            im = ImageEnhance.Contrast(im).enhance(val)
        elif op == SATURATION:
            im = ImageEnhance.Color(im).enhance(val)
        else:
            h, s, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            np_h = (np_h.astype(np.int64) + int(val * 255)).astype(np.uint8)      # uint8 wrap-around, as np_h += np.uint8(hue * 255)
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return np.ascontiguousarray(np.transpose(np.asarray(im), (2, 0, 1)))
