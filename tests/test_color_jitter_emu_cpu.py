"""csrc/color_jitter.hip on the SIMT emulator (tests/simt), without a GPU: the unmodified kernel source compiled for the host and run
through the C ABI of include/ffb6d_train.h.  Every golden case (tests/golden/color_jitter.npz: PILLOW's outputs) comes out as
Pillow's bytes, through each of the three access widths the launcher chooses from (16-byte, 4-byte, single bytes: the same image at
offsets 0, 4 and 1 of an aligned buffer where its size allows the wider forms); a batch that mixes a copied frame, a frame without
contrast and frames with the contrast in different positions equals the restatement; argument errors return their code and leave a
pre-filled output untouched; a short workspace is refused; bad records are refused by the host check and copied by the kernels."""
import json
import os

import numpy as np
import pytest

import color_jitter_ref as ref
from tests.simt.build import load

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_jitter.npz")
FILL = 0xA5


@pytest.fixture(scope="module")
def emu_jitter():
    """the emulated library (tests/simt/build.py)"""
    return load()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    imgs = [z[f"img_{i}"] for i in range(len(meta["images"]))]
    return [(imgs[c["img"]], c["params"], z[f"out_{k}"], c["what"]) for k, c in enumerate(meta["cases"])]


GUARD = 0x3C


def placed(a, offset):
    """a copy of `a` that starts `offset` bytes behind a 64-byte boundary, in the middle of a buffer of GUARD bytes"""
    raw = np.full(a.size + 256, GUARD, np.uint8)
    at = 64 + (-raw.ctypes.data) % 64 + offset
    view = raw[at:at + a.size].reshape(a.shape)
    view[...] = a
    return view


def guards_intact(view):
    raw = view.base if view.base.ndim == 1 else view.base.base
    at = view.ctypes.data - raw.ctypes.data
    return (raw[:at] == GUARD).all() and (raw[at + view.size:] == GUARD).all()


def run(lib, rgb, params, offset=0, ws_fill=0xFF, **kw):
    """ffb6d_color_jitter_u8 with numpy arrays as "device" memory; kw overrides arguments by name -> (rc, out)"""
    from ffb6d_amd import train_data
    B, _, H, W = rgb.shape
    rec = params if isinstance(params, np.ndarray) else train_data.jitter_records(params)
    src = placed(rgb, offset)
    out = placed(np.full(rgb.shape, FILL, np.uint8), offset)
    need = lib.ffb6d_color_jitter_workspace_bytes(B, H, W)
    ws = np.full(max(need, 8), ws_fill, np.uint8)                       # the workspace may hold anything on entry
    a = dict(inp=src.ctypes.data, frames=rec.ctypes.data, out=out.ctypes.data, B=B, H=H, W=W, workspace=ws.ctypes.data,
             workspace_bytes=need)
    a.update(kw)
    rc = lib.ffb6d_color_jitter_u8(*a.values(), None)
    assert guards_intact(out) and np.array_equal(src, rgb), "a store outside the output"
    return rc, out


def test_golden_cases_come_out_as_pillows_bytes_at_every_access_width(emu_jitter, golden):
    widths = set()
    for img, params, want, what in golden:
        hw = img.shape[1] * img.shape[2]
        for offset in (0, 4, 1):
            rc, out = run(emu_jitter, img[None], [params], offset)
            assert rc == 0, emu_jitter.ffb6d_last_error()
            assert np.array_equal(out[0], want), (what, params, img.shape, offset, int(np.count_nonzero(out[0] != want)))
            widths.add(16 if hw % 16 == 0 and offset == 0 else 4 if hw % 4 == 0 and offset % 4 == 0 else 1)
    assert widths == {16, 4, 1}


def test_a_mixed_batch_equals_the_restatement(emu_jitter):
    """37 x 53: odd planes, single bytes; 48 x 100 = 4800 pixels: 16-byte form, two workgroups per frame and a last tile that is
    not full; 41 x 100 = 4100: 4-byte form, two workgroups and a last run of 4 pixels that goes byte by byte"""
    rng = np.random.RandomState(3)
    params = [None,
              dict(order=(3, 0, 2, 1), brightness=1.15, saturation=0.85, hue=-0.05),                    # no contrast
              dict(order=(1, 0, 2, 3), brightness=0.9, contrast=1.2, saturation=1.1, hue=0.03),          # contrast first
              dict(order=(0, 3, 1, 2), brightness=1.2, contrast=0.8, saturation=0.9, hue=0.05),          # ... third
              dict(order=(2, 3, 0, 1), brightness=0.8, contrast=1.1, saturation=1.2, hue=-0.02)]         # ... last
    for H, W in ((37, 53), (48, 100), (41, 100)):
        rgb = rng.randint(0, 256, (5, 3, H, W)).astype(np.uint8)
        rc, out = run(emu_jitter, rgb, params)
        assert rc == 0, emu_jitter.ffb6d_last_error()
        want = ref.color_jitter_batch(rgb, params)
        assert np.array_equal(out[0], rgb[0])
        for b in range(5):
            assert np.array_equal(out[b], want[b]), (H, W, b, int(np.count_nonzero(out[b] != want[b])))


def test_argument_errors_return_their_code_and_leave_the_output_untouched(emu_jitter):
    rng = np.random.RandomState(4)
    rgb = rng.randint(0, 256, (2, 3, 5, 7)).astype(np.uint8)
    params = [dict(order=(0, 1, 2, 3), brightness=1.1, contrast=1.1, saturation=1.1, hue=0.05)] * 2
    assert emu_jitter.ffb6d_color_jitter_workspace_bytes(2, 5, 7) == 256 and emu_jitter.ffb6d_color_jitter_workspace_bytes(0, 5, 7) == 0
    assert emu_jitter.ffb6d_color_jitter_workspace_bytes(1, 4096, 4096) == 8 * 1024          # at most 1024 partial sums per frame
    small = np.zeros(64, np.uint8)
    cases = [(dict(inp=None), -1, "null pointer"), (dict(frames=None), -1, "null pointer"), (dict(out=None), -1, "null pointer"),
             (dict(B=-1), -1, "B = -1"), (dict(H=-5), -1, "H = -5"), (dict(B=65536), -1, "grid"),
             (dict(workspace=None), -3, "workspace"), (dict(workspace_bytes=255), -3, "workspace"),
             (dict(workspace=small.ctypes.data, workspace_bytes=64), -3, "workspace")]
    for kw, code, text in cases:
        rc, out = run(emu_jitter, rgb, params, **kw)
        assert rc == code, kw
        assert text in emu_jitter.ffb6d_last_error().decode(), (kw, emu_jitter.ffb6d_last_error())
        assert (out == FILL).all(), kw
    assert not small.any()
    src = placed(rgb, 0)
    before = src.copy()
    rc, _ = run(emu_jitter, rgb, params, inp=src.ctypes.data, out=src.ctypes.data)           # in == out
    assert rc == -1 and "in == out" in emu_jitter.ffb6d_last_error().decode() and np.array_equal(src, before)
    rc, out = run(emu_jitter, rgb[:0], [])                                                   # an empty batch is no error
    assert rc == 0


def test_bad_records_are_refused_on_the_host_and_copied_by_the_kernels(emu_jitter):
    from ffb6d_amd import train_data
    good = train_data.jitter_records([dict(order=(1, 3), contrast=1.2, hue=0.05), None])
    assert emu_jitter.ffb6d_jitter_frames_check(good.ctypes.data, 2) == 0
    assert emu_jitter.ffb6d_jitter_frames_check(None, 0) == 0 and emu_jitter.ffb6d_jitter_frames_check(None, 1) == -1

    def broken(**kw):
        rec = good.copy()
        for k, v in kw.items():
            rec[0][k] = v
        return rec

    bad = [broken(n_ops=5), broken(n_ops=-1), broken(op=[1, 1, 0, 0]), broken(op=[1, 4, 0, 0]), broken(op=[-1, 3, 0, 0]),
           broken(alpha=[-0.5, 0, 0, 0]), broken(alpha=[np.nan, 0, 0, 0]), broken(alpha=[np.inf, 0, 0, 0]), broken(hue_shift=256),
           broken(hue_shift=-1)]
    rgb = np.random.RandomState(5).randint(0, 256, (2, 3, 4, 4)).astype(np.uint8)
    for rec in bad:
        assert emu_jitter.ffb6d_jitter_frames_check(rec.ctypes.data, 2) == -1, rec[0]
        assert "frame 0" in emu_jitter.ffb6d_last_error().decode()
        rc, out = run(emu_jitter, rgb, rec)
        assert rc == 0 and np.array_equal(out, rgb), rec[0]                           # both frames copied, nothing else touched
    rec = broken(alpha=[0, np.nan, 0, 0])                                             # the hue's factor is not used
    assert emu_jitter.ffb6d_jitter_frames_check(rec.ctypes.data, 2) == 0
