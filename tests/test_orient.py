"""`-vf hflip / vflip / transpose`, the parts that need no GPU: the profile's parsing and
composition of a leading run of orientation filters against the filters'
definitions applied one at a time, the rejected forms, the worker's decisions before it touches
the GPU, and mjg_open_orient's argument checks.

The profile parses vflip and transpose; a graph that names hflip stays outside it, as
tests/test_crop.py and tests/test_pad.py have it (`hflip`, `hflip,pad=64:48`).  Its map (orient 2)
is in the library and in profile.compose_orient all the same, so the composition table below
covers the runs with hflip through compose_orient and parses the others.  The library's version
stays 105 (tests/test_abi.py pins it): the new calls are looked up by name."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from orient_ref import apply_filters, orient_frame, oriented_size
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import i420_frame_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()


def _parse(vf):
    return profile.try_parse(["-vf", vf, *ARGS])


def _ramp(w, h, c):
    """Every byte of the frame different from its neighbours, no symmetry."""
    n = i420_frame_bytes(w, h, c)
    return ((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8)


GRAPHS = [
    ("hflip", 2), ("vflip", 4), ("hflip,vflip", 6), ("vflip,hflip", 6),
    ("transpose=0", 1), ("transpose=1", 3), ("transpose=2", 5), ("transpose=3", 7),
    ("transpose", 1), ("transpose=dir=1", 3), ("transpose=clock", 3), ("transpose=dir=cclock", 5),
    ("transpose=cclock_flip", 1), ("transpose=clock_flip:passthrough=none", 7), ("transpose=2:none", 5),
    ("transpose=1,transpose=1", 6), ("transpose=clock,hflip", 1), ("hflip,transpose=clock", 7),
    ("transpose=1,transpose=2", 0), ("transpose=1,transpose=1,transpose=1", 5),
    ("vflip,transpose=2,scale=64:128", 7), ("hflip,hflip", 0), ("hflip,vflip,hflip,vflip", 0),
    ("transpose=0,vflip,transpose=3,hflip", 6),
]


@pytest.mark.parametrize("vf,orient", GRAPHS)
def test_composition_matches_the_filters_applied_one_by_one(vf, orient):
    names = [f for f in vf.split(",") if f.split("=")[0] in ("hflip",) + profile.ORIENT_FILTERS]
    assert profile.compose_orient(names) == orient
    prof, why = _parse(vf)
    if "hflip" in names:
        assert prof is None and "hflip" in why
    else:
        assert prof is not None, why
        assert prof.orient == orient
    for c in ("444", "420"):
        f = _ramp(7, 5, c)
        want, ww, wh = apply_filters(f, 7, 5, c, names)
        assert (ww, wh) == oriented_size(7, 5, orient)
        got = orient_frame(f, 7, 5, c, orient)
        assert got.shape == want.shape and (got == want).all(), (c, np.flatnonzero(got != want)[:4])


def test_the_table_of_the_single_filters():
    """The encoding's own statement: hflip 2, vflip 4, transpose=N 1 | (N & 1) << 1 | (N >> 1) << 2."""
    f = _ramp(7, 5, "444")
    for names, o in ((["hflip"], 2), (["vflip"], 4), (["transpose=0"], 1), (["transpose=1"], 3),
                     (["transpose=2"], 5), (["transpose=3"], 7)):
        assert (apply_filters(f, 7, 5, "444", names)[0] == orient_frame(f, 7, 5, "444", o)).all(), names


def test_what_follows_the_run_is_parsed_as_before():
    prof, why = _parse("vflip,transpose=2,scale=64:128")
    assert prof is not None, why
    assert (prof.orient, prof.crop, prof.scale, prof.pad) == (7, None, (64, 128), None)
    prof, why = _parse("transpose=1,crop=62:126:2:2,scale=32:64,pad=48:80:8:8")
    assert prof is not None, why
    assert prof.orient == 3 and prof.crop == dict(w=62, h=126, x=2, y=2) and prof.scale == (32, 64)
    assert prof.pad == dict(w=48, h=80, x=8, y=8)
    prof, why = _parse("vflip,pad=64:48")
    assert prof is not None and prof.orient == 4 and prof.pad == dict(w=64, h=48, x=None, y=None), why
    prof, why = _parse("scale=64:32")
    assert prof is not None and prof.orient == 0, why
    assert profile.parse(ARGS).orient == 0


@pytest.mark.parametrize("vf,names", [
    ("crop=126:62,vflip", ["vflip after crop", "2 filters"]),
    ("scale=64:32,vflip", ["vflip after scale"]),
    ("vflip,scale=64:32,transpose=1", ["transpose after scale", "3 filters"]),
    ("pad=64:48,transpose=2", ["transpose after pad"]),
    ("hflip", ["hflip"]),
    ("vflip,hflip", ["hflip is not GPU-accelerated"]),
    ("transpose=clock,hflip,scale=64:128", ["hflip is not GPU-accelerated"]),
    ("hflip,vflip", ["hflip,vflip"]),
    ("transpose=4", ["dir=4", "0..3"]),
    ("transpose=7", ["dir=7"]),
    ("transpose=dir=5", ["dir=5"]),
    ("transpose=sideways", ["dir=sideways"]),
    ("transpose=1:passthrough=portrait", ["passthrough=portrait", "none"]),
    ("transpose=1:landscape", ["passthrough=landscape"]),
    ("transpose=1:none:3", ["'3'", "positional"]),
    ("transpose=rotate=1", ["'rotate'"]),
    ("vflip=1", ["vflip option"]),
    ("vflip=x=2", ["vflip option"]),
    ("vflip,crop=126:62,scale=64:32,pad=80:56,scale=32:16", ["pad is not the last filter"]),
    ("vflip,scale=64:32,crop=32:16", ["scale before crop"]),
    ("vflip,crop=10:10,crop=5:5,scale=4:4", ["3 filters"]),     # the limit applies to what follows the run
    ("vflip;transpose", ["vflip;transpose"]),
])
def test_unsupported_reasons_name_the_cause(vf, names):
    prof, why = _parse(vf)
    assert prof is None
    for n in names:
        assert n in why, why


# ---------------------------------------------------------------------- the worker, up to the GPU
class _Reached(Exception):
    pass


def _y4m(w, h, c="420", sar="1:1"):
    tag = {"420": "420jpeg", "422": "422", "444": "444"}[c]
    return (f"YUV4MPEG2 W{w} H{h} F25:1 Ip A{sar} C{tag}\n".encode() + b"FRAME\n"
            + np.full(i420_frame_bytes(w, h, c), 16, np.uint8).tobytes())


def _run(monkeypatch, w, h, c, vf, sar="1:1"):
    """worker.run up to the encoder's constructor, which records its arguments and stops the
    run; ffmpeg_fallthrough is recorded instead of run: no GPU, no ffmpeg."""
    calls, opened = [], []

    def fallthrough(src, args, stdout, stderr=None):
        calls.append(list(args))
        src.close(kill=True)
        return 0

    class Enc:
        def __init__(self, *a, **kw):
            opened.append((a, kw))
            raise _Reached()

    from ffmpeg_distributed_amd import encoder
    monkeypatch.setattr(worker, "ffmpeg_fallthrough", fallthrough)
    monkeypatch.setattr(worker, "bind_numa", lambda device: -1)
    monkeypatch.setattr(encoder, "MjpegEncoder", Enc)
    out, err = io.BytesIO(), io.StringIO()
    args = ["-vf", vf] + ARGS
    try:
        rc = worker.run(3, args, stdin=io.BytesIO(_y4m(w, h, c, sar)), stdout=out, stderr=err)
    except _Reached:
        rc = None
    return rc, calls, [l for l in err.getvalue().splitlines() if l.strip()], args, opened


def test_worker_sends_a_transpose_of_422_to_ffmpeg(monkeypatch):
    rc, calls, lines, args, opened = _run(monkeypatch, 130, 66, "422", "transpose=1")
    assert rc == 0 and calls == [args] and opened == []
    assert lines == ["gpu:3: transpose of a 4:2:2 input: FFmpeg converts the format first; running ffmpeg on the CPU"]


def test_worker_keeps_a_flip_of_422_on_the_gpu(monkeypatch):
    rc, calls, lines, _, opened = _run(monkeypatch, 130, 66, "422", "vflip")
    assert rc is None and calls == [] and lines == []
    (a, kw), = opened
    assert kw["orient"] == 4 and a[1:5] == (130, 66, 130, 66)


def test_worker_swaps_the_size_and_the_sar_under_a_transpose(monkeypatch):
    rc, calls, lines, _, opened = _run(monkeypatch, 130, 66, "420", "transpose=1,scale=64:128", sar="4:3")
    assert rc is None and calls == [] and lines == []
    (a, kw), = opened
    assert a[1:5] == (130, 66, 64, 128) and kw["orient"] == 3 and kw["crop"] is None
    # 1 / SAR = 3:4 of the 66 x 130 frame, then the scale's: 3/4 * (128 * 66) / (64 * 130)
    assert kw["sar"] == profile.scaled_sar((3, 4), (66, 130), (64, 128)) == (99, 130)
    # a flip keeps it, an unknown one stays unknown
    _, _, _, _, opened = _run(monkeypatch, 130, 66, "420", "vflip,scale=64:128", sar="4:3")
    assert opened[0][1]["sar"] == profile.scaled_sar((4, 3), (130, 66), (64, 128))
    _, _, _, _, opened = _run(monkeypatch, 130, 66, "420", "transpose=2", sar="0:0")
    assert opened[0][1]["sar"] == (0, 0) and opened[0][0][3:5] == (66, 130)
    assert worker.oriented_sar((4, 3), 5) == (3, 4) and worker.oriented_sar((4, 3), 6) == (4, 3)
    assert worker.oriented_sar((0, 0), 1) == (0, 0)


def test_worker_resolves_the_crop_against_the_oriented_frame(monkeypatch):
    """crop=60:120 fits 66 x 130 (the transposed frame), not 130 x 66; absent x / y centre in it."""
    rc, calls, lines, _, opened = _run(monkeypatch, 130, 66, "420", "transpose=1,crop=60:120")
    assert rc is None and calls == [] and lines == []
    (a, kw), = opened
    assert kw["crop"] == (2, 4, 60, 120) and a[3:5] == (60, 120)
    # without the transpose the same request fails as ffmpeg does
    rc, calls, lines, _, opened = _run(monkeypatch, 130, 66, "420", "vflip,crop=60:120")
    assert rc == 1 and calls == [] and opened == [] and lines[0].startswith("gpu:3: crop: ")


def test_encoder_key_differs_by_orientation():
    info = container.StreamInfo(130, 66, chroma="420")
    prof, why = _parse("vflip")
    assert prof is not None, why
    k = [worker.encoder_key(prof, info, 130, 66, (1, 1), False, 8, orient=o) for o in (0, 2, 4, 6)]
    assert len(set(k)) == 4
    assert k[0] == worker.encoder_key(prof, info, 130, 66, (1, 1), False, 8)


# ---------------------------------------------------------------------- the interface
def test_header_declares_and_library_exports_open_orient():
    with open(os.path.join(ROOT, "include", "mjgpu.h")) as f:
        hdr = f.read()
    ints = r"\s*,\s*".join(r"int\s+" + n for n in ("src_chroma_format", "orient", "crop_x", "crop_y", "crop_w", "crop_h",
                                                    "pad_x", "pad_y", "pad_w", "pad_h"))
    assert re.search(r"\bint\s+mjg_open_orient\s*\(\s*int\s+device\s*,\s*const\s+mjg_config\s*\*\s*cfg\s*,\s*"
                     + ints + r"\s*,\s*mjg_ctx\s*\*\*\s*out\s*\)\s*;", hdr)
    L = _lib.load()
    for name in ("mjg_open_orient", "mjg_debug_oriented", "mjg_debug_orient"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.mjg_debug_orient(None) == _lib.MJG_E_INVALID


def _open_orient(cf, orient, crop=None, dst=None, w=130, h=66):
    L = _lib.load()
    ow, oh = oriented_size(w, h, orient) if 0 <= orient <= 7 else (w, h)
    crop = crop or (0, 0, ow, oh)
    dst = dst or crop[2:]
    cfg = _lib.MjgConfig(w, h, dst[0], dst[1], 1, 5, 1, 1, 1, 0, _lib.CHROMA_FORMATS[cf])
    hnd = C.c_void_p()
    rc = L.mjg_open_orient(0, C.byref(cfg), _lib.CHROMA_FORMATS[cf], orient, *crop, 0, 0, *dst, C.byref(hnd))
    msg = L.mjg_last_error().decode()
    if hnd.value:
        L.mjg_close(hnd)
    return rc, msg


@pytest.mark.parametrize("c,orient,crop,words", [
    ("420", 8, None, ["orient 8", "0..7"]),
    ("420", -1, None, ["orient -1", "0..7"]),
    ("422", 1, None, ["orient 1", "4:2:2"]),
    ("422", 7, None, ["orient 7", "4:2:2"]),
    ("420", 3, (0, 0, 128, 64), ["crop 128x64", "outside the 66x130 frame"]),   # fits 130 x 66 only
    ("444", 5, (0, 70, 66, 66), ["crop 66x66", "outside the 66x130 frame"]),
    ("420", 2, (0, 0, 64, 128), ["crop 64x128", "outside the 130x66 frame"]),   # fits the transposed one only
])
def test_open_orient_rejects_bad_arguments_before_any_hip_call(c, orient, crop, words):
    """MJG_E_INVALID with a message that names the cause, with or without a GPU: on a machine
    without one, any HIP call would give MJG_E_HIP instead."""
    rc, msg = _open_orient(c, orient, crop)
    assert rc == _lib.MJG_E_INVALID, (rc, msg)
    for w_ in words:
        assert w_ in msg, msg
