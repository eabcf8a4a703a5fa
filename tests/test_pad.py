"""`-vf ...,pad`, the parts that need no GPU: the profile's parsing of a graph that ends in pad,
the resolution of a pad request against its input, the numpy reference, why
only black is taken, the worker's decisions before it touches the GPU, and the interface."""
import io
import os
import re

import numpy as np
import pytest

import oracle
from chroma_resample_ref import composed_frame, source_frames
from pad_ref import pad_planes, padded_ref
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import i420_frame_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()


def _parse(vf):
    return profile.try_parse(["-vf", vf, *ARGS])


@pytest.mark.parametrize("vf,crop,scale,pad", [
    ("pad=64:48:0:8", None, None, dict(w=64, h=48, x=0, y=8)),
    ("pad=64:48:0:8:black", None, None, dict(w=64, h=48, x=0, y=8)),
    ("pad=width=64:height=48:x=2:y=4:color=black", None, None, dict(w=64, h=48, x=2, y=4)),
    ("pad=w=64:h=48:c=black", None, None, dict(w=64, h=48, x=None, y=None)),
    ("pad=0:48", None, None, dict(w=0, h=48, x=None, y=None)),
    ("pad=64:48:-1:-1", None, None, dict(w=64, h=48, x=-1, y=-1)),
    ("pad=64:48:(ow-iw)/2:(oh-ih)/2", None, None, dict(w=64, h=48, x="(ow-iw)/2", y="(oh-ih)/2")),
    ("pad=64:48:x=(ow-iw)/2:y=(oh-ih)/2", None, None, dict(w=64, h=48, x="(ow-iw)/2", y="(oh-ih)/2")),
    ("scale=64:32,pad=64:48:0:8", None, (64, 32), dict(w=64, h=48, x=0, y=8)),
    ("scale=1920:800:flags=bicubic,pad=1920:1080:0:140", None, (1920, 800), dict(w=1920, h=1080, x=0, y=140)),
    ("crop=34:18:6:10,pad=64:48:2:2", dict(w=34, h=18, x=6, y=10), None, dict(w=64, h=48, x=2, y=2)),
    ("crop=126:62:2:2,scale=64:32,pad=80:56:6:10", dict(w=126, h=62, x=2, y=2), (64, 32),
     dict(w=80, h=56, x=6, y=10)),
])
def test_parse_accepts_pad_forms(vf, crop, scale, pad):
    prof, why = _parse(vf)
    assert prof is not None, why
    assert (prof.crop, prof.scale, prof.pad) == (crop, scale, pad)


def test_a_graph_without_pad_has_none():
    prof, why = _parse("crop=126:62:2:2,scale=64:32")
    assert prof is not None and prof.pad is None, why


@pytest.mark.parametrize("vf,names", [
    ("pad=iw+10:ih", ["iw+10", "expression"]),
    ("pad=64:48:x=(iw-ow)/2", ["(iw-ow)/2", "expression"]),
    ("pad=64:48:(oh-ih)/2:0", ["(oh-ih)/2", "expression"]),      # y's form given for x
    ("pad=64:48:color=red", ["color=red", "black"]),
    ("pad=64:48:0:8:0x102030", ["0x102030", "black"]),
    ("pad=64:48,scale=32:24", ["pad=64:48,scale=32:24", "pad is not the last filter"]),
    ("pad=64:48,crop=32:24,scale=16:16", ["pad is not the last filter"]),
    ("pad=64:48:aspect=16/9", ["aspect=16/9"]),
    ("pad=64:48:eval=frame", ["eval=frame"]),
    ("pad=64:48:0:8:black:init", ["'init'", "positional"]),
    ("pad=64:48:z=3", ["'z'"]),
    ("crop=126:62,scale=64:32,hflip", ["hflip", "3 filters"]),    # unchanged wording
    ("scale=64:32,crop=32:16", ["scale before crop"]),
    ("hflip,pad=64:48", ["hflip"]),
    ("crop=126:62,scale=64:32,hflip,pad=64:48", ["hflip", "4 filters"]),
])
def test_unsupported_reasons_name_the_cause(vf, names):
    prof, why = _parse(vf)
    assert prof is None
    for n in names:
        assert n in why, why


@pytest.mark.parametrize("req,in_w,in_h,c,want", [
    ("64:48:0:8", 64, 32, "420", (0, 8, 64, 48)),
    ("64:48:6:10", 34, 18, "420", (6, 10, 64, 48)),
    ("64:48:-1:-1", 34, 18, "420", (14, 14, 64, 48)),                 # (64 - 34) / 2 = 15 -> 14, 15 -> 14
    ("64:48:-1:-1", 34, 18, "422", (14, 15, 64, 48)),
    ("64:48:-1:-1", 34, 18, "444", (15, 15, 64, 48)),
    ("64:48:(ow-iw)/2:(oh-ih)/2", 34, 18, "444", (15, 15, 64, 48)),
    ("64:48:x=(ow-iw)/2", 34, 18, "420", (14, 0, 64, 48)),            # absent y = 0
    ("64:48:40:40", 34, 18, "444", (15, 15, 64, 48)),                 # x + in_w > W: centred
    ("64:48:30:30", 34, 18, "444", (30, 30, 64, 48)),                 # flush bottom-right stays
    ("64:48:31:3", 34, 18, "444", (15, 3, 64, 48)),                   # x alone centred
    ("65:49:3:5", 34, 18, "420", (2, 4, 64, 48)),                     # rounding down, 4:2:0
    ("65:49:3:5", 34, 18, "422", (2, 5, 64, 49)),
    ("65:49:3:5", 34, 18, "444", (3, 5, 65, 49)),
    ("0:48", 64, 32, "420", (0, 0, 64, 48)),                          # W = 0: the input's
    ("h=48", 64, 32, "420", (0, 0, 64, 48)),                          # W absent
    ("0:0", 64, 32, "420", (0, 0, 64, 32)),
    ("1920:1080:0:140", 1920, 800, "420", (0, 140, 1920, 1080)),
])
def test_resolve_pad_table(req, in_w, in_h, c, want):
    prof, why = _parse("pad=" + req)
    assert prof is not None, why
    assert profile.resolve_pad(prof.pad, in_w, in_h, c) == want


@pytest.mark.parametrize("req,in_w,in_h,c", [
    ("32:48", 34, 18, "420"),     # canvas narrower than the input (x centres to -1 -> -2)
    ("64:16", 34, 18, "444"),     # canvas shorter than the input
    ("35:48", 35, 18, "420"),     # W rounds down to 34 < in_w (resolve_pad alone: the worker sends odd pictures to ffmpeg)
    ("34:19", 34, 19, "420"),     # H rounds down to 18 < in_h
])
def test_resolve_pad_rejects_a_canvas_the_input_does_not_fit(req, in_w, in_h, c):
    prof, why = _parse("pad=" + req)
    assert prof is not None, why
    with pytest.raises(ValueError) as e:
        profile.resolve_pad(prof.pad, in_w, in_h, c)
    assert isinstance(e.value, profile.PadError) and not isinstance(e.value, profile.Unsupported)


@pytest.mark.parametrize("c", ["420", "422", "444"])
@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
def test_padded_ref_with_the_trivial_pad_is_the_composed_frame(c, full):
    w, h = 34, 18
    for f in source_frames(w, h, 2, 11, c):
        assert padded_ref(f, w, h, c, None, c, full, None, None, (0, 0, w, h)) == \
            composed_frame(f, w, h, c, c, full)


def test_pad_planes_places_every_plane():
    yy, uu, vv = (np.full(s, v, np.uint8) for s, v in (((18, 34), 7), ((9, 17), 8), ((9, 17), 9)))
    Y, U, V = pad_planes(yy, uu, vv, "420", 6, 10, 64, 48)
    assert Y.shape == (48, 64) and U.shape == V.shape == (24, 32)
    assert (Y[10:28, 6:40] == 7).all() and Y.sum() == 7 * 18 * 34
    for P, v in ((U, 8), (V, 9)):
        assert (P[5:14, 3:20] == v).all() and (P == 128).sum() == 24 * 32 - 9 * 17


def test_black_is_the_same_before_and_after_the_tv_to_pc_converter():
    """Without a scale FFmpeg pads in the source range (tv black: Y 16, Cb = Cr 128) and its
    converter follows; its one-tap identity filters map 16 -> 0 and 128 -> 128, so converting the
    picture and then padding with 0 / 128 gives the same bytes.  No other colour has this."""
    y = oracle.scale_plane(np.full((8, 16), 16, np.uint8), 16, 8, range_mode=1, chroma=False)
    c = oracle.scale_plane(np.full((8, 16), 128, np.uint8), 16, 8, range_mode=2, chroma=True)
    assert (y == 0).all() and (c == 128).all()
    # and a full-range source is not converted at all
    assert (oracle.scale_plane(np.full((8, 16), 0, np.uint8), 16, 8, range_mode=0, chroma=False) == 0).all()
    assert (oracle.scale_plane(np.full((8, 16), 128, np.uint8), 16, 8, range_mode=0, chroma=True) == 128).all()


# ---------------------------------------------------------------------- the worker, up to the GPU
class _Reached(Exception):
    pass


def _y4m(w, h, c="420", n=1):
    tag = {"420": "420jpeg", "422": "422", "444": "444"}[c]
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C{tag}\n".encode())
    for i in range(n):
        b.write(b"FRAME\n" + np.full(i420_frame_bytes(w, h, c), 16 + i, np.uint8).tobytes())
    return b.getvalue()


def _run(monkeypatch, w, h, c, extra):
    """worker.run up to the first step after the pre-checks (bind_numa, which precedes every GPU
    call), with ffmpeg_fallthrough recorded instead of run: no GPU, no ffmpeg."""
    calls = []

    def fallthrough(src, args, stdout, stderr=None):
        calls.append(list(args))
        src.close(kill=True)
        return 0

    def reached(device):
        raise _Reached()

    monkeypatch.setattr(worker, "ffmpeg_fallthrough", fallthrough)
    monkeypatch.setattr(worker, "bind_numa", reached)
    out, err = io.BytesIO(), io.StringIO()
    args = list(extra) + ARGS
    try:
        rc = worker.run(3, args, stdin=io.BytesIO(_y4m(w, h, c)), stdout=out, stderr=err)
    except _Reached:
        rc = None
    return rc, calls, [l for l in err.getvalue().splitlines() if l.strip()], args, out.getvalue()


def test_worker_sends_an_odd_picture_with_pad_to_ffmpeg(monkeypatch):
    rc, calls, lines, args, _ = _run(monkeypatch, 33, 18, "420", ["-vf", "pad=64:48:2:2"])
    assert rc == 0 and calls == [args]
    assert len(lines) == 1 and lines[0].startswith("gpu:3: pad of a 33x18 picture in 420")
    assert "sub-sampling" in lines[0] and lines[0].endswith("; running ffmpeg on the CPU")


def test_worker_sends_pad_under_a_pix_fmt_conversion_without_scale_to_ffmpeg(monkeypatch):
    rc, calls, lines, args, _ = _run(monkeypatch, 64, 32, "444",
                                     ["-vf", "pad=64:48:0:8", "-pix_fmt", "yuvj420p"])
    assert rc == 0 and calls == [args]
    assert len(lines) == 1 and "444 -> 420" in lines[0] and "pad" in lines[0] and "no scale" in lines[0]
    assert lines[0].startswith("gpu:3: ") and lines[0].endswith("; running ffmpeg on the CPU")


def test_worker_keeps_scale_pad_under_a_pix_fmt_conversion_on_the_gpu(monkeypatch):
    rc, calls, lines, _, _ = _run(monkeypatch, 130, 66, "444",
                                  ["-vf", "scale=64:32,pad=64:48:0:8", "-pix_fmt", "yuvj420p"])
    assert rc is None and calls == [] and lines == []  # went on towards the GPU


def test_worker_keeps_a_plain_pad_on_the_gpu(monkeypatch):
    rc, calls, lines, _, _ = _run(monkeypatch, 34, 18, "420", ["-vf", "pad=64:48:(ow-iw)/2:(oh-ih)/2"])
    assert rc is None and calls == [] and lines == []


def test_worker_fails_like_ffmpeg_when_the_canvas_is_too_small(monkeypatch):
    rc, calls, lines, _, out = _run(monkeypatch, 64, 32, "420", ["-vf", "pad=32:48"])
    assert rc == 1 and calls == [] and out == b""
    assert len(lines) == 1 and lines[0].startswith("gpu:3: pad: ") and "ffmpeg" not in lines[0]


def test_encoder_key_differs_for_two_pads():
    info = container.StreamInfo(130, 66, chroma="420")
    prof, why = _parse("scale=64:32,pad=64:48:0:8")
    assert prof is not None, why
    k = [worker.encoder_key(prof, info, 64, 32, (1, 1), False, 8, pad=p)
         for p in ((0, 8, 64, 48), (0, 16, 64, 48), None)]
    assert len(set(k)) == 3
    assert k[0] == worker.encoder_key(prof, info, 64, 32, (1, 1), False, 8, pad=[0, 8, 64, 48])


# ---------------------------------------------------------------------- the interface
def test_header_declares_and_library_exports_open_pad():
    with open(os.path.join(ROOT, "include", "mjgpu.h")) as f:
        hdr = f.read()
    ints = r"\s*,\s*".join(r"int\s+" + n for n in ("crop_x", "crop_y", "crop_w", "crop_h",
                                                    "pad_x", "pad_y", "pad_w", "pad_h"))
    assert re.search(r"\bint\s+mjg_open_pad\s*\(\s*int\s+device\s*,\s*const\s+mjg_config\s*\*\s*cfg\s*,\s*"
                     r"int\s+src_chroma_format\s*,\s*" + ints + r"\s*,\s*mjg_ctx\s*\*\*\s*out\s*\)\s*;", hdr)
    L = _lib.load()
    assert "mjg_open_pad" in _lib.EXPORTS and hasattr(L, "mjg_open_pad")
    assert L.mjg_version() >= 104


def _open_pad(cf, dst, pad, w=130, h=66):
    import ctypes as C
    L = _lib.load()
    cfg = _lib.MjgConfig(w, h, dst[0], dst[1], 1, 5, 1, 1, 1, 0, _lib.CHROMA_FORMATS[cf])
    hnd = C.c_void_p()
    rc = L.mjg_open_pad(0, C.byref(cfg), _lib.CHROMA_FORMATS[cf], 0, 0, w, h, *pad, C.byref(hnd))
    msg = L.mjg_last_error().decode()
    if hnd.value:
        L.mjg_close(hnd)
    return rc, msg


@pytest.mark.parametrize("c,dst,pad,word", [
    ("420", (64, 32), (2, 8, 64, 48), "outside"),        # 2 + 64 > 64
    ("420", (64, 32), (0, 18, 64, 48), "outside"),       # 18 + 32 > 48
    ("444", (64, 32), (-1, 0, 80, 48), "outside"),
    ("420", (64, 32), (0, 0, 0, 48), "not positive"),
    ("420", (64, 32), (0, 0, 64, -2), "not positive"),
    ("420", (64, 32), (3, 8, 80, 48), "sub-sampling"),   # odd pad_x, 4:2:0
    ("420", (64, 32), (2, 7, 80, 48), "sub-sampling"),   # odd pad_y
    ("422", (64, 32), (2, 7, 81, 48), "sub-sampling"),   # odd pad_w, 4:2:2 (the odd pad_y is fine there)
    ("420", (63, 32), (2, 8, 80, 48), "sub-sampling"),   # odd picture width under a pad
])
def test_open_pad_rejects_a_bad_pad_before_any_hip_call(c, dst, pad, word):
    """MJG_E_INVALID with a message that names the pad, with or without a GPU: on a machine
    without one, any HIP call would give MJG_E_HIP instead."""
    rc, msg = _open_pad(c, dst, pad)
    assert rc == _lib.MJG_E_INVALID, (rc, msg)
    assert word in msg and f"pad {pad[2]}x{pad[3]} with the picture at ({pad[0]},{pad[1]})" in msg, msg
