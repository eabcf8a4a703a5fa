"""`-vf crop[,scale]`, the parts that need no GPU: the profile's filter-graph parsing, the
resolution of a crop request against an input, the numpy reference cut, the
library's rectangle validation (before any HIP call) and the worker's encoder cache key."""
import ctypes as C

import numpy as np
import pytest

from chroma_resample_ref import source_frames
from crop_ref import crop_frame, same_inside
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import i420_frame_bytes, split_i420

ARGS = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()


def _parse(vf):
    return profile.try_parse(["-vf", vf, *ARGS])


@pytest.mark.parametrize("vf,crop,scale", [
    ("crop=126:62:2:2", dict(w=126, h=62, x=2, y=2), None),
    ("crop=w=126:h=62:x=2:y=2", dict(w=126, h=62, x=2, y=2), None),
    ("crop=out_w=126:out_h=62:y=4", dict(w=126, h=62, x=None, y=4), None),
    ("crop=51:31", dict(w=51, h=31, x=None, y=None), None),
    ("crop=126:62:2:2:keep_aspect=0:exact=0", dict(w=126, h=62, x=2, y=2), None),
    ("crop=3840:1600:0:280,scale=1920:800", dict(w=3840, h=1600, x=0, y=280), (1920, 800)),
    ("crop=126:62:2:2,scale=64:32:flags=bicubic", dict(w=126, h=62, x=2, y=2), (64, 32)),
    ("scale=64:32", None, (64, 32)),
])
def test_parse_accepts_crop_forms(vf, crop, scale):
    prof, why = _parse(vf)
    assert prof is not None, why
    assert prof.crop == crop and prof.scale == scale


@pytest.mark.parametrize("vf,names", [
    ("crop=iw/2:ih/2", ["iw/2", "expression"]),
    ("crop=126:in_h-280", ["in_h-280", "expression"]),
    ("crop=126:62:x=(iw-ow)/2", ["(iw-ow)/2", "expression"]),
    ("crop=126:62:2:2:exact=1", ["exact=1"]),
    ("crop=126:62:keep_aspect=1", ["keep_aspect=1"]),
    ("scale=64:32,crop=32:16", ["scale=64:32,crop=32:16", "scale before crop"]),
    ("crop=126:62,scale=64:32,hflip", ["hflip", "3 filters"]),
    ("crop=126:62,hflip", ["crop=126:62,hflip"]),
    ("hflip", ["hflip"]),
    ("crop=1:2:3:4:5", ["'5'"]),
])
def test_unsupported_reasons_name_the_cause(vf, names):
    prof, why = _parse(vf)
    assert prof is None
    for n in names:
        assert n in why, why


@pytest.mark.parametrize("in_w,in_h,c,req,want", [
    (101, 57, "420", "51:31:13:7", (12, 6, 50, 30)),
    (101, 57, "422", "51:31:13:7", (12, 7, 50, 31)),
    (101, 57, "444", "51:31:13:7", (13, 7, 51, 31)),
    (100, 60, "420", "51:31", (24, 14, 50, 30)),
    (100, 60, "444", "51:31", (24, 14, 51, 31)),            # (100 - 51) // 2, (60 - 31) // 2
    (130, 66, "420", "64:32:1000:1000", (66, 34, 64, 32)),  # x, y beyond the frame: clamped
    (131, 67, "420", "64:32:1000:1000", (66, 34, 64, 32)),  # clamped to 67, 35, then rounded down
    (130, 66, "420", "x=4", (0, 0, 130, 66)),               # the whole frame leaves no room: x clamps to 0
    (130, 66, "422", "130:66", (0, 0, 130, 66)),
    (131, 67, "420", "w=131", (0, 0, 130, 66)),             # absent h = in_h, both rounded down
])
def test_resolve_crop_table(in_w, in_h, c, req, want):
    prof, why = _parse("crop=" + req)
    assert prof is not None, why
    assert profile.resolve_crop(prof.crop, in_w, in_h, c) == want


@pytest.mark.parametrize("req", ["132:66", "130:68:0:0", "0:10", "1:10"])
def test_resolve_crop_rejects_a_size_outside_the_input(req):
    """w > in_w, h > in_h, w = 0, and w = 1 on a 4:2:0 input (rounds down to 0): a ValueError
    subclass, not Unsupported (the worker fails as ffmpeg does, it does not pass through)."""
    prof, why = _parse("crop=" + req)
    assert prof is not None, why
    with pytest.raises(ValueError) as e:
        profile.resolve_crop(prof.crop, 130, 66, "420")
    assert isinstance(e.value, profile.CropError) and not isinstance(e.value, profile.Unsupported)


@pytest.mark.parametrize("c", ["420", "422", "444"])
def test_crop_frame_of_the_full_rectangle_is_the_frame(c):
    w, h = 33, 17
    for f in source_frames(w, h, 2, 3, c):
        np.testing.assert_array_equal(crop_frame(f, w, h, c, (0, 0, w, h)), f)


def test_crop_frame_cuts_every_plane():
    w, h, c, rect = 130, 66, "420", (6, 10, 33, 17)
    f = source_frames(w, h, 2, 5, c)[0]
    y, u, v = split_i420(f, w, h, c)
    got = crop_frame(f, w, h, c, rect)
    assert got.size == i420_frame_bytes(33, 17, c)
    gy, gu, gv = split_i420(got, 33, 17, c)
    np.testing.assert_array_equal(gy, y[10:27, 6:39])
    np.testing.assert_array_equal(gu, u[5:14, 3:20])
    np.testing.assert_array_equal(gv, v[5:14, 3:20])
    other = same_inside(f[None], w, h, c, rect, 9)[0]
    assert (other != f).any()
    np.testing.assert_array_equal(crop_frame(other, w, h, c, rect), got)


def _open_crop(src_cf, rect, w=130, h=66, dst=(64, 32)):
    """mjg_open_crop of a w x h source with an otherwise valid config (dst: a valid encoded size,
    so that only the rectangle can be refused)."""
    L = _lib.load()
    dw, dh = dst
    cfg = _lib.MjgConfig(w, h, dw, dh, 1, 5, 1, 1, 1, 0, _lib.CHROMA_FORMATS[src_cf])
    hnd = C.c_void_p()
    rc = L.mjg_open_crop(0, C.byref(cfg), _lib.CHROMA_FORMATS[src_cf], *rect, C.byref(hnd))
    msg = L.mjg_last_error().decode()
    if hnd.value:
        L.mjg_close(hnd)
    return rc, msg


@pytest.mark.parametrize("c,rect,word", [
    ("420", (68, 0, 64, 32), "outside"),     # 68 + 64 > 130
    ("420", (0, 36, 64, 32), "outside"),     # 36 + 32 > 66
    ("444", (-1, 0, 64, 32), "outside"),
    ("420", (0, 0, 0, 32), "not positive"),
    ("420", (0, 0, 64, 0), "not positive"),
    ("420", (3, 0, 64, 32), "sub-sampling"),  # odd x on a 4:2:0 source
    ("420", (2, 3, 64, 32), "sub-sampling"),  # odd y on a 4:2:0 source
    ("422", (3, 3, 64, 32), "sub-sampling"),  # odd x on a 4:2:2 source (an odd y is fine there)
])
def test_open_crop_rejects_a_bad_rectangle_before_any_hip_call(c, rect, word):
    """MJG_E_INVALID with a message that names the rectangle, with or without a GPU: on a
    machine without one, any HIP call would give MJG_E_HIP instead."""
    assert _lib.load().mjg_version() >= 102
    rc, msg = _open_crop(c, rect)
    assert rc == _lib.MJG_E_INVALID, (rc, msg)
    assert word in msg and f"{rect[2]}x{rect[3]} at ({rect[0]},{rect[1]})" in msg, msg


def test_encoder_key_differs_for_two_rectangles():
    info = container.StreamInfo(130, 66, chroma="420")
    prof, why = _parse("crop=64:32:2:2")
    assert prof is not None, why
    k = [worker.encoder_key(prof, info, 64, 32, (1, 1), False, 8, rect=r)
         for r in ((2, 2, 64, 32), (4, 2, 64, 32), None)]
    assert len(set(k)) == 3
    assert k[0] == worker.encoder_key(prof, info, 64, 32, (1, 1), False, 8, rect=[2, 2, 64, 32])
