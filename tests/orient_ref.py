"""The reference for `-vf hflip / vflip / transpose` (tests/test_orient.py, tests/test_gpu_orient.py).
The filters are permutations of each plane's bytes, so the reference is numpy indexing:

  - orient_frame: the eight plane maps in the library's encoding, orient = T | FX << 1 | FY << 2:
    every plane P becomes flip(T ? P.T : P), the columns mirrored with FX, the rows with FY;
  - apply_filters: FFmpeg's filters one at a time, each by its own definition (vf_hflip.c,
    vf_vflip.c, vf_transpose.c), written as index loops over the output, not as the maps above.

The chroma planes are planes of their own ((w + hs) >> hs by (h + vs) >> vs), as the filters
treat them.  Everything after the orientation is the existing composed reference
(tests/crop_ref.py, tests/pad_ref.py) applied to the oriented frame."""
import numpy as np

from crop_ref import cropped_planes, cropped_ref
from pad_ref import padded_planes, padded_ref
from ffmpeg_distributed_amd.encoder import pack_i420, split_i420

TRANSPOSE_NAMES = {"cclock_flip": 0, "clock": 1, "cclock": 2, "clock_flip": 3}


def oriented_size(w, h, orient):
    return (h, w) if orient & 1 else (w, h)


def orient_plane(p, orient):
    q = p.T if orient & 1 else p
    if orient & 2:
        q = q[:, ::-1]
    if orient & 4:
        q = q[::-1]
    return q


def orient_frame(frame, w, h, chroma, orient):
    """The packed planar oriented frame (oriented_size(w, h, orient), same format) of one packed
    planar w x h frame."""
    assert not (orient & 1 and str(chroma) == "422")
    return pack_i420(*(orient_plane(p, orient) for p in split_i420(frame, w, h, chroma)))


def _filter_plane(p, name):
    """One filter on one plane, by the filter's definition: out[y][x] = in[...]."""
    h, w = p.shape
    if name == "hflip":
        out = np.empty((h, w), np.uint8)
        for y in range(h):
            for x in range(w):
                out[y, x] = p[y, w - 1 - x]
        return out
    if name == "vflip":
        out = np.empty((h, w), np.uint8)
        for y in range(h):
            for x in range(w):
                out[y, x] = p[h - 1 - y, x]
        return out
    opts = name.split("=", 1)[1].split(":")[0] if "=" in name else "0"
    d = opts.split("=")[-1]
    d = TRANSPOSE_NAMES[d] if d in TRANSPOSE_NAMES else int(d)
    out = np.empty((w, h), np.uint8)     # w rows of h bytes
    for y in range(w):
        for x in range(h):
            out[y, x] = p[h - 1 - x if d & 1 else x, w - 1 - y if d & 2 else y]
    return out


def apply_filters(frame, w, h, chroma, names):
    """The frame after the filters `names` (hflip, vflip, transpose=...), one at a time; returns
    (packed frame, its width, its height)."""
    planes = split_i420(frame, w, h, chroma)
    for name in names:
        assert name.split("=")[0] in ("hflip", "vflip", "transpose"), name
        planes = tuple(_filter_plane(p, name) for p in planes)
    return pack_i420(*planes), planes[0].shape[1], planes[0].shape[0]


def oriented_planes(frame, w, h, src, orient, rect, dst, full, dw=None, dh=None, pad=None):
    """(Y, U, V) encoder-input planes of one w x h source frame: oriented, cropped to rect (in the
    oriented frame; None: all of it), converted to `dst` at dw x dh, placed at pad (or not)."""
    ow, oh = oriented_size(w, h, orient)
    f = orient_frame(frame, w, h, src, orient)
    if pad is not None:
        return padded_planes(f, ow, oh, src, rect, dst, full, dw, dh, pad)
    return cropped_planes(f, ow, oh, src, rect or (0, 0, ow, oh), dst, full, dw, dh)


def oriented_ref(frame, w, h, src, orient, rect=None, dst=None, full=False, dw=None, dh=None, pad=None,
                 **kw) -> bytes:
    """The expected JPEG of that frame."""
    ow, oh = oriented_size(w, h, orient)
    f = orient_frame(frame, w, h, src, orient)
    if pad is not None:
        return padded_ref(f, ow, oh, src, rect, dst or src, full, dw, dh, pad, **kw)
    return cropped_ref(f, ow, oh, src, rect or (0, 0, ow, oh), dst or src, full, dw, dh, **kw)
