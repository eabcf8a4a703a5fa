"""The reference for `-vf crop` (tests/test_crop.py, tests/test_gpu_crop.py): a cropped frame is
the packed sub-rectangles of its planes, cut by numpy slicing; everything after that is the
existing composed reference (tests/chroma_resample_ref.py: scale_plane per plane, then
encode_frame), which with nothing else to do is oracle.encode_frame itself."""
import numpy as np

from chroma_resample_ref import composed_frame, composed_planes
from ffmpeg_distributed_amd.encoder import CHROMA_SHIFTS, chroma_size, pack_i420, split_i420


def crop_frame(frame, w, h, chroma, rect):
    """The packed planar rw x rh frame at (x, y) of a packed planar w x h frame in `chroma`:
    luma rows y .. y + rh, columns x .. x + rw; the chroma planes at (x >> hs, y >> vs) with
    the chroma plane size of an rw x rh frame.  rect = (x, y, rw, rh), x and y multiples of the
    format's sub-sampling."""
    x, y, rw, rh = rect
    hs, vs = CHROMA_SHIFTS[str(chroma)]
    assert x % (1 << hs) == 0 and y % (1 << vs) == 0 and x + rw <= w and y + rh <= h
    yy, uu, vv = split_i420(frame, w, h, chroma)
    cw, ch = chroma_size(rw, rh, chroma)
    cx, cy = x >> hs, y >> vs
    return pack_i420(yy[y:y + rh, x:x + rw], uu[cy:cy + ch, cx:cx + cw], vv[cy:cy + ch, cx:cx + cw])


def cropped_ref(frame, w, h, src, rect, dst=None, full_range=False, dw=None, dh=None, **kw) -> bytes:
    """The expected JPEG of one w x h source frame in `src`: cropped to rect, then converted to
    `dst` at dw x dh (default: the source format, the rectangle's size)."""
    return composed_frame(crop_frame(frame, w, h, src, rect), rect[2], rect[3], src, dst or src, full_range,
                          dw, dh, **kw)


def cropped_planes(frame, w, h, src, rect, dst, full_range, dw=None, dh=None):
    return composed_planes(crop_frame(frame, w, h, src, rect), rect[2], rect[3], src, dst, full_range, dw, dh)


def same_inside(frames, w, h, chroma, rect, seed):
    """A copy of `frames` with every sample outside rect replaced by other noise."""
    rng = np.random.default_rng(seed)
    x, y, rw, rh = rect
    hs, vs = CHROMA_SHIFTS[str(chroma)]
    cw, ch = chroma_size(rw, rh, chroma)
    out = []
    for f in frames:
        g = rng.integers(0, 256, f.size, dtype=np.uint8)
        src, dst = split_i420(f, w, h, chroma), split_i420(g, w, h, chroma)
        dst[0][y:y + rh, x:x + rw] = src[0][y:y + rh, x:x + rw]
        for p in (1, 2):
            dst[p][y >> vs:(y >> vs) + ch, x >> hs:(x >> hs) + cw] = src[p][y >> vs:(y >> vs) + ch,
                                                                          x >> hs:(x >> hs) + cw]
        out.append(g)
    return np.stack(out)
