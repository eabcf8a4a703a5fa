"""The reference for `-vf ...,pad` (tests/test_pad.py, tests/test_gpu_pad.py): the full-range
encoder-input planes of the picture, composed from the CPU oracle's pieces as for crop and
-pix_fmt (tests/crop_ref.py, tests/chroma_resample_ref.py), placed by numpy into constant
planes of Y = 0, Cb = Cr = 128 (black in the encoder's full-range input), and those encoded
by oracle.encode_frame as they are (full_range=True: no further conversion)."""
import numpy as np

import oracle
from chroma_resample_ref import composed_planes
from crop_ref import crop_frame
from ffmpeg_distributed_amd.encoder import CHROMA_SHIFTS, chroma_size

BORDER = (0, 128, 128)


def pad_planes(yy, uu, vv, dst, x, y, W, H):
    """The W x H canvas planes in `dst` with the picture planes (yy, uu, vv) at luma (x, y): the
    chroma planes at (x >> hs, y >> vs).  x, y, W, H and the picture's size are multiples of the
    format's sub-sampling."""
    hs, vs = CHROMA_SHIFTS[str(dst)]
    ph, pw = yy.shape
    m, n = (1 << hs) - 1, (1 << vs) - 1
    assert not ((x | W | pw) & m or (y | H | ph) & n) and 0 <= x <= W - pw and 0 <= y <= H - ph
    cw, ch = chroma_size(W, H, dst)
    out = []
    for p, (pl, (cx, cy), (w, h)) in enumerate(zip((yy, uu, vv), ((x, y), (x >> hs, y >> vs), (x >> hs, y >> vs)),
                                                    ((W, H), (cw, ch), (cw, ch)))):
        c = np.full((h, w), BORDER[p], np.uint8)
        c[cy:cy + pl.shape[0], cx:cx + pl.shape[1]] = pl
        out.append(c)
    return tuple(out)


def padded_planes(frame, w, h, src, rect, dst, full, dw, dh, pad):
    """(Y, U, V) canvas planes of one w x h source frame in `src`: cropped to rect (None: the
    whole frame), converted to `dst` at dw x dh, placed at pad = (x, y, W, H)."""
    rect = rect or (0, 0, w, h)
    yy, uu, vv = composed_planes(crop_frame(frame, w, h, src, rect), rect[2], rect[3], src, dst, full, dw, dh)
    return pad_planes(yy, uu, vv, dst, *pad)


def padded_ref(frame, w, h, src, rect, dst, full, dw, dh, pad, qscale=5, sar=(1, 1), huffman="default",
               rst=False) -> bytes:
    """The expected JPEG of that frame."""
    yy, uu, vv = padded_planes(frame, w, h, src, rect, dst, full, dw, dh, pad)
    return oracle.encode_frame(yy, uu, vv, full_range=True, qscale=qscale, sar=sar, huffman=huffman,
                               chroma=dst, rst=rst)
