"""The reference for a `-pix_fmt` chroma conversion, composed from the CPU oracle's own pieces
(tests/test_chroma_resample.py, tests/test_gpu_chroma_resample.py):

  - the source frame split by its own format,
  - Y' = scale_plane(Y, dw, dh, range 0|1), U', V' = scale_plane(U|V, dcw, dch, range 0|2,
    chroma siting) with (dcw, dch) the encoded format's chroma plane size: swscale's one
    context per conversion (bicubic on every plane whose size changes, one-tap identity
    filters on the others, tv->pc in the same pass),
  - encode_frame(Y', U', V', full_range=True, chroma=dst).

With source format == encoded format this is what oracle.encode_frame does by itself."""
import numpy as np

import oracle
from ffmpeg_distributed_amd.encoder import chroma_size, i420_frame_bytes, pack_i420, split_i420


def composed_planes(frame, w, h, src, dst, full_range, dw=None, dh=None):
    """(Y', U', V'): the full-range encoder-input planes of one source frame."""
    dw, dh = dw or w, dh or h
    y, u, v = split_i420(frame, w, h, src)
    dcw, dch = chroma_size(dw, dh, dst)
    yy = oracle.scale_plane(y, dw, dh, range_mode=0 if full_range else 1, chroma=False)
    uu = oracle.scale_plane(u, dcw, dch, range_mode=0 if full_range else 2, chroma=True)
    vv = oracle.scale_plane(v, dcw, dch, range_mode=0 if full_range else 2, chroma=True)
    return yy, uu, vv


def composed_frame(frame, w, h, src, dst, full_range, dw=None, dh=None, qscale=5, sar=(1, 1),
                   huffman="default", rst=False) -> bytes:
    yy, uu, vv = composed_planes(frame, w, h, src, dst, full_range, dw, dh)
    return oracle.encode_frame(yy, uu, vv, full_range=True, qscale=qscale, sar=sar, huffman=huffman,
                               chroma=dst, rst=rst)


def source_frames(w, h, n, seed, chroma):
    """n - 1 frames of seeded noise and one smooth frame, packed planar in `chroma`."""
    rng = np.random.default_rng(seed)
    fb = i420_frame_bytes(w, h, chroma)
    cw, ch = chroma_size(w, h, chroma)
    out = [rng.integers(0, 256, fb, dtype=np.uint8) for _ in range(n - 1)]
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:ch, 0:cw]
    y = (128 + 100 * np.sin(xx / 7 + yy / 9)).clip(0, 255).astype(np.uint8)
    u = (128 + 90 * np.cos(cx / 4 + cy / 11)).clip(0, 255).astype(np.uint8)
    v = (128 + 90 * np.sin(cy / 3 - cx / 13)).clip(0, 255).astype(np.uint8)
    out.append(pack_i420(y, u, v))
    return np.stack(out)
