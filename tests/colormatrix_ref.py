"""`-vf colormatrix=SRC:DST` on 8-bit planar frames as DESIGN §4.16 restates vf_colormatrix.c, held twice:
an index loop in Python ints (`convert_frame_loop`, `pixel`) and a numpy form (`convert_frames`).  The
restatement is unpinned against FFmpeg; the tests pin the product to this text, and the two forms to
each other.  Imports no product code.

    bs = 0.5 / (B - 1), rs = 0.5 / (R - 1)
    M = [G, B, R], [bs G, 0.5, bs R], [rs G, rs B, 0.5]          (G, B, R: the space's luma weights)
    C = M_dst inverse(M_src); NS(n) = n < 0 ? int(n 65536 - 0.5 + DBL_EPSILON) : int(n 65536 + 0.5)
    c2, c3 = NS(C[0][1]), NS(C[0][2]); c4, c5 = NS(C[1][1]), NS(C[1][2]); c6, c7 = NS(C[2][1]), NS(C[2][2])
    u = U - 128, v = V - 128                                      (U, V at x >> hs, y >> vs)
    Y' = clip8((65536 (Y - 16) + c2 u + c3 v + 1081344) >> 16)
    U' = clip8((c4 u + c5 v + 8421376) >> 16),  V' = clip8((c6 u + c7 v + 8421376) >> 16)
"""
import sys
import zlib

import numpy as np

LUMA = {"bt709": (0.7152, 0.0722, 0.2126), "fcc": (0.59, 0.11, 0.30), "bt601": (0.587, 0.114, 0.299),
        "smpte240m": (0.701, 0.087, 0.212), "bt2020": (0.678, 0.0593, 0.2627)}
ALIASES = {"bt470": "bt601", "bt470bg": "bt601", "smpte170m": "bt601"}
SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
IDENTITY = (0, 0, 65536, 0, 0, 65536)
# every coefficient different, none near unity's neighbours: a swapped U / V or a swapped pair shows
MADE_UP = (9001, -15013, 61007, 11003, -7019, 70001)


def yuv_matrix(name):
    g, b, r = LUMA[ALIASES.get(name, name)]
    bs, rs = 0.5 / (b - 1.0), 0.5 / (r - 1.0)
    return np.array([[g, b, r], [bs * g, 0.5, bs * r], [rs * g, rs * b, 0.5]], np.float64)


def ns(n):
    n = float(n)
    return int(n * 65536.0 - 0.5 + sys.float_info.epsilon) if n < 0 else int(n * 65536.0 + 0.5)


def matrix(src, dst):
    """All nine 16.16 entries of the conversion, row by row."""
    c = yuv_matrix(dst) @ np.linalg.inv(yuv_matrix(src))
    return [[ns(v) for v in row] for row in c]


def coefs(src, dst):
    m = matrix(src, dst)
    return (m[0][1], m[0][2], m[1][1], m[1][2], m[2][1], m[2][2])


def clip8(x):
    return 0 if x < 0 else 255 if x > 255 else x


def pixel(y, u, v, c):
    """(Y, U, V) -> (Y', U', V'), Python ints (>> of a negative int floors, as C's arithmetic shift)."""
    c2, c3, c4, c5, c6, c7 = c
    u, v = u - 128, v - 128
    uvval = c2 * u + c3 * v + 1081344
    return (clip8((65536 * (y - 16) + uvval) >> 16), clip8((c4 * u + c5 * v + 8421376) >> 16),
            clip8((c6 * u + c7 * v + 8421376) >> 16))


def plane_sizes(w, h, chroma):
    hs, vs = SHIFTS[str(chroma)]
    return (w, h), ((w + hs) >> hs, (h + vs) >> vs)


def convert_frame_loop(frame, w, h, chroma, c):
    """One packed planar frame, sample by sample."""
    hs, vs = SHIFTS[str(chroma)]
    (_, _), (cw, ch) = plane_sizes(w, h, chroma)
    f = [int(b) for b in np.asarray(frame, np.uint8).reshape(-1)]
    out = list(f)
    uo, vo = w * h, w * h + cw * ch
    for y in range(h):
        for x in range(w):
            ci = (y >> vs) * cw + (x >> hs)
            out[y * w + x] = pixel(f[y * w + x], f[uo + ci], f[vo + ci], c)[0]
    for i in range(cw * ch):
        _, out[uo + i], out[vo + i] = pixel(16, f[uo + i], f[vo + i], c)
    return np.array(out, np.uint8)


def _sums(frames, w, h, chroma, c):
    """The three planes' values in front of the clip, int64: (N, h, w), (N, ch, cw), (N, ch, cw)."""
    c2, c3, c4, c5, c6, c7 = (int(v) for v in c)
    hs, vs = SHIFTS[str(chroma)]
    (_, _), (cw, ch) = plane_sizes(w, h, chroma)
    f = np.asarray(frames, np.uint8).reshape(-1, w * h + 2 * cw * ch).astype(np.int64)
    Y = f[:, :w * h].reshape(-1, h, w)
    u = f[:, w * h:w * h + cw * ch].reshape(-1, ch, cw) - 128
    v = f[:, w * h + cw * ch:].reshape(-1, ch, cw) - 128
    k = (c2 * u + c3 * v + 1081344) >> 16
    kk = k[:, (np.arange(h) >> vs)][:, :, (np.arange(w) >> hs)]
    return Y - 16 + kk, (c4 * u + c5 * v + 8421376) >> 16, (c6 * u + c7 * v + 8421376) >> 16


def convert_frames(frames, w, h, chroma, c):
    """Packed planar frames (any leading shape) through the matrix, numpy form (the luma identity
    (65536 a + b) >> 16 == a + (b >> 16) is used here and not in the loop form)."""
    frames = np.asarray(frames, np.uint8)
    ys, us, vs_ = _sums(frames, w, h, chroma, c)
    n = ys.shape[0]
    out = np.concatenate([np.clip(p, 0, 255).reshape(n, -1) for p in (ys, us, vs_)], axis=1).astype(np.uint8)
    return out.reshape(frames.shape)


def clip_counts(frames, w, h, chroma, c):
    """(samples clipped at 0, samples clipped at 255) over all three planes."""
    lo = hi = 0
    for p in _sums(frames, w, h, chroma, c):
        lo += int((p < 0).sum())
        hi += int((p > 255).sum())
    return lo, hi


def uv_tables(c):
    """U', V' (uint8) and k (int16) over all 256 x 256 (U, V) pairs, U the outer index."""
    c2, c3, c4, c5, c6, c7 = (int(v) for v in c)
    u = (np.arange(256, dtype=np.int64) - 128)[:, None]
    v = (np.arange(256, dtype=np.int64) - 128)[None, :]
    uo = np.clip((c4 * u + c5 * v + 8421376) >> 16, 0, 255).astype(np.uint8)
    vo = np.clip((c6 * u + c7 * v + 8421376) >> 16, 0, 255).astype(np.uint8)
    k = ((c2 * u + c3 * v + 1081344) >> 16).astype("<i2")
    return uo, vo, k


def uv_tables_loop(c):
    uo, vo, k = bytearray(), bytearray(), []
    for u in range(256):
        for v in range(256):
            _, a, b = pixel(16, u, v, c)
            uo.append(a)
            vo.append(b)
            k.append((c[0] * (u - 128) + c[1] * (v - 128) + 1081344) >> 16)
    return np.frombuffer(bytes(uo), np.uint8), np.frombuffer(bytes(vo), np.uint8), np.array(k, "<i2")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def noise_frames(w, h, chroma, n, extreme_plane, seed=0):
    """n frames of seeded noise; plane `extreme_plane` (0 Y, 1 U, 2 V) is drawn from {0..20, 235..255}, so
    that both clips of the matrix occur."""
    (_, _), (cw, ch) = plane_sizes(w, h, chroma)
    rng = np.random.default_rng([w, h, int(chroma), n, extreme_plane, seed])
    f = rng.integers(0, 256, (n, w * h + 2 * cw * ch), dtype=np.uint8)
    ext = np.concatenate([np.arange(0, 21), np.arange(235, 256)]).astype(np.uint8)
    lo, hi = [(0, w * h), (w * h, w * h + cw * ch), (w * h + cw * ch, w * h + 2 * cw * ch)][extreme_plane]
    f[:, lo:hi] = ext[rng.integers(0, len(ext), (n, hi - lo))]
    return f
