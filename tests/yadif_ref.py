"""The reference for `-vf yadif` (tests/test_yadif.py, tests/test_gpu_yadif.py): the filter as the
project restates it (the C path of vf_yadif.c's filter_line_c / filter_edges and
yadif_common.c's frame sequencing, modes 0 and 2, deint=all, 8-bit planar; written from the
project's own text of it, not compared with an FFmpeg build), twice:

  - yadif_plane_loop: index loops over the output, one sample at a time, in Python ints;
  - yadif_plane_vec: the same formula on whole rows with numpy (int32), for the larger shapes.

Every plane is filtered alike, the chroma planes at their own size.  deint_frames runs a sequence:
output i is made from frames max(i - 1, 0), i and min(i + 1, N - 1).  Everything after the
deinterlacer is the existing composed reference (orient_ref.oriented_ref and what it calls) on the
deinterlaced frames."""
import numpy as np

from orient_ref import oriented_planes, oriented_ref
from ffmpeg_distributed_amd.encoder import pack_i420, split_i420


def yadif_plane_loop(prev, cur, nxt, mode, tff):
    """One plane (h x w uint8 arrays prev, cur, next) -> the deinterlaced plane, by index loops."""
    h, w = cur.shape
    assert h >= 3 and w >= 3 and mode in (0, 2)
    P, C, N = (np.asarray(a).astype(np.int64).tolist() for a in (prev, cur, nxt))
    parity = tff ^ 1
    prev2, next2 = P, C          # parity ^ tff == 1 in these modes
    out = [row[:] for row in C]
    for y in range(h):
        if not ((y ^ parity) & 1):
            continue             # a kept row: cur's bytes
        ym = y - 1 if y else y + 1
        yp = y + 1 if y + 1 < h else y - 1
        y2m = y - 2 if y else y + 2
        y2p = y + 2 if y + 1 < h else y - 2
        md = 2 if (y == 1 or y + 2 == h) else mode
        for x in range(w):
            c, e = C[ym][x], C[yp][x]
            d = (prev2[y][x] + next2[y][x]) >> 1
            t0 = abs(prev2[y][x] - next2[y][x])
            t1 = (abs(P[ym][x] - c) + abs(P[yp][x] - e)) >> 1
            t2 = (abs(N[ym][x] - c) + abs(N[yp][x] - e)) >> 1
            diff = max(t0 >> 1, t1, t2)
            sp = (c + e) >> 1
            if 3 <= x < w - 3:
                def S(j):
                    return (abs(C[ym][x - 1 + j] - C[yp][x - 1 - j]) + abs(C[ym][x + j] - C[yp][x - j])
                            + abs(C[ym][x + 1 + j] - C[yp][x + 1 - j]))
                score = S(0) - 1
                for s in (-1, 1):
                    if S(s) < score:
                        score = S(s)
                        sp = (C[ym][x + s] + C[yp][x - s]) >> 1
                        if S(2 * s) < score:
                            score = S(2 * s)
                            sp = (C[ym][x + 2 * s] + C[yp][x - 2 * s]) >> 1
            if not (md & 2):
                b = (prev2[y2m][x] + next2[y2m][x]) >> 1
                f = (prev2[y2p][x] + next2[y2p][x]) >> 1
                mx = max(d - e, d - c, min(b - c, f - e))
                mn = min(d - e, d - c, max(b - c, f - e))
                diff = max(diff, mn, -mx)
            if sp > d + diff:
                sp = d + diff
            elif sp < d - diff:
                sp = d - diff
            out[y][x] = sp
    res = np.array(out, np.int64)
    assert res.min() >= 0 and res.max() <= 255
    return res.astype(np.uint8)


def yadif_plane_vec(prev, cur, nxt, mode, tff):
    """The same plane with numpy: all interpolated rows at once, int32."""
    h, w = cur.shape
    assert h >= 3 and w >= 3 and mode in (0, 2)
    P, C, N = (np.asarray(a).astype(np.int32) for a in (prev, cur, nxt))
    parity = tff ^ 1
    ys = np.array([y for y in range(h) if (y ^ parity) & 1], np.int64)
    out = np.asarray(cur).copy()
    if not ys.size:
        return out
    ym = np.where(ys > 0, ys - 1, ys + 1)
    yp = np.where(ys + 1 < h, ys + 1, ys - 1)
    nosp = (ys == 1) | (ys + 2 == h) | bool(mode & 2)
    y2m = np.where(nosp, ys, np.where(ys > 0, ys - 2, ys + 2))     # unused rows: any row inside the plane
    y2p = np.where(nosp, ys, np.where(ys + 1 < h, ys + 2, ys - 2))
    A, B = C[ym], C[yp]
    c, e = A, B
    p2, n2 = P[ys], C[ys]
    d = (p2 + n2) >> 1
    t0 = np.abs(p2 - n2)
    t1 = (np.abs(P[ym] - c) + np.abs(P[yp] - e)) >> 1
    t2 = (np.abs(N[ym] - c) + np.abs(N[yp] - e)) >> 1
    diff = np.maximum(np.maximum(t0 >> 1, t1), t2)
    sp = (c + e) >> 1
    Ap, Bp = np.pad(A, ((0, 0), (3, 3))), np.pad(B, ((0, 0), (3, 3)))

    def a(k):
        return Ap[:, 3 + k:3 + k + w]

    def b_(k):
        return Bp[:, 3 + k:3 + k + w]

    def S(j):
        return np.abs(a(j - 1) - b_(-1 - j)) + np.abs(a(j) - b_(-j)) + np.abs(a(j + 1) - b_(1 - j))

    score = S(0) - 1
    sx = sp.copy()
    for s in (-1, 1):
        t1_ = S(s) < score
        sc1 = np.where(t1_, S(s), score)
        sp1 = np.where(t1_, (a(s) + b_(-s)) >> 1, sx)
        t2_ = t1_ & (S(2 * s) < sc1)
        score = np.where(t2_, S(2 * s), sc1)
        sx = np.where(t2_, (a(2 * s) + b_(-2 * s)) >> 1, sp1)
    xs = np.arange(w)
    inner = (xs >= 3) & (xs < w - 3)
    sp = np.where(inner[None, :], sx, sp)
    bb = (P[y2m] + C[y2m]) >> 1
    ff = (P[y2p] + C[y2p]) >> 1
    mx = np.maximum(np.maximum(d - e, d - c), np.minimum(bb - c, ff - e))
    mn = np.minimum(np.minimum(d - e, d - c), np.maximum(bb - c, ff - e))
    diff = np.where(nosp[:, None], diff, np.maximum(np.maximum(diff, mn), -mx))
    res = np.where(sp > d + diff, d + diff, np.where(sp < d - diff, d - diff, sp))
    assert res.min() >= 0 and res.max() <= 255
    out[ys] = res.astype(np.uint8)
    return out


def deint_frame(prev, cur, nxt, w, h, chroma, mode, tff, vec=True):
    """One packed planar frame from its two neighbours (packed planar too)."""
    fn = yadif_plane_vec if vec else yadif_plane_loop
    planes = [fn(p, c, n, mode, tff) for p, c, n in zip(split_i420(prev, w, h, chroma), split_i420(cur, w, h, chroma),
                                                         split_i420(nxt, w, h, chroma))]
    return pack_i420(*planes)


def deint_frames(frames, w, h, chroma, mode, tff, vec=True):
    """A sequence of N packed planar frames -> its N deinterlaced frames (N x frame_bytes)."""
    n = len(frames)
    return np.stack([deint_frame(frames[max(i - 1, 0)], frames[i], frames[min(i + 1, n - 1)], w, h, chroma, mode, tff, vec)
                     for i in range(n)])


def deint_ref(dframe, w, h, src, orient=0, rect=None, dst=None, full=False, dw=None, dh=None, pad=None, **kw) -> bytes:
    """The expected JPEG of one deinterlaced frame: the composed reference of the rest of the chain."""
    return oriented_ref(dframe, w, h, src, orient, rect, dst, full, dw, dh, pad, **kw)


def deint_planes(dframe, w, h, src, orient, rect, dst, full, dw=None, dh=None, pad=None):
    return oriented_planes(dframe, w, h, src, orient, rect, dst, full, dw, dh, pad)
