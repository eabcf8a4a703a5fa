"""The reference for `-vf unsharp` (tests/test_unsharp.py, tests/test_gpu_unsharp.py,
tools/unsharp_host_check.py): the 8-bit planar path of FFmpeg's vf_unsharp.c as this project restates
it.  No FFmpeg build has been compared with it; the tests pin the kernel to this text.

Two forms of one plane filter:
  unsharp_plane_loop   the filter's own running pair sums (2 sx along the row, 2 sy down the column,
                       accumulators that start at zero, x from -sx and y from -sy, every value
                       masked to 32 bits as a uint32_t is), sample by sample;
  unsharp_plane_vec    the closed form, numpy int64:
      blur[y][x] = (sum_j sum_i C(2sy, j) C(2sx, i) P[clamp(y + j - sy)][clamp(x + i - sx)] + half) >> scalebits
      out[y][x]  = clip_uint8(P[y][x] + (((P[y][x] - blur[y][x]) * amount_i) >> 16))
with sx = mx // 2, sy = my // 2, scalebits = 2 (sx + sy), half = 1 << (scalebits - 1) and amount_i =
int(amount * 65536.0).  A plane with amount_i == 0 is returned as it is.

The composed reference of a graph `[yadif,][vflip|transpose...,][crop,][scale,]unsharp[,pad]`: the
deinterlaced / oriented frame (tests/yadif_ref.py, tests/orient_ref.py), crop_ref.crop_frame,
chroma_resample_ref.composed_planes, the filter on each plane (luma with lx:ly:la, Cb and Cr with
cx:cy:ca at their own size), pad_ref.pad_planes, oracle.encode_frame(full_range=True)."""
from math import comb

import numpy as np

import oracle
from chroma_resample_ref import composed_planes
from crop_ref import crop_frame
from orient_ref import orient_frame, oriented_size
from pad_ref import pad_planes

M32 = 0xFFFFFFFF
DEFAULT = (5, 5, 1.0, 5, 5, 0.0)


def amount_i(amount: float) -> int:
    """(int)(amount * 65536.0): C truncation of the double."""
    return int(float(amount) * 65536.0)


def unsharp_plane_loop(p, mx, my, amount, half_on=True):
    """One plane through the filter's loop; `amount` is amount_i.  half_on=False drops the rounding
    constant (tests use it to show that an input can tell)."""
    p = np.asarray(p, np.uint8)
    h, w = p.shape
    if amount == 0:
        return p.copy()
    sx, sy = mx // 2, my // 2
    scalebits = 2 * (sx + sy)
    half = (1 << (scalebits - 1)) if half_on else 0
    src = p.tolist()
    out = np.empty((h, w), np.uint8)
    sc = [[0] * (w + 2 * sx) for _ in range(2 * sy)]
    for y in range(-sy, h + sy):
        row = src[min(max(y, 0), h - 1)]
        sr = [0] * (2 * sx)
        for x in range(-sx, w + sx):
            tmp1 = row[min(max(x, 0), w - 1)]
            for z in range(0, 2 * sx, 2):
                tmp2 = (sr[z] + tmp1) & M32
                sr[z] = tmp1
                tmp1 = (sr[z + 1] + tmp2) & M32
                sr[z + 1] = tmp2
            for z in range(0, 2 * sy, 2):
                tmp2 = (sc[z][x + sx] + tmp1) & M32
                sc[z][x + sx] = tmp1
                tmp1 = (sc[z + 1][x + sx] + tmp2) & M32
                sc[z + 1][x + sx] = tmp2
            if x >= sx and y >= sy:
                s = src[y - sy][x - sx]
                blur = ((tmp1 + half) & M32) >> scalebits
                res = s + (((s - blur) * amount) >> 16)      # Python's >> on a negative int is arithmetic
                out[y - sy][x - sx] = min(max(res, 0), 255)
    return out


def unsharp_plane_vec(p, mx, my, amount, half_on=True, reflect=False):
    """One plane by the closed form; `amount` is amount_i.  reflect=True mirrors the edge instead of
    replicating it (tests use it to show that an input can tell)."""
    p = np.asarray(p, np.uint8)
    h, w = p.shape
    if amount == 0:
        return p.copy()
    sx, sy = mx // 2, my // 2
    scalebits = 2 * (sx + sy)
    half = (1 << (scalebits - 1)) if half_on else 0

    def idx(n, s):
        i = np.arange(-s, n + s)
        if reflect:
            i = np.where(i < 0, -i, i)
            i = np.where(i >= n, 2 * (n - 1) - i, i)
        return np.clip(i, 0, n - 1)

    e = p.astype(np.int64)[idx(h, sy)][:, idx(w, sx)]
    rows = sum(comb(2 * sx, i) * e[:, i:i + w] for i in range(2 * sx + 1))
    acc = sum(comb(2 * sy, j) * rows[j:j + h] for j in range(2 * sy + 1))
    assert int(acc.max()) + half <= M32
    blur = (acc + half) >> scalebits
    s = p.astype(np.int64)
    return np.clip(s + (((s - blur) * int(amount)) >> 16), 0, 255).astype(np.uint8)


def unsharp_planes(yy, uu, vv, us, fn=unsharp_plane_vec):
    """The three picture planes through the filter: us = (lx, ly, la, cx, cy, ca), amounts as floats."""
    lx, ly, la, cx, cy, ca = us
    return (fn(yy, lx, ly, amount_i(la)), fn(uu, cx, cy, amount_i(ca)), fn(vv, cx, cy, amount_i(ca)))


def presharp_planes(frame, w, h, src, orient, rect, dst, full, dw=None, dh=None):
    """(Y, U, V) of the sws stage's picture for one decoded (or deinterlaced) w x h frame: oriented,
    cropped to rect (in the oriented frame; None: all of it), converted to `dst` at dw x dh."""
    ow, oh = oriented_size(w, h, orient)
    f = orient_frame(frame, w, h, src, orient)
    rect = rect or (0, 0, ow, oh)
    return composed_planes(crop_frame(f, ow, oh, src, rect), rect[2], rect[3], src, dst, full, dw or rect[2], dh or rect[3])


def sharp_planes(frame, w, h, src, us, orient=0, rect=None, dst=None, full=False, dw=None, dh=None, pad=None):
    """(the sws stage's output, the encoder's input): each (Y, U, V), on the canvas under a pad."""
    dst = dst or src
    pre = presharp_planes(frame, w, h, src, orient, rect, dst, full, dw, dh)
    post = unsharp_planes(*pre, us)
    if pad is not None:
        pre, post = pad_planes(*pre, dst, *pad), pad_planes(*post, dst, *pad)
    return pre, post


def sharp_ref(frame, w, h, src, us, orient=0, rect=None, dst=None, full=False, dw=None, dh=None, pad=None,
              qscale=5, sar=(1, 1), huffman="default", rst=False) -> bytes:
    """The expected JPEG of that frame."""
    _, (yy, uu, vv) = sharp_planes(frame, w, h, src, us, orient, rect, dst, full, dw, dh, pad)
    return oracle.encode_frame(yy, uu, vv, full_range=True, qscale=qscale, sar=sar, huffman=huffman,
                               chroma=dst or src, rst=rst)


def kernel_constant(name):
    """A `constexpr int` of scale.hip (kSharpTileW, kSharpTileH)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "ffmpeg_distributed_amd", "csrc", "scale.hip")) as f:
        return int(re.search(r"constexpr int " + name + r" = (\d+);", f.read()).group(1))


# The encoded geometry of every GPU test (tests/test_gpu_unsharp.py), which tools/unsharp_host_check.py
# walks on the CPU first: (canvas W, H, format, picture x, y, w, h, unsharp).  TILES: wider than a tile
# and four columns, taller than two tiles, so tiles abut in both directions and the last is partial.
TILES = (kernel_constant("kSharpTileW") + 7, 2 * kernel_constant("kSharpTileH") + 5)
US2 = (3, 7, 1.5, 7, 3, -0.5)
US_TILES = (5, 5, 1.0, 3, 5, 0.7)
US_WIDE = (23, 3, 1.0, 3, 23, 1.0)
US_LIMIT = (13, 13, 1.0, 13, 13, 2.0)
GPU_GEOMETRY = [
    (70, 38, "420", 0, 0, 70, 38, DEFAULT),
    (70, 38, "420", 0, 0, 70, 38, US2),
    (TILES[0], TILES[1], "444", 0, 0, TILES[0], TILES[1], US_TILES),
    (6, 6, "444", 0, 0, 6, 6, US_WIDE),
    (40, 24, "444", 0, 0, 40, 24, US_LIMIT),
    (80, 48, "420", 8, 8, 64, 32, DEFAULT),
    (48, 80, "420", 8, 8, 32, 64, DEFAULT),
    (50, 38, "420", 8, 10, 34, 18, US2),
    (64, 32, "420", 0, 0, 64, 32, DEFAULT),
]

# The encoded geometry of tests/test_gpu_filter_chain.py, in the same form and walked by the same
# tool: planes of three and more tile columns (aprons of 11 across tile seams, the staging loop's
# third iteration), <5, 5> on all three planes, pictures whose left edge cuts a quad (pic masks 8,
# 12, 14) inside canvases whose outer tiles only copy, a 4:2:2 frame, and a copied luma of 12 tiles.
US_23 = (23, 3, 1.0, 3, 23, 0.7)
US_13 = (13, 13, 1.0, 9, 15, -1.0)
US_55 = (5, 5, 1.0, 5, 5, 1.0)
US_73 = (7, 3, 1.5, 3, 7, 0.5)
US_422 = (7, 5, 1.5, 5, 5, 0.5)
US_LUMA0 = (5, 5, 0.0, 3, 3, 1.0)
WIDE = (3 * kernel_constant("kSharpTileW") + 5, 2 * kernel_constant("kSharpTileH") + 6)      # 197 x 70
GPU_GEOMETRY_CHAIN = [
    (*WIDE, "444", 0, 0, *WIDE, US_23),
    (*WIDE, "444", 0, 0, *WIDE, US_13),
    (*WIDE, "444", 0, 0, *WIDE, US_55),
    (201, 99, "444", 67, 33, 70, 34, US_55),
    (203, 101, "444", 69, 35, 66, 33, US_73),
    (264, 136, "420", 70, 38, 130, 66, US_55),
    (134, 70, "422", 0, 0, 134, 70, US_422),
    (*WIDE, "444", 0, 0, *WIDE, US_LUMA0),
]
