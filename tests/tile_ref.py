"""The reference for `-vf ...,tile` (tests/test_tile.py, tests/test_gpu_tile.py, tools/tile_host_check.py):
FFmpeg's vf_tile.c as this project restates it.  No FFmpeg build has been compared with
it; the tests pin the kernel to this text.

With cells of w x h, a sheet = (cols, rows, nb_frames, margin, padding) and N = nb_frames or cols * rows:
  the sheet is W = cols w + (cols - 1) padding + 2 margin by H = rows h + (rows - 1) padding + 2 margin;
  frame i of a sequence goes to sheet i // N, cell t = i % N, whose top left corner is
  (margin + (w + padding) (t % cols), margin + (h + padding) (t // cols)); the chroma planes sit at that
  corner shifted by the format's sub-sampling, with the cell's chroma size;
  every sample that is not in a cell that holds a frame is the pad's black (pad_ref.BORDER: Y = 0,
  Cb = Cr = 128 in the full-range encoder input); the last sheet of a sequence is emitted partly filled.

Two forms of the composition: sheets_loop (an index loop per sheet sample that asks which cell, if any,
the sample lies in) and sheets_numpy (slices of constant planes).  The cells are the planes the composed
references of the chain in front give (cell_planes: yadif_ref / orient_ref / crop_ref /
chroma_resample_ref / unsharp_ref through unsharp_ref.presharp_planes); a sheet's expected JPEG comes
from oracle.encode_frame(full_range=True) on its planes, as pad_ref gets a canvas's."""
import numpy as np

import oracle
from pad_ref import BORDER
from unsharp_ref import presharp_planes, unsharp_planes
from ffmpeg_distributed_amd.encoder import CHROMA_SHIFTS


def resolve(sheet):
    """(cols, rows, N, margin, padding) with nb_frames 0 resolved to cols * rows."""
    cols, rows, nb, margin, padding = sheet
    return cols, rows, nb or cols * rows, margin, padding


def sheet_size(w, h, sheet):
    cols, rows, _, margin, padding = sheet
    return cols * w + (cols - 1) * padding + 2 * margin, rows * h + (rows - 1) * padding + 2 * margin


def frames_out(n, sheet):
    N = resolve(sheet)[2]
    return (n + N - 1) // N


def _plane_geometry(w, h, chroma, sheet, p):
    """Of plane p (0 Y, 1 U, 2 V): the cell's size, the sheet's, the margin and the two pitches."""
    cols, rows, _, margin, padding = sheet
    hs, vs = CHROMA_SHIFTS[str(chroma)] if p else (0, 0)
    W, H = sheet_size(w, h, sheet)
    assert not ((w | margin | padding) & ((1 << hs) - 1) or (h | margin | padding) & ((1 << vs) - 1))
    return (w >> hs, h >> vs), (W >> hs, H >> vs), (margin >> hs, margin >> vs), ((w + padding) >> hs, (h + padding) >> vs)


def sheets_loop(cells, w, h, chroma, sheet):
    """The sheets of one sequence, sample by sample.  cells: a (Y, U, V) of w x h in `chroma` per frame.
    Returns a (Y, U, V) per sheet."""
    cols, rows, N, _, _ = resolve(sheet)
    out = []
    for j in range(frames_out(len(cells), sheet)):
        planes = []
        for p in range(3):
            (cw, ch), (W, H), (mx, my), (pw, ph) = _plane_geometry(w, h, chroma, sheet, p)
            s = np.empty((H, W), np.uint8)
            for y in range(H):
                for x in range(W):
                    v = BORDER[p]
                    ry, cx = y - my, x - mx
                    if ry >= 0 and cx >= 0:
                        r, yy = divmod(ry, ph)
                        c, xx = divmod(cx, pw)
                        t = r * cols + c
                        if yy < ch and xx < cw and c < cols and r < rows and t < N and j * N + t < len(cells):
                            v = cells[j * N + t][p][yy, xx]
                    s[y, x] = v
            planes.append(s)
        out.append(tuple(planes))
    return out


def sheets_numpy(cells, w, h, chroma, sheet):
    """The same sheets by slices."""
    cols, rows, N, _, _ = resolve(sheet)
    out = []
    for j in range(frames_out(len(cells), sheet)):
        planes = []
        for p in range(3):
            (cw, ch), (W, H), (mx, my), (pw, ph) = _plane_geometry(w, h, chroma, sheet, p)
            s = np.full((H, W), BORDER[p], np.uint8)
            for t, cell in enumerate(cells[j * N:(j + 1) * N]):
                x0, y0 = mx + pw * (t % cols), my + ph * (t // cols)
                assert cell[p].shape == (ch, cw)
                s[y0:y0 + ch, x0:x0 + cw] = cell[p]
            planes.append(s)
        out.append(tuple(planes))
    return out


def cell_planes(frame, w, h, src, us=None, orient=0, rect=None, dst=None, full=False, dw=None, dh=None):
    """(Y, U, V) of the cell one decoded (or deinterlaced, or colour-converted) w x h frame gives: the
    sws stage's picture, under an unsharp the sharpened one."""
    pre = presharp_planes(frame, w, h, src, orient, rect, dst or src, full, dw, dh)
    return unsharp_planes(*pre, us) if us is not None else pre


def sheet_jpeg(planes, chroma, qscale=5, sar=(1, 1), huffman="default", rst=False) -> bytes:
    """The expected JPEG of one sheet."""
    return oracle.encode_frame(*planes, full_range=True, qscale=qscale, sar=sar, huffman=huffman, chroma=chroma, rst=rst)


def pack(planes) -> np.ndarray:
    return np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in planes])


# The geometry of every GPU test (tests/test_gpu_tile.py), which tools/tile_host_check.py walks on the CPU
# first: (cell w, h, encoded format, sheet, the frames of each segment of a submit)
GPU_GEOMETRY = [
    (8, 8, "420", (5, 3, 0, 0, 0), (17,)),
    (33, 17, "444", (2, 2, 0, 3, 5), (4,)),
    (33, 17, "444", (2, 2, 0, 3, 5), (5,)),
    (208, 120, "422", (2, 2, 3, 0, 0), (7,)),
    (64, 32, "420", (3, 2, 0, 0, 0), (6,)),
    (64, 32, "420", (3, 2, 0, 0, 0), (7,)),
    (16, 16, "420", (2, 2, 0, 0, 0), (4, 1, 6)),
    (16, 16, "420", (2, 2, 0, 0, 0), (4,)),
    (16, 16, "420", (2, 2, 0, 0, 0), (1,)),
    (16, 16, "420", (2, 2, 0, 0, 0), (6,)),
    (32, 16, "420", (2, 1, 0, 0, 0), (5,)),
    (32, 16, "420", (2, 1, 0, 0, 0), (4,)),
    (32, 48, "420", (2, 2, 0, 0, 0), (3,)),
    (32, 24, "420", (3, 2, 0, 0, 0), (6,)),
]
