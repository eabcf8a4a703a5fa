"""k_encode's column skip, decided in the row pass: a column (2-7) of a chunk is left out of the
column screen when max|u| of the column over all 8 rows of all 64 blocks is at most
A_c = min(amax_c, floor(Rmax_c / 2)) (build_tabs; restated by test_kernel_arith._skip_limits).

The sweeps put one patterned block into every chunk of 1024x16 frames (6 chunks, 63 flat blocks
each) and step its amplitude from frame to frame across the limit of every column; the CPU part
proves, with the integer row pass, that each sweep holds chunks just inside and just outside
every column's limit.  The expected bytes are the oracle's alone.
"""
import numpy as np
import pytest

from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes, split_i420
from test_gpu_parity import first_diff, oracle_frames
from test_kernel_arith import _skip_limits, pass1_int, range_int

W, H = 1024, 16
QS = (2, 5, 12)
FAMILIES = ("rows_equal", "rows_alternate")
NSWEEP = 64  # frames of one sweep; frame i carries amplitude step i (max|u| up to ~900)
# Block (in coding order) that carries chunk k's pattern, lanes 5, 17, 40, 63, 0 and 30: a mix
# of Y, U and V blocks (b % 6: 5, 3, 0, 3, 4, 2).  Chunk k sweeps the sign pattern of column k + 2.
OFFS = (5, 17, 40, 63, 0, 30)
# One amplitude step moves one pixel by one level; tv->pc maps a level onto at most two, and a
# pixel weighs at most 11363 / 512 < 22.2 in a row-pass output (16 in output 4): a step moves
# max|u| by less than 2 * 22.2 + 1.  "Just" inside / outside the limit is within TOL of it.
TOL = 46


def limit(q, col):
    rmax, amax = _skip_limits(q, col)
    return min(amax, rmax // 2)


def sign_pattern(c):
    x = np.arange(8)
    return np.where(np.cos((2 * x + 1) * c * np.pi / 16) >= 0, 1, -1)


def patterned_block(c, t, family):
    """base + e(x) s_c(x) with e = t // 8 (+ 1 on the first t % 8 pixels): amplitude in eighths."""
    e = t // 8 + (np.arange(8) < t % 8)
    row = e * sign_pattern(c)
    rows = np.tile(row, (8, 1))
    if family == "rows_alternate":
        rows[1::2] *= -1
    return np.clip(128 + rows, 0, 255).astype(np.uint8)


def put_block(frame, w, h, b, blk):
    """Write an 8x8 block at coding-order position b of a 4:2:0 frame."""
    y, u, v = split_i420(frame, w, h)
    mbw = (w + 15) // 16
    m, j = divmod(b, 6)
    mx, my = m % mbw, m // mbw
    if j < 4:
        y[my * 16 + 8 * (j >> 1):, mx * 16 + 8 * (j & 1):][:8, :8] = blk
    else:
        (u if j == 4 else v)[my * 8:, mx * 8:][:8, :8] = blk


def get_block(frame, w, h, b):
    y, u, v = split_i420(frame, w, h)
    mbw = (w + 15) // 16
    m, j = divmod(b, 6)
    mx, my = m % mbw, m // mbw
    if j < 4:
        return y[my * 16 + 8 * (j >> 1):, mx * 16 + 8 * (j & 1):][:8, :8], False
    return (u if j == 4 else v)[my * 8:, mx * 8:][:8, :8], True


_SWEEPS = {}


def sweep_frames(family):
    key = family
    if key not in _SWEEPS:
        frames = np.full((NSWEEP, i420_frame_bytes(W, H)), 128, np.uint8)
        for i in range(NSWEEP):
            for k, o in enumerate(OFFS):
                put_block(frames[i], W, H, 64 * k + o, patterned_block(k + 2, i, family))
        frames.setflags(write=False)
        _SWEEPS[key] = frames
    return _SWEEPS[key]


def chunk_maxima(frames, full):
    """max|u_c| per (frame, chunk, column): the flat blocks give 0 in columns 1-7."""
    out = np.zeros((len(frames), len(OFFS), 8), np.int64)
    for i, f in enumerate(frames):
        for k, o in enumerate(OFFS):
            blk, chroma = get_block(f, W, H, 64 * k + o)
            p = blk.astype(np.int64)
            if not full:
                p = range_int(p, chroma)
            out[i, k] = np.abs(pass1_int(p)).max(0)
    return out


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("family", FAMILIES)
def test_sweep_straddles_every_limit(family, q, full):
    """A condition on the inputs: for every column 2-7 the sweep holds a chunk whose max|u| is
    within TOL below (or at) the limit and one within TOL above it."""
    mx = chunk_maxima(sweep_frames(family), full)
    for col in range(2, 8):
        a = limit(q, col)
        assert a > 0, (q, col)
        m = mx[:, :, col].reshape(-1)
        inside = m[(m <= a) & (m > 0)]
        outside = m[m > a]
        assert inside.size and inside.max() >= a - TOL, (family, q, full, col, a, inside.max() if inside.size else None)
        assert outside.size and outside.min() <= a + TOL, (family, q, full, col, a, outside.min() if outside.size else None)


def check(frames, w, h, q, full, huffman="default"):
    with MjpegEncoder(0, w, h, qscale=q, full_range=full, max_batch=len(frames), huffman=huffman) as enc:
        got = enc.encode(frames)
    ref = oracle_frames(frames, w, h, q, full, huffman=huffman)
    for i in range(len(frames)):
        assert got[i] == ref[i], (i, len(got[i]), len(ref[i]), first_diff(got[i], ref[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("family", FAMILIES)
def test_limit_sweep_matches_oracle(family, q, full):
    check(sweep_frames(family), W, H, q, full)


AW, AH = 1024, 48  # 1152 blocks: 18 chunks in one segment
PERIODS = (1, 2, 3, 5)
_ADAPT = []


def adaptive_frames():
    """One frame per period p: chunk k is flat (every column skippable) when (k // p) is even and
    carries a noise block (no column skippable) when it is odd.  The waves' skip state flips at
    every change, and skippable chunks that follow a detailed one wait for the fourth-chunk retest."""
    if not _ADAPT:
        rng = np.random.default_rng(7)
        frames = np.full((len(PERIODS), i420_frame_bytes(AW, AH)), 128, np.uint8)
        nchunks = (AW // 16) * (AH // 16) * 6 // 64
        assert nchunks >= 13
        for i, p in enumerate(PERIODS):
            for k in range(nchunks):
                if (k // p) & 1:
                    put_block(frames[i], AW, AH, 64 * k + int(rng.integers(0, 64)),
                              rng.integers(0, 256, (8, 8)).astype(np.uint8))
        frames.setflags(write=False)
        _ADAPT.append(frames)
    return _ADAPT[0]


@pytest.mark.gpu
@pytest.mark.parametrize("huffman", ["default", "optimal"])
@pytest.mark.parametrize("full", [True, False])
def test_alternating_chunks_match_oracle(full, huffman):
    check(adaptive_frames(), AW, AH, 5, full, huffman)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_limit_sweep_huffman_optimal(family):
    check(sweep_frames(family), W, H, 5, False, "optimal")
