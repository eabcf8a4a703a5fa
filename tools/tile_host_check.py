#!/usr/bin/env python3
"""k_tile_plane's body on the CPU: tools/stage_host.hip's tile (the kernel's __host__ __device__ body run over
every (workgroup, thread) of the launches api.hip plans: host_check.py) with AddressSanitizer and UBSan on the host side, and compares
its sheets with tests/tile_ref.py for every geometry of tests/test_gpu_tile.py (tile_ref.GPU_GEOMETRY) and
a few more: cells of one sample, cells of exactly 16 and of 17 bytes a row, one column, one row, a margin
wider than a piece, a padding of a piece and more, N = 1.  Each geometry runs with the buffers at three
alignments (the pieces are cut on the sheet plane's alignment) and once with U and V in a launch each.
Every buffer is allocated at exactly its size, so a load or store outside the frames stops the program.
--long walks tests/test_gpu_long_stages.py's shapes of 32,768 sheets and more, where the library's own rule
launches U and V apart.  No GPU.

usage: python3 tools/tile_host_check.py [--keep] [--csrc DIR] [--long]   (--csrc: the sources from DIR, a changed
copy of ffmpeg_distributed_amd/csrc: the recorded mutations of profiles/tile/mutations.txt)"""
import sys

import numpy as np

from host_check import SHIFTS, run_check, split_arg
import tile_ref  # noqa: E402
from ffmpeg_distributed_amd.encoder import i420_frame_bytes, split_i420  # noqa: E402

MORE = [
    (1, 1, "444", (3, 2, 0, 0, 0), (7,)),
    (2, 2, "420", (9, 1, 0, 2, 2), (9, 1)),
    (16, 4, "444", (3, 2, 4, 0, 0), (9,)),
    (17, 3, "444", (2, 3, 0, 1, 1), (5, 6)),
    (32, 6, "422", (1, 4, 0, 0, 2), (3,)),
    (20, 4, "444", (4, 1, 0, 19, 0), (4,)),
    (24, 8, "420", (2, 2, 0, 32, 16), (3, 4, 1, 2)),
    (48, 8, "420", (2, 2, 1, 0, 18), (3,)),
    (300, 20, "444", (2, 3, 5, 7, 33), (11,)),
]
# --long: one frame a sheet at 32,768 frames; 65,535 frames on 32,768 sheets, the last partial; four segments whose
# last starts at sheet 32767
LONG = [
    (8, 8, "420", (2, 1, 1, 0, 0), (32768,)),
    (8, 8, "420", (2, 1, 0, 0, 0), (65535,)),
    (8, 8, "420", (2, 1, 0, 0, 0), (12345, 20421, 32765, 3)),
]


def check(host, args):
    def run(frames, w, h, c, sheet, segs, apart, shift):
        fin, fout = host.path("in.bin"), host.path("out.bin")
        frames.tofile(fin)
        host.run("tile", [fin, fout, w, h, *SHIFTS[c], *tile_ref.resolve(sheet), split_arg(segs), apart, shift],
                 f"{w}x{h} {c} sheet {sheet} segments {segs} apart {apart} shift {shift}")
        return np.fromfile(fout, np.uint8)

    rng = np.random.default_rng(17)
    bad = 0
    if "--long" in args:      # tests/test_gpu_long_stages.py's regimes A and C and its segments: 32,768 sheets and more, so
        #                       the library's own rule launches U and V apart (apart 0)
        for (w, h, c, sheet, segs) in LONG:
            n = sum(segs)
            base = rng.integers(1, 256, (61, i420_frame_bytes(w, h, c)), dtype=np.uint8)
            base[:, w * h:][base[:, w * h:] == 128] = 127
            i = np.arange(n)
            frames = base[(7 * i + i // 1000) % 61]
            want, at = [], 0
            for k in segs:
                cells = [split_i420(f, w, h, c) for f in frames[at:at + k]]
                want += [tile_ref.pack(s) for s in tile_ref.sheets_numpy(cells, w, h, c, sheet)]
                at += k
            want = np.concatenate(want)
            ok = []
            for shift in (0, 1):
                got = run(frames, w, h, c, sheet, segs, 0, shift)
                ok.append(got.size == want.size and bool((got == want).all()))
            m = sum(tile_ref.frames_out(k, sheet) for k in segs)
            print(f"{w}x{h} {c} sheet {sheet}, segments {segs}: {n} frames on {m} sheets, U and V apart: shift 0 {ok[0]}, 1 {ok[1]}",
                  flush=True)
            bad += ok.count(False)
        return bad
    for (w, h, c, sheet, segs) in tile_ref.GPU_GEOMETRY + MORE:
        n = sum(segs)
        frames = rng.integers(1, 256, (n, i420_frame_bytes(w, h, c)), dtype=np.uint8)  # (no 0: a blank luma byte shows)
        frames[:, w * h:][frames[:, w * h:] == 128] = 127                               # (nor a blank chroma byte)
        want, at = [], 0
        for k in segs:
            cells = [split_i420(f, w, h, c) for f in frames[at:at + k]]
            want += [tile_ref.pack(s) for s in tile_ref.sheets_numpy(cells, w, h, c, sheet)]
            at += k
        want = np.concatenate(want)
        ok = []
        for apart, shift in ((0, 0), (0, 1), (0, 9), (1, 0)):
            got = run(frames, w, h, c, sheet, segs, apart, shift)
            ok.append(got.size == want.size and bool((got == want).all()))
        W, H = tile_ref.sheet_size(w, h, sheet)
        print(f"{w}x{h} {c} sheet {sheet} -> {W}x{H}, segments {segs}: shift 0 {ok[0]}, 1 {ok[1]}, 9 {ok[2]}, U and V apart {ok[3]}")
        bad += ok.count(False)
    return bad


if __name__ == "__main__":
    sys.exit(run_check(check))
