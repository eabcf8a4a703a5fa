#!/usr/bin/env python3
"""k_cmat_frame's body on the CPU: tools/stage_host.hip's cmat (the kernel's __host__ __device__ body run
over every (workgroup, thread) of the launch api.hip plans: host_check.py) with AddressSanitizer and UBSan on the host side, and
compares its output with tests/colormatrix_ref.py for every shape of tests/test_gpu_colormatrix.py and a
few smaller ones: three frames into a second buffer, in place, and five frames as segments of 1 + 3 + 1
and 1 + 1 + 2 + 1 in allocations of their own, each one byte in; with bt709 -> bt601, bt601 -> bt709 and
the made-up matrix whose six coefficients all differ.  One plane of every case is drawn from {0..20,
235..255}, so both clips occur.  Every buffer is allocated at exactly its size, so a load or store
outside a frame stops the program.  --long walks 16x16 4:2:0 in one submit of 32,768 frames.  No GPU.

usage: python3 tools/cmat_host_check.py [--keep] [--csrc DIR] [--long]"""
import sys

import numpy as np

from host_check import run_check, split_arg
import colormatrix_ref as ref  # noqa: E402

# tests/test_gpu_colormatrix.py's frames (203x301: 301x203 behind a transpose; 40x24: the worker's), and smaller ones
SHAPES = [(33, 17, "420"), (33, 17, "444"), (34, 16, "422"), (8, 8, "420"), (301, 203, "420"), (4100, 6, "420"),
          (130, 66, "420"), (130, 66, "444"), (203, 301, "420"), (40, 24, "420"),
          (1, 1, "444"), (1, 1, "420"), (2, 2, "420"), (16, 1, "444"), (31, 3, "420"), (32, 2, "420"), (32, 3, "422"),
          (31, 2, "422"), (17, 3, "422"), (47, 5, "444"), (1030, 5, "420")]
SPLITS = [(1, 3, 1), (1, 1, 2, 1)]
MATRICES = [("bt709->bt601", ref.coefs("bt709", "bt601")), ("bt601->bt709", ref.coefs("bt601", "bt709")),
            ("made up", ref.MADE_UP)]


def check(host, args):
    def run(frames, c, w, h, fmt, split=0, inplace=0):
        fin, fout = host.path("in.bin"), host.path("out.bin")
        frames.tofile(fin)
        n = frames.shape[0]
        host.run("cmat", [fin, fout, w, h, *ref.SHIFTS[fmt], n, split_arg(split), inplace, *c],
                 f"{w}x{h} {fmt} split {split} inplace {inplace}")
        return np.fromfile(fout, np.uint8).reshape(n, -1)

    bad = 0
    if "--long" in args:      # tests/test_gpu_long_stages.py's: one launch of gxy * 32768 workgroups, the frame by a division
        w, h, fmt, n = 16, 16, "420", 32768
        frames = ref.noise_frames(w, h, fmt, 61, 1, seed=5)[np.arange(n) % 61]
        name, c = MATRICES[0]
        want = ref.convert_frames(frames, w, h, fmt, c)
        ok = [(run(frames, c, w, h, fmt) == want).all(), (run(frames, c, w, h, fmt, inplace=1) == want).all()]
        print(f"{w}x{h} {fmt} {n} frames {name}: copy {ok[0]} in place {ok[1]}", flush=True)
        return ok.count(False)
    for i, (w, h, fmt) in enumerate(SHAPES):
        frames = ref.noise_frames(w, h, fmt, 5, i % 3, seed=5)
        line = []
        for name, c in MATRICES:
            want = ref.convert_frames(frames, w, h, fmt, c)
            ok = [(run(frames[:3], c, w, h, fmt) == want[:3]).all(), (run(frames[:3], c, w, h, fmt, inplace=1) == want[:3]).all()]
            ok += [(run(frames, c, w, h, fmt, split=s) == want).all() for s in SPLITS]
            lo, hi = ref.clip_counts(frames, w, h, fmt, c)
            line.append(f"{name}: copy {ok[0]} in place {ok[1]} 1+3+1 {ok[2]} 1+1+2+1 {ok[3]} (clipped {lo} low, {hi} high)")
            bad += ok.count(False)
        print(f"{w}x{h} {fmt}: " + ", ".join(line), flush=True)
    return bad


if __name__ == "__main__":
    sys.exit(run_check(check))
