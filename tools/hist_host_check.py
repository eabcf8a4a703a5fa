#!/usr/bin/env python3
"""k_frame_hist's body on the CPU: tools/stage_host.hip's hist (the kernel's two __host__ __device__ steps run
over every (workgroup, thread) of the launch that api.hip's hist_plan gives: host_check.py) with
AddressSanitizer and UBSan on the host side, compared with np.bincount per plane (tests/thumbnail_ref.py) for
every shape and content of tests/test_gpu_thumbnail.py and a few more: one sample, planes of exactly one
piece and of one piece and a byte, planes of exactly one and two workgroups' bytes and of one byte less.  Each shape
runs with the frames 0, 1 and 9 bytes into their allocation (the pieces are cut on the source's alignment)
and once as two segments in allocations of their own.  Every buffer is allocated at exactly its size, so a
load outside the frames stops the program.  --long walks one call of 33,000 frames of 8x8 4:2:0.  No GPU.

usage: python3 tools/hist_host_check.py [--keep] [--csrc DIR] [--long]   (--csrc: the sources from DIR, a changed
copy of ffmpeg_distributed_amd/csrc)"""
import sys

import numpy as np

from host_check import SHIFTS, run_check, split_arg
import thumbnail_ref  # noqa: E402

MORE = [
    (1, 1, "420", 2),
    (16, 1, "444", 3),
    (17, 1, "444", 3),
    (128, 128, "444", 2),   # 16384 bytes a plane: one workgroup exactly (behind a head: one piece less and a tail)
    (129, 127, "444", 2),   # 16383
    (16384, 2, "422", 2),    # two workgroups exactly, chroma one
]


def check(host, args):
    def run(frames, w, h, c, segs, lead):
        fin, fout = host.path("in.bin"), host.path("out.bin")
        frames.tofile(fin)
        host.run("hist", [fin, fout, w, h, *SHIFTS[c], len(frames), split_arg(segs), lead],
                 f"{w}x{h} {c} {len(frames)} frames segments {segs} lead {lead}")
        return np.fromfile(fout, np.uint32)

    bad = 0
    if "--long" in args:      # tests/test_gpu_long_stages.py's: 33,000 frames of 8x8 4:2:0 in one call, t up to 98,999
        w, h, c, n = 8, 8, "420", 33000
        base = thumbnail_ref.make_frames("noise", w, h, c, 61, 5)
        i = np.arange(n)
        idx = (7 * i + i // 1000) % 61
        want = thumbnail_ref.hist_ref(base, w, h, c)[idx].reshape(-1)
        got = run(base[idx], w, h, c, None, 1)
        ok = got.size == want.size and bool((got == want).all())
        print(f"{w}x{h} {c} {n} frames at lead 1, {thumbnail_ref.hist_gpf(w, h, c)} workgroups a frame: {ok}")
        return int(not ok)
    for (w, h, c, n) in thumbnail_ref.GPU_SHAPES + MORE:
        for kind in thumbnail_ref.CONTENTS:
            frames = thumbnail_ref.make_frames(kind, w, h, c, n, 5)
            want = thumbnail_ref.hist_ref(frames, w, h, c).reshape(-1)
            ok = []
            for segs, lead in ((None, 0), (None, 1), (None, 9), ((1, n - 1), 3)):
                got = run(frames, w, h, c, segs, lead)
                ok.append(got.size == want.size and bool((got == want).all()))
            print(f"{w}x{h} {c} {n} frames {kind}: lead 0 {ok[0]}, 1 {ok[1]}, 9 {ok[2]}, two segments at lead 3 {ok[3]}")
            bad += ok.count(False)
    return bad


if __name__ == "__main__":
    sys.exit(run_check(check))
