#!/usr/bin/env python3
"""k_dn_rows, k_dn_cols and k_dn_time's bodies on the CPU: tools/stage_host.hip's hqdn3d (the kernels'
__host__ __device__ steps, split at their barriers, run over every (workgroup, thread) of the launches that
api.hip's plan_ctx and dn_launch give: host_check.py) with AddressSanitizer and UBSan on the host side,
compared byte for byte, frames and carried state, with tests/hqdn3d_ref.py for every shape and content of
tests/test_gpu_hqdn3d.py and a few more: one sample, one row, one column, planes of exactly one tile and of
one tile and a sample, 128 and 129 rows (one workgroup of k_dn_rows and one row more), 512 and 513 columns
(one workgroup of k_dn_cols and one column more).  Each shape runs as one submit with the frames 0, 1 and 9
bytes into their allocation (the time scan cuts its pieces on the destination's alignment), as continued
submits of 2 + 3 and of 1 + 1 + 3 frames, as one submit of two segments (two sequences) in allocations of
their own, and as the same two segments in one buffer with their starts kept, which is what the denoiser gets
behind a deinterlacer.  Every buffer is
allocated at exactly its size, so a load or store outside it stops the program.  --long walks 8x8 4:2:0 in one
submit of 32,768 frames one byte in, and 38,000 frames as four segments in one buffer (12345, 20422, 3000, 2233:
the third starts at frame 32767), where U and V get a launch each (tests/test_gpu_long_stages.py's).  No GPU.

usage: python3 tools/hqdn3d_host_check.py [--keep] [--csrc DIR] [--long]   (--csrc: the sources from DIR, a changed
copy of ffmpeg_distributed_amd/csrc)"""
import sys

import numpy as np

from host_check import SHIFTS, run_check, split_arg
import hqdn3d_ref  # noqa: E402

MORE = [
    (1, 1, "444"),
    (70, 1, "444"),
    (1, 70, "444"),
    (64, 64, "444"),
    (65, 65, "444"),
    (20, 128, "444"),
    (20, 129, "422"),
    (512, 3, "444"),
    (513, 3, "420"),
]


def check(host, args):
    tabs = np.stack(hqdn3d_ref.tables(*hqdn3d_ref.STRENGTHS))
    ftab = host.path("tabs.bin")
    tabs.astype(np.int16).tofile(ftab)

    def run(frames, w, h, c, segs, lead, chunks, behind=0):
        fin, fout, fst = host.path("in.bin"), host.path("out.bin"), host.path("state.bin")
        frames.tofile(fin)
        host.run("hqdn3d", [fin, ftab, fout, fst, w, h, *SHIFTS[c], len(frames), split_arg(segs), lead, split_arg(chunks),
                                behind],
                 f"{w}x{h} {c} {len(frames)} frames segments {segs} lead {lead} submits {chunks} behind {behind}")
        return np.fromfile(fout, np.uint8).reshape(len(frames), -1), np.fromfile(fst, np.uint16)

    bad = 0
    if "--long" in args:      # tests/test_gpu_long_stages.py's shapes: from 32,768 frames on U and V get a launch each
        import chain_geom as cg
        w, h, c = 8, 8, "420"
        base = np.random.default_rng(5).integers(88, 113, (cg.LONG_K, hqdn3d_ref.frame_bytes(w, h, c)), dtype=np.uint8)
        for n, segs, lead, behind in ((cg.LONG, None, 1, 0), (38000, (12345, 20422, 3000, 2233), 1, 1)):
            idx = cg.long_frame_index(n)
            cuts = np.cumsum((0,) + (segs or (n,)))
            want, wst = hqdn3d_ref.denoise_indexed(base, idx, w, h, c, tabs, [(int(a), int(b - a)) for a, b in zip(cuts, cuts[1:])])
            got, gst = run(base[idx], w, h, c, segs, lead, None, behind)
            ok = got.shape == want.shape and bool((got == want).all()) and gst.size == wst.size and bool((gst == wst).all())
            print(f"{w}x{h} {c} {n} frames, U and V apart, segments {segs} lead {lead} in one buffer {behind}: {ok}", flush=True)
            bad += not ok
        return bad
    n = hqdn3d_ref.NFRAMES
    for (w, h, c) in hqdn3d_ref.GPU_SHAPES + MORE:
        for kind in hqdn3d_ref.CONTENTS:
            frames = hqdn3d_ref.make_frames(kind, w, h, c, n, 5)
            want, wst = hqdn3d_ref.denoise(frames, w, h, c, tabs)
            a, _ = hqdn3d_ref.denoise(frames[:3], w, h, c, tabs)
            b, bst = hqdn3d_ref.denoise(frames[3:], w, h, c, tabs)
            two = np.concatenate([a, b])
            ok = []
            for segs, lead, chunks, behind, (ref, rst) in ((None, 0, None, 0, (want, wst)), (None, 1, None, 0, (want, wst)),
                                                           (None, 9, None, 0, (want, wst)), (None, 0, (2, 3), 0, (want, wst)),
                                                           (None, 3, (1, 1, 3), 0, (want, wst)), ((3, 2), 5, None, 0, (two, bst)),
                                                           ((3, 2), 7, None, 1, (two, bst))):
                got, gst = run(frames, w, h, c, segs, lead, chunks, behind)
                ok.append(got.shape == ref.shape and bool((got == ref).all()) and gst.size == rst.size
                          and bool((gst == rst).all()))
            print(f"{w}x{h} {c} {n} frames {kind}: lead 0 {ok[0]}, 1 {ok[1]}, 9 {ok[2]}, submits 2+3 {ok[3]}, "
                  f"1+1+3 at lead 3 {ok[4]}, segments 3+2 at lead 5 {ok[5]}, in one buffer at lead 7 {ok[6]}")
            bad += ok.count(False)
    return bad


if __name__ == "__main__":
    sys.exit(run_check(check))
