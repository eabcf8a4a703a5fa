#!/usr/bin/env python3
"""k_yadif_plane's body on the CPU: builds tools/yadif_host.hip (the kernel's __host__ __device__ body
run over every (workgroup, thread) of its launches) with AddressSanitizer and UBSan on the host
side, and compares its output with tests/yadif_ref.py for every shape of the GPU tests and a few
smaller ones, both parities, both modes: one submit of 5 frames, the same frames as halo submits of
2 + 2 + 1, and as two segments of 3 + 2.  The source and destination buffers are allocated at
exactly their sizes, so a load or store outside a readable frame stops the program.  No GPU.

usage: python3 tools/yadif_host_check.py [--keep]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yadif_ref import deint_frames  # noqa: E402
from ffmpeg_distributed_amd.encoder import i420_frame_bytes  # noqa: E402

SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
SHAPES = [(130, 66, "420"), (131, 67, "420"), (130, 66, "422"), (33, 17, "444"), (6, 6, "420"), (20, 8, "444"),
          (4100, 5, "444"), (3, 3, "444"), (16, 3, "444"), (19, 4, "444"), (40, 7, "420")]


def main():
    tmp = tempfile.mkdtemp(prefix="yadif_host_")
    exe = os.path.join(tmp, "yadif_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-omit-frame-pointer", "-Wno-pass-failed", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "ffmpeg_distributed_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "yadif_host.hip")], check=True)

    def run(frames, w, h, c, mode, tff, n, halo, split):
        hs, vs = SHIFTS[c]
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        frames.tofile(fin)
        r = subprocess.run([exe, fin, fout, str(w), str(h), str(hs), str(vs), str(1 if mode == 2 else 0), str(tff ^ 1),
                            str(n), str(halo), str(split)], capture_output=True, text=True)
        if r.returncode:
            sys.exit(f"yadif_host failed ({r.returncode}) at {w}x{h} {c} mode {mode} tff {tff} halo {halo} split {split}:\n"
                     + r.stderr[-4000:])
        return np.fromfile(fout, np.uint8).reshape(n, -1)

    rng = np.random.default_rng(5)
    bad = 0
    for (w, h, c) in SHAPES:
        fb = i420_frame_bytes(w, h, c)
        frames = rng.integers(0, 256, (5, fb), dtype=np.uint8)
        frames[3] = (np.arange(fb) * 3 % 256).astype(np.uint8)
        for tff in (1, 0):
            for mode in (0, 2):
                want = deint_frames(frames, w, h, c, mode, tff)
                one = run(frames, w, h, c, mode, tff, 5, 0, 0)
                halo = np.concatenate([run(frames[0:3], w, h, c, mode, tff, 2, 2, 0), run(frames[1:5], w, h, c, mode, tff, 2, 3, 0),
                                       run(frames[3:5], w, h, c, mode, tff, 1, 1, 0)])
                segs = run(frames, w, h, c, mode, tff, 5, 0, 3)
                want_segs = np.concatenate([deint_frames(frames[:3], w, h, c, mode, tff),
                                            deint_frames(frames[3:], w, h, c, mode, tff)])
                ok = [(one == want).all(), (halo == want).all(), (segs == want_segs).all()]
                print(f"{w}x{h} {c} {'tff' if tff else 'bff'} mode {mode}: one submit {ok[0]}, halo 2+2+1 {ok[1]}, "
                      f"segments 3+2 {ok[2]}")
                bad += ok.count(False)
    if "--keep" not in sys.argv:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)
    print("all equal" if not bad else f"{bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
