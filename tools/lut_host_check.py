#!/usr/bin/env python3
"""k_lut_plane's body on the CPU: tools/stage_host.hip's lut (the kernel's __host__ __device__ body run
over every (workgroup, thread) of the launches api.hip plans: host_check.py) with AddressSanitizer and UBSan on the host side, and
compares its output with tests/eq_ref.py for every shape of tests/test_gpu_eq.py and
tests/test_gpu_eq_chain.py and a few smaller ones.  Slot "in": three frames into a second buffer, in place, and as segments of 1 + 3 + 1 and 1 + 1 + 2
+ 1 in allocations of their own, each one byte in; with permutation tables, with an identity Y and
with an identity U.  Slot "out": the picture of a padded canvas in place, where every byte outside it
must stay.  Every buffer is allocated at exactly its size, so a load or store outside a frame stops
the program.  --long walks 8x8 4:2:0 in one submit of 32,768 frames, where U and V get a launch each,
and five frames forced apart, and slot "out" on 32,768 padded canvases.  No GPU.

usage: python3 tools/lut_host_check.py [--keep] [--csrc DIR] [--long]"""
import sys

import numpy as np

from host_check import SHIFTS, run_check, split_arg
import eq_ref  # noqa: E402
from ffmpeg_distributed_amd.encoder import i420_frame_bytes  # noqa: E402

# tests/test_gpu_eq.py's frames (203x301: 301x203 behind a transpose; 36x20, 40x24, 24x16: the worker's), and smaller ones
SHAPES = [(9, 5, "420"), (33, 17, "444"), (130, 66, "420"), (4100, 5, "444"), (203, 301, "420"), (130, 66, "444"),
          (130, 66, "422"), (40, 24, "420"), (1, 1, "444"), (2, 2, "420"), (15, 1, "444"), (16, 1, "444"), (17, 3, "422"),
          (1030, 5, "420"),
          # tests/test_gpu_eq_chain.py's: planes past one workgroup (301x203: odd frame bytes; 208x562: eight workgroups)
          (301, 203, "420"), (256, 160, "420"), (256, 160, "444"), (208, 562, "444"), (197, 70, "444"), (260, 132, "420"),
          (500, 280, "420"), (200, 100, "444")]
# slot "out": (canvas w, h, format, px, py, picture w, h), each one a pad that check_config accepts (the place, the
# canvas and the picture multiples of the sub-sampling)
CANVASES = [(80, 48, "420", 6, 10, 64, 32), (80, 48, "444", 3, 5, 64, 32), (64, 32, "420", 0, 0, 64, 32),
            (32, 24, "420", 4, 4, 24, 16), (70, 40, "422", 2, 3, 30, 17), (40, 9, "444", 25, 2, 15, 7),
            (300, 20, "444", 1, 1, 290, 18),
            # tests/test_gpu_eq_chain.py's: spans past one workgroup (16 KB), strided (row ends 8 bytes apart; skipped
            # pieces; the chroma past one workgroup; odd offsets) and flat (301x203: frames at odd addresses)
            (208, 120, "444", 5, 7, 200, 100), (520, 300, "420", 12, 14, 500, 280), (540, 300, "420", 20, 14, 500, 280),
            (264, 136, "420", 70, 38, 130, 66), (203, 101, "444", 69, 35, 66, 33), (1040, 40, "422", 4, 1, 1000, 37),
            (256, 160, "444", 0, 0, 256, 160), (301, 203, "420", 0, 0, 301, 203), (197, 70, "444", 0, 0, 197, 70)]
SPLITS = [(1, 3, 1), (1, 1, 2, 1)]


def check(host, args):
    def run(frames, tabs, w, h, c, split=0, apart=0, inplace=0, canvas=()):
        fin, ftab, fout = (host.path(nm) for nm in ("in.bin", "tab.bin", "out.bin"))
        frames.tofile(fin)
        np.asarray(tabs, np.uint8).tofile(ftab)
        n = frames.shape[0]
        host.run("lut", [fin, ftab, fout, w, h, *SHIFTS[c], n, split_arg(split), apart, inplace, *canvas],
                 f"{w}x{h} {c} split {split} inplace {inplace} canvas {canvas}")
        return np.fromfile(fout, np.uint8).reshape(n, -1)

    rng = np.random.default_rng(11)
    perm = eq_ref.perm_tables(3)
    id_y = perm.copy()
    id_y[0] = eq_ref.IDENTITY
    id_u = perm.copy()
    id_u[1] = eq_ref.IDENTITY
    bad = 0
    if "--long" in args:
        w, h, c = 8, 8, "420"
        n = 32768
        base = rng.integers(0, 256, (61, i420_frame_bytes(w, h, c)), dtype=np.uint8)
        frames = base[np.arange(n) % 61]
        ok = [(run(frames, perm, w, h, c) == eq_ref.map_frames(frames, w, h, c, perm)).all(),
              (run(frames, id_u, w, h, c, inplace=1) == eq_ref.map_frames(frames, w, h, c, id_u)).all(),
              (run(frames[:5], perm, w, h, c, apart=1) == eq_ref.map_frames(frames[:5], w, h, c, perm)).all()]
        print(f"{w}x{h} {c} U, V apart: one submit of {n} {ok[0]}, in place with an identity U {ok[1]}, 5 frames forced apart {ok[2]}")
        bad += ok.count(False)
        # slot "out" (tests/test_gpu_long_stages.py's): the 8x8 picture at (4, 6) of a 16x16 canvas, V's offset no plane start
        cw, ch, px, py = 16, 16, 4, 6
        canv = rng.integers(0, 256, (61, i420_frame_bytes(cw, ch, c)), dtype=np.uint8)[np.arange(n) % 61]
        ok = (run(canv, perm, w, h, c, canvas=(cw, ch, px, py)) == eq_ref.map_picture(canv, cw, ch, c, px, py, w, h, perm)).all()
        print(f"out {w}x{h} at ({px},{py}) of {cw}x{ch} {c} U, V apart: one submit of {n} {ok}")
        bad += not ok
    for (w, h, c) in ([] if "--long" in args else SHAPES):
        fb = i420_frame_bytes(w, h, c)
        frames = rng.integers(0, 256, (5, fb), dtype=np.uint8)
        frames[3] = (np.arange(fb) * 3 % 256).astype(np.uint8)
        ok = []
        for tabs in (perm, id_y, id_u):
            want = eq_ref.map_frames(frames, w, h, c, tabs)
            ok.append((run(frames[:3], tabs, w, h, c) == want[:3]).all())
            ok.append((run(frames[:3], tabs, w, h, c, inplace=1) == want[:3]).all())
            for split in SPLITS:
                ok.append((run(frames, tabs, w, h, c, split=split) == want).all())
        print(f"in {w}x{h} {c}: " + ", ".join(
            f"{nm}: copy {o[0]} in place {o[1]} 1+3+1 {o[2]} 1+1+2+1 {o[3]}"
            for nm, o in zip(("perm", "identity Y", "identity U"), (ok[0:4], ok[4:8], ok[8:12]))))
        bad += ok.count(False)
    for (cw, ch, c, px, py, w, h) in ([] if "--long" in args else CANVASES):
        fb = i420_frame_bytes(cw, ch, c)
        frames = rng.integers(0, 256, (3, fb), dtype=np.uint8)    # (a random border: any byte written there shows)
        ok = []
        for tabs in (perm, id_y, id_u):
            want = eq_ref.map_picture(frames, cw, ch, c, px, py, w, h, tabs)
            ok.append((run(frames, tabs, w, h, c, canvas=(cw, ch, px, py)) == want).all())
        print(f"out {w}x{h} at ({px},{py}) of {cw}x{ch} {c}: perm {ok[0]}, identity Y {ok[1]}, identity U {ok[2]}")
        bad += ok.count(False)
    return bad


if __name__ == "__main__":
    sys.exit(run_check(check))
