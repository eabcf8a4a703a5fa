#!/usr/bin/env python3
"""k_unsharp_plane's body on the CPU: builds tools/unsharp_host.hip (the kernel's __host__ __device__
steps and address arithmetic run over every (workgroup, thread, iteration) of its launches) with
AddressSanitizer and UBSan on the host side, for the encoded geometry of every GPU test
(tests/unsharp_ref.py GPU_GEOMETRY and GPU_GEOMETRY_CHAIN) and a few smaller ones: two frames, U and V in one launch and in
one each.  The program itself asserts that every staged load lies inside the picture rectangle and
that every byte of every plane is stored exactly once, on buffers allocated at exactly the frames'
size; this script compares its output with tests/unsharp_ref.py.  --sweep walks instead the encoded
geometry of every sharpened configuration of the seeded sweep (tests/chain_geom.py
filter_sweep_configs, tests/test_gpu_filter_chain.py).  --long walks the sharpened geometries of
tests/test_gpu_long_submit.py at 32,770 frames, where U and V get a launch each (poff 0, V's off
advanced by the chroma plane, frame indices 32,767 and 32,768); the frames cycle through 61 pictures
as in that file.  No GPU.

usage: python3 tools/unsharp_host_check.py [--keep] [--sweep | --long]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from unsharp_ref import GPU_GEOMETRY, GPU_GEOMETRY_CHAIN, amount_i, unsharp_planes  # noqa: E402
from pad_ref import pad_planes  # noqa: E402
from ffmpeg_distributed_amd.encoder import chroma_size, pack_i420  # noqa: E402

SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
EXTRA = [(3, 3, "444", 0, 0, 3, 3, (23, 3, 1.0, 3, 23, -2.0)), (17, 9, "422", 0, 0, 17, 9, (5, 5, 0.3, 5, 5, 0.3)),
         (132, 34, "422", 2, 1, 128, 32, (7, 19, 5.0, 5, 5, 1.0)), (66, 70, "420", 64, 32, 2, 38, (5, 5, 1.0, 9, 3, 1.0)),
         (40, 24, "444", 0, 0, 40, 24, (23, 23, 0.0, 3, 3, 1.0))]


def main():
    tmp = tempfile.mkdtemp(prefix="unsharp_host_")
    exe = os.path.join(tmp, "unsharp_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-omit-frame-pointer", "-Wno-pass-failed", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "ffmpeg_distributed_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "unsharp_host.hip")], check=True)
    rng = np.random.default_rng(7)
    bad = 0
    geoms = GPU_GEOMETRY + GPU_GEOMETRY_CHAIN + EXTRA
    if "--sweep" in sys.argv:
        import chain_geom as cg
        cfgs = cg.filter_sweep_configs(cg.FILTER_SWEEP_SEED, 120)
        geoms = [(*cg.encoded_geometry(k)[:2], k.dst, *cg.encoded_geometry(k)[2:], k.unsharp) for k in cfgs if k.unsharp]
    if "--long" in sys.argv:
        import chain_geom as cg
        geoms = []
        for name in ("unsharp55", "unsharp_chroma", "chain"):      # (scale_sharp encodes unsharp55's geometry)
            k = cg.LONG_CASES[name]
            ow, oh = (k.h, k.w) if k.orient & 1 else (k.w, k.h)
            pw, ph = k.dw or (k.rect[2] if k.rect else ow), k.dh or (k.rect[3] if k.rect else oh)
            geoms.append((k.pad[2], k.pad[3], k.dst, k.pad[0], k.pad[1], pw, ph, k.unsharp) if k.pad
                         else (pw, ph, k.dst, 0, 0, pw, ph, k.unsharp))
        n = cg.LONG + 2
        assert len(cg.plane_launches(n)) == 3
        idx = cg.long_frame_index(n)
        for (PW, PH, c, px, py, w, h, us) in geoms:
            hs, vs = SHIFTS[c]
            cw, ch = chroma_size(w, h, c)
            pics = [[rng.integers(0, 256, (hh, ww), dtype=np.uint8) for ww, hh in ((w, h), (cw, ch), (cw, ch))]
                    for _ in range(cg.LONG_K)]
            padded = (px, py, w, h) != (0, 0, PW, PH)
            place = (lambda pl: pad_planes(*pl, c, px, py, PW, PH)) if padded else (lambda pl: pl)
            src = np.stack([pack_i420(*place(pl)) for pl in pics])[idx]
            want = np.stack([pack_i420(*place(unsharp_planes(*pl, us))) for pl in pics])[idx]
            ints = (us[0], us[1], amount_i(us[2]), us[3], us[4], amount_i(us[5]))
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            src.tofile(fin)
            r = subprocess.run([exe, fin, fout] + [str(v) for v in (PW, PH, hs, vs, px, py, w, h, *ints, n, 0)],
                               capture_output=True, text=True)
            if r.returncode:
                sys.exit(f"unsharp_host failed ({r.returncode}) at {PW}x{PH} {c} picture {w}x{h}+{px}+{py} {us} {n} frames:\n"
                         + r.stderr[-4000:])
            ok = bool((np.fromfile(fout, np.uint8).reshape(n, -1) == want).all())
            print(f"{PW}x{PH} {c} picture {w}x{h}+{px}+{py} unsharp {':'.join(str(v) for v in us)} {n} frames, U, V apart: "
                  f"equal {ok}; {r.stdout.strip()}")
            bad += not ok
        geoms = []
    for (PW, PH, c, px, py, w, h, us) in geoms:
        hs, vs = SHIFTS[c]
        cw, ch = chroma_size(w, h, c)
        pics = []
        for k in range(2):   # noise with saturated patches, then a noisy ramp
            if k == 0:
                pl = [rng.integers(0, 256, (hh, ww), dtype=np.uint8) for ww, hh in ((w, h), (cw, ch), (cw, ch))]
                for p in pl:
                    p[: p.shape[0] // 2, : p.shape[1] // 2] = 255
            else:
                pl = [((np.add.outer(3 * np.arange(hh), 5 * np.arange(ww)) + rng.integers(0, 9, (hh, ww))) % 256).astype(np.uint8)
                      for ww, hh in ((w, h), (cw, ch), (cw, ch))]
            pics.append(pl)
        padded = (px, py, w, h) != (0, 0, PW, PH)
        place = (lambda pl: pad_planes(*pl, c, px, py, PW, PH)) if padded else (lambda pl: pl)
        src = np.stack([pack_i420(*place(pl)) for pl in pics])
        want = np.stack([pack_i420(*place(unsharp_planes(*pl, us))) for pl in pics])
        ints = (us[0], us[1], amount_i(us[2]), us[3], us[4], amount_i(us[5]))
        for split in (0, 1):
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            src.tofile(fin)
            r = subprocess.run([exe, fin, fout] + [str(v) for v in (PW, PH, hs, vs, px, py, w, h, *ints, 2, split)],
                               capture_output=True, text=True)
            if r.returncode:
                sys.exit(f"unsharp_host failed ({r.returncode}) at {PW}x{PH} {c} picture {w}x{h}+{px}+{py} {us} split {split}:\n"
                         + r.stderr[-4000:])
            got = np.fromfile(fout, np.uint8).reshape(2, -1)
            ok = bool((got == want).all())
            print(f"{PW}x{PH} {c} picture {w}x{h}+{px}+{py} unsharp {':'.join(str(v) for v in us)} "
                  f"{'U, V apart' if split else 'U + V paired'}: equal {ok}; {r.stdout.strip()}")
            bad += not ok
    if "--keep" not in sys.argv:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)
    print("all equal" if not bad else f"{bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
