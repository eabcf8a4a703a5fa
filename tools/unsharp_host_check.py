#!/usr/bin/env python3
"""k_unsharp_plane's body on the CPU: tools/stage_host.hip's unsharp (the kernel's __host__ __device__
steps and address arithmetic run over every (workgroup, thread, iteration) of the launches api.hip plans: host_check.py) with
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

usage: python3 tools/unsharp_host_check.py [--keep] [--csrc DIR] [--sweep | --long]"""
import sys

import numpy as np

from host_check import SHIFTS, run_check, split_arg
from unsharp_ref import GPU_GEOMETRY, GPU_GEOMETRY_CHAIN, amount_i, unsharp_planes  # noqa: E402
from pad_ref import pad_planes  # noqa: E402
from ffmpeg_distributed_amd.encoder import chroma_size, pack_i420  # noqa: E402

EXTRA = [(3, 3, "444", 0, 0, 3, 3, (23, 3, 1.0, 3, 23, -2.0)), (17, 9, "422", 0, 0, 17, 9, (5, 5, 0.3, 5, 5, 0.3)),
         (132, 34, "422", 2, 1, 128, 32, (7, 19, 5.0, 5, 5, 1.0)), (66, 70, "420", 64, 32, 2, 38, (5, 5, 1.0, 9, 3, 1.0)),
         (40, 24, "444", 0, 0, 40, 24, (23, 23, 0.0, 3, 3, 1.0))]


def check(host, args):
    def run(src, PW, PH, c, px, py, w, h, us, n, apart):
        fin, fout = host.path("in.bin"), host.path("out.bin")
        src.tofile(fin)
        ints = (us[0], us[1], amount_i(us[2]), us[3], us[4], amount_i(us[5]))
        out = host.run("unsharp", [fin, fout, PW, PH, *SHIFTS[c], px, py, w, h, *ints, n, apart],
                       f"{PW}x{PH} {c} picture {w}x{h}+{px}+{py} {us} {n} frames apart {apart}")
        return np.fromfile(fout, np.uint8).reshape(n, -1), out.strip()

    rng = np.random.default_rng(7)
    bad = 0
    geoms = GPU_GEOMETRY + GPU_GEOMETRY_CHAIN + EXTRA
    if "--sweep" in args:
        import chain_geom as cg
        cfgs = cg.filter_sweep_configs(cg.FILTER_SWEEP_SEED, 120)
        geoms = [(*cg.encoded_geometry(k)[:2], k.dst, *cg.encoded_geometry(k)[2:], k.unsharp) for k in cfgs if k.unsharp]
    if "--long" in args:
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
            cw, ch = chroma_size(w, h, c)
            pics = [[rng.integers(0, 256, (hh, ww), dtype=np.uint8) for ww, hh in ((w, h), (cw, ch), (cw, ch))]
                    for _ in range(cg.LONG_K)]
            padded = (px, py, w, h) != (0, 0, PW, PH)
            place = (lambda pl: pad_planes(*pl, c, px, py, PW, PH)) if padded else (lambda pl: pl)
            src = np.stack([pack_i420(*place(pl)) for pl in pics])[idx]
            want = np.stack([pack_i420(*place(unsharp_planes(*pl, us))) for pl in pics])[idx]
            got, counts = run(src, PW, PH, c, px, py, w, h, us, n, 0)
            ok = bool((got == want).all())
            print(f"{PW}x{PH} {c} picture {w}x{h}+{px}+{py} unsharp {':'.join(str(v) for v in us)} {n} frames, U, V apart: "
                  f"equal {ok}; {counts}")
            bad += not ok
        geoms = []
    for (PW, PH, c, px, py, w, h, us) in geoms:
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
        for split in (0, 1):
            got, counts = run(src, PW, PH, c, px, py, w, h, us, 2, split)
            ok = bool((got == want).all())
            print(f"{PW}x{PH} {c} picture {w}x{h}+{px}+{py} unsharp {':'.join(str(v) for v in us)} "
                  f"{'U, V apart' if split else 'U + V paired'}: equal {ok}; {counts}")
            bad += not ok
    return bad


if __name__ == "__main__":
    sys.exit(run_check(check))
