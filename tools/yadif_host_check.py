#!/usr/bin/env python3
"""k_yadif_plane's body on the CPU: tools/stage_host.hip's yadif (the kernel's __host__ __device__ body
run over every (workgroup, thread) of the launches api.hip plans: host_check.py) with AddressSanitizer and UBSan on the host
side, and compares its output with tests/yadif_ref.py for every shape of the GPU tests and a few
smaller ones, both parities, both modes: one submit of 5 frames, the same frames as halo submits of
2 + 2 + 1, and as segments of their own in one launch: 3 + 2, 1 + 3 + 1 (a one-frame segment
between others) and 1 + 1 + 2 + 1 (kMaxSegs segments), the splits of tests/test_gpu_yadif.py and
tests/test_gpu_filter_chain.py; the shapes of the latter's cases are in the list too.  The source and destination buffers are allocated at
exactly their sizes, so a load or store outside a readable frame stops the program.  --sweep walks
instead every deinterlaced configuration of the seeded sweep (tests/chain_geom.py
filter_sweep_configs): its source shape, mode and parity, three frames in one submit and as
segments of 2 + 1.  --long walks the deinterlaced shapes of tests/test_gpu_long_submit.py past 32,767
frames, where U and V get a launch each (poff 0, off advanced by the chroma plane, frame indices
32,767 and 32,768): one submit of 32,770 frames, a halo submit of 32,770 out of 32,772, and four
segments of 38,000 with a boundary at frame 32,767; the frames cycle through 61 base frames as in
that file, so the reference is made once per distinct (prev, cur, next).  No GPU.

usage: python3 tools/yadif_host_check.py [--keep] [--csrc DIR] [--sweep | --long]"""
import sys

import numpy as np

from host_check import SHIFTS, run_check, split_arg
from yadif_ref import deint_frame, deint_frames  # noqa: E402
from ffmpeg_distributed_amd.encoder import i420_frame_bytes  # noqa: E402

SHAPES = [(130, 66, "420"), (131, 67, "420"), (130, 66, "422"), (33, 17, "444"), (6, 6, "420"), (20, 8, "444"),
          (4100, 5, "444"), (3, 3, "444"), (16, 3, "444"), (19, 4, "444"), (40, 7, "420"),
          (256, 160, "420"), (256, 160, "444"), (130, 66, "444"), (301, 203, "420")]      # tests/test_gpu_filter_chain.py
SPLITS = [(3, 2), (1, 3, 1), (1, 1, 2, 1)]


def check(host, args):
    def run(frames, w, h, c, mode, tff, n, halo, split, apart=0):
        fin, fout = host.path("in.bin"), host.path("out.bin")
        frames.tofile(fin)
        host.run("yadif", [fin, fout, w, h, *SHIFTS[c], 1 if mode == 2 else 0, tff ^ 1, n, halo, split_arg(split), apart],
                 f"{w}x{h} {c} mode {mode} tff {tff} halo {halo} split {split}")
        return np.fromfile(fout, np.uint8).reshape(n, -1)

    rng = np.random.default_rng(5)
    bad = 0
    if "--long" in args:
        import chain_geom as cg

        def want_of(base, idx, seqs, w, h, c, mode, tff):      # seqs: (first, count) of each sequence in the buffer
            made, out = {}, np.empty((len(idx), base.shape[1]), np.uint8)
            for first, count in seqs:
                for j in range(first, first + count):
                    key = (idx[max(j - 1, first)], idx[j], idx[min(j + 1, first + count - 1)])
                    if key not in made:
                        made[key] = deint_frame(base[key[0]], base[key[1]], base[key[2]], w, h, c, mode, tff)
                    out[j] = made[key]
            return out

        lens = (12345, 20422, 3000, 2233)
        cuts = np.cumsum((0,) + lens)
        assert cuts[2] == cg.LONG - 1
        for name in ("yadif", "chain"):
            k = cg.LONG_CASES[name]
            w, h, c = k.w, k.h, k.src
            base = rng.integers(0, 256, (cg.LONG_K, i420_frame_bytes(w, h, c)), dtype=np.uint8)
            n = cg.LONG + 2
            assert len(cg.plane_launches(n)) == 3
            idx = cg.long_frame_index(sum(lens)).tolist()
            one = run(base[idx[:n]], w, h, c, 0, 1, n, 0, 0)
            ok = [(one == want_of(base, idx[:n], [(0, n)], w, h, c, 0, 1)).all()]
            halo = run(base[idx[:n + 2]], w, h, c, 2, 1, n, 3, 0)
            ok.append((halo == want_of(base, idx[:n + 2], [(0, n + 2)], w, h, c, 2, 1)[1:n + 1]).all())
            segs = run(base[idx], w, h, c, 0, 1, sum(lens), 0, lens)
            ok.append((segs == want_of(base, idx, [(int(a), int(b - a)) for a, b in zip(cuts, cuts[1:])], w, h, c, 0, 1)).all())
            few = run(base[idx[:5]], w, h, c, 0, 0, 5, 0, 0, apart=1)      # five frames, U and V apart all the same
            ok.append((few == deint_frames(base[idx[:5]], w, h, c, 0, 0)).all())
            print(f"{w}x{h} {c} U, V apart: one submit of {n} (mode 0 tff) {ok[0]}, halo 3 of {n} out of {n + 2} (mode 2 tff) {ok[1]}, "
                  f"segments {'+'.join(map(str, lens))} {ok[2]}, 5 frames bff forced apart {ok[3]}")
            bad += ok.count(False)
    if "--sweep" in args:
        import chain_geom as cg
        seen = set()
        for k in cg.filter_sweep_configs(cg.FILTER_SWEEP_SEED, 120):
            key = (*cg.source_size(k), k.src, k.deint)
            if not k.deint or key in seen:
                continue
            seen.add(key)
            (w, h), c = cg.source_size(k), k.src
            mode, tff = (2 if "nospatial" in k.deint else 0), int(k.deint.startswith("tff"))
            frames = rng.integers(0, 256, (3, i420_frame_bytes(w, h, c)), dtype=np.uint8)
            one = run(frames, w, h, c, mode, tff, 3, 0, 0)
            segs = run(frames, w, h, c, mode, tff, 3, 0, (2, 1))
            want_segs = np.concatenate([deint_frames(frames[:2], w, h, c, mode, tff), deint_frames(frames[2:], w, h, c, mode, tff)])
            ok = [(one == deint_frames(frames, w, h, c, mode, tff)).all(), (segs == want_segs).all()]
            print(f"{w}x{h} {c} {k.deint}: one submit {ok[0]}, segments 2+1 {ok[1]}")
            bad += ok.count(False)
    for (w, h, c) in ([] if "--sweep" in args or "--long" in args else SHAPES):
        fb = i420_frame_bytes(w, h, c)
        frames = rng.integers(0, 256, (5, fb), dtype=np.uint8)
        frames[3] = (np.arange(fb) * 3 % 256).astype(np.uint8)
        for tff in (1, 0):
            for mode in (0, 2):
                want = deint_frames(frames, w, h, c, mode, tff)
                one = run(frames, w, h, c, mode, tff, 5, 0, 0)
                halo = np.concatenate([run(frames[0:3], w, h, c, mode, tff, 2, 2, 0), run(frames[1:5], w, h, c, mode, tff, 2, 3, 0),
                                       run(frames[3:5], w, h, c, mode, tff, 1, 1, 0)])
                ok = [(one == want).all(), (halo == want).all()]
                for split in SPLITS:      # each segment is a sequence of its own
                    segs = run(frames, w, h, c, mode, tff, 5, 0, split)
                    cuts = np.cumsum((0,) + split)
                    want_segs = np.concatenate([deint_frames(frames[a:b], w, h, c, mode, tff) for a, b in zip(cuts, cuts[1:])])
                    ok.append((segs == want_segs).all())
                print(f"{w}x{h} {c} {'tff' if tff else 'bff'} mode {mode}: one submit {ok[0]}, halo 2+2+1 {ok[1]}, "
                      + ", ".join(f"segments {'+'.join(map(str, sp))} {o}" for sp, o in zip(SPLITS, ok[2:])))
                bad += ok.count(False)
    return bad


if __name__ == "__main__":
    sys.exit(run_check(check))
