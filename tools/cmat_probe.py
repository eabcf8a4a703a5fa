#!/usr/bin/env python3
"""The cost of the colour matrix (k_cmat_frame, `-vf colormatrix`) on the GPU against the table stage:
4K 4:2:0 tv-range frames, one 120-frame segment resident in HBM, submitted by device pointer and synced
launch by launch, in
  cmat     a matrix-only context (bt709 -> bt601): the MJG_K_SCALE interval is k_cmat_frame's one launch
           (the caller's frames -> d_lut), then k_encode reads d_lut in place;
  lut_in   a slot-"in" table context: the interval is k_lut_plane's luma and U + V launch on the same
           frames into the same buffer.
Both stages move each frame once in and once out.  The variants alternate round by round in one
process after a prewarm.  Prints, per variant, the median, minimum and maximum of the MJG_K_SCALE
interval over the launches and per round, the bytes moved and the rate, and the ratio of the two medians
next to the spread of the rounds.

usage (GPU box): python3 tools/cmat_probe.py [--frames 120] [--launches 24] [--rounds 4]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, Q = 3840, 2160, 5


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=120, help="frames per launch")
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant, over the rounds")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--prewarm-s", type=float, default=1.0)
    a = p.parse_args()
    import numpy as np
    import torch
    from ffmpeg_distributed_amd import profile
    from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes
    from ffmpeg_distributed_amd.testsrc import testsrc2_i420_torch
    dev = torch.device("cuda", 0)
    n, fb = a.frames, i420_frame_bytes(W, H, "420")
    pool = torch.empty((n, fb), dtype=torch.uint8, device=dev)
    for i in range(0, n, 10):
        k = min(10, n - i)
        pool[i:i + k] = testsrc2_i420_torch(W, H, i, k, dev)
    torch.cuda.synchronize()
    tabs = profile.eq_tables(dict(contrast=1.2, brightness=-0.07, saturation=1.3))      # no identity plane
    kw = {"cmat": dict(cmat=profile.colormatrix_coefs("bt709", "bt601")), "lut_in": dict(lut_in=tabs)}
    encs = {v: MjpegEncoder(0, W, H, full_range=False, qscale=Q, max_batch=n, timing=True, chroma="420", **k)
            for v, k in kw.items()}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.prewarm_s:  # leave the idle clocks; every variant's code loaded
        for enc in encs.values():
            enc.submit(device_ptr=pool.data_ptr(), nframes=n)
            enc.sync()
    per = max(1, -(-a.launches // a.rounds))
    res = {v: [] for v in encs}
    for _ in range(a.rounds):
        for v, enc in encs.items():
            row = []
            for _ in range(per):
                enc.kernel_times(reset=True)
                enc.submit(device_ptr=pool.data_ptr(), nframes=n)
                enc.sync()
                row.append(enc.kernel_times()[0]["scale"])
            res[v].append(row)
    moved = 2.0 * fb * n
    print(f"{W}x{H} 4:2:0 tv, {n} frames/launch resident in HBM; {moved / 1e6:.0f} MB per pass over the frames (one frame "
          f"read + one written per frame); {per * a.rounds} launches per variant in {a.rounds} alternating rounds")
    med = {}
    for v in encs:
        s = np.array(res[v])
        med[v] = float(np.median(s))
        rounds = ", ".join(f"{np.median(r):.4f}" for r in s)
        print(f"{v:7s}: MJG_K_SCALE median {med[v]:.4f} ms (min {s.min():.4f}, max {s.max():.4f}) = "
              f"{moved / (med[v] * 1e6):.0f} GB/s; medians of the rounds: {rounds}", flush=True)
    spread = max(float(np.median(r)) for r in res["lut_in"]) / min(float(np.median(r)) for r in res["lut_in"])
    print(f"ratio cmat / lut_in: {med['cmat'] / med['lut_in']:.3f}; spread of lut_in's rounds (max / min of their medians): "
          f"{spread:.3f}")
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
