#!/usr/bin/env python3
"""The cost of the contact sheet (k_tile_plane, `-vf ...,tile`) on the GPU: 4K 4:2:0 tv-range frames scaled
to 160x90 thumbnails, one 120-frame segment resident in HBM, submitted by device pointer and synced launch
by launch, in
  sheet    scale=160:90,tile=6x5: the MJG_K_SCALE interval is the sws stage's launches and k_tile_plane's
           luma and U + V launch (120 cells onto four 960x450 sheets), then k_encode codes four sheets;
  plain    scale=160:90 alone: the interval is the sws stage's launches, and k_encode codes 120 thumbnails.
The difference of the two intervals is the tile stage: it reads every cell once and writes every sheet once.
The variants alternate round by round in one process after a prewarm.  Prints, per variant, the median,
minimum and maximum of the MJG_K_SCALE interval over the launches and per round, the difference of the
medians next to the spread of plain's rounds, and the bytes the stage moves with the rate that difference
would mean.

usage (GPU box): python3 tools/tile_probe.py [--frames 120] [--launches 24] [--rounds 4]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, Q = 3840, 2160, 5
DW, DH = 160, 90
SHEET = (6, 5, 0, 0, 0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=120, help="frames per launch")
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant, over the rounds")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--prewarm-s", type=float, default=1.0)
    a = p.parse_args()
    import numpy as np
    import torch
    from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes
    from ffmpeg_distributed_amd.testsrc import testsrc2_i420_torch
    dev = torch.device("cuda", 0)
    n, fb = a.frames, i420_frame_bytes(W, H, "420")
    pool = torch.empty((n, fb), dtype=torch.uint8, device=dev)
    for i in range(0, n, 10):
        k = min(10, n - i)
        pool[i:i + k] = testsrc2_i420_torch(W, H, i, k, dev)
    torch.cuda.synchronize()
    kw = {"sheet": dict(sheet=SHEET), "plain": dict()}
    encs = {v: MjpegEncoder(0, W, H, DW, DH, full_range=False, qscale=Q, max_batch=n, timing=True, chroma="420", **k)
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
    sheets = encs["sheet"].frames_out(n)
    cell_b = i420_frame_bytes(DW, DH, "420")
    sheet_b = i420_frame_bytes(encs["sheet"].enc_w, encs["sheet"].enc_h, "420")
    moved = float(n * cell_b + sheets * sheet_b)
    print(f"{W}x{H} 4:2:0 tv -> {DW}x{DH}, {n} frames/launch resident in HBM, tile={SHEET[0]}x{SHEET[1]}: {sheets} sheets of "
          f"{encs['sheet'].enc_w}x{encs['sheet'].enc_h}; the tile stage reads {n * cell_b / 1e6:.2f} MB of cells and writes "
          f"{sheets * sheet_b / 1e6:.2f} MB of sheets; {per * a.rounds} launches per variant in {a.rounds} alternating rounds")
    med = {}
    for v in encs:
        s = np.array(res[v])
        med[v] = float(np.median(s))
        rounds = ", ".join(f"{np.median(r):.4f}" for r in s)
        print(f"{v:6s}: MJG_K_SCALE median {med[v]:.4f} ms (min {s.min():.4f}, max {s.max():.4f}); medians of the rounds: "
              f"{rounds}", flush=True)
    pr = [float(np.median(r)) for r in res["plain"]]
    diff = med["sheet"] - med["plain"]
    print(f"sheet - plain: {diff * 1e3:.1f} us per launch; spread of plain's rounds (max - min of their medians): "
          f"{(max(pr) - min(pr)) * 1e3:.1f} us")
    if diff > 0:
        print(f"the stage's {moved / 1e6:.2f} MB in that difference: {moved / (diff * 1e6):.1f} GB/s (two launches, mostly "
              f"launch latency at this size)")
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
