#!/usr/bin/env python3
"""The cost of `-vf hflip / vflip / transpose` on the GPU: 4K 4:2:0 tv-range frames, one
120-frame segment resident in HBM, submitted by device pointer and synced launch by launch, in an
orientation-only context (k_orient_plane, then k_encode reading its buffer in place).  Prints, per
orientation 1..7 (T | FX << 1 | FY << 2), the medians over the launches of the MJG_K_SCALE
interval (the luma launch and the U + V launch of k_orient_plane) and of k_encode, the bytes the
interval moves (every frame read once and written once) and the rate, against k_plane_copy's
measured rate on the same kind of traffic; `plain` is the same frames with no
filter (no interval: k_encode reads the caller's frames).  The variants alternate round by round
in one process after a prewarm.

usage (GPU box): python3 tools/orient_probe.py [--frames 120] [--launches 24] [--rounds 4] [--variants 1,2,...]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, Q = 3840, 2160, 5
PLANE_COPY_GBS = 5600.0  # k_plane_copy on a 4K luma plane, read + written bytes per second
NAMES = {0: "plain", 1: "transpose=0", 2: "hflip", 3: "transpose=1", 4: "vflip", 5: "transpose=2", 6: "hflip,vflip",
         7: "transpose=3"}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=120, help="frames per launch")
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant (>= 20), over the rounds")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--variants", default="0,1,2,3,4,5,6,7")
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
    vs = [int(v) for v in a.variants.split(",")]
    encs = {v: MjpegEncoder(0, W, H, full_range=False, qscale=Q, max_batch=n, timing=True, chroma="420", orient=v)
            for v in vs}
    sizes = {}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.prewarm_s:  # leave the idle clocks; every variant's code loaded
        for v, enc in encs.items():
            enc.submit(device_ptr=pool.data_ptr(), nframes=n)
            sizes[v] = enc.sync().copy()
    per = max(1, -(-a.launches // a.rounds))
    res = {v: {"scale": [], "encode": []} for v in vs}
    for _ in range(a.rounds):
        for v, enc in encs.items():
            for _ in range(per):
                enc.kernel_times(reset=True)
                enc.submit(device_ptr=pool.data_ptr(), nframes=n)
                enc.sync()
                kt, _n = enc.kernel_times()
                res[v]["scale"].append(kt["scale"])
                res[v]["encode"].append(kt["encode"])
    moved = 2 * fb * n
    print(f"{W}x{H} 4:2:0 tv, {n} frames/launch resident in HBM, orientation only; {moved / 1e6:.0f} MB read + "
          f"written per launch; {per * a.rounds} launches per variant in {a.rounds} alternating rounds")
    for v in vs:
        s, e = np.array(res[v]["scale"]), np.array(res[v]["encode"])
        line = f"orient {v} ({NAMES[v]:12s}): "
        if v:
            gbs = moved / (np.median(s) * 1e6)
            line += (f"MJG_K_SCALE median {np.median(s):.4f} ms (min {s.min():.4f}, max {s.max():.4f}) = {gbs:.0f} GB/s, "
                     f"{100 * gbs / PLANE_COPY_GBS:.0f}% of k_plane_copy's {PLANE_COPY_GBS:.0f} GB/s; ")
        else:
            line += "no MJG_K_SCALE interval; "
        line += (f"k_encode median {np.median(e):.4f} ms (min {e.min():.4f}, max {e.max():.4f}), "
                 f"mean JPEG {sizes[v].mean():.0f} B")
        print(line, flush=True)
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
