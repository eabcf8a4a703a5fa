#!/usr/bin/env python3
"""The cost of `-vf unsharp` on the GPU: 4K 4:2:0 tv-range frames, one 120-frame segment resident in
HBM, submitted by device pointer and synced launch by launch, `scale=1920:1080` alone against
`scale=1920:1080,unsharp` (the defaults: luma 5x5 at 1.0 through k_unsharp_plane<5, 5>, the chroma
planes copied by the same kernel) and, with --variants, other sizes through the run-time path.
Prints, per variant, the medians over the launches of the MJG_K_SCALE interval (the sws stage's
launches and, with a sharpen, the luma and the U + V launch of k_unsharp_plane) and of k_encode;
the sharpen's share is the difference of the two intervals.  The bytes it must move: the 1080p
planes read once and written once, two frames per frame.  Its rate stands beside k_plane_copy's
measured copy rate (profiles/pix_fmt/resample_copy_rate.txt).  The variants alternate round by
round in one process after a prewarm.

usage (GPU box): python3 tools/unsharp_probe.py [--frames 120] [--launches 24] [--rounds 4]
                 [--variants none,5:5:1.0:5:5:0.0,7:7:1.0:7:7:1.0]"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, DW, DH, Q = 3840, 2160, 1920, 1080, 3


def plane_copy_gbs():
    """k_plane_copy's measured rate, read + written bytes per second, from its profile file."""
    with open(os.path.join(ROOT, "profiles", "pix_fmt", "resample_copy_rate.txt")) as f:
        return float(re.search(r"k_plane_copy:.*?: (\d+) GB/s", f.read()).group(1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=120, help="frames per launch")
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant (>= 20), over the rounds")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--variants", default="none,5:5:1.0:5:5:0.0,5:5:1.0:5:5:1.0,7:7:1.0:7:7:1.0,13:13:1.0:13:13:1.0")
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

    def spec(v):
        if v == "none":
            return None
        t = v.split(":")
        return (int(t[0]), int(t[1]), float(t[2]), int(t[3]), int(t[4]), float(t[5]))

    vs = a.variants.split(",")
    encs = {v: MjpegEncoder(0, W, H, DW, DH, full_range=False, qscale=Q, max_batch=n, timing=True, chroma="420",
                            unsharp=spec(v)) for v in vs}
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
    copy_gbs = plane_copy_gbs()
    moved = 2.0 * i420_frame_bytes(DW, DH, "420") * n
    print(f"{W}x{H} -> {DW}x{DH} 4:2:0 tv, {n} frames/launch resident in HBM; the sharpen moves {moved / 1e6:.0f} MB per "
          f"launch (the {DW}x{DH} planes read once and written once); {per * a.rounds} launches per variant in {a.rounds} "
          f"alternating rounds")
    base = float(np.median(res["none"]["scale"])) if "none" in res else None
    for v in vs:
        s, e = np.array(res[v]["scale"]), np.array(res[v]["encode"])
        line = f"unsharp {v:24s}: MJG_K_SCALE median {np.median(s):.4f} ms (min {s.min():.4f}, max {s.max():.4f})"
        if v != "none" and base is not None:
            d = float(np.median(s)) - base
            gbs = moved / (d * 1e6)
            line += (f"; the sharpen {d:.4f} ms = {gbs:.0f} GB/s, {100 * gbs / copy_gbs:.0f}% of k_plane_copy's "
                     f"{copy_gbs:.0f} GB/s")
        line += (f"; k_encode median {np.median(e):.4f} ms (min {e.min():.4f}, max {e.max():.4f}), "
                 f"mean JPEG {sizes[v].mean():.0f} B")
        print(line, flush=True)
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
