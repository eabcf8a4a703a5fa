#!/usr/bin/env python3
"""The cost of `-vf yadif` on the GPU: 4K 4:2:0 tv-range frames, one 120-frame segment resident in
HBM, submitted by device pointer and synced launch by launch, in a deinterlacer-only context
(k_yadif_plane, then k_encode reading its buffer in place) against a plain one (no interval:
k_encode reads the caller's frames).  Prints, per variant, the medians over the launches of the
MJG_K_SCALE interval (the luma launch and the U + V launch of k_yadif_plane) and of k_encode, the
bytes the kernel must move and the rate, as a share of k_plane_copy's measured copy rate
(profiles/pix_fmt/resample_copy_rate.txt).  The byte count: per output frame all of prev (its rows
ym, yp, y, y2m, y2p cover both fields), all of cur (the kept rows are copied and are the rows ym /
yp of the interpolated ones, which are read themselves as next2) and half of next (rows ym, yp: the
kept field) are read and one frame is written: 3.5 frames, each distinct byte counted once.  The
variants alternate round by round in one process after a prewarm.

usage (GPU box): python3 tools/yadif_probe.py [--frames 120] [--launches 24] [--rounds 4] [--variants 0,1,3]"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, Q = 3840, 2160, 5
NAMES = {0: "plain", 1: "yadif=0:tff", 3: "yadif=2:tff", 5: "yadif=0:bff", 7: "yadif=2:bff"}


def plane_copy_gbs():
    """k_plane_copy's measured rate, read + written bytes per second, from its profile file."""
    with open(os.path.join(ROOT, "profiles", "pix_fmt", "resample_copy_rate.txt")) as f:
        return float(re.search(r"k_plane_copy:.*?: (\d+) GB/s", f.read()).group(1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=120, help="frames per launch")
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant (>= 20), over the rounds")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--variants", default="0,1,3")
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
    encs = {v: MjpegEncoder(0, W, H, full_range=False, qscale=Q, max_batch=n, timing=True, chroma="420",
                            deint=v or None) for v in vs}
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
    moved = 3.5 * fb * n
    print(f"{W}x{H} 4:2:0 tv, {n} frames/launch resident in HBM, deinterlacer only; {moved / 1e6:.0f} MB per launch "
          f"(2.5 frames read + 1 written per frame); {per * a.rounds} launches per variant in {a.rounds} alternating rounds")
    for v in vs:
        s, e = np.array(res[v]["scale"]), np.array(res[v]["encode"])
        line = f"deint {v} ({NAMES.get(v, '?'):11s}): "
        if v:
            gbs = moved / (np.median(s) * 1e6)
            line += (f"MJG_K_SCALE median {np.median(s):.4f} ms (min {s.min():.4f}, max {s.max():.4f}) = {gbs:.0f} GB/s, "
                     f"{100 * gbs / copy_gbs:.0f}% of k_plane_copy's {copy_gbs:.0f} GB/s; ")
        else:
            line += "no MJG_K_SCALE interval; "
        line += (f"k_encode median {np.median(e):.4f} ms (min {e.min():.4f}, max {e.max():.4f}), "
                 f"mean JPEG {sizes[v].mean():.0f} B")
        print(line, flush=True)
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
