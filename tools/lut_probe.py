#!/usr/bin/env python3
"""The cost of the table stage (k_lut_plane, `-vf eq`) on the GPU: 4K 4:2:0 tv-range frames, one
120-frame segment resident in HBM, submitted by device pointer and synced launch by launch, in
  plain    no interval: k_encode reads the caller's frames;
  lut_in   a slot-"in" context: the MJG_K_SCALE interval is k_lut_plane's luma and U + V launch (the
           caller's frames -> d_lut), then k_encode reads d_lut in place;
  lut_out  a slot-"out" context without a resize: the interval is k_plane_copy<RANGE> on the same
           planes (luma and U + V) and then k_lut_plane on them in place.
The variants alternate round by round in one process after a prewarm.  Prints, per variant, the
medians over the launches of the MJG_K_SCALE interval and of k_encode, and for lut_in the bytes moved
(one frame read, one written) and the rate as a share of k_plane_copy's rate on record
(profiles/pix_fmt/resample_copy_rate.txt).  The interval of lut_out holds both kernels, so the
kernel-by-kernel comparison in the same run comes from a kernel trace of this program
(rocprofv3 --kernel-trace --stats -- python3 tools/lut_probe.py --launches 8 --rounds 2), whose
k_plane_copy and k_lut_plane rows are per-launch durations on the same planes.

usage (GPU box): python3 tools/lut_probe.py [--frames 120] [--launches 24] [--rounds 4]"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, Q = 3840, 2160, 5


def plane_copy_gbs():
    """k_plane_copy's measured rate, read + written bytes per second, from its profile file."""
    with open(os.path.join(ROOT, "profiles", "pix_fmt", "resample_copy_rate.txt")) as f:
        return float(re.search(r"k_plane_copy:.*?: (\d+) GB/s", f.read()).group(1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=120, help="frames per launch")
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant (>= 20), over the rounds")
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
    kw = {"plain": {}, "lut_in": dict(lut_in=tabs), "lut_out": dict(lut_out=tabs)}
    encs = {v: MjpegEncoder(0, W, H, full_range=False, qscale=Q, max_batch=n, timing=True, chroma="420", **k)
            for v, k in kw.items()}
    sizes = {}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.prewarm_s:  # leave the idle clocks; every variant's code loaded
        for v, enc in encs.items():
            enc.submit(device_ptr=pool.data_ptr(), nframes=n)
            sizes[v] = enc.sync().copy()
    per = max(1, -(-a.launches // a.rounds))
    res = {v: {"scale": [], "encode": []} for v in encs}
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
    moved = 2.0 * fb * n
    print(f"{W}x{H} 4:2:0 tv, {n} frames/launch resident in HBM; {moved / 1e6:.0f} MB per pass over the frames (one frame "
          f"read + one written per frame); {per * a.rounds} launches per variant in {a.rounds} alternating rounds")
    for v in encs:
        s, e = np.array(res[v]["scale"]), np.array(res[v]["encode"])
        line = f"{v:8s}: "
        if v == "plain":
            line += "no MJG_K_SCALE interval; "
        else:
            line += f"MJG_K_SCALE median {np.median(s):.4f} ms (min {s.min():.4f}, max {s.max():.4f})"
            if v == "lut_in":
                gbs = moved / (np.median(s) * 1e6)
                line += f" = {gbs:.0f} GB/s, {100 * gbs / copy_gbs:.0f}% of k_plane_copy's {copy_gbs:.0f} GB/s on record"
            else:
                line += " (k_plane_copy<RANGE>, then k_lut_plane in place)"
            line += "; "
        line += (f"k_encode median {np.median(e):.4f} ms (min {e.min():.4f}, max {e.max():.4f}), "
                 f"mean JPEG {sizes[v].mean():.0f} B")
        print(line, flush=True)
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
