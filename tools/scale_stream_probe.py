#!/usr/bin/env python3
"""The cost of `-vf scale` past 4:1 on the GPU: 4K 4:2:0 tv-range frames, one 120-frame segment
resident in HBM, submitted by device pointer and synced launch by launch.  Prints, per variant,
the medians over the launches of the MJG_K_SCALE and MJG_K_ENCODE intervals and of the launch's
wall time (submit to sync); the variants alternate round by round in one process after a
prewarm, and the spread of the per-round medians is printed beside each median.  Variants:

  tile_960     3840x2160 -> 960x540 (4:1), the tile kernel k_scale: the yardstick (the largest
               ratio it takes; it reads the same 1.49 GB)
  stream_960   the same with MJG_SCALE_STREAM=1: k_scale_stream on a shape both kernels take
  stream_854   3840x2160 -> 854x480 (4.5:1), k_scale_stream
  stream_640   3840x2160 -> 640x360 (6:1), k_scale_stream
  stream_320   3840x2160 -> 320x180 (12:1), k_scale_stream
  stream_64    3840x2160 -> 64x36 (60:1, 244 taps), k_scale_stream

A library without k_scale_stream (MJG_LIBRARY=<the parent's build>) runs tile_960 alone:
--variants tile_960.  The floor printed with each line is the input bytes at k_plane_copy's
measured rate (5.6 TB/s).

usage (GPU box): python3 tools/scale_stream_probe.py [--launches 24] [--rounds 4] [--variants a,b,...]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N, Q = 3840, 2160, 120, 5
COPY_RATE = 5.6e12  # bytes/s, k_plane_copy
# variant -> (encoded size, environment at open, the path expected for the luma plane)
VARIANTS = {
    "tile_960": ((960, 540), {}, 2),
    "stream_960": ((960, 540), {"MJG_SCALE_STREAM": "1"}, 3),
    "stream_854": ((854, 480), {}, 3),
    "stream_640": ((640, 360), {}, 3),
    "stream_320": ((320, 180), {}, 3),
    "stream_64": ((64, 36), {}, 3),
}
ENV = ("MJG_SCALE_STREAM",)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant (>= 20), over the rounds")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--variants", default=",".join(VARIANTS))
    p.add_argument("--prewarm-s", type=float, default=1.0)
    a = p.parse_args()
    import numpy as np
    import torch
    from ffmpeg_distributed_amd import build
    from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes
    from ffmpeg_distributed_amd.testsrc import testsrc2_i420_torch
    dev = torch.device("cuda", 0)
    vs = a.variants.split(",")
    fb = i420_frame_bytes(W, H, "420")
    pool = torch.empty((N, fb), dtype=torch.uint8, device=dev)
    for i in range(0, N, 10):
        pool[i:i + 10] = testsrc2_i420_torch(W, H, i, 10, dev)
    torch.cuda.synchronize()
    encs = {}
    for v in vs:
        (dw, dh), env, path = VARIANTS[v]
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(env)  # read when the context opens
        encs[v] = MjpegEncoder(0, W, H, dw, dh, full_range=False, qscale=Q, max_batch=N, timing=True)
        if hasattr(encs[v]._L, "mjg_debug_scale_path"):
            assert encs[v].scale_path(0) == path, (v, encs[v].scale_path(0))
    for k in ENV:
        os.environ.pop(k, None)
    sizes = {}

    def launch(v):
        enc = encs[v]
        t = time.perf_counter()
        enc.submit(device_ptr=pool.data_ptr(), nframes=N)
        s = enc.sync()
        return s, time.perf_counter() - t

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.prewarm_s:  # leave the idle clocks; every variant's code loaded
        for v in vs:
            sizes[v] = launch(v)[0].copy()
    if "tile_960" in sizes and "stream_960" in sizes:  # (the tests compare the bytes)
        assert (sizes["tile_960"] == sizes["stream_960"]).all(), "tile_960 and stream_960 differ"
    per = max(1, -(-a.launches // a.rounds))
    res = {v: {"scale": [], "encode": [], "wall": []} for v in vs}
    for _ in range(a.rounds):
        for v in vs:
            for _ in range(per):
                encs[v].kernel_times(reset=True)
                _s, wall = launch(v)
                kt, _n = encs[v].kernel_times()
                res[v]["scale"].append(kt["scale"])
                res[v]["encode"].append(kt["encode"])
                res[v]["wall"].append(wall * 1e3)
    lib = os.environ.get("MJG_LIBRARY")
    print(f"# library: {os.path.basename(lib) if lib else 'in-tree, source digest ' + build.source_digest()}; input {N * fb} B per launch, "
          f"floor at {COPY_RATE / 1e12:.1f} TB/s {N * fb / COPY_RATE * 1e3:.4f} ms", flush=True)
    for v in vs:
        (dw, dh), env, path = VARIANTS[v]
        s, e, wl = (np.array(res[v][k]) for k in ("scale", "encode", "wall"))
        rm = np.median(s.reshape(a.rounds, -1), axis=1)  # per-round medians: the run-to-run spread
        what = f"{W}x{H} -> {dw}x{dh}" + "".join(f" {k}={x}" for k, x in env.items())
        print(f"{v:11s} {what}, {N} frames/launch: MJG_K_SCALE median {np.median(s):.4f} ms "
              f"(rounds {rm.min():.4f}..{rm.max():.4f}, min {s.min():.4f}) = {N * fb / np.median(s) / 1e6:.0f} GB/s of input, "
              f"{100 * (N * fb / COPY_RATE * 1e3) / np.median(s):.0f}% of the floor; k_encode median {np.median(e):.4f} ms, "
              f"launch wall median {np.median(wl):.3f} ms = {N / np.median(wl) * 1e3:.0f} frames/s, "
              f"{len(s)} launches in {a.rounds} alternating rounds", flush=True)
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
