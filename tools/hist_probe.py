#!/usr/bin/env python3
"""The cost of the thumbnail's histograms (k_frame_hist, `-vf thumbnail`) on the GPU, against a copy of the
same bytes: 120 4K 4:2:0 frames resident in HBM, for three contents,
  testsrc   testsrc2 frames;
  noise     uniform random bytes (a wave's 64 lanes on 64 random bins);
  constant  one value a plane (all 64 lanes of a wave on one bin: the contention case).
Per content the launches alternate in one process: a submit by device pointer to a slot-"out" table context
without a resize, whose sws stage is k_plane_copy over the luma and the U + V planes of those very frames
(every byte read once and written once), then one FrameHist.count of them by device pointer (k_frame_hist:
every byte read once, 768 counters a frame written).

Run without --trace it does the launches and prints the wall time of count() (zero, launch, 368 KB read
back, wait).  The kernels' own times come from a kernel trace of that run:
  rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python3 tools/hist_probe.py
  python3 tools/hist_probe.py --trace DIR
which prints, per content, k_frame_hist's time, k_plane_copy's (its luma and its U + V launch together),
and the ratio; both from the same run.

usage (GPU box): python3 tools/hist_probe.py [--frames 120] [--launches 12] [--prewarm 4] [--trace DIR]"""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, Q = 3840, 2160, 5
CONTENTS = ("testsrc", "noise", "constant")


def workload(a):
    import numpy as np
    import torch
    from ffmpeg_distributed_amd import profile
    from ffmpeg_distributed_amd.encoder import FrameHist, MjpegEncoder, i420_frame_bytes
    from ffmpeg_distributed_amd.testsrc import testsrc2_i420_torch
    dev = torch.device("cuda", 0)
    n, fb = a.frames, i420_frame_bytes(W, H, "420")
    pools = {}
    pools["testsrc"] = torch.empty((n, fb), dtype=torch.uint8, device=dev)
    for i in range(0, n, 10):
        k = min(10, n - i)
        pools["testsrc"][i:i + k] = testsrc2_i420_torch(W, H, i, k, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    pools["noise"] = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device=dev, generator=g)
    pools["constant"] = torch.empty((n, fb), dtype=torch.uint8, device=dev)
    pools["constant"][:, :W * H] = 90
    pools["constant"][:, W * H:W * H * 5 // 4] = 120
    pools["constant"][:, W * H * 5 // 4:] = 140
    torch.cuda.synchronize()
    tabs = profile.eq_tables(dict(contrast=1.2, brightness=-0.07, saturation=1.3))      # no identity plane
    enc = MjpegEncoder(0, W, H, full_range=True, qscale=Q, max_batch=n, chroma="420", lut_out=tabs)  # (full range: a plain copy)
    assert enc.scale_path(0) == 1 and enc.scale_path(1) == 1, "the sws stage is not k_plane_copy"
    hist = FrameHist(0, W, H, "420", n)
    for _ in range(a.prewarm):  # leave the idle clocks; both kernels' code loaded
        enc.submit(device_ptr=pools["testsrc"].data_ptr(), nframes=n)
        enc.sync()
        hist.count(device_ptr=pools["testsrc"].data_ptr(), nframes=n)
    print(f"{W}x{H} 4:2:0, {n} frames a launch resident in HBM: {n * fb / 1e6:.0f} MB read by either kernel; {a.prewarm} "
          f"prewarm and {a.launches} timed launches of each per content, copy and count alternating")
    for c in CONTENTS:
        wall, ptr = [], pools[c].data_ptr()
        for _ in range(a.launches):
            enc.submit(device_ptr=ptr, nframes=n)
            enc.sync()
            t0 = time.perf_counter()
            got = hist.count(device_ptr=ptr, nframes=n)
            wall.append((time.perf_counter() - t0) * 1e3)
        assert int(got[0].sum()) == fb and (got.sum(axis=1) == fb).all()
        wall = np.array(wall)
        print(f"{c:9s}: count() wall median {np.median(wall):.4f} ms (min {wall.min():.4f}, max {wall.max():.4f}); "
              f"non-empty bins of frame 0: Y {np.count_nonzero(got[0, :256])}, U {np.count_nonzero(got[0, 256:512])}, "
              f"V {np.count_nonzero(got[0, 512:])}", flush=True)
    enc.close()
    hist.close()


def trace(a):
    import numpy as np
    from ffmpeg_distributed_amd.encoder import i420_frame_bytes
    paths = glob.glob(os.path.join(a.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    rows = []
    with open(paths[0], newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    us = {k: [(e - s) / 1e3 for s, e, name in rows if k in name] for k in ("k_frame_hist", "k_plane_copy")}
    nh, nc = len(us["k_frame_hist"]), len(us["k_plane_copy"])
    per = a.launches
    assert nh == a.prewarm + 3 * per and nc == 2 * nh, (nh, nc, "not this program's --prewarm / --launches")
    mb = a.frames * i420_frame_bytes(W, H, "420") / 1e6
    print(f"kernel trace of the run above ({os.path.basename(paths[0])}): per content {per} launches of each, in microseconds; "
          f"{mb:.0f} MB read by either")
    for i, c in enumerate(CONTENTS):
        lo = a.prewarm + i * per
        h = np.array(us["k_frame_hist"][lo:lo + per])
        cp = np.array(us["k_plane_copy"][2 * lo:2 * (lo + per)]).reshape(per, 2).sum(axis=1)   # luma + (U + V)
        print(f"{c:9s}: k_frame_hist median {np.median(h):.1f} (min {h.min():.1f}, max {h.max():.1f}) = {mb / np.median(h) * 1e3:.0f} GB/s "
              f"read; k_plane_copy median {np.median(cp):.1f} (min {cp.min():.1f}, max {cp.max():.1f}) = {mb / np.median(cp) * 1e3:.0f} GB/s "
              f"read (and as much written); hist / copy = {np.median(h) / np.median(cp):.2f}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=120, help="frames per launch")
    p.add_argument("--launches", type=int, default=12, help="timed launches of each kernel per content")
    p.add_argument("--prewarm", type=int, default=4)
    p.add_argument("--trace", help="a directory that holds rocprofv3's kernel trace of a run with the same arguments")
    a = p.parse_args()
    (trace if a.trace else workload)(a)


if __name__ == "__main__":
    main()
