#!/usr/bin/env python3
"""The -pix_fmt conversion's cost on the GPU: 4K 4:4:4 tv-range frames -> yuvj420p, one
120-frame segment resident in HBM, submitted by device pointer and synced launch by launch.
Prints, for the unchanged luma plane streamed by k_plane_copy and for the same plane through
k_scale's identity filters (MJG_PLANE_COPY=0, read when a context opens), the medians over
the launches of the MJG_K_SCALE interval (luma + both chroma planes) and of k_encode; the
two variants alternate round by round in one process after a prewarm.

usage (GPU box): python3 tools/resample_probe.py [--launches 24] [--rounds 4]
       the copy kernel's own time: a run of its own under the profiler,
         rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \\
             python3 tools/resample_probe.py --variants copy --launches 24 --rounds 1
         python3 tools/resample_probe.py --stats-csv DIR/.../run_kernel_stats.csv
       which reports its achieved bytes/s (luma read + write) against the float4-copy rate."""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N, Q = 3840, 2160, 120, 5
SRC, DST = "444", "420"
COPY_PEAK_GBS = 6290.0  # MI355X float4 copy, measured (read + write bytes per second)


def stats(csv_path):
    """k_plane_copy's mean duration in a rocprofv3 kernel-stats CSV -> achieved GB/s."""
    rows = [r for r in csv.DictReader(open(csv_path)) if "k_plane_copy" in r["Name"]]
    if not rows:
        sys.exit(f"no k_plane_copy in {csv_path}")
    calls = sum(int(r["Calls"]) for r in rows)
    ns = sum(float(r["TotalDurationNs"]) for r in rows) / calls
    moved = 2 * W * H * N  # the luma plane of every frame, read once and written once
    gbs = moved / ns
    print(f"k_plane_copy: {calls} launches, mean {ns / 1e3:.1f} us per launch of {N} {W}x{H} luma planes "
          f"({moved / 1e6:.0f} MB read + written): {gbs:.0f} GB/s, {100 * gbs / COPY_PEAK_GBS:.0f}% of the "
          f"{COPY_PEAK_GBS:.0f} GB/s float4-copy rate")
    for r in csv.DictReader(open(csv_path)):
        if "mjg::" in r["Name"]:
            print(f"  {float(r['AverageNs']) / 1e3:10.1f} us x {int(r['Calls']):4d}  {r['Name'][:100]}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant (>= 20), over the rounds")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--variants", default="copy,identity")
    p.add_argument("--prewarm-s", type=float, default=1.0)
    p.add_argument("--stats-csv")
    a = p.parse_args()
    if a.stats_csv:
        return stats(a.stats_csv)
    import numpy as np
    import torch
    from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes
    from ffmpeg_distributed_amd.testsrc import testsrc2_i420_torch
    dev = torch.device("cuda", 0)
    fb420, fb = i420_frame_bytes(W, H, "420"), i420_frame_bytes(W, H, SRC)
    # the bench's test pattern as 4:4:4: its luma, its 4:2:0 chroma planes replicated 2x2
    pool = torch.empty((N, fb), dtype=torch.uint8, device=dev)
    for i in range(0, N, 10):
        f = testsrc2_i420_torch(W, H, i, 10, dev)
        assert f.shape == (10, fb420)
        pool[i:i + 10, :W * H] = f[:, :W * H]
        for k in range(2):
            c = f[:, W * H + k * (W // 2) * (H // 2):W * H + (k + 1) * (W // 2) * (H // 2)].reshape(10, H // 2, W // 2)
            c = c.repeat_interleave(2, 1).repeat_interleave(2, 2)
            pool[i:i + 10, (1 + k) * W * H:(2 + k) * W * H] = c.reshape(10, W * H)
    torch.cuda.synchronize()
    encs = {}
    for v in a.variants.split(","):
        if v == "identity":
            os.environ["MJG_PLANE_COPY"] = "0"
        else:
            os.environ.pop("MJG_PLANE_COPY", None)
        encs[v] = MjpegEncoder(0, W, H, full_range=False, qscale=Q, max_batch=N, timing=True, chroma=DST,
                               src_chroma=SRC)
    os.environ.pop("MJG_PLANE_COPY", None)
    sizes = {}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.prewarm_s:  # leave the idle clocks; every variant's code loaded
        for v, enc in encs.items():
            enc.submit(device_ptr=pool.data_ptr(), nframes=N)
            sizes[v] = enc.sync().copy()
    vs = list(encs)
    if len(vs) > 1:  # the same JPEG sizes from every variant (the tests compare the bytes)
        assert all((sizes[v] == sizes[vs[0]]).all() for v in vs), "variants differ"
    per = max(1, -(-a.launches // a.rounds))
    res = {v: {"scale": [], "encode": []} for v in vs}
    for _ in range(a.rounds):
        for v, enc in encs.items():
            for _ in range(per):
                enc.kernel_times(reset=True)
                enc.submit(device_ptr=pool.data_ptr(), nframes=N)
                enc.sync()
                kt, _n = enc.kernel_times()
                res[v]["scale"].append(kt["scale"])
                res[v]["encode"].append(kt["encode"])
    name = {"copy": "k_plane_copy", "identity": "k_scale identity (MJG_PLANE_COPY=0)"}
    for v in vs:
        s, e = np.array(res[v]["scale"]), np.array(res[v]["encode"])
        print(f"{W}x{H} {SRC} tv -> yuvj{DST}p, {N} frames/launch, luma via {name.get(v, v)}: "
              f"MJG_K_SCALE median {np.median(s):.4f} ms (min {s.min():.4f}, max {s.max():.4f}), "
              f"k_encode median {np.median(e):.4f} ms (min {e.min():.4f}, max {e.max():.4f}), "
              f"{len(s)} launches in {a.rounds} alternating rounds, mean JPEG {sizes[v].mean():.0f} B", flush=True)
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
