#!/usr/bin/env python3
"""The cost of `-vf ...,pad` on the GPU: 4:2:0 tv-range frames, one segment resident in HBM,
submitted by device pointer and synced launch by launch.  Prints, per variant, the medians over
the launches of the MJG_K_SCALE and MJG_K_ENCODE intervals and of the launch's wall time (submit
to sync, as frames/s); the variants alternate round by round in one process after a prewarm, so
each padded case and its unpadded twins are timed on the same box.  Variants:

  plain1600   3840x1600, no filter (no sws stage: k_encode reads the frames in place)
  plain2160   3840x2160, no filter
  pad         3840x1600, pad=3840:2160:0:280   k_pad_plane copies the picture and writes the border
  scale       3840x1600, scale=1920:800
  scale_pad   3840x1600, scale=1920:800,pad=1920:1080:0:140   k_scale into the canvas + the border

and for `pad` the bytes k_pad_plane moves per second of the MJG_K_SCALE interval (the picture
read once, the canvas written once; the interval holds the luma and the chroma launch).

usage (GPU box): python3 tools/pad_probe.py [--frames 60] [--launches 24] [--rounds 4] [--variants a,b,...]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = 5
# variant -> (source size, scale size or None, pad (x, y, W, H) or None)
VARIANTS = {
    "plain1600": ((3840, 1600), None, None),
    "plain2160": ((3840, 2160), None, None),
    "pad": ((3840, 1600), None, (0, 280, 3840, 2160)),
    "scale": ((3840, 1600), (1920, 800), None),
    "scale_pad": ((3840, 1600), (1920, 800), (0, 140, 1920, 1080)),
}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=60, help="frames per launch")
    p.add_argument("--launches", type=int, default=24, help="timed launches per variant (>= 20), over the rounds")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--variants", default=",".join(VARIANTS))
    p.add_argument("--prewarm-s", type=float, default=1.0)
    a = p.parse_args()
    import numpy as np
    import torch
    from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes
    from ffmpeg_distributed_amd.testsrc import testsrc2_i420_torch
    dev = torch.device("cuda", 0)
    vs = a.variants.split(",")
    n = a.frames
    pools = {}
    for v in vs:  # the bench's test pattern at each source size
        w, h = VARIANTS[v][0]
        if (w, h) not in pools:
            pool = torch.empty((n, i420_frame_bytes(w, h, "420")), dtype=torch.uint8, device=dev)
            for i in range(0, n, 10):
                k = min(10, n - i)
                pool[i:i + k] = testsrc2_i420_torch(w, h, i, k, dev)
            pools[(w, h)] = pool
    torch.cuda.synchronize()
    encs = {}
    for v in vs:
        (w, h), scale, pad = VARIANTS[v]
        dw, dh = scale or (None, None)
        encs[v] = MjpegEncoder(0, w, h, dw, dh, full_range=False, qscale=Q, max_batch=n, timing=True, chroma="420",
                               pad=pad)
    sizes = {}

    def launch(v):
        enc = encs[v]
        t = time.perf_counter()
        enc.submit(device_ptr=pools[VARIANTS[v][0]].data_ptr(), nframes=n)
        s = enc.sync()
        return s, time.perf_counter() - t

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.prewarm_s:  # leave the idle clocks; every variant's code loaded
        for v in vs:
            sizes[v] = launch(v)[0].copy()
    per = max(1, -(-a.launches // a.rounds))
    res = {v: {"scale": [], "encode": [], "wall": []} for v in vs}
    for _ in range(a.rounds):
        for v in vs:
            for _ in range(per):
                encs[v].kernel_times(reset=True)
                _s, wall = launch(v)
                kt, _n = encs[v].kernel_times()
                res[v]["scale"].append(kt["scale"])  # (0 without an sws stage)
                res[v]["encode"].append(kt["encode"])
                res[v]["wall"].append(wall * 1e3)
    for v in vs:
        (w, h), scale, pad = VARIANTS[v]
        s, e, wl = (np.array(res[v][k]) for k in ("scale", "encode", "wall"))
        enc = encs[v]
        what = "no filter" if not (scale or pad) else ",".join(
            x for x in (f"scale={scale[0]}:{scale[1]}" if scale else "",
                        f"pad={pad[2]}:{pad[3]}:{pad[0]}:{pad[1]}" if pad else "") if x)
        line = (f"{v:10s} {w}x{h} 420 tv, {what} -> {enc.enc_w}x{enc.enc_h}, {n} frames/launch, sws paths "
                f"{enc.scale_path(0)}/{enc.scale_path(1)}: MJG_K_SCALE median {np.median(s):.4f} ms "
                f"(min {s.min():.4f}, max {s.max():.4f}), k_encode median {np.median(e):.4f} ms (min {e.min():.4f}, "
                f"max {e.max():.4f}), launch wall median {np.median(wl):.3f} ms = {n / np.median(wl) * 1e3:.0f} frames/s, "
                f"{len(e)} launches in {a.rounds} alternating rounds, mean JPEG {sizes[v].mean():.0f} B")
        if pad and not scale:  # k_pad_plane<.., COPY> alone fills the interval
            moved = n * (i420_frame_bytes(w, h, "420") + i420_frame_bytes(pad[2], pad[3], "420"))
            line += (f"; k_pad_plane: {moved / 1e6:.1f} MB read + written per launch = "
                     f"{moved / (np.median(s) * 1e-3) / 1e12:.2f} TB/s of the interval (luma + chroma launches)")
        print(line, flush=True)
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
