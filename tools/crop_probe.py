#!/usr/bin/env python3
"""The cost of `-vf crop` on the GPU: 4K tv-range frames, one 120-frame segment resident in
HBM, submitted by device pointer and synced launch by launch.  Prints, per variant, the medians
over the launches of the MJG_K_ENCODE and MJG_K_SCALE intervals and of the launch's wall time
(submit to sync, as frames/s); the variants alternate round by round in one process after a
prewarm.  Variants (4:2:0 input unless said):

  full        no crop (3840x2160)
  aligned     crop=3840:2144:0:8     every block passes k_encode's alignment test: the yardstick
  ua          crop=3836:2156:2:2     every block misaligned, the 8-byte rows at any alignment
  bytes       the same with MJG_UNALIGNED_FETCH=0: those blocks load byte by byte
  ua_content  crop=3836:2156:0:0 of the frames moved up and left by (2, 2): the samples of `ua` at
              aligned addresses (today's fast path on the same content, the same JPEGs)
  letterbox   crop=3840:1600:0:280
  rect_copy   4:4:4 input, crop=3836:2156:2:2 -pix_fmt yuvj420p: luma by k_plane_copy's rectangle form
  rect_ident  the same with MJG_PLANE_COPY=0: luma through k_scale's identity filters

usage (GPU box): python3 tools/crop_probe.py [--launches 24] [--rounds 4] [--variants a,b,...]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N, Q = 3840, 2160, 120, 5
# variant -> (source format, encoded format, crop rectangle (x, y, w, h) or None, environment at open)
VARIANTS = {
    "full": ("420", "420", None, {}),
    "aligned": ("420", "420", (0, 8, 3840, 2144), {}),
    "ua": ("420", "420", (2, 2, 3836, 2156), {}),
    "bytes": ("420", "420", (2, 2, 3836, 2156), {"MJG_UNALIGNED_FETCH": "0"}),
    "ua_content": ("420", "420", (0, 0, 3836, 2156), {}),
    "letterbox": ("420", "420", (0, 280, 3840, 1600), {}),
    "rect_copy": ("444", "420", (2, 2, 3836, 2156), {}),
    "rect_ident": ("444", "420", (2, 2, 3836, 2156), {"MJG_PLANE_COPY": "0"}),
}
ENV = ("MJG_UNALIGNED_FETCH", "MJG_PLANE_COPY")


def main():
    p = argparse.ArgumentParser()
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
    fb420, fb444 = i420_frame_bytes(W, H, "420"), i420_frame_bytes(W, H, "444")
    pools = {}
    if any(VARIANTS[v][0] == "420" for v in vs):
        pools["420"] = torch.empty((N, fb420), dtype=torch.uint8, device=dev)
    if any(VARIANTS[v][0] == "444" for v in vs):  # the bench's test pattern as 4:4:4: chroma replicated 2x2
        pools["444"] = torch.empty((N, fb444), dtype=torch.uint8, device=dev)
    for i in range(0, N, 10):
        f = testsrc2_i420_torch(W, H, i, 10, dev)
        assert f.shape == (10, fb420)
        if "420" in pools:
            pools["420"][i:i + 10] = f
        if "444" in pools:
            pools["444"][i:i + 10, :W * H] = f[:, :W * H]
            for k in range(2):
                c = f[:, W * H + k * (W // 2) * (H // 2):W * H + (k + 1) * (W // 2) * (H // 2)]
                c = c.reshape(10, H // 2, W // 2).repeat_interleave(2, 1).repeat_interleave(2, 2)
                pools["444"][i:i + 10, (1 + k) * W * H:(2 + k) * W * H] = c.reshape(10, W * H)
    if "ua_content" in vs:  # every plane rolled so that (0, 0) holds what (2, 2) held
        cw, ch = W // 2, H // 2
        sh = torch.empty_like(pools["420"])
        sh[:, :W * H] = pools["420"][:, :W * H].reshape(N, H, W).roll((-2, -2), (1, 2)).reshape(N, W * H)
        for k in range(2):
            o = W * H + k * cw * ch
            sh[:, o:o + cw * ch] = pools["420"][:, o:o + cw * ch].reshape(N, ch, cw).roll((-1, -1), (1, 2)).reshape(N, cw * ch)
        pools["420 moved"] = sh
    torch.cuda.synchronize()
    encs = {}
    for v in vs:
        src, dst, rect, env = VARIANTS[v]
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(env)  # read when the context opens
        encs[v] = MjpegEncoder(0, W, H, full_range=False, qscale=Q, max_batch=N, timing=True, chroma=dst,
                               src_chroma=src, crop=rect)
    for k in ENV:
        os.environ.pop(k, None)
    sizes = {}

    def launch(v):
        enc = encs[v]
        t = time.perf_counter()
        enc.submit(device_ptr=pools["420 moved" if v == "ua_content" else VARIANTS[v][0]].data_ptr(), nframes=N)
        s = enc.sync()
        return s, time.perf_counter() - t

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.prewarm_s:  # leave the idle clocks; every variant's code loaded
        for v in vs:
            sizes[v] = launch(v)[0].copy()
    for x, y in (("ua", "bytes"), ("ua", "ua_content"), ("rect_copy", "rect_ident")):  # (the tests compare the bytes)
        if x in sizes and y in sizes:
            assert (sizes[x] == sizes[y]).all(), f"{x} and {y} differ"
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
    for v in vs:
        src, dst, rect, env = VARIANTS[v]
        s, e, wl = (np.array(res[v][k]) for k in ("scale", "encode", "wall"))
        area = (rect[2] * rect[3] if rect else W * H) / (W * H)
        what = (f"crop={rect[2]}:{rect[3]}:{rect[0]}:{rect[1]}" if rect else "no crop") + \
               (f" -pix_fmt yuvj{dst}p" if src != dst else "") + "".join(f" {k}={x}" for k, x in env.items())
        print(f"{v:10s} {W}x{H} {src} tv, {what} ({100 * area:.1f}% of the frame), {N} frames/launch: "
              f"k_encode median {np.median(e):.4f} ms (min {e.min():.4f}, max {e.max():.4f}), "
              f"MJG_K_SCALE median {np.median(s):.4f} ms, launch wall median {np.median(wl):.3f} ms = "
              f"{N / np.median(wl) * 1e3:.0f} frames/s, {len(e)} launches in {a.rounds} alternating rounds, "
              f"mean JPEG {sizes[v].mean():.0f} B", flush=True)
    for enc in encs.values():
        enc.close()


if __name__ == "__main__":
    main()
