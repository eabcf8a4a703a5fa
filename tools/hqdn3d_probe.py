#!/usr/bin/env python3
"""The cost of `-vf hqdn3d` on the GPU (k_dn_rows, k_dn_cols, k_dn_time) against a copy of the same frames: 120
4K 4:2:0 frames resident in HBM, for two contents,
  noise     low-contrast noise, 100 +- 12 (the tables act: the lookups spread over the table's middle);
  testsrc   testsrc2 frames (edges and flat areas: both ends of the table).
Per content the submits alternate in one process, both by device pointer and both with MJG_F_TIMING, whose
MJG_K_SCALE interval is what is compared:
  denoise   a context with the denoiser and nothing else (the interval holds its three kernels; k_encode then
            reads the denoised frames in place);
  copy      a slot-"out" table context without a resize, whose sws stage is k_plane_copy over the luma and
            the U + V planes of those very frames and whose interval also holds k_lut_plane in place.
Bytes moved by the denoiser, a frame of B bytes: rows read B and write 2 B (uint16), columns read 2 B and write
2 B, time reads 2 B and writes B (the source again only at a sequence's first frame, the state once a submit):
about 10 B.

usage (GPU box): python3 tools/hqdn3d_probe.py [--frames 120] [--launches 6] [--prewarm 2]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, Q = 3840, 2160, 5
CONTENTS = ("noise", "testsrc")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=120, help="frames per submit")
    p.add_argument("--launches", type=int, default=6, help="timed submits of each context per content")
    p.add_argument("--prewarm", type=int, default=2)
    a = p.parse_args()
    import numpy as np
    import torch
    from ffmpeg_distributed_amd import profile
    from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes
    from ffmpeg_distributed_amd.testsrc import testsrc2_i420_torch
    dev = torch.device("cuda", 0)
    n, fb = a.frames, i420_frame_bytes(W, H, "420")
    pools = {}
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    pools["noise"] = torch.randint(88, 113, (n, fb), dtype=torch.uint8, device=dev, generator=g)
    pools["testsrc"] = torch.empty((n, fb), dtype=torch.uint8, device=dev)
    for i in range(0, n, 10):
        k = min(10, n - i)
        pools["testsrc"][i:i + k] = testsrc2_i420_torch(W, H, i, k, dev)
    torch.cuda.synchronize()
    dn = MjpegEncoder(0, W, H, full_range=True, qscale=Q, max_batch=n, chroma="420", timing=True,
                      denoise=profile.hqdn3d_tables({"ls": 4.0, "cs": 3.0, "lt": 6.0, "ct": 4.5}))
    cp = MjpegEncoder(0, W, H, full_range=True, qscale=Q, max_batch=n, chroma="420", timing=True,
                      lut_out=profile.eq_tables(dict(contrast=1.2, brightness=-0.07, saturation=1.3)))
    assert cp.scale_path(0) == 1 and cp.scale_path(1) == 1, "the sws stage is not k_plane_copy"

    def once(enc, ptr):
        enc.kernel_times(reset=True)
        enc.submit(device_ptr=ptr, nframes=n)
        enc.sync()
        ms, k = enc.kernel_times()
        assert k == 1
        return ms["scale"]

    for _ in range(a.prewarm):  # leave the idle clocks; every kernel's code loaded
        once(dn, pools["noise"].data_ptr()), once(cp, pools["noise"].data_ptr())
    mb = n * fb / 1e6
    print(f"{W}x{H} 4:2:0, {n} frames a submit resident in HBM ({mb:.0f} MB); {a.prewarm} prewarm and {a.launches} timed submits "
          f"of each context per content, denoise and copy alternating; the MJG_K_SCALE interval in ms")
    for c in CONTENTS:
        ptr = pools[c].data_ptr()
        t = np.array([(once(dn, ptr), once(cp, ptr)) for _ in range(a.launches)])
        d, k = t[:, 0], t[:, 1]
        print(f"{c:8s}: denoise median {np.median(d):.3f} (min {d.min():.3f}, max {d.max():.3f}) = {np.median(d) / n * 1e3:.1f} us a "
              f"frame, about {10 * mb / np.median(d):.0f} GB/s moved; copy + table median {np.median(k):.3f} (min {k.min():.3f}, "
              f"max {k.max():.3f}); denoise / copy = {np.median(d) / np.median(k):.1f}", flush=True)
    dn.close()
    cp.close()


if __name__ == "__main__":
    main()
