"""`-vf scale` past 4:1 (k_scale_stream), the parts that need no GPU: which size pairs still need
swscale's cascade (a filter of 256 taps or more), the worker's pre-check that sends those to
ffmpeg before any GPU call, and the interface."""
import io
import os
import re

import numpy as np
import pytest

from ffmpeg_distributed_amd import _lib, worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()


def _y4m420(w, h, n=1):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg\n".encode())
    for i in range(n):
        b.write(b"FRAME\n" + np.full(w * h * 3 // 2, 16 + i, np.uint8).tobytes())
    return b.getvalue()


def test_filter_tap_counts_at_the_edge_of_the_cascade():
    coeff, pos = _lib.sws_filter(2048, 33, 1 << 14, 4)
    assert coeff.shape == (33, 248) and pos.min() >= 0
    with pytest.raises(_lib.MjgError):
        _lib.sws_filter(1024, 16, 1 << 14, 4)  # 256 taps: swscale cascades


@pytest.mark.parametrize("size,scale,src,dst,refused", [
    ((1024, 64), (16, 8), "420", "420", True),
    ((256, 160), (32, 20), "420", "420", False),
    ((2048, 32), (33, 8), "420", "420", False),
    ((48, 1000), (16, 17), "420", "420", False),
    ((3840, 2160), (640, 360), "420", "420", False),
    ((3840, 2160), (64, 36), "420", "420", False),   # 60:1: 244 taps
    ((64, 2000), (64, 30), "444", "444", True),      # vertical only
    ((64, 48), (64, 48), "444", "420", False),       # no resize of the luma, chroma 2:1
])
def test_scale_cascade_reason(size, scale, src, dst, refused):
    why = worker.scale_cascade_reason(size, scale, src, dst)
    if refused:
        assert why == f"scale {size[0]}x{size[1]} -> {scale[0]}x{scale[1]} needs swscale's cascade"
    else:
        assert why is None


class _Reached(Exception):
    pass


def _run(monkeypatch, w, h, vf):
    """worker.run up to the first step after the pre-check (bind_numa, which precedes every GPU
    call), with ffmpeg_fallthrough recorded instead of run: no GPU, no ffmpeg."""
    calls = []

    def fallthrough(src, args, stdout, stderr=None):
        calls.append(list(args))
        src.close(kill=True)
        return 0

    def reached(device):
        raise _Reached()

    monkeypatch.setattr(worker, "ffmpeg_fallthrough", fallthrough)
    monkeypatch.setattr(worker, "bind_numa", reached)
    out, err = io.BytesIO(), io.StringIO()
    args = ["-vf", vf] + ARGS
    try:
        rc = worker.run(3, args, stdin=io.BytesIO(_y4m420(w, h)), stdout=out, stderr=err)
    except _Reached:
        rc = None
    return rc, calls, err.getvalue(), args


def test_worker_sends_a_cascade_scale_to_ffmpeg_before_any_gpu_call(monkeypatch):
    rc, calls, err, args = _run(monkeypatch, 1024, 64, "scale=16:8:flags=bicubic")
    assert rc == 0 and calls == [args]
    lines = [l for l in err.splitlines() if l.strip()]
    assert lines == ["gpu:3: scale 1024x64 -> 16x8 needs swscale's cascade; running ffmpeg on the CPU"]


def test_worker_keeps_an_8_to_1_scale_on_the_gpu(monkeypatch):
    rc, calls, err, _ = _run(monkeypatch, 256, 160, "scale=32:20:flags=bicubic")
    assert rc is None and calls == [] and "running ffmpeg" not in err  # went on towards the GPU


def test_header_declares_and_library_exports_scale_path():
    with open(os.path.join(ROOT, "include", "mjgpu.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint\s+mjg_debug_scale_path\s*\(\s*mjg_ctx\s*\*\s*ctx\s*,\s*int\s+plane\s*\)\s*;", hdr)
    L = _lib.load()
    assert "mjg_debug_scale_path" in _lib.EXPORTS and hasattr(L, "mjg_debug_scale_path")
    assert L.mjg_version() >= 103
