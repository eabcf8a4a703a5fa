"""`-vf unsharp` on the GPU (MjpegEncoder(unsharp=...): k_unsharp_plane behind the sws stage and in
front of the pad), byte for byte against tests/unsharp_ref.py.  Every case checks debug_presharp()
(the sws stage's output, the kernel's input), then debug_planes() (the sharpened planes, the
encoder's input), then the JPEGs, so a failure names the stage and the first differing sample.
tools/unsharp_host_check.py walks the launches of every geometry here (unsharp_ref.GPU_GEOMETRY) on
the CPU under AddressSanitizer."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import unsharp_ref
from unsharp_ref import DEFAULT, GPU_GEOMETRY, TILES, US2, US_LIMIT, US_TILES, US_WIDE, amount_i, sharp_planes, sharp_ref
from yadif_ref import deint_frames
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, chroma_size, i420_frame_bytes, pack_i420, split_i420

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 130, 66
NF = 3


def first_diff(a: bytes, b: bytes):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i
    return n if len(a) != len(b) else -1


def _check(got, ref):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a == b, (i, len(a), len(b), first_diff(a, b))


_SRC = {}


def _frames(w, h, c):
    """3 frames per shape and format, made once: noise with a saturated quarter, a noisy ramp, noise."""
    if (w, h, c) not in _SRC:
        rng = np.random.default_rng(1000 * w + 10 * h + int(c))
        cw, ch = chroma_size(w, h, c)
        sizes = ((w, h), (cw, ch), (cw, ch))
        a = [rng.integers(0, 256, (hh, ww), dtype=np.uint8) for ww, hh in sizes]
        for p in a:
            p[: p.shape[0] // 2, : p.shape[1] // 2] = 255
        b = [((np.add.outer(3 * np.arange(hh), 5 * np.arange(ww)) + rng.integers(0, 9, (hh, ww))) % 256).astype(np.uint8)
             for ww, hh in sizes]
        d = [rng.integers(0, 256, (hh, ww), dtype=np.uint8) for ww, hh in sizes]
        f = np.stack([pack_i420(*a), pack_i420(*b), pack_i420(*d)])
        f.setflags(write=False)
        _SRC[(w, h, c)] = f
    return _SRC[(w, h, c)]


_REF = {}


def _ref(frames_key, frames, w, h, c, us, **kw):
    """(pre planes, post planes, JPEGs) per frame for a configuration, computed once."""
    enc_kw = {k: kw.pop(k) for k in ("qscale", "sar", "huffman", "rst") if k in kw}
    key = (frames_key, w, h, c, us, tuple(sorted(kw.items())), tuple(sorted(enc_kw.items())))
    if key not in _REF:
        pl = [sharp_planes(f, w, h, c, us, **kw) for f in frames]
        jp = [sharp_ref(f, w, h, c, us, **kw, **enc_kw) for f in frames]
        _REF[key] = ([p[0] for p in pl], [p[1] for p in pl], jp)
    return _REF[key]


def _check_stage(enc, what, get, planes, dst):
    for i, want in enumerate(planes):
        got = split_i420(get(i), enc.enc_w, enc.enc_h, dst)
        for name, a, b in zip("YUV", got, want):
            bad = np.argwhere(a != b)
            if bad.size:
                y, x = bad[0]
                print(f"{what}: frame {i} plane {name}: first difference at y={y} x={x}: got {a[y, x]}, want {b[y, x]}, "
                      f"{len(bad)} of {a.size} differ")
                pytest.fail(f"{what}: frame {i} plane {name} differs first at (y={y}, x={x})")


def _run(w, h, c, us, full=False, dw=None, dh=None, dst=None, rect=None, pad=None, orient=0, frames=None, deint=None,
         q=5, **enc_kw):
    """One encoder, one encode of the shape's frames: the three stages against the reference."""
    src_frames = _frames(w, h, c)
    chain = src_frames if frames is None else frames      # what the rest of the chain sees (deinterlaced frames)
    in_size = rect[2:] if rect else ((h, w) if orient & 1 else (w, h))
    sar = profile.scaled_sar((1, 1), in_size, (dw or in_size[0], dh or in_size[1]))
    pre, post, jp = _ref((w, h, c, deint), chain, w, h, c, us, orient=orient, rect=rect, dst=dst or c, full=full, dw=dw, dh=dh,
                         pad=pad, qscale=q, sar=sar, **enc_kw)
    with MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, sar=sar, max_batch=NF, chroma=dst or c, src_chroma=c,
                      crop=rect, pad=pad, orient=orient, deint=deint, unsharp=us, **enc_kw) as enc:
        want_us = (us[0], us[1], amount_i(us[2]), us[3], us[4], amount_i(us[5]))
        assert enc.debug_unsharp() == want_us
        assert enc.scale_path(0) != 0 and enc.encode_path() & 1 == 0      # the sws stage always runs with a sharpen
        got = enc.encode(src_frames)
        _check_stage(enc, "presharp (the sws stage's output)", enc.debug_presharp, pre, dst or c)
        _check_stage(enc, "planes (k_unsharp_plane's output)", enc.debug_planes, post, dst or c)
    _check(got, jp)
    return got


def test_the_geometry_list_is_what_the_cases_below_encode():
    """tools/unsharp_host_check.py walks unsharp_ref.GPU_GEOMETRY: keep it in step with the cases."""
    assert [g[:3] + g[7:] for g in GPU_GEOMETRY] == [
        (70, 38, "420", DEFAULT), (70, 38, "420", US2), (TILES[0], TILES[1], "444", US_TILES), (6, 6, "444", US_WIDE),
        (40, 24, "444", US_LIMIT), (80, 48, "420", DEFAULT), (48, 80, "420", DEFAULT), (50, 38, "420", US2),
        (64, 32, "420", DEFAULT)]
    assert TILES[0] > unsharp_ref.kernel_constant("kSharpTileW") + 4
    assert TILES[1] > 2 * unsharp_ref.kernel_constant("kSharpTileH")


# ------------------------------------------------------------------------- 1, 2. scale, then the filter
def test_scale_unsharp_defaults_copy_the_chroma():
    """130 x 66 4:2:0 tv -> scale=70:38,unsharp: luma 5x5 at 1.0, the 35 x 19 chroma planes copied."""
    _run(W, H, "420", DEFAULT, dw=70, dh=38)


def test_scale_unsharp_asymmetric_windows_and_a_blur():
    _run(W, H, "420", US2, dw=70, dh=38)


# ------------------------------------------------------------------------- 3. tiles
def test_tiles_abut_in_both_directions_and_the_last_is_partial():
    """A 4:4:4 plane of two tile columns and three tile rows; luma through <5, 5>, chroma 3x5 at run time."""
    _run(100, 90, "444", US_TILES, dw=TILES[0], dh=TILES[1])


# ------------------------------------------------------------------------- 4, 5. windows
def test_window_wider_than_the_plane_every_tap_clamps():
    """23:3 luma and 3:23 chroma on a 6 x 6 4:4:4 full-range source without a scale."""
    _run(6, 6, "444", US_WIDE, full=True)


def test_13x13_the_32_bit_limit():
    """sx + sy = 12 on 40 x 24: the saturated quarter of frame 0 takes the sum to 255 * 2^24."""
    _run(40, 24, "444", US_LIMIT, full=True)


# ------------------------------------------------------------------------- 6, 7. the pad and the chain
def test_scale_unsharp_pad_picture_edges_against_the_border():
    _run(W, H, "420", DEFAULT, dw=64, dh=32, pad=(8, 8, 80, 48))


def test_yadif_transpose_crop_scale_unsharp_pad_chain():
    d = deint_frames(_frames(W, H, "420"), W, H, "420", 0, 1)
    _run(W, H, "420", DEFAULT, orient=3, rect=(2, 2, 62, 126), dw=32, dh=64, pad=(8, 8, 48, 80), frames=d,
         deint=_lib.MJG_DEINT_YADIF)


def test_unsharp_pad_without_a_scale_the_planes_keep_their_size():
    """A full-range source, no scale: k_pad_plane copies the picture into the canvas, then the sharpen."""
    _run(34, 18, "420", US2, full=True, pad=(8, 10, 50, 38))


def test_crop_unsharp_without_a_scale():
    """The rectangle of wider rows through k_plane_copy, then the sharpen; the tile is exactly one 64 x 32."""
    _run(W, H, "420", DEFAULT, full=True, rect=(2, 2, 64, 32))


# ------------------------------------------------------------------------- 8. -pix_fmt
def test_pix_fmt_420_from_444_with_a_scale():
    _run(W, H, "444", US2, dw=70, dh=38, dst="420")


# ------------------------------------------------------------------------- 9. merged submits and segments
def _single(w, h, c, us, dw, dh):
    return _run(w, h, c, us, dw=dw, dh=dh)


def test_merged_submits_and_segments_give_the_bytes_of_single_submits():
    import torch
    frames = _frames(W, H, "420")
    want = _single(W, H, "420", DEFAULT, 70, 38)
    sar = profile.scaled_sar((1, 1), (W, H), (70, 38))
    segs = [torch.from_numpy(frames[lo:lo + n].copy()).to("cuda:0") for lo, n in ((0, 2), (2, 1))]
    torch.cuda.synchronize()
    got = []
    with MjpegEncoder(0, W, H, 70, 38, full_range=False, qscale=5, sar=sar, max_batch=NF, chroma="420", merge=True,
                      unsharp=DEFAULT) as enc:
        for t in segs:
            enc.submit(device_ptr=t.data_ptr(), nframes=t.shape[0])
        for _ in segs:
            enc.sync()
            got += enc.fetch()
    _check(got, want)
    with MjpegEncoder(0, W, H, 70, 38, full_range=False, qscale=5, sar=sar, max_batch=NF, chroma="420",
                      unsharp=DEFAULT) as enc:
        enc.submit_segments([(t.data_ptr(), t.shape[0]) for t in segs])
        got = enc.fetch()
    _check(got, want)


# ------------------------------------------------------------------------- 10. RST and -huffman optimal
@pytest.mark.parametrize("kw", [dict(huffman="optimal"), dict(rst=True)], ids=["optimal", "rst"])
def test_unsharp_huffman_optimal_and_rst(kw):
    _run(W, H, "420", DEFAULT, dw=70, dh=38, **kw)


# ------------------------------------------------------------------------- no filter
def test_zero_amounts_open_a_context_without_a_sharpen():
    frames = _frames(W, H, "420")
    out = []
    for extra in (dict(), dict(unsharp=(5, 5, 0.0, 7, 3, 0.0))):
        with MjpegEncoder(0, W, H, 70, 38, full_range=False, qscale=5, max_batch=NF, chroma="420", timing=True,
                          **extra) as enc:
            assert enc.debug_unsharp() is None
            jp = enc.encode(frames)
            with pytest.raises(_lib.MjgError) as e:
                enc.debug_presharp(0)
            assert e.value.code == _lib.MJG_E_STATE
            out.append((jp, enc.scale_path(0), enc.scale_path(1), enc.encode_path()))
    _check(out[1][0], out[0][0])
    assert out[0][1:] == out[1][1:]


def test_the_sharpen_runs_inside_the_scale_interval():
    with MjpegEncoder(0, 6, 6, full_range=True, qscale=5, max_batch=NF, chroma="444", timing=True, unsharp=US_WIDE) as enc:
        enc.encode(_frames(6, 6, "444"))
        ms, n = enc.kernel_times()
    assert n == 1 and ms["scale"] > 0


# ------------------------------------------------------------------------- 11. the worker
def _y4m420(frames, w, h, mpeg=False):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def test_worker_scale_unsharp():
    frames = _frames(W, H, "420")
    args = ["-vf", "scale=70:38,unsharp"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, W, H)), stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets = [d for _, d in r.frames(1)]
    info = r.info(1)
    assert (info.width, info.height, info.codec) == (70, 38, "V_MJPEG")
    sar = profile.scaled_sar((1, 1), (W, H), (70, 38))
    _, _, ref = _ref((W, H, "420", None), frames, W, H, "420", DEFAULT, orient=0, rect=None, dst="420", full=False, dw=70,
                     dh=38, pad=None, qscale=profile.effective_qscale(5), sar=sar)
    _check(packets, ref)


def test_worker_sends_a_tv_source_without_a_scale_to_ffmpeg(tmp_path):
    log = tmp_path / "shim.log"
    env = dict(os.environ, PATH=os.path.join(HERE, "shims") + os.pathsep + os.environ["PATH"],
               SHIM_LOG=str(log), PYTHONPATH=ROOT)
    w, h = 16, 8
    fr = np.full((3, w * h + 2 * 8 * 4), 0x41, np.uint8)      # ASCII-safe: the shim reads text
    args = ["-vf", "unsharp"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    p = subprocess.run([sys.executable, "-m", "ffmpeg_distributed_amd.worker", "--device", "0", *args],
                       input=_y4m420(fr, w, h), capture_output=True, env=env, timeout=60)
    assert p.returncode == 0, p.stderr
    assert b"unsharp without a scale on a tv-range / converted input: FFmpeg sharpens before its converter" in p.stderr
    assert b"running ffmpeg on the CPU" in p.stderr
    calls = [json.loads(l) for l in open(log)]
    assert calls == [{"prog": "ffmpeg", "argv": ["-f", "yuv4mpegpipe", "-i", "pipe:", *args, "-f", "matroska", "pipe:"],
                      "host": "localhost"}]
