"""`-vf crop[,scale]` on the GPU (MjpegEncoder(crop=(x, y, w, h)): whole frames in, a rectangle of
them encoded), byte for byte against the reference cut by numpy and composed from the CPU
oracle (tests/crop_ref.py).  Crop only: k_encode reads the rectangle in place (fetch_rows at any
alignment).  With a resize or a -pix_fmt conversion the sws stage reads it (k_scale's windows,
k_plane_copy's rectangle form) and k_encode its packed output.  The noise outside the rectangle
is what shows a read past the crop's edge."""
import io
from fractions import Fraction

import numpy as np
import pytest

from chroma_resample_ref import source_frames
from crop_ref import crop_frame, cropped_planes, cropped_ref, same_inside
from ffmpeg_distributed_amd import container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes, pack_i420, split_i420

pytestmark = pytest.mark.gpu

W, H = 130, 66
RECTS = [(0, 0, 130, 66), (16, 16, 64, 32), (2, 2, 126, 62), (6, 10, 33, 17), (122, 58, 8, 8)]
CROP_ONLY = ([(c, W, H, r) for c in ("420", "422", "444") for r in RECTS]
             + [("444", W, H, (1, 3, 9, 17)), ("422", W, H, (2, 3, 33, 17)),
                ("444", 33, 17, (1, 1, 24, 16))])  # 33x17 4:4:4: odd frame bytes, every frame base misaligned


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


def _refs(frames, w, h, src, rect, **kw):
    return [cropped_ref(f, w, h, src, rect, **kw) for f in frames]


def _check_planes(enc, frames, w, h, src, rect, dst, full, dw=None, dh=None):
    """debug_planes() of the last submit against the composed planes of the cropped frames."""
    dw, dh = dw or rect[2], dh or rect[3]
    for i, f in enumerate(frames):
        got = split_i420(enc.debug_planes(i), dw, dh, dst)
        for name, a, b in zip("YUV", got, cropped_planes(f, w, h, src, rect, dst, full, dw, dh)):
            bad = np.argwhere(a != b)
            assert bad.size == 0, (i, name, len(bad), bad[:4].tolist())


_SRC = {}


def _frames(w, h, c):
    """3 frames (two noise, one smooth) per source shape and format, made once."""
    if (w, h, c) not in _SRC:
        f = source_frames(w, h, 3, 100 * w + h, c)
        f.setflags(write=False)
        _SRC[(w, h, c)] = f
    return _SRC[(w, h, c)]


@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
@pytest.mark.parametrize("c,w,h,rect", CROP_ONLY, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_crop_only_matches_reference(c, w, h, rect, full):
    frames = _frames(w, h, c)
    with MjpegEncoder(0, w, h, full_range=full, qscale=4, max_batch=3, chroma=c, crop=rect) as enc:
        assert enc.frame_bytes == i420_frame_bytes(w, h, c)  # whole frames are handed over
        assert (enc.dst_w, enc.dst_h) == rect[2:]
        got = enc.encode(frames)
    _check(got, _refs(frames, w, h, c, rect, full_range=full, qscale=4))
    if rect == (0, 0, w, h):  # the full rectangle: the bytes of an encoder opened without crop
        with MjpegEncoder(0, w, h, full_range=full, qscale=4, max_batch=3, chroma=c) as enc:
            assert enc.encode(frames) == got


@pytest.mark.parametrize("c", ["420", "422", "444"])
def test_nothing_outside_the_rectangle_reaches_the_result(c):
    rect = (6, 10, 33, 17)
    a = _frames(W, H, c)
    b = same_inside(a, W, H, c, rect, 77)
    assert (a != b).mean() > 0.5
    with MjpegEncoder(0, W, H, full_range=False, qscale=4, max_batch=3, chroma=c, crop=rect) as enc:
        ga = enc.encode(a)
        gb = enc.encode(b)
    _check(gb, ga)


@pytest.mark.parametrize("c", ["420", "422", "444"])
def test_unaligned_fetch_off_gives_the_same_bytes(c, monkeypatch):
    """MJG_UNALIGNED_FETCH=0 (read at open): the misaligned blocks take fetch_rows_edge's byte
    loads instead of the 8-byte rows at any alignment."""
    rect = (2, 2, 126, 62)
    frames = _frames(W, H, c)
    out = []
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("MJG_UNALIGNED_FETCH", env)
        with MjpegEncoder(0, W, H, full_range=False, qscale=4, max_batch=3, chroma=c, crop=rect) as enc:
            out.append(enc.encode(frames))
    _check(out[1], out[0])
    _check(out[0], _refs(frames, W, H, c, rect, qscale=4))


@pytest.mark.parametrize("c", ["420", "444"])
def test_crop_then_scale(c):
    rect, dw, dh = (2, 2, 126, 62), 64, 32
    frames = _frames(W, H, c)
    sar = profile.scaled_sar((1, 1), rect[2:], (dw, dh))
    with MjpegEncoder(0, W, H, dw, dh, full_range=False, qscale=5, sar=sar, max_batch=3, chroma=c,
                      crop=rect) as enc:
        got = enc.encode(frames)
        _check_planes(enc, frames, W, H, c, rect, c, False, dw, dh)
    _check(got, _refs(frames, W, H, c, rect, dw=dw, dh=dh, sar=sar))


def test_crop_then_exact_2to1_matrix_core_tiles():
    """1012x608 4:2:0, (6,4,1000,600) -> 500x300: luma has 8 tile columns and 5 tile rows, so
    interior tiles take both matrix-core passes; the luma window loads start at odd multiples of
    2 bytes in 1012-byte rows, the chroma ones at byte 3 of 506-byte rows."""
    w, h, rect, dw, dh, c = 1012, 608, (6, 4, 1000, 600), 500, 300, "420"
    frames = _frames(w, h, c)
    with MjpegEncoder(0, w, h, dw, dh, full_range=False, qscale=5, max_batch=3, chroma=c, crop=rect) as enc:
        got = enc.encode(frames)
        _check_planes(enc, frames, w, h, c, rect, c, False, dw, dh)
    _check(got, _refs(frames, w, h, c, rect, dw=dw, dh=dh))


PIX_FMT = [("444", "420", (3, 5, 101, 57)), ("444", "422", (3, 5, 101, 57)), ("422", "420", (2, 5, 100, 57))]


@pytest.mark.parametrize("copy_kernel", [True, False], ids=["k_plane_copy", "k_scale_identity"])
@pytest.mark.parametrize("src,dst,rect", PIX_FMT, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_crop_with_pix_fmt_no_resize(src, dst, rect, copy_kernel, monkeypatch):
    """Luma keeps its size: rows of 101 (100) bytes out of 130, gathered into the packed plane by
    k_plane_copy's rectangle form, or (MJG_PLANE_COPY=0) by k_scale's identity filters."""
    if not copy_kernel:
        monkeypatch.setenv("MJG_PLANE_COPY", "0")
    frames = _frames(W, H, src)
    with MjpegEncoder(0, W, H, full_range=False, qscale=4, max_batch=3, chroma=dst, src_chroma=src,
                      crop=rect) as enc:
        got = enc.encode(frames)
        _check_planes(enc, frames, W, H, src, rect, dst, False)
    _check(got, _refs(frames, W, H, src, rect, dst=dst, qscale=4))


@pytest.mark.parametrize("copy_kernel", [True, False], ids=["k_plane_copy", "k_scale_identity"])
def test_cropped_luma_with_every_byte_value(copy_kernel, monkeypatch):
    """444 -> 422, tv range: the cropped luma (33x17 at (3,5)) holds every byte value, so the
    rectangle copy's tv->pc table is read at every entry."""
    if not copy_kernel:
        monkeypatch.setenv("MJG_PLANE_COPY", "0")
    src, dst, rect = "444", "422", (3, 5, 33, 17)
    rng = np.random.default_rng(3)
    y, u, v = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    y[5:22, 3:36] = (np.arange(33 * 17) % 256).astype(np.uint8).reshape(17, 33)
    frames = np.stack([pack_i420(y, u, v), pack_i420(y[::-1], v, u)])
    assert len(np.unique(split_i420(crop_frame(frames[0], W, H, src, rect), 33, 17, src)[0])) == 256
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=2, chroma=dst, src_chroma=src,
                      crop=rect) as enc:
        got = enc.encode(frames)
        _check_planes(enc, frames, W, H, src, rect, dst, False)
    _check(got, _refs(frames, W, H, src, rect, dst=dst))


def test_crop_scale_and_pix_fmt_together():
    src, dst, rect, dw, dh = "444", "420", (3, 5, 120, 56), 64, 32
    frames = _frames(W, H, src)
    sar = profile.scaled_sar((1, 1), rect[2:], (dw, dh))
    with MjpegEncoder(0, W, H, dw, dh, full_range=False, qscale=5, sar=sar, max_batch=3, chroma=dst,
                      src_chroma=src, crop=rect) as enc:
        got = enc.encode(frames)
        _check_planes(enc, frames, W, H, src, rect, dst, False, dw, dh)
    _check(got, _refs(frames, W, H, src, rect, dst=dst, dw=dw, dh=dh, sar=sar))


@pytest.mark.parametrize("kw", [dict(huffman="optimal"), dict(rst=True)], ids=["optimal", "rst"])
def test_crop_huffman_optimal_and_rst(kw):
    """The counting instantiation of k_encode reads the source rectangle too."""
    rect, c = (2, 2, 126, 62), "420"
    frames = _frames(W, H, c)
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=3, chroma=c, crop=rect, **kw) as enc:
        got = enc.encode(frames)
    _check(got, _refs(frames, W, H, c, rect, **kw))


def test_submit_segments_from_odd_device_pointers():
    """Two segments of 2 and 1 frames, each a uint8 tensor sliced from byte 1 of its allocation."""
    import torch
    rect, c = (2, 2, 126, 62), "420"
    frames = _frames(W, H, c)
    dev = torch.device("cuda", 0)
    segs = []
    for lo, n in ((0, 2), (2, 1)):
        pool = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device=dev)
        pool[1:] = torch.from_numpy(frames[lo:lo + n].reshape(-1).copy()).to(dev)
        segs.append((pool[1:], n))
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 2 == 1 for t, _ in segs)
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=3, chroma=c, crop=rect) as enc:
        enc.submit_segments([(t.data_ptr(), n) for t, n in segs])
        got = enc.fetch()
    _check(got, _refs(frames, W, H, c, rect))


def _y4m420(frames, w, h):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


@pytest.mark.parametrize("scale", [None, (64, 32)], ids=["crop", "crop_scale_64x32"])
def test_worker_crop(scale):
    rect, c = (2, 2, 126, 62), "420"
    frames = _frames(W, H, c)
    vf = "crop=126:62:2:2" + (f",scale={scale[0]}:{scale[1]}" if scale else "")
    args = ["-vf", vf] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, W, H)), stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets = [d for _, d in r.frames(1)]
    dw, dh = scale or rect[2:]
    info = r.info(1)
    assert (info.width, info.height, info.codec) == (dw, dh, "V_MJPEG")
    sar = profile.scaled_sar((1, 1), rect[2:], (dw, dh))
    # the crop leaves the SAR alone, the scale changes it from the rectangle's size: in the
    # Matroska track as the display width (rounded to a pixel), exactly in every JPEG's APP0
    assert sar == ((1, 1) if scale is None else (63, 62))
    assert Fraction(*info.sar) == Fraction(round(Fraction(dw * sar[0], sar[1])), dw)
    _check(packets, _refs(frames, W, H, c, rect, dw=dw, dh=dh, qscale=profile.effective_qscale(5), sar=sar))


def test_worker_crop_larger_than_the_input_fails_like_ffmpeg(monkeypatch, tmp_path):
    """One line on stderr, a nonzero exit, no ffmpeg child (PATH holds nothing to start)."""
    monkeypatch.setenv("PATH", str(tmp_path))
    frames = _frames(W, H, "420")
    args = ["-vf", "crop=200:62:2:2"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, W, H)), stdout=out, stderr=err)
    assert rc == 1
    lines = [l for l in err.getvalue().splitlines() if l.strip()]
    assert len(lines) == 1 and "crop" in lines[0] and "200" in lines[0], err.getvalue()
    assert "ffmpeg" not in err.getvalue() and out.getvalue() == b""
