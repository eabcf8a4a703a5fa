"""`-vf scale` past 4:1 on the GPU: k_scale_stream (scale.hip), byte for byte against the
reference composed from the CPU oracle (tests/chroma_resample_ref.py, tests/crop_ref.py:
oracle.scale_plane per plane, then oracle.encode_frame).  The planes are compared first
(mjg_debug_planes), so a failure names the stage, and every test asserts through
enc.scale_path() that the plane it is about ran on the kernel it means to check.  Without the
streaming kernel each shape of SHAPES is refused at open ("scale ratio too large for one LDS
tile")."""
import io

import numpy as np
import pytest

from chroma_resample_ref import composed_frame, composed_planes, source_frames
from crop_ref import cropped_planes, cropped_ref, same_inside
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, chroma_size, i420_frame_bytes, pack_i420, split_i420

pytestmark = pytest.mark.gpu

COPY, TILE, STREAM = 1, 2, 3


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


def _check_planes(enc, frames, w, h, src, dst, full, dw, dh, planes=None):
    for i, f in enumerate(frames):
        got = split_i420(enc.debug_planes(i), dw, dh, dst)
        ref = planes[i] if planes is not None else composed_planes(f, w, h, src, dst, full, dw, dh)
        for name, a, b in zip("YUV", got, ref):
            bad = np.argwhere(a != b)
            assert bad.size == 0, (i, name, len(bad), bad[:4].tolist())


_SRC = {}


def _frames(w, h, c, n=3):
    """n frames (noise, the last one smooth) per source shape and format, made once."""
    if (w, h, c, n) not in _SRC:
        f = source_frames(w, h, n, 100 * w + h, c)
        f.setflags(write=False)
        _SRC[(w, h, c, n)] = f
    return _SRC[(w, h, c, n)]


def _run(frames, w, h, dw, dh, c, full=False, q=5, paths=(STREAM, None), batch=None, src=None, **kw):
    """Encode (host submits of at most `batch` frames), check paths, planes and bytes."""
    src = src or c
    refs = [composed_frame(f, w, h, src, c, full, dw, dh, qscale=q, **kw) for f in frames]
    n = len(frames)
    with MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, max_batch=batch or n, chroma=c,
                      src_chroma=src, **kw) as enc:
        for p in (0, 1):
            if paths[p] is not None:
                assert enc.scale_path(p) == paths[p], (p, enc.scale_path(p))
        got = enc.encode(frames)
        last = (n - 1) % (batch or n) + 1  # frames of the last submit
        _check_planes(enc, frames[n - last:], w, h, src, c, full, dw, dh)
    _check(got, refs)
    return got


# (w, h, dw, dh, chroma, frames, what it reaches): each refused by the tile kernel's LDS check
SHAPES = [
    (256, 160, 32, 20, "420", 3, (STREAM, TILE)),    # 8:1, 32 taps both ways; luma stream + chroma tile
    (640, 480, 160, 96, "422", 2, (STREAM, None)),   # 4:1 x 5:1: D4 coefficients, 3 strips, 2 bands
    (523, 301, 97, 55, "444", 2, (STREAM, STREAM)),  # odd everything, partial strip, odd plane offsets
    (1100, 700, 200, 100, "420", 1, (STREAM, None)),  # 4 strips, 2 bands: the band overlap
    (2048, 32, 33, 8, "420", 2, (STREAM, None)),     # 248 h taps: the widest window and coefficient rows
    (48, 1000, 16, 17, "420", 2, (STREAM, None)),    # 234 v taps: the deepest ring
    (40, 1000, 80, 17, "420", 2, (STREAM, None)),    # ... under a 1:2 h upscale (4 h taps)
    (64, 640, 128, 40, "420", 2, (STREAM, None)),    # 64 v taps under an h upscale
]
_IDS = [f"{s[0]}x{s[1]}_{s[2]}x{s[3]}_{s[4]}" for s in SHAPES]


@pytest.mark.parametrize("full", [False, True], ids=["tv", "pc"])
@pytest.mark.parametrize("w,h,dw,dh,c,n,paths", SHAPES, ids=_IDS)
def test_shapes_past_one_tile_match_reference(w, h, dw, dh, c, n, paths, full):
    _run(_frames(w, h, c, n), w, h, dw, dh, c, full=full, paths=paths)


def test_filters_of_the_extreme_shapes():
    """The tap counts the table above names (the library's own tables, device-free)."""
    assert _lib.sws_filter(2048, 33, 1 << 14, 4)[0].shape[1] == 248
    assert _lib.sws_filter(1000, 17, 1 << 12, 2)[0].shape[1] == 234
    assert _lib.sws_filter(640, 40, 1 << 12, 2)[0].shape[1] == 64
    assert _lib.sws_filter(256, 32, 1 << 14, 4)[0].shape[1] == 32


@pytest.mark.parametrize("q", [2, 31])
def test_quality_ends(q):
    _run(_frames(256, 160, "420"), 256, 160, 32, 20, "420", q=q, paths=(STREAM, TILE))


@pytest.mark.parametrize("kw", [dict(huffman="optimal"), dict(rst=True)], ids=["optimal", "rst"])
@pytest.mark.parametrize("w,h,dw,dh,c", [(523, 301, 97, 55, "444"), (640, 480, 160, 96, "422")])
def test_huffman_optimal_and_rst(w, h, dw, dh, c, kw):
    _run(_frames(w, h, c, 2), w, h, dw, dh, c, **kw)


@pytest.mark.parametrize("w,h,dw,dh,c", [(256, 160, 32, 20, "420"), (523, 301, 97, 55, "444")])
def test_ragged_submits(w, h, dw, dh, c):
    """3 frames with max_batch 2: a submit of 2 and one of 1 through the same context."""
    _run(_frames(w, h, c), w, h, dw, dh, c, batch=2)


def test_pix_fmt_with_scale_luma_tile_chroma_stream():
    """4:4:4 384x240 -pix_fmt yuvj420p at 128x80: luma 3:1 on the tile kernel, chroma 384x240 ->
    64x40 (6:1) on the streaming one, in one context."""
    w, h, dw, dh = 384, 240, 128, 80
    for full in (False, True):
        _run(_frames(w, h, "444"), w, h, dw, dh, "420", src="444", full=full, paths=(TILE, STREAM))


# A cropped source: rows of rect[2] bytes out of W at an offset (s_stride != sw, s_off).  The
# 262x151 rectangle's planes are small enough for one tile each at any target size (the tile is
# then the whole plane: 62,464 B for 49x28 by the tile kernel's LDS formula), so that shape runs
# the streaming kernel through MJG_SCALE_STREAM=1; the 523x301 rectangle reaches it by itself.
CROPS = [(320, 200, (30, 20, 262, 151), 49, 28, True), (640, 400, (30, 20, 523, 301), 97, 55, False)]


@pytest.mark.parametrize("src,dst", [("420", "420"), ("444", "420")], ids=["crop_scale", "crop_scale_pix_fmt"])
@pytest.mark.parametrize("W,H,rect,dw,dh,force", CROPS, ids=["262x151_49x28", "523x301_97x55"])
def test_crop_then_scale_on_the_stream_kernel(W, H, rect, dw, dh, force, src, dst, monkeypatch):
    """Noise outside the rectangle must not reach the result."""
    if force:
        monkeypatch.setenv("MJG_SCALE_STREAM", "1")
    a = _frames(W, H, src)
    b = same_inside(a, W, H, src, rect, 78)
    assert (a != b).mean() > 0.3
    refs = [cropped_ref(f, W, H, src, rect, dst=dst, dw=dw, dh=dh) for f in a]
    with MjpegEncoder(0, W, H, dw, dh, full_range=False, qscale=5, max_batch=3, chroma=dst, src_chroma=src,
                      crop=rect) as enc:
        # (the 4:2:0 chroma planes of the larger rectangle are 262x151 again: one tile)
        assert enc.scale_path(0) == STREAM
        assert enc.scale_path(1) == (STREAM if force or src == "444" else TILE)
        ga = enc.encode(a)
        planes = [cropped_planes(f, W, H, src, rect, dst, False, dw, dh) for f in a]
        _check_planes(enc, a, W, H, src, dst, False, dw, dh, planes=planes)
        gb = enc.encode(b)
    _check(ga, refs)
    _check(gb, ga)


def _patterns(w, h, c):
    """Full-swing content against the filters' negative lobes: stripes, checkers, and bands of
    0 / 255 rows and columns of several widths."""
    cw, ch = chroma_size(w, h, c)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:ch, 0:cw]
    out = []
    for k in (1, 3, 8):
        out.append(pack_i420((255 * ((xx // k) & 1)).astype(np.uint8), (255 * ((cy // k) & 1)).astype(np.uint8),
                             (255 * (((cx + cy) // k) & 1)).astype(np.uint8)))
        out.append(pack_i420((255 * (((xx // k) + (yy // k)) & 1)).astype(np.uint8),
                             (255 * ((cx // k) & 1)).astype(np.uint8), (255 * ((cy // k) & 1)).astype(np.uint8)))
    y = np.zeros((h, w), np.uint8)
    y[h // 3:h // 3 + 37] = 255
    y[:, w // 4:w // 4 + 53] ^= 255
    u = np.full((ch, cw), 255, np.uint8)
    u[ch // 2:ch // 2 + 11] = 0
    v = np.zeros((ch, cw), np.uint8)
    v[:, cw // 3:cw // 3 + 29] = 255
    out.append(pack_i420(y, u, v))
    out.append(pack_i420(255 - y, 255 - u, 255 - v))
    return np.stack(out)


@pytest.mark.parametrize("full", [False, True], ids=["tv", "pc"])
@pytest.mark.parametrize("w,h,dw,dh,c", [(256, 160, 32, 20, "420"), (523, 301, 97, 55, "444")])
def test_full_swing_patterns(w, h, dw, dh, c, full):
    _run(_patterns(w, h, c), w, h, dw, dh, c, full=full)


def test_two_device_segments_and_a_host_submit():
    """One mjg_submit_segments of 2 + 1 frames, each a tensor sliced from byte 1 of its allocation
    (the byte after the last frame belongs to nobody), then the same frames as one host submit."""
    import torch
    w, h, dw, dh, c = 523, 301, 97, 55, "444"
    frames = _frames(w, h, c)
    refs = [composed_frame(f, w, h, c, c, False, dw, dh) for f in frames]
    dev = torch.device("cuda", 0)
    segs = []
    for lo, n in ((0, 2), (2, 1)):
        pool = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device=dev)
        pool[1:] = torch.from_numpy(frames[lo:lo + n].reshape(-1).copy()).to(dev)
        segs.append((pool[1:], n))
    torch.cuda.synchronize()
    with MjpegEncoder(0, w, h, dw, dh, full_range=False, qscale=5, max_batch=3, chroma=c) as enc:
        assert enc.scale_path(0) == STREAM and enc.scale_path(1) == STREAM
        enc.submit_segments([(t.data_ptr(), n) for t, n in segs])
        got = enc.fetch()
        _check_planes(enc, frames, w, h, c, c, False, dw, dh)
        host = enc.encode(frames)
    _check(got, refs)
    _check(host, refs)


# Shapes the tile kernel takes: with MJG_SCALE_STREAM=1 the streaming kernel must give the bytes of
# the default path and of the oracle.  (w, h, dw, dh, src, dst)
AB = [
    (128, 96, 64, 48, "420", "420"),     # 2:1
    (250, 130, 125, 65, "420", "420"),   # 2:1, odd chroma planes
    (192, 120, 64, 40, "420", "420"),    # 3:1
    (256, 160, 64, 40, "422", "422"),    # 4:1
    (300, 200, 100, 50, "444", "444"),   # 3:1 x 4:1
    (200, 120, 100, 40, "420", "420"),   # 2:1 x 3:1, more than one strip
    (64, 40, 128, 80, "420", "420"),     # 1:2 up
    (97, 55, 200, 100, "444", "444"),    # up, no integer ratio, 4 strips and 2 bands
    (130, 66, 130, 66, "422", "420"),    # chroma: identity across, 2:1 down (luma: the copy)
    (130, 66, 130, 66, "444", "422"),    # chroma: 2:1 across, identity down
    (33, 17, 16, 9, "444", "444"),       # odd plane offsets and frame strides
    (9, 9, 8, 8, "420", "420"),
]


@pytest.mark.parametrize("w,h,dw,dh,src,dst", AB, ids=["_".join(map(str, s)) for s in AB])
def test_stream_kernel_equals_tile_kernel_and_oracle(w, h, dw, dh, src, dst, monkeypatch):
    frames = _frames(w, h, src)
    resized = (w, h) != (dw, dh)
    out = []
    for env in (None, "1"):
        if env is not None:
            monkeypatch.setenv("MJG_SCALE_STREAM", env)
        want = (STREAM if env else TILE)
        with MjpegEncoder(0, w, h, dw, dh, full_range=False, qscale=4, max_batch=3, chroma=dst,
                          src_chroma=src) as enc:
            assert enc.scale_path(0) == (want if resized else COPY)
            assert enc.scale_path(1) == want
            out.append(enc.encode(frames))
            _check_planes(enc, frames, w, h, src, dst, False, dw, dh)
    _check(out[1], out[0])
    _check(out[1], [composed_frame(f, w, h, src, dst, False, dw, dh, qscale=4) for f in frames])


def _taps_ok(s, d, one, align):
    try:
        _lib.sws_filter(s, d, one, align)
        return True
    except _lib.MjgError:
        return False


def _sweep_configs(seed, count):
    """`count` configurations: sources 64..700 x 48..500, a ratio of 4.2..12 drawn per direction,
    every format, both ranges, q / huffman / rst drawn.  A draw whose filter would reach 256 taps
    is drawn again (none does below 64:1; the loop says so rather than skip)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        w, h = int(rng.integers(64, 701)), int(rng.integers(48, 501))
        rx, ry = rng.uniform(4.2, 12, 2)
        dw, dh = max(1, int(round(w / rx))), max(1, int(round(h / ry)))
        c = ("420", "422", "444")[int(rng.integers(3))]
        full = bool(rng.integers(2))
        q = int((2, 5, 31)[int(rng.integers(3))])
        kw = ({}, dict(huffman="optimal"), dict(rst=True))[int(rng.integers(3))]
        cw, ch = chroma_size(w, h, c)
        dcw, dch = chroma_size(dw, dh, c)
        if not all(_taps_ok(s, d, one, al) for s, d, one, al in
                   ((w, dw, 1 << 14, 4), (h, dh, 1 << 12, 2), (cw, dcw, 1 << 14, 4), (ch, dch, 1 << 12, 2))):
            continue
        out.append((w, h, dw, dh, c, full, q, kw, int(rng.integers(1 << 30))))
    return out


def test_seeded_sweep():
    """40 drawn configurations, one frame each.  A small source fits one tile at any ratio (the
    tile is the whole plane), and of 400 seeds the median draws 29 shapes past the tile kernel's
    LDS limit; seed 119 draws 38 (counted on the CPU with that kernel's LDS formula, before the
    streaming kernel ran once), so at least 36 must report k_scale_stream."""
    ran = 0
    for i, (w, h, dw, dh, c, full, q, kw, fseed) in enumerate(_sweep_configs(119, 40)):
        frame = np.random.default_rng(fseed).integers(0, 256, i420_frame_bytes(w, h, c), dtype=np.uint8)
        ref = composed_frame(frame, w, h, c, c, full, dw, dh, qscale=q, **kw)
        with MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, max_batch=1, chroma=c, **kw) as enc:
            ran += STREAM in (enc.scale_path(0), enc.scale_path(1))
            got = enc.encode(frame[None])
            _check_planes(enc, frame[None], w, h, c, c, full, dw, dh)
        assert got[0] == ref, (i, w, h, dw, dh, c, full, q, kw, first_diff(got[0], ref))
    assert ran >= 36, ran


def _y4m420(frames, w, h):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def test_worker_scale_8_to_1():
    w, h, dw, dh = 256, 160, 32, 20
    frames = _frames(w, h, "420")
    args = ["-vf", f"scale={dw}:{dh}:flags=bicubic"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, w, h)), stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets = [d for _, d in r.frames(1)]
    info = r.info(1)
    assert (info.width, info.height, info.codec) == (dw, dh, "V_MJPEG")
    sar = profile.scaled_sar((1, 1), (w, h), (dw, dh))
    _check(packets, [composed_frame(f, w, h, "420", "420", False, dw, dh, qscale=profile.effective_qscale(5), sar=sar)
                     for f in frames])
