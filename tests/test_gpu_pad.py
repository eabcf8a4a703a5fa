"""`-vf ...,pad` on the GPU (MjpegEncoder(pad=(x, y, W, H)): the picture on a black canvas), byte
for byte against the reference placed by numpy and composed from the CPU oracle
(tests/pad_ref.py).  Pad only: k_pad_plane copies the picture (tv->pc through its table) and
writes the border.  With a resize or a -pix_fmt conversion k_scale / k_scale_stream write the
picture into the canvas at its stride and k_pad_plane only the border.  debug_planes() is the
canvas k_encode reads: its picture part must be the composed planes, every other byte 0 / 128."""
import io
from fractions import Fraction

import numpy as np
import pytest

from chroma_resample_ref import source_frames
from crop_ref import same_inside
from pad_ref import BORDER, pad_planes, padded_planes, padded_ref
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import CHROMA_SHIFTS, MjpegEncoder, i420_frame_bytes, split_i420

pytestmark = pytest.mark.gpu

NONE, COPY, TILE, STREAM, PADCOPY = 0, 1, 2, 3, 4
W, H = 130, 66


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
    """3 frames (two noise, one smooth) per source shape and format, made once."""
    if (w, h, c) not in _SRC:
        f = source_frames(w, h, 3, 100 * w + h + 7, c)
        f.setflags(write=False)
        _SRC[(w, h, c)] = f
    return _SRC[(w, h, c)]


_REF = {}


def _ref(w, h, src, rect, dst, full, dw, dh, pad, **kw):
    """(canvas planes, JPEG) per frame of _frames(w, h, src), computed once per configuration."""
    key = (w, h, src, rect, dst, full, dw, dh, pad, tuple(sorted(kw.items())))
    if key not in _REF:
        fr = _frames(w, h, src)
        _REF[key] = ([padded_planes(f, w, h, src, rect, dst, full, dw, dh, pad) for f in fr],
                     [padded_ref(f, w, h, src, rect, dst, full, dw, dh, pad, **kw) for f in fr])
    return _REF[key]


def _check_planes(enc, planes, dst, pad, dw, dh):
    """debug_planes() of the last submit: the canvas planes, and explicitly every border byte."""
    x, y, cw_, ch_ = pad
    hs, vs = CHROMA_SHIFTS[dst]
    for i, want in enumerate(planes):
        got = split_i420(enc.debug_planes(i), cw_, ch_, dst)
        for p, (name, a, b) in enumerate(zip("YUV", got, want)):
            bad = np.argwhere(a != b)
            assert bad.size == 0, (i, name, len(bad), bad[:4].tolist())
            border = np.ones(a.shape, bool)
            sx, sy = (0, 0) if p == 0 else (hs, vs)
            border[y >> sy:(y >> sy) + ((dh + (1 << sy) - 1) >> sy), x >> sx:(x >> sx) + ((dw + (1 << sx) - 1) >> sx)] = False
            assert (a[border] == BORDER[p]).all(), (i, name)


def _run(w, h, src, dst, full, pad, dw=None, dh=None, rect=None, paths=None, q=5, sar=(1, 1), **kw):
    frames = _frames(w, h, src)
    pw, ph = (dw, dh) if dw else (rect[2:] if rect else (w, h))
    planes, ref = _ref(w, h, src, rect, dst, full, dw, dh, pad, qscale=q, sar=sar,
                       **{k: v for k, v in kw.items() if k in ("huffman", "rst")})
    with MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, sar=sar, max_batch=3, chroma=dst, src_chroma=src,
                      crop=rect, pad=pad, **kw) as enc:
        assert enc.frame_bytes == i420_frame_bytes(w, h, src)
        assert (enc.dst_w, enc.dst_h) == (pw, ph) and (enc.enc_w, enc.enc_h) == tuple(pad[2:])
        if paths is not None:
            assert (enc.scale_path(0), enc.scale_path(1)) == paths
        got = enc.encode(frames)
        _check_planes(enc, planes, dst, pad, pw, ph)
    _check(got, ref)
    return got


PAD_ONLY = ([(c, 34, 18, (x, y, 64, 48)) for c in ("420", "422", "444") for x, y in ((0, 0), (2, 2), (16, 16), (30, 30))]
            + [(c, 34, 18, (8, 10, 50, 38)) for c in ("420", "422", "444")]   # no MCU multiple: edge replication over border
            + [("444", 33, 17, (1, 3, 47, 29)),    # odd strides, odd frame bytes
               ("420", 8, 8, (8, 8, 24, 24))])     # 12-byte chroma rows: every piece spans rows


@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
@pytest.mark.parametrize("c,w,h,pad", PAD_ONLY, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pad_only_matches_reference(c, w, h, pad, full):
    _run(w, h, c, c, full, pad, paths=(PADCOPY, PADCOPY), q=4)


def test_plane_copy_off_sends_the_picture_through_the_identity_filters(monkeypatch):
    """MJG_PLANE_COPY=0 (read at open): k_scale's one-tap filters write the picture into the canvas
    and k_pad_plane only the border; the same bytes."""
    monkeypatch.setenv("MJG_PLANE_COPY", "0")
    _run(34, 18, "420", "420", False, (8, 10, 50, 38), paths=(TILE, TILE), q=4)


@pytest.mark.parametrize("c", ["420", "444"])
def test_canvas_equal_to_the_picture_is_no_pad(c):
    """pad = (0, 0, w, h): the bytes, and the kernels, of an encoder opened without pad."""
    frames = _frames(34, 18, c)
    for kw, paths in ((dict(), (NONE, NONE)), (dict(dst_w=20, dst_h=12), (TILE, TILE))):
        out = []
        for pad in (None, (0, 0, kw.get("dst_w", 34), kw.get("dst_h", 18))):
            with MjpegEncoder(0, 34, 18, full_range=False, qscale=4, max_batch=3, chroma=c, pad=pad, **kw) as enc:
                assert (enc.scale_path(0), enc.scale_path(1)) == paths
                out.append(enc.encode(frames))
        _check(out[1], out[0])


@pytest.mark.parametrize("c", ["420", "444"])
def test_crop_then_pad(c):
    """Noise outside the rectangle must not reach the result."""
    rect, pad = (6, 10, 34, 18), (2, 2, 64, 48)
    got = _run(W, H, c, c, False, pad, rect=rect, paths=(PADCOPY, PADCOPY), q=4)
    b = same_inside(_frames(W, H, c), W, H, c, rect, 77)
    with MjpegEncoder(0, W, H, full_range=False, qscale=4, max_batch=3, chroma=c, crop=rect, pad=pad) as enc:
        _check(enc.encode(b), got)


SCALE_PAD = [((0, 8, 64, 48)), ((6, 10, 80, 56))]


@pytest.mark.parametrize("stream", [False, True], ids=["auto", "MJG_SCALE_STREAM"])
@pytest.mark.parametrize("c", ["420", "444"])
@pytest.mark.parametrize("pad", SCALE_PAD, ids=lambda v: "_".join(map(str, v)))
def test_scale_then_pad(pad, c, stream, monkeypatch):
    if stream:
        monkeypatch.setenv("MJG_SCALE_STREAM", "1")
    sar = profile.scaled_sar((1, 1), (W, H), (64, 32))
    _run(W, H, c, c, False, pad, 64, 32, paths=(STREAM, STREAM) if stream else (TILE, TILE), sar=sar)


def test_scale_then_pad_matrix_core_tiles():
    """1000x600 -> 500x300 at (6, 10) in 512x320: luma has 8 tile columns and 5 tile rows, so the
    interior tiles take both matrix-core passes and store 16 bytes at a row stride of 512, not 500."""
    _run(1000, 600, "420", "420", False, (6, 10, 512, 320), 500, 300, paths=(TILE, TILE))


def test_steep_scale_then_pad_on_the_stream_kernel():
    """256x160 -> 32x20 (8:1): luma on k_scale_stream by itself, chroma on the tile kernel."""
    _run(256, 160, "420", "420", False, (6, 10, 48, 36), 32, 20, paths=(STREAM, TILE))


def test_crop_scale_pad():
    rect = (2, 2, 126, 62)
    sar = profile.scaled_sar((1, 1), rect[2:], (64, 32))
    _run(W, H, "420", "420", False, (6, 10, 80, 56), 64, 32, rect=rect, paths=(TILE, TILE), sar=sar)


def test_scale_pad_and_pix_fmt_444_to_420():
    _run(W, H, "444", "420", False, (6, 10, 80, 56), 64, 32, paths=(TILE, TILE))


def test_pad_and_pix_fmt_luma_copied_chroma_scaled():
    """The library takes a pad under a pure -pix_fmt conversion (the worker does not send it):
    luma by k_pad_plane's copy, chroma by k_scale into the canvas."""
    _run(34, 18, "444", "420", False, (6, 10, 64, 48), paths=(PADCOPY, TILE))


@pytest.mark.parametrize("kw", [dict(huffman="optimal"), dict(rst=True)], ids=["optimal", "rst"])
def test_pad_huffman_optimal_and_rst(kw):
    _run(34, 18, "420", "420", False, (8, 10, 50, 38), **kw)


def _refs_of(w, h, c, pad, full=False, q=5):
    return _ref(w, h, c, None, c, full, None, None, pad, qscale=q, sar=(1, 1))[1]


def test_device_submit_from_a_pointer_that_is_not_16_aligned():
    import torch
    c, pad = "420", (2, 2, 64, 48)
    frames = _frames(34, 18, c)
    pool = torch.zeros(frames.size + 3, dtype=torch.uint8, device="cuda:0")
    pool[3:] = torch.from_numpy(frames.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    assert pool[3:].data_ptr() % 16 == 3
    with MjpegEncoder(0, 34, 18, full_range=False, qscale=5, max_batch=3, chroma=c, pad=pad) as enc:
        enc.submit(device_ptr=pool[3:].data_ptr(), nframes=3)
        got = enc.fetch()
    _check(got, _refs_of(34, 18, c, pad))


def test_submit_segments_ragged():
    """Two segments of 2 and 1 frames, each a tensor sliced from byte 1 of its allocation."""
    import torch
    c, pad = "444", (1, 3, 47, 29)
    frames = _frames(33, 17, c)
    segs = []
    for lo, n in ((0, 2), (2, 1)):
        pool = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device="cuda:0")
        pool[1:] = torch.from_numpy(frames[lo:lo + n].reshape(-1).copy()).to("cuda:0")
        segs.append((pool[1:], n))
    torch.cuda.synchronize()
    with MjpegEncoder(0, 33, 17, full_range=False, qscale=5, max_batch=3, chroma=c, pad=pad) as enc:
        enc.submit_segments([(t.data_ptr(), n) for t, n in segs])
        got = enc.fetch()
    _check(got, _refs_of(33, 17, c, pad))


def test_merged_single_submits():
    import torch
    c, pad = "420", (16, 16, 64, 48)
    frames = _frames(34, 18, c)
    segs = [torch.from_numpy(frames[lo:lo + n].copy()).to("cuda:0") for lo, n in ((0, 2), (2, 1))]
    torch.cuda.synchronize()
    got = []
    with MjpegEncoder(0, 34, 18, full_range=False, qscale=5, max_batch=3, chroma=c, pad=pad, merge=True) as enc:
        for t in segs:
            enc.submit(device_ptr=t.data_ptr(), nframes=t.shape[0])
        for _ in segs:
            enc.sync()
            got += enc.fetch()
    _check(got, _refs_of(34, 18, c, pad))


def test_a_slot_used_again_gets_a_whole_new_canvas():
    """Three encodes through one context (two slots): the third runs in the first one's slot, with
    other frames; each must match its own reference."""
    c, pad = "420", (30, 30, 64, 48)
    frames = _frames(34, 18, c)
    ref = _refs_of(34, 18, c, pad)
    with MjpegEncoder(0, 34, 18, full_range=False, qscale=5, max_batch=3, chroma=c, pad=pad) as enc:
        for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
            _check(enc.encode(frames[order]), [ref[i] for i in order])


@pytest.mark.parametrize("c,dst,pad,word", [
    ("420", (34, 18), (32, 2, 64, 48), "outside"),
    ("420", (34, 18), (3, 2, 64, 48), "sub-sampling"),
    ("420", (33, 18), (2, 2, 64, 48), "sub-sampling"),
])
def test_constructor_refuses_a_bad_pad(c, dst, pad, word):
    with pytest.raises(_lib.MjgError) as e:
        MjpegEncoder(0, dst[0], dst[1], full_range=False, qscale=5, max_batch=3, chroma=c, pad=pad)
    assert e.value.code == _lib.MJG_E_INVALID
    assert "pad" in str(e.value) and word in str(e.value)


def _y4m420(frames, w, h):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def _raw_mkv(frames, w, h):
    buf = io.BytesIO()
    wr = container.MkvWriter(buf, w, h, Fraction(25), (1, 1), codec="V_UNCOMPRESSED", colour_space=b"I420")
    for f in frames:
        wr.write_frame(f.tobytes())
    wr.close()
    return buf.getvalue()


@pytest.mark.parametrize("make", [_y4m420, _raw_mkv], ids=["y4m", "raw_mkv"])
def test_worker_scale_pad(make):
    frames = _frames(W, H, "420")
    args = ["-vf", "scale=64:32,pad=64:48:0:8"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(make(frames, W, H)), stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets = [d for _, d in r.frames(1)]
    info = r.info(1)
    assert (info.width, info.height, info.codec) == (64, 48, "V_MJPEG")
    sar = profile.scaled_sar((1, 1), (W, H), (64, 32))   # the scale's, from the picture: the pad leaves it
    assert sar == (65, 66)
    assert Fraction(*info.sar) == Fraction(round(Fraction(64 * sar[0], sar[1])), 64)
    _, ref = _ref(W, H, "420", None, "420", False, 64, 32, (0, 8, 64, 48), qscale=profile.effective_qscale(5), sar=sar)
    _check(packets, ref)
