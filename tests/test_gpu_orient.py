"""`-vf hflip / vflip / transpose` on the GPU (MjpegEncoder(orient=...): k_orient_plane in front of
everything else), byte for byte against numpy indexing (tests/orient_ref.py) followed by the
composed references of the crop, the scale and the pad.  debug_oriented() is the frame the rest
of the chain reads; with an orientation alone k_encode reads it in place."""
import io
from fractions import Fraction

import numpy as np
import pytest

from chroma_resample_ref import source_frames
from orient_ref import orient_frame, oriented_planes, oriented_ref, oriented_size
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes, split_i420

pytestmark = pytest.mark.gpu

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
    """3 frames (two noise, one smooth) per source shape and format, made once."""
    if (w, h, c) not in _SRC:
        f = source_frames(w, h, NF, 100 * w + h + 13, c)
        f.setflags(write=False)
        _SRC[(w, h, c)] = f
    return _SRC[(w, h, c)]


_REF = {}


def _ref(w, h, src, orient, rect=None, dst=None, full=False, dw=None, dh=None, pad=None, **kw):
    """The expected JPEGs of _frames(w, h, src), computed once per configuration."""
    key = (w, h, src, orient, rect, dst, full, dw, dh, pad, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = [oriented_ref(f, w, h, src, orient, rect, dst, full, dw, dh, pad, **kw)
                     for f in _frames(w, h, src)]
    return _REF[key]


def _check_oriented(enc, frames, w, h, c, orient):
    """debug_oriented() of the last submit against numpy, naming the first differing sample."""
    ow, oh = oriented_size(w, h, orient)
    for i, f in enumerate(frames):
        got = enc.debug_oriented(i)
        want = orient_frame(f, w, h, c, orient)
        assert got.size == want.size
        if (got == want).all():
            continue
        for name, a, b in zip("YUV", split_i420(got, ow, oh, c), split_i420(want, ow, oh, c)):
            bad = np.argwhere(a != b)
            if bad.size:
                y, x = bad[0]
                print(f"frame {i} plane {name}: first difference at y={y} x={x}: got {a[y, x]}, want {b[y, x]}, "
                      f"{len(bad)} of {a.size} differ")
                pytest.fail(f"orient {orient} {w}x{h} {c}: frame {i} plane {name} differs first at (y={y}, x={x})")


def _check_planes(enc, planes, dst):
    for i, want in enumerate(planes):
        got = split_i420(enc.debug_planes(i), enc.enc_w, enc.enc_h, dst)
        for name, a, b in zip("YUV", got, want):
            bad = np.argwhere(a != b)
            assert bad.size == 0, (i, name, len(bad), bad[:4].tolist())


# (70 x 150: more source rows than one 128-row tile of the transposing form, with a partial second one)
SHAPES = [(130, 66, "420"), (130, 66, "444"), (131, 67, "420"), (33, 17, "444"), (8, 8, "420"), (70, 150, "420")]
CASES = ([(w, h, c, o) for (w, h, c) in SHAPES for o in range(1, 8)]
         + [(130, 66, "422", o) for o in (2, 4, 6)])


@pytest.mark.parametrize("w,h,c,orient", CASES, ids=lambda v: str(v))
def test_orientation_alone_matches_reference(w, h, c, orient):
    """The oriented bytes, then the JPEGs in tv and in full range: k_encode reads d_orient in place."""
    frames = _frames(w, h, c)
    ow, oh = oriented_size(w, h, orient)
    for full in (False, True):
        with MjpegEncoder(0, w, h, full_range=full, qscale=4, max_batch=NF, chroma=c, orient=orient) as enc:
            assert enc.frame_bytes == i420_frame_bytes(w, h, c)
            assert (enc.dst_w, enc.dst_h, enc.enc_w, enc.enc_h) == (ow, oh, ow, oh)
            assert (enc.scale_path(0), enc.encode_path() & 1) == (0, 1)    # no sws stage: read in place
            got = enc.encode(frames)
            if not full:
                _check_oriented(enc, frames, w, h, c, orient)
        _check(got, _ref(w, h, c, orient, full=full, qscale=4))


def test_transpose_crop_scale_pad_chain():
    """orient 3 (transpose=1), crop (2, 2, 62, 126) of the 66 x 130 frame, scale 32 x 64, pad to 48 x 80."""
    orient, rect, pad = 3, (2, 2, 62, 126), (8, 8, 48, 80)
    frames = _frames(W, H, "420")
    sar = profile.scaled_sar((1, 1), rect[2:], (32, 64))
    with MjpegEncoder(0, W, H, 32, 64, full_range=False, qscale=5, sar=sar, max_batch=NF, chroma="420",
                      crop=rect, pad=pad, orient=orient) as enc:
        got = enc.encode(frames)
        _check_oriented(enc, frames, W, H, "420", orient)
        _check_planes(enc, [oriented_planes(f, W, H, "420", orient, rect, "420", False, 32, 64, pad) for f in frames],
                      "420")
    _check(got, _ref(W, H, "420", orient, rect, "420", False, 32, 64, pad, qscale=5, sar=sar))


def test_transpose_and_pix_fmt_444_to_420():
    orient = 5
    frames = _frames(W, H, "444")
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="420", src_chroma="444",
                      orient=orient) as enc:
        assert (enc.enc_w, enc.enc_h) == (H, W)
        got = enc.encode(frames)
        _check_oriented(enc, frames, W, H, "444", orient)
        _check_planes(enc, [oriented_planes(f, W, H, "444", orient, None, "420", False) for f in frames], "420")
    _check(got, _ref(W, H, "444", orient, None, "420", False, qscale=5))


def test_transpose_with_rst():
    orient = 1
    frames = _frames(W, H, "420")
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="420", rst=True, orient=orient) as enc:
        got = enc.encode(frames)
    _check(got, _ref(W, H, "420", orient, qscale=5, rst=True))


@pytest.mark.parametrize("merge", [False, True], ids=["segments", "MJG_F_MERGE"])
def test_two_segments_give_the_bytes_of_two_submits(merge):
    """Two segments of 2 and 1 frames at different device pointers, each sliced from byte 1 of its
    allocation: one mjg_submit_segments launch, or two merged single submits."""
    import torch
    w, h, c, orient = 33, 17, "444", 3
    frames = _frames(w, h, c)
    segs = []
    for lo, n in ((0, 2), (2, 1)):
        pool = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device="cuda:0")
        pool[1:] = torch.from_numpy(frames[lo:lo + n].reshape(-1).copy()).to("cuda:0")
        segs.append((pool[1:], n))
    torch.cuda.synchronize()
    single = []
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=NF, chroma=c, orient=orient) as enc:
        for t, n in segs:
            enc.submit(device_ptr=t.data_ptr(), nframes=n)
            single += enc.fetch()
    got = []
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=NF, chroma=c, orient=orient, merge=merge) as enc:
        if merge:
            for t, n in segs:
                enc.submit(device_ptr=t.data_ptr(), nframes=n)
            for _ in segs:
                enc.sync()
                got += enc.fetch()
        else:
            enc.submit_segments([(t.data_ptr(), n) for t, n in segs])
            got = enc.fetch()
            _check_oriented(enc, frames, w, h, c, orient)
    _check(got, single)
    _check(got, _ref(w, h, c, orient, qscale=5))


@pytest.mark.parametrize("kw", [dict(), dict(dst_w=64, dst_h=32)], ids=["in_place", "scale"])
def test_orient_zero_is_an_encoder_opened_without_it(kw):
    frames = _frames(W, H, "420")
    out = []
    for extra in (dict(), dict(orient=0)):
        with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="420", timing=True, **kw,
                          **extra) as enc:
            assert enc._L.mjg_debug_orient(enc._h) == 0
            jp = enc.encode(frames) + enc.encode(frames[:1])
            with pytest.raises(_lib.MjgError) as e:
                enc.debug_oriented(0)
            assert e.value.code == _lib.MJG_E_STATE
            out.append((jp, enc.kernel_times()[1], enc.scale_path(0), enc.encode_path()))
    _check(out[1][0], out[0][0])
    assert out[0][1:] == out[1][1:] and out[0][1] == 2


def test_the_scale_interval_opens_for_an_orientation_alone():
    frames = _frames(W, H, "420")
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="420", timing=True, orient=6) as enc:
        assert enc._L.mjg_debug_orient(enc._h) == 6
        enc.encode(frames)
        ms, n = enc.kernel_times()
    assert n == 1 and ms["scale"] > 0


def test_constructor_refuses_a_transpose_of_422():
    with pytest.raises(_lib.MjgError) as e:
        MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="422", orient=3)
    assert e.value.code == _lib.MJG_E_INVALID and "orient 3" in str(e.value)


def _y4m420(frames, w, h):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def test_worker_transpose_scale():
    frames = _frames(W, H, "420")
    args = ["-vf", "transpose=1,scale=64:128"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, W, H)), stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets = [d for _, d in r.frames(1)]
    info = r.info(1)
    assert (info.width, info.height, info.codec) == (64, 128, "V_MJPEG")
    sar = profile.scaled_sar((1, 1), (H, W), (64, 128))     # 1 / (1:1), then the scale's from 66 x 130
    assert sar == (66, 65)
    assert Fraction(*info.sar) == Fraction(round(Fraction(64 * sar[0], sar[1])), 64)
    _check(packets, _ref(W, H, "420", 3, None, "420", False, 64, 128, qscale=profile.effective_qscale(5), sar=sar))
