"""`-pix_fmt` chroma conversion on the GPU (MjpegEncoder(src_chroma=..., chroma=...): the source
frames in one planar format, the JPEGs in another), byte for byte against the reference
composed from the CPU oracle (tests/chroma_resample_ref.py): luma through k_plane_copy (or,
with a resize, k_scale), chroma through k_scale, then k_encode and the tail as always."""
import io

import numpy as np
import pytest

import oracle
from chroma_resample_ref import composed_frame, composed_planes, source_frames
from ffmpeg_distributed_amd import container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes, pack_i420, split_i420

pytestmark = pytest.mark.gpu

DOWN = [("444", "422"), ("444", "420"), ("422", "420")]
SIZES = [(8, 8), (9, 17), (33, 17), (101, 57), (130, 66)]


def first_diff(a: bytes, b: bytes):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i
    return n if len(a) != len(b) else -1


def _refs(frames, w, h, src, dst, full, dw=None, dh=None, **kw):
    return [composed_frame(f, w, h, src, dst, full, dw, dh, **kw) for f in frames]


def _check(got, ref):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a == b, (i, len(a), len(b), first_diff(a, b))


def _check_planes(enc, frames, w, h, src, dst, full, dw=None, dh=None):
    """debug_planes() of the last submit against the composed planes, plane by plane."""
    dw, dh = dw or w, dh or h
    for i, f in enumerate(frames):
        got = split_i420(enc.debug_planes(i), dw, dh, dst)
        for name, a, b in zip("YUV", got, composed_planes(f, w, h, src, dst, full, dw, dh)):
            bad = np.argwhere(a != b)
            assert bad.size == 0, (i, name, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("src,dst", DOWN)
def test_down_sampling_pairs_match_composed_reference(src, dst, w, h, full):
    """No resize: luma is the unchanged plane (odd frame strides and plane offsets for the copy's
    heads and tails), the chroma planes single-tile with edge replication."""
    frames = source_frames(w, h, 3, 100 * w + h, src)
    with MjpegEncoder(0, w, h, full_range=full, qscale=4, max_batch=3, chroma=dst, src_chroma=src) as enc:
        assert enc.frame_bytes == i420_frame_bytes(w, h, src)
        got = enc.encode(frames)
        _check_planes(enc, frames, w, h, src, dst, full)  # first: a failure there names the sws stage
    _check(got, _refs(frames, w, h, src, dst, full, qscale=4))


@pytest.mark.parametrize("w,h", [(1002, 602), (1000, 600)])
def test_444_to_420_exact_2to1_matrix_core_tiles(w, h):
    """The chroma planes are an exact 2:1 with 8 tile columns and 5 tile rows, so interior tiles
    take the matrix-core h- and v-passes: 1002x602 with dw = 501 (no multiple of 16) and an odd
    V-plane offset for the v-pass's 16-byte stores, 1000x600 the same with even offsets."""
    src, dst = "444", "420"
    frames = source_frames(w, h, 3, w, src)
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=3, chroma=dst, src_chroma=src) as enc:
        got = enc.encode(frames)
        _check_planes(enc, frames, w, h, src, dst, False)
    _check(got, _refs(frames, w, h, src, dst, False))


@pytest.mark.parametrize("src,w,h,dw,dh", [("444", 128, 96, 80, 56), ("422", 130, 66, 64, 34)])
def test_resize_and_resample_together(src, w, h, dw, dh):
    dst = "420"
    frames = source_frames(w, h, 3, 7, src)
    sar = profile.scaled_sar((1, 1), (w, h), (dw, dh))
    with MjpegEncoder(0, w, h, dw, dh, full_range=False, qscale=5, sar=sar, max_batch=3, chroma=dst,
                      src_chroma=src) as enc:
        got = enc.encode(frames)
        _check_planes(enc, frames, w, h, src, dst, False, dw, dh)
    _check(got, _refs(frames, w, h, src, dst, False, dw, dh, sar=sar))


def test_up_sampling_pair_at_library_level():
    """The library takes any (source, encoded) pair; the worker sends only the down-sampling ones."""
    w, h, src, dst = 34, 18, "420", "444"
    frames = source_frames(w, h, 3, 9, src)
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=3, chroma=dst, src_chroma=src) as enc:
        got = enc.encode(frames)
    _check(got, _refs(frames, w, h, src, dst, False))


@pytest.mark.parametrize("kw", [dict(huffman="optimal"), dict(rst=True)], ids=["optimal", "rst"])
def test_444_to_420_huffman_optimal_and_rst(kw):
    w, h, src, dst = 72, 40, "444", "420"
    frames = source_frames(w, h, 3, 11, src)
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=3, chroma=dst, src_chroma=src, **kw) as enc:
        got = enc.encode(frames)
    _check(got, _refs(frames, w, h, src, dst, False, **kw))


@pytest.fixture(scope="module")
def submit_case():
    w, h, src, dst = 101, 57, "444", "420"
    frames = source_frames(w, h, 4, 13, src)
    return w, h, src, dst, frames, _refs(frames, w, h, src, dst, False)


@pytest.mark.parametrize("path", ["host", "device_plus_1", "segments", "merged"])
def test_submit_paths(path, submit_case):
    """Host frames, a device pointer one byte past its allocation, two 2-frame segments in one
    submit and two merged submits: each the bytes of the per-frame reference."""
    import torch
    w, h, src, dst, frames, ref = submit_case
    dev = torch.device("cuda", 0)
    kw = dict(full_range=False, qscale=5, max_batch=4, chroma=dst, src_chroma=src)
    if path == "host":
        with MjpegEncoder(0, w, h, **kw) as enc:
            enc.submit(frames)
            got = enc.fetch()
    elif path == "device_plus_1":
        pool = torch.zeros(frames.size + 1, dtype=torch.uint8, device=dev)
        pool[1:] = torch.from_numpy(frames.reshape(-1)).to(dev)
        torch.cuda.synchronize()
        with MjpegEncoder(0, w, h, **kw) as enc:
            enc.submit(device_ptr=pool.data_ptr() + 1, nframes=4)
            got = enc.fetch()
    elif path == "segments":
        segs = [torch.from_numpy(frames[o:o + 2].copy()).to(dev) for o in (0, 2)]
        torch.cuda.synchronize()
        with MjpegEncoder(0, w, h, **kw) as enc:
            enc.submit_segments([(t.data_ptr(), 2) for t in segs])
            got = enc.fetch()
    else:
        segs = [torch.from_numpy(frames[o:o + 2].copy()).to(dev) for o in (0, 2)]
        torch.cuda.synchronize()
        with MjpegEncoder(0, w, h, merge=True, **kw) as enc:
            for t in segs:
                enc.submit(device_ptr=t.data_ptr(), nframes=2)
            got = []
            for _ in segs:
                enc.sync()
                got += enc.fetch()
    _check(got, ref)


@pytest.mark.parametrize("copy_kernel", [True, False], ids=["k_plane_copy", "k_scale_identity"])
def test_unchanged_luma_plane_every_byte_value(copy_kernel, monkeypatch):
    """444 -> 422, tv range, 33x17: luma keeps its size and holds every byte value.  The copy
    kernel's table and k_scale's identity filters (MJG_PLANE_COPY=0) both give swscale's
    one-tap path through the 15-bit intermediate."""
    w, h, src, dst = 33, 17, "444", "422"
    if not copy_kernel:
        monkeypatch.setenv("MJG_PLANE_COPY", "0")
    rng = np.random.default_rng(3)
    y = (np.arange(w * h) % 256).astype(np.uint8).reshape(h, w)
    u, v = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    frame = pack_i420(y, u, v)
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=2, chroma=dst, src_chroma=src) as enc:
        got = enc.encode(np.stack([frame, frame[::-1].copy()]))
        planes = [split_i420(enc.debug_planes(i), w, h, dst) for i in range(2)]
    np.testing.assert_array_equal(planes[0][0], oracle.scale_plane(y, w, h, range_mode=1))
    y1 = split_i420(frame[::-1].copy(), w, h, src)[0]
    np.testing.assert_array_equal(planes[1][0], oracle.scale_plane(y1, w, h, range_mode=1))
    _check(got, _refs([frame, frame[::-1].copy()], w, h, src, dst, False))


def _y4m444(frames, w, h):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C444\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


@pytest.mark.parametrize("scale", [None, (48, 24)], ids=["same_size", "scale_48x24"])
def test_worker_444_input_pix_fmt_yuvj420p(scale):
    """The request the GPU pool could not serve: a 4:4:4 segment re-encoded with -pix_fmt
    yuvj420p stays on the GPU (no ffmpeg child), every packet the composed reference."""
    w, h, n = 72, 40, 5
    frames = source_frames(w, h, n, 17, "444")
    args = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact -pix_fmt yuvj420p".split()
    if scale:
        args = ["-vf", f"scale={scale[0]}:{scale[1]}"] + args
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m444(frames, w, h)), stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets = [d for _, d in r.frames(1)]
    dw, dh = scale or (w, h)
    info = r.info(1)
    assert (info.width, info.height, info.codec) == (dw, dh, "V_MJPEG")
    sar = profile.scaled_sar((1, 1), (w, h), (dw, dh))
    _check(packets, _refs(frames, w, h, "444", "420", False, dw, dh, qscale=profile.effective_qscale(5),
                          sar=sar))
