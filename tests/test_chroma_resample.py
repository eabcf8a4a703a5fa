"""`-pix_fmt` chroma conversion, the parts that need no GPU: the composed reference the GPU
tests compare with (tests/chroma_resample_ref.py) is anchored to the oracle's own worker path,
the worker's routing of (input, requested) sampling pairs, its encoder cache key, and the
packed-frame helpers at odd sizes."""
import numpy as np
import pytest

import oracle
from chroma_resample_ref import composed_frame, source_frames
from ffmpeg_distributed_amd import container, profile, worker
from ffmpeg_distributed_amd.encoder import chroma_size, i420_frame_bytes, pack_i420, split_i420

ARGS = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
DOWN = [("444", "422"), ("444", "420"), ("422", "420")]
UP = [("420", "422"), ("420", "444"), ("422", "444")]


@pytest.mark.parametrize("c", ["420", "422", "444"])
@pytest.mark.parametrize("w,h,dw,dh", [(72, 40, 48, 24), (33, 17, None, None)])
def test_composed_reference_equals_oracle_worker_path(c, w, h, dw, dh):
    """Source format == encoded format: planes scaled one by one, then encoded as full range,
    are the bytes of oracle.encode_frame's own resize + tv->pc + encode (with no resize: its
    tv->pc table, i.e. swscale's one-tap identity filters through the 15-bit intermediate)."""
    sar = profile.scaled_sar((1, 1), (w, h), (dw or w, dh or h))
    for f in source_frames(w, h, 3, 5, c):
        y, u, v = split_i420(f, w, h, c)
        ref = oracle.encode_frame(y, u, v, dw, dh, full_range=False, qscale=5, sar=sar, chroma=c)
        assert composed_frame(f, w, h, c, c, False, dw, dh, qscale=5, sar=sar) == ref


def _prof(*extra):
    prof, why = profile.try_parse([*ARGS, *extra])
    assert prof is not None, why
    return prof


@pytest.mark.parametrize("src,dst", DOWN)
def test_resample_plan_sends_down_sampling_pairs_to_the_gpu(src, dst):
    info = container.StreamInfo(64, 48, chroma=src)
    assert worker.resample_plan(_prof("-pix_fmt", f"yuvj{dst}p"), info) == (src, dst)


@pytest.mark.parametrize("src,dst", UP)
def test_resample_plan_leaves_up_sampling_pairs_to_ffmpeg(src, dst):
    info = container.StreamInfo(64, 48, chroma=src)
    why = worker.resample_plan(_prof("-pix_fmt", f"yuvj{dst}p"), info)
    assert why == f"-pix_fmt needs {src} -> {dst} chroma resampling"  # the worker's log line, as before


@pytest.mark.parametrize("c", ["420", "422", "444"])
def test_resample_plan_equal_pair_and_no_pix_fmt(c):
    info = container.StreamInfo(64, 48, chroma=c)
    assert worker.resample_plan(_prof("-pix_fmt", f"yuvj{c}p"), info) == (c, c)
    assert worker.resample_plan(_prof(), info) == (c, c)


def test_encoder_cache_key_differs_when_only_pix_fmt_differs():
    """A resident worker fed two segments of one 4:4:4 stream, one with -pix_fmt yuvj420p and
    one with yuvj422p (or none), must not reuse the first one's encoder context."""
    info = container.StreamInfo(64, 48, chroma="444")
    keys = [worker.encoder_key(p, info, 64, 48, (1, 1), False, 8)
            for p in (_prof(), _prof("-pix_fmt", "yuvj444p"), _prof("-pix_fmt", "yuvj422p"),
                      _prof("-pix_fmt", "yuvj420p"))]
    assert keys[0] == keys[1]  # -pix_fmt naming the input's sampling changes nothing
    assert len({keys[1], keys[2], keys[3]}) == 3
    other = container.StreamInfo(64, 48, chroma="422")  # same request from another input sampling
    assert worker.encoder_key(_prof("-pix_fmt", "yuvj420p"), other, 64, 48, (1, 1), False, 8) != keys[3]


@pytest.mark.parametrize("w,h", [(33, 17), (9, 17), (101, 57), (8, 8)])
@pytest.mark.parametrize("c", ["420", "422", "444"])
def test_frame_bytes_and_split_round_trip_at_odd_sizes(w, h, c):
    cw, ch = chroma_size(w, h, c)
    hs, vs = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[c]
    assert (cw, ch) == (-(-w // (1 << hs)), -(-h // (1 << vs)))
    fb = i420_frame_bytes(w, h, c)
    assert fb == w * h + 2 * cw * ch == container.StreamInfo(w, h, chroma=c).frame_bytes
    f = np.arange(fb, dtype=np.uint32).astype(np.uint8)
    y, u, v = split_i420(f, w, h, c)
    assert y.shape == (h, w) and u.shape == v.shape == (ch, cw)
    np.testing.assert_array_equal(pack_i420(y, u, v), f)
