"""`-vf yadif` on the GPU (MjpegEncoder(deint=...): k_yadif_plane in front of everything else), byte
for byte against tests/yadif_ref.py followed by the composed references of the orientation, the
crop, the scale and the pad.  debug_deint() is the frame the rest of the chain reads; with a
deinterlacer alone k_encode reads it in place."""
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from yadif_ref import deint_frames, deint_planes, deint_ref
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, chroma_size, i420_frame_bytes, pack_i420, split_i420

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 130, 66
NF = 5
YADIF, NOSPATIAL, BFF = _lib.MJG_DEINT_YADIF, _lib.MJG_DEINT_NOSPATIAL, _lib.MJG_DEINT_BFF


def _kernel_constant(name):
    with open(os.path.join(ROOT, "ffmpeg_distributed_amd", "csrc", "scale.hip")) as f:
        return int(re.search(r"constexpr int " + name + r" = (\d+);", f.read()).group(1))


# k_yadif_plane: one 16-byte piece per thread, so a workgroup covers 16 * kDeintThreads (4096) bytes
# of a plane's byte string.  A 4100 x 5 4:4:4 frame: every row of every plane is longer than that,
# so a workgroup holds less than one row, a row's pieces come from two workgroups, and each plane
# takes six of them.  (130 x 66 is the other way round: its luma takes three workgroups of about
# 31 rows each.)
WG_BYTES = 16 * _kernel_constant("kDeintThreads")
BIG = (WG_BYTES + 4, 5, "444")
assert BIG[0] > WG_BYTES and BIG[0] * BIG[1] > 4 * WG_BYTES


def flags(mode, tff):
    return YADIF | (NOSPATIAL if mode == 2 else 0) | (0 if tff else BFF)


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
    """5 frames per shape and format, made once: three of noise, two smooth ones with motion."""
    if (w, h, c) not in _SRC:
        rng = np.random.default_rng(1000 * w + 10 * h + int(c))
        fb = i420_frame_bytes(w, h, c)
        cw, ch = chroma_size(w, h, c)
        out = [rng.integers(0, 256, fb, dtype=np.uint8) for _ in range(3)]
        for t in (0, 1):
            yy, xx = np.mgrid[0:h, 0:w]
            cy, cx = np.mgrid[0:ch, 0:cw]
            y = (128 + 100 * np.sin((xx + 5 * t) / 7 + yy / 9)).clip(0, 255).astype(np.uint8)
            u = (128 + 90 * np.cos((cx - 3 * t) / 4 + cy / 11)).clip(0, 255).astype(np.uint8)
            v = (128 + 90 * np.sin((cy + 2 * t) / 3 - cx / 13)).clip(0, 255).astype(np.uint8)
            out.append(pack_i420(y, u, v))
        f = np.stack([out[0], out[3], out[1], out[4], out[2]])
        f.setflags(write=False)
        _SRC[(w, h, c)] = f
    return _SRC[(w, h, c)]


_DEINT = {}


def _deint(w, h, c, mode, tff, lo=0, hi=NF):
    """The deinterlaced frames of the sequence _frames(w, h, c)[lo:hi], computed once."""
    key = (w, h, c, mode, tff, lo, hi)
    if key not in _DEINT:
        d = deint_frames(_frames(w, h, c)[lo:hi], w, h, c, mode, tff)
        d.setflags(write=False)
        _DEINT[key] = d
    return _DEINT[key]


_REF = {}


def _ref(w, h, c, mode, tff, lo=0, hi=NF, orient=0, rect=None, dst=None, full=False, dw=None, dh=None, pad=None, **kw):
    """The expected JPEGs of that sequence, computed once per configuration."""
    key = (w, h, c, mode, tff, lo, hi, orient, rect, dst, full, dw, dh, pad, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = [deint_ref(f, w, h, c, orient, rect, dst, full, dw, dh, pad, **kw)
                     for f in _deint(w, h, c, mode, tff, lo, hi)]
    return _REF[key]


def _check_deint(enc, want, w, h, c, what=""):
    """debug_deint() of the last submit against the reference, naming the first differing sample."""
    for i, wf in enumerate(want):
        got = enc.debug_deint(i)
        assert got.size == wf.size
        if (got == wf).all():
            continue
        for name, a, b in zip("YUV", split_i420(got, w, h, c), split_i420(wf, w, h, c)):
            bad = np.argwhere(a != b)
            if bad.size:
                y, x = bad[0]
                print(f"frame {i} plane {name}: first difference at y={y} x={x}: got {a[y, x]}, want {b[y, x]}, "
                      f"{len(bad)} of {a.size} differ")
                pytest.fail(f"yadif {what} {w}x{h} {c}: frame {i} plane {name} differs first at (y={y}, x={x})")


def _check_planes(enc, planes, dst):
    for i, want in enumerate(planes):
        got = split_i420(enc.debug_planes(i), enc.enc_w, enc.enc_h, dst)
        for name, a, b in zip("YUV", got, want):
            bad = np.argwhere(a != b)
            assert bad.size == 0, (i, name, len(bad), bad[:4].tolist())


# 131 x 67: odd chroma sizes; 33 x 17 4:4:4: odd frame bytes, every frame at another alignment; 6 x 6
# 4:2:0: 3 x 3 chroma, the smallest legal plane; 20 x 8 4:4:4: rows shorter than a piece and its aprons
SHAPES = [(130, 66, "420"), (131, 67, "420"), (130, 66, "422"), (33, 17, "444"), (6, 6, "420"), (20, 8, "444"), BIG]
CASES = ([(w, h, c, 0, tff) for (w, h, c) in SHAPES for tff in (1, 0)]
         + [(130, 66, "420", 2, 1), (33, 17, "444", 2, 0)])


# ------------------------------------------------------------------------- 1. the deinterlacer alone
@pytest.mark.parametrize("w,h,c,mode,tff", CASES, ids=lambda v: str(v))
def test_deinterlacer_alone_matches_reference(w, h, c, mode, tff):
    """The deinterlaced bytes, then the JPEGs in tv and in full range: k_encode reads d_deint in place."""
    frames = _frames(w, h, c)
    for full in (False, True):
        with MjpegEncoder(0, w, h, full_range=full, qscale=4, max_batch=NF, chroma=c, deint=flags(mode, tff)) as enc:
            assert enc.frame_bytes == i420_frame_bytes(w, h, c)
            assert enc._L.mjg_debug_deint_flags(enc._h) == flags(mode, tff)
            assert (enc.scale_path(0), enc.encode_path() & 1) == (0, 1)    # no sws stage: read in place
            got = enc.encode(frames)
            if not full:
                _check_deint(enc, _deint(w, h, c, mode, tff), w, h, c, f"mode {mode} tff {tff}")
        _check(got, _ref(w, h, c, mode, tff, full=full, qscale=4))


# ------------------------------------------------------------------------- 2. sequences
@pytest.mark.parametrize("n", [1, 2, 5])
def test_a_submit_is_a_whole_sequence(n):
    w, h, c = 33, 17, "444"
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=NF, chroma=c, deint=flags(0, 1)) as enc:
        got = enc.encode(_frames(w, h, c)[:n])
        _check_deint(enc, _deint(w, h, c, 0, 1, 0, n), w, h, c, f"{n} frames")
    _check(got, _ref(w, h, c, 0, 1, 0, n, qscale=5))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_halo_submits_give_the_bytes_of_one_submit(dev):
    """The 5 frames as 2 + 2 + 1 with their neighbour frames: halo 2, 3, 1."""
    w, h, c = 33, 17, "444"
    frames = _frames(w, h, c)
    want = _deint(w, h, c, 0, 0)
    pieces = [(0, 3, 2, 2, 0), (1, 5, 2, 3, 2), (3, 5, 1, 1, 4)]   # buffer frames [lo, hi), encoded, halo, first encoded
    got = []
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=2, chroma=c, deint=flags(0, 0)) as enc:
        if dev:
            import torch
            pool = torch.zeros(NF * frames.shape[1] + 1, dtype=torch.uint8, device="cuda:0")
            pool[1:] = torch.from_numpy(frames.reshape(-1).copy()).to("cuda:0")    # from byte 1 of its allocation
            torch.cuda.synchronize()
        for lo, hi, n, halo, first in pieces:
            if dev:
                enc.submit(device_ptr=pool.data_ptr() + 1 + lo * frames.shape[1], nframes=n, halo=halo)
            else:
                enc.submit(frames[lo:hi], halo=halo)
            got += enc.fetch()
            _check_deint(enc, want[first:first + n], w, h, c, f"halo {halo}")
        one = enc.encode(frames)      # more frames than max_batch: encode() makes the same halo submits
    _check(got, _ref(w, h, c, 0, 0, qscale=5))
    _check(one, got)


def test_each_segment_is_a_sequence_of_its_own():
    """Two segments (3 and 2 frames) in one launch: the bytes of two single submits, which are not
    the bytes of the 5-frame sequence."""
    import torch
    w, h, c = 33, 17, "444"
    frames = _frames(w, h, c)
    segs = []
    for lo, n in ((0, 3), (3, 2)):
        pool = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device="cuda:0")
        pool[1:] = torch.from_numpy(frames[lo:lo + n].reshape(-1).copy()).to("cuda:0")
        segs.append((pool[1:], n))
    torch.cuda.synchronize()
    single = []
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=NF, chroma=c, deint=flags(0, 1)) as enc:
        for t, n in segs:
            enc.submit(device_ptr=t.data_ptr(), nframes=n)
            single += enc.fetch()
        enc.submit_segments([(t.data_ptr(), n) for t, n in segs])
        got = enc.fetch()
        want = np.concatenate([_deint(w, h, c, 0, 1, 0, 3), _deint(w, h, c, 0, 1, 3, 5)])
        _check_deint(enc, want, w, h, c, "segments 3 + 2")
    _check(got, single)
    _check(got, _ref(w, h, c, 0, 1, 0, 3, qscale=5) + _ref(w, h, c, 0, 1, 3, 5, qscale=5))
    whole = _ref(w, h, c, 0, 1, qscale=5)
    assert got[2] != whole[2] and got[3] != whole[3]      # the frames at the boundary see other neighbours
    assert got[0] == whole[0] and got[1] == whole[1] and got[4] == whole[4]


# ------------------------------------------------------------------------- 3. the chain
def test_yadif_transpose_crop_scale_pad_chain():
    """yadif, orient 3 (transpose=1), crop (2, 2, 62, 126) of the 66 x 130 frame, scale 32 x 64, pad to 48 x 80."""
    orient, rect, pad = 3, (2, 2, 62, 126), (8, 8, 48, 80)
    frames = _frames(W, H, "420")
    sar = profile.scaled_sar((1, 1), rect[2:], (32, 64))
    with MjpegEncoder(0, W, H, 32, 64, full_range=False, qscale=5, sar=sar, max_batch=NF, chroma="420",
                      crop=rect, pad=pad, orient=orient, deint=flags(0, 1)) as enc:
        got = enc.encode(frames)
        d = _deint(W, H, "420", 0, 1)
        _check_deint(enc, d, W, H, "420", "chain")
        _check_planes(enc, [deint_planes(f, W, H, "420", orient, rect, "420", False, 32, 64, pad) for f in d], "420")
    _check(got, _ref(W, H, "420", 0, 1, 0, NF, orient, rect, "420", False, 32, 64, pad, qscale=5, sar=sar))


def test_yadif_scale():
    frames = _frames(W, H, "420")
    sar = profile.scaled_sar((1, 1), (W, H), (64, 32))
    with MjpegEncoder(0, W, H, 64, 32, full_range=False, qscale=5, sar=sar, max_batch=NF, chroma="420",
                      deint=flags(2, 0)) as enc:
        assert enc.scale_path(0) == 2
        got = enc.encode(frames)
        d = _deint(W, H, "420", 2, 0)
        _check_deint(enc, d, W, H, "420", "scale")
        _check_planes(enc, [deint_planes(f, W, H, "420", 0, None, "420", False, 64, 32) for f in d], "420")
    _check(got, _ref(W, H, "420", 2, 0, 0, NF, 0, None, "420", False, 64, 32, qscale=5, sar=sar))


# ------------------------------------------------------------------------- 4. deint=0
@pytest.mark.parametrize("kw", [dict(), dict(dst_w=64, dst_h=32), dict(orient=6)], ids=["in_place", "scale", "orient"])
def test_deint_zero_is_an_encoder_opened_without_it(kw):
    frames = _frames(W, H, "420")[:3]
    out = []
    for extra in (dict(), dict(deint=0)):
        with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=3, chroma="420", timing=True, **kw,
                          **extra) as enc:
            assert enc._L.mjg_debug_deint_flags(enc._h) == 0
            jp = enc.encode(frames) + enc.encode(frames[:1])
            with pytest.raises(_lib.MjgError) as e:
                enc.debug_deint(0)
            assert e.value.code == _lib.MJG_E_STATE
            ms, n = enc.kernel_times()
            out.append((jp, n, ms["scale"] > 0, enc.scale_path(0), enc.scale_path(1), enc.encode_path()))
    _check(out[1][0], out[0][0])
    assert out[0][1:] == out[1][1:] and out[0][1] == 2


def test_the_scale_interval_opens_for_a_deinterlacer_alone_and_merge_has_no_effect():
    frames = _frames(W, H, "420")
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="420", timing=True, merge=True,
                      deint=flags(0, 1)) as enc:
        assert enc.depth == enc.host_depth
        got = enc.encode(frames)
        ms, n = enc.kernel_times()
    assert n == 1 and ms["scale"] > 0
    _check(got, _ref(W, H, "420", 0, 1, qscale=5))


# ------------------------------------------------------------------------- 5. the worker
def _y4m420(frames, w, h, field):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 I{field} A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def test_worker_yadif_across_batch_boundaries():
    """5 frames, batches of 2: three submits with their halo frames give the bff sequence's packets."""
    frames = _frames(W, H, "420")
    args = ["-vf", "yadif"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    opts = worker.Options.from_env({"MJG_WORKER_BATCH": "2"})
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, W, H, "b")), stdout=out, stderr=err, opts=opts)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets = [d for _, d in r.frames(1)]
    info = r.info(1)
    assert (info.width, info.height, info.codec) == (W, H, "V_MJPEG")
    want = _ref(W, H, "420", 0, 0, qscale=profile.effective_qscale(5), sar=(1, 1))
    _check(packets, want)
    assert want != _ref(W, H, "420", 0, 1, qscale=profile.effective_qscale(5), sar=(1, 1))   # the tag was read


def test_worker_sends_mixed_field_order_to_ffmpeg(tmp_path):
    log = tmp_path / "shim.log"
    env = dict(os.environ, PATH=os.path.join(HERE, "shims") + os.pathsep + os.environ["PATH"],
               SHIM_LOG=str(log), PYTHONPATH=ROOT)
    w, h = 16, 8
    fr = np.full((3, w * h + 2 * 8 * 4), 0x41, np.uint8)      # ASCII-safe: the shim reads text
    args = ["-vf", "yadif"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    p = subprocess.run([sys.executable, "-m", "ffmpeg_distributed_amd.worker", "--device", "0", *args],
                       input=_y4m420(fr, w, h, "m"), capture_output=True, env=env, timeout=60)
    assert p.returncode == 0, p.stderr
    assert b"Im" in p.stderr and b"running ffmpeg on the CPU" in p.stderr
    calls = [json.loads(l) for l in open(log)]
    assert calls == [{"prog": "ffmpeg", "argv": ["-f", "yuv4mpegpipe", "-i", "pipe:", *args, "-f", "matroska", "pipe:"],
                      "host": "localhost"}]
    assert p.stdout[len(b"ENC["):].startswith(b"YUV4MPEG2 W16 H8 F25:1 Im A1:1 C420jpeg\n")


# ------------------------------------------------------------------------- 6. errors
@pytest.mark.parametrize("bad", [8, 9, 2, 4, 6, 17, -1])
def test_constructor_refuses_bad_deint_bits(bad):
    with pytest.raises(_lib.MjgError) as e:
        MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="420", deint=bad)
    assert e.value.code == _lib.MJG_E_INVALID and f"deint {bad}" in str(e.value)


@pytest.mark.parametrize("w,h,c", [(4, 2, "444"), (4, 4, "420"), (2, 16, "444")], ids=lambda v: str(v))
def test_constructor_refuses_a_plane_below_3x3(w, h, c):
    with pytest.raises(_lib.MjgError) as e:
        MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=NF, chroma=c, deint=YADIF)
    assert e.value.code == _lib.MJG_E_INVALID and "deint 1" in str(e.value) and "3x3" in str(e.value)


def test_halo_on_a_plain_context_is_refused():
    frames = _frames(W, H, "420")
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="420") as enc:
        with pytest.raises(_lib.MjgError) as e:
            enc.submit(frames[:3], 2, halo=2)
        assert e.value.code == _lib.MJG_E_INVALID and "deint" in str(e.value) and "halo 2" in str(e.value)
        assert enc.pending == 0
        got = enc.encode(frames[:1])      # the context is unharmed
    assert len(got) == 1
    with MjpegEncoder(0, W, H, full_range=False, qscale=5, max_batch=NF, chroma="420", deint=YADIF) as enc:
        with pytest.raises(_lib.MjgError) as e:
            enc.submit(frames[:3], 2, halo=4)
        assert e.value.code == _lib.MJG_E_INVALID and "halo 4" in str(e.value)
