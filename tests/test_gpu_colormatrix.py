"""The colour matrix on the GPU (MjpegEncoder(cmat=): k_cmat_frame behind the deinterlacer and the
orientation, in front of lut_in, the crop and the sws stage), byte for byte against
tests/colormatrix_ref.py.  Frames are seeded noise with one plane per case drawn from {0..20, 235..255},
and every case asserts from the reference that samples are clipped at both ends.  Every case compares
debug_cmat_out() first (k_cmat_frame's output), then debug_planes() where the sws stage runs, then the
JPEGs against the composed reference of the existing stages (yadif_ref, orient_ref, eq_ref, crop_ref,
chroma_resample_ref, pad_ref, oracle) on the reference's output, so a failure names the stage and the
first differing sample.  tools/cmat_host_check.py walks the launches of the shapes here on the CPU under
AddressSanitizer."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import colormatrix_ref as ref
import eq_ref
import oracle
from chroma_resample_ref import composed_planes
from crop_ref import crop_frame
from orient_ref import orient_frame, oriented_size
from pad_ref import pad_planes
from yadif_ref import deint_frames
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, split_i420

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NF = 3
C_79 = ref.coefs("bt709", "bt601")
C_67 = ref.coefs("bt601", "bt709")
MATRICES = {"bt709_bt601": C_79, "bt601_bt709": C_67, "made_up": ref.MADE_UP}
T_IN = eq_ref.perm_tables(101)


def test_the_matrices_are_what_the_cases_need():
    assert C_79 == (6657, 12850, 64871, -7252, -4748, 64448) and C_67 == (-7746, -13939, 66758, 7512, 4918, 67196)
    assert len(set(ref.MADE_UP)) == 6 and ref.MADE_UP != ref.IDENTITY


def first_diff(a: bytes, b: bytes):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i
    return n if len(a) != len(b) else -1


def _check(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (what, i, len(a), len(b), first_diff(a, b))


_SRC = {}


def _frames(w, h, c, n=NF, plane=1):
    """n frames per shape, format and extreme plane, made once and left unchanged."""
    if (w, h, c, n, plane) not in _SRC:
        f = ref.noise_frames(w, h, c, n, plane)
        f.setflags(write=False)
        _SRC[(w, h, c, n, plane)] = f
    return _SRC[(w, h, c, n, plane)]


def _same(what, i, got, want, w, h, c):
    for name, a, b in zip("YUV", split_i420(got, w, h, c), split_i420(want, w, h, c)):
        bad = np.argwhere(a != b)
        if bad.size:
            y, x = bad[0]
            print(f"{what}: frame {i} plane {name}: first difference at y={y} x={x}: got {a[y, x]}, want {b[y, x]}, "
                  f"{len(bad)} of {a.size} differ")
            pytest.fail(f"{what}: frame {i} plane {name} differs first at (y={y}, x={x})")


def chain_ref(frame, w, h, src, cmat, lut_in=None, orient=0, rect=None, dst=None, full=False, dw=None, dh=None, pad=None,
              qscale=5, sar=(1, 1), huffman="default", rst=False):
    """One decoded (or deinterlaced) frame through the composed reference: the orientation, the matrix
    on the whole oriented frame, the slot-"in" tables, the crop, the sws stage, the pad, the encoder.
    Returns {"clips": (low, high) samples the matrix clips, "cmat": the converted frame, "cmat_out": what
    the stage's buffer holds in the end (mapped by lut_in), "planes": the encoder's input, "jpeg"}."""
    dst = dst or src
    ow, oh = oriented_size(w, h, orient)
    f = orient_frame(frame, w, h, src, orient)
    out = {"clips": ref.clip_counts(f, ow, oh, src, cmat)}
    f = out["cmat"] = ref.convert_frames(f, ow, oh, src, cmat)
    if lut_in is not None:
        f = eq_ref.map_frames(f, ow, oh, src, lut_in)
    out["cmat_out"] = f
    rect = rect or (0, 0, ow, oh)
    planes = composed_planes(crop_frame(f, ow, oh, src, rect), rect[2], rect[3], src, dst, full, dw or rect[2], dh or rect[3])
    if pad is not None:
        planes = pad_planes(*planes, dst, *pad)
    out["planes"] = planes
    out["jpeg"] = oracle.encode_frame(*planes, full_range=True, qscale=qscale, sar=sar, huffman=huffman, chroma=dst, rst=rst)
    return out


def _clipped(refs):
    lo, hi = sum(r["clips"][0] for r in refs), sum(r["clips"][1] for r in refs)
    assert lo > 0 and hi > 0, ("the case clips at both ends", lo, hi)


def _check_stages(enc, refs, c, dst):
    """debug_cmat_out, then debug_planes where the sws stage runs, against refs (chain_ref per frame)."""
    for i, r in enumerate(refs):
        _same("cmat_out (k_cmat_frame's output)", i, enc.debug_cmat_out(i), r["cmat_out"], enc.or_w, enc.or_h, c)
    if enc.encode_path() & 1:      # k_encode reads the frames in place: no sws stage to read back
        return
    for i, r in enumerate(refs):
        got = split_i420(enc.debug_planes(i), enc.enc_w, enc.enc_h, dst)
        for name, a, b in zip("YUV", got, r["planes"]):
            assert (a == b).all(), ("planes (the encoder's input)", i, name, np.argwhere(a != b)[0].tolist())


def _run(w, h, c, cmat=C_79, lut_in=None, full=False, dw=None, dh=None, dst=None, rect=None, pad=None, orient=0, device=False,
         q=5, env=None, monkeypatch=None, want_paths=None, plane=1, **enc_kw):
    """One encoder, one encode of the shape's frames (from a host buffer, or from a device pointer at
    byte 1 of its allocation): every stage against the reference."""
    src_frames = _frames(w, h, c, plane=plane)
    ow, oh = oriented_size(w, h, orient)
    in_size = rect[2:] if rect else (ow, oh)
    sar = profile.scaled_sar((1, 1), in_size, (dw or in_size[0], dh or in_size[1]))
    refs = [chain_ref(f, w, h, c, cmat, lut_in, orient, rect, dst, full, dw, dh, pad, q, sar, **enc_kw) for f in src_frames]
    _clipped(refs)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    with MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, sar=sar, max_batch=NF, chroma=dst or c, src_chroma=c,
                      crop=rect, pad=pad, orient=orient, lut_in=lut_in, cmat=cmat, **enc_kw) as enc:
        assert enc.debug_cmat() == tuple(cmat)
        if want_paths is not None:
            assert (enc.scale_path(0), enc.scale_path(1), enc.encode_path() & 3) == want_paths
        if device:
            import torch
            pool = torch.zeros(src_frames.size + 1, dtype=torch.uint8, device="cuda:0")
            pool[1:] = torch.from_numpy(src_frames.reshape(-1).copy()).to("cuda:0")
            torch.cuda.synchronize()
            enc.submit(device_ptr=pool.data_ptr() + 1, nframes=len(src_frames))
            got = enc.fetch()
        else:
            got = enc.encode(src_frames)
        _check_stages(enc, refs, c, dst or c)
        if device:      # the caller's frames are never written
            assert (pool[1:].cpu().numpy() == src_frames.reshape(-1)).all()
    _check(got, [r["jpeg"] for r in refs])
    return got


# ------------------------------------------------------------------------- the stage alone, k_encode in place
ALONE = [(33, 17, "420"), (33, 17, "444"), (34, 16, "422"), (8, 8, "420"), (301, 203, "420"), (4100, 6, "420")]


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("w,h,c", ALONE, ids=[f"{w}x{h}_{c}" for w, h, c in ALONE])
def test_the_stage_alone_k_encode_reads_the_converted_frames_in_place(w, h, c, name):
    """33x17 4:2:0: odd both ways, the last cell half-empty; 33x17 4:4:4: odd frame bytes; 34x16 4:2:2; 8x8: narrower
    than one piece; 301x203: several workgroups a frame, pieces over row ends in later workgroups; 4100x6: long rows."""
    _run(w, h, c, cmat=MATRICES[name], want_paths=(0, 0, 1), plane=ALONE.index((w, h, c)) % 3)


# ------------------------------------------------------------------------- a device pointer at byte 1
@pytest.mark.parametrize("w,h,c", [(33, 17, "444"), (301, 203, "420")], ids=["33x17_444", "301x203_420"])
def test_a_device_pointer_at_byte_1(w, h, c):
    _run(w, h, c, cmat=ref.MADE_UP, device=True, want_paths=(0, 0, 1), plane=0)


# ------------------------------------------------------------------------- the buffers
def test_in_place_in_d_deint_under_halo_submits():
    w, h, c = 130, 66, "420"
    frames = _frames(w, h, c, 5, plane=2)
    d = deint_frames(frames, w, h, c, 0, 1)
    refs = [chain_ref(f, w, h, c, C_79) for f in d]
    _clipped(refs)
    got = []
    with MjpegEncoder(0, w, h, qscale=5, max_batch=NF, chroma=c, deint=_lib.MJG_DEINT_YADIF, cmat=C_79) as enc:
        for lo, n, halo in ((0, 3, 2), (3, 2, 1)):
            first = lo - (halo & 1)
            enc.submit(frames[first:lo + n + (halo >> 1 & 1)], n, halo=halo)
            got += enc.fetch()
            for i in range(n):
                _same(f"cmat_out in d_deint, halo {halo}", lo + i, enc.debug_cmat_out(i), refs[lo + i]["cmat_out"], w, h, c)
                _same(f"debug_deint returns the converted frame, halo {halo}", lo + i, enc.debug_deint(i),
                      refs[lo + i]["cmat_out"], w, h, c)
    _check(got, [r["jpeg"] for r in refs])


def test_in_place_in_d_orient_with_a_transpose():
    _run(301, 203, "420", cmat=C_67, orient=3, want_paths=(0, 0, 1), plane=0)


def test_into_d_lut_with_a_lut_in_in_place_behind_it():
    """A permutation table behind the matrix: table(matrix(x)) is not matrix(table(x)), so the stage order shows."""
    w, h, c = 130, 66, "420"
    f = _frames(w, h, c)
    swapped = ref.convert_frames(eq_ref.map_frames(f, w, h, c, T_IN), w, h, c, C_79)
    assert (swapped != eq_ref.map_frames(ref.convert_frames(f, w, h, c, C_79), w, h, c, T_IN)).any()
    _run(w, h, c, cmat=C_79, lut_in=T_IN, want_paths=(0, 0, 1))
    _run(w, h, c, cmat=C_79, lut_in=T_IN, device=True, dw=64, dh=32)


# ------------------------------------------------------------------------- submit modes
@pytest.mark.parametrize("split", [(1, 3, 1), (1, 1, 2, 1)], ids=["1+3+1", "four"])
def test_submit_segments_each_from_byte_1_of_its_own_allocation(split):
    import torch
    w, h, c = 130, 66, "420"
    frames = _frames(w, h, c, 5, plane=0)
    refs = [chain_ref(f, w, h, c, ref.MADE_UP) for f in frames]
    _clipped(refs)
    segs, at = [], 0
    for n in split:
        t = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device="cuda:0")
        t[1:] = torch.from_numpy(frames[at:at + n].reshape(-1).copy()).to("cuda:0")
        segs.append((t, n))
        at += n
    torch.cuda.synchronize()
    with MjpegEncoder(0, w, h, qscale=5, max_batch=5, chroma=c, cmat=ref.MADE_UP) as enc:
        enc.submit_segments([(t.data_ptr() + 1, n) for t, n in segs])
        got = enc.fetch()
        for i in range(5):
            _same(f"cmat_out, segments {split}", i, enc.debug_cmat_out(i), refs[i]["cmat_out"], w, h, c)
    at = 0
    for t, n in segs:      # the caller's frames are never written
        assert (t[1:].cpu().numpy() == frames[at:at + n].reshape(-1)).all()
        at += n
    _check(got, [r["jpeg"] for r in refs])


def test_two_merged_device_submits():
    import torch
    w, h, c = 130, 66, "420"
    frames = _frames(w, h, c)
    sar = profile.scaled_sar((1, 1), (w, h), (64, 32))
    refs = [chain_ref(f, w, h, c, C_79, dw=64, dh=32, sar=sar) for f in frames]
    _clipped(refs)
    ts = [torch.from_numpy(frames[lo:lo + n].copy()).to("cuda:0") for lo, n in ((0, 2), (2, 1))]
    torch.cuda.synchronize()
    got = []
    with MjpegEncoder(0, w, h, 64, 32, qscale=5, sar=sar, max_batch=NF, chroma=c, merge=True, cmat=C_79) as enc:
        for t in ts:
            enc.submit(device_ptr=t.data_ptr(), nframes=t.shape[0])
        for t in ts:
            enc.sync()
            got += enc.fetch()
        # (a read-back syncs whatever is queued, so only the last job's: its frame lies behind the first job's two)
        _same("cmat_out, merged submits", 2, enc.debug_cmat_out(0), refs[2]["cmat_out"], w, h, c)
    _check(got, [r["jpeg"] for r in refs])


# ------------------------------------------------------------------------- every reader behind the stage
def test_crop_read_in_place_through_the_unaligned_fetch():
    _run(130, 66, "420", rect=(6, 2, 64, 32), want_paths=(0, 0, 3))


def test_crop_read_in_place_through_the_aligned_fetch(monkeypatch):
    _run(130, 66, "420", rect=(16, 2, 64, 32), env={"MJG_UNALIGNED_FETCH": "0"}, monkeypatch=monkeypatch,
         want_paths=(0, 0, 1))


def test_k_scale_reads_the_converted_frames():
    _run(130, 66, "420", dw=64, dh=32, want_paths=(2, 2, 0))


def test_k_scale_stream_reads_the_converted_frames(monkeypatch):
    _run(130, 66, "420", dw=64, dh=32, env={"MJG_SCALE_STREAM": "1"}, monkeypatch=monkeypatch, want_paths=(3, 3, 0))


def test_the_pix_fmt_copy_reads_the_converted_frames():
    """tv 4:4:4 -> yuvj420p without a resize: luma through k_plane_copy's tv->pc table behind the matrix."""
    _run(130, 66, "444", dst="420", want_paths=(1, 2, 0), plane=2)


def test_the_pad_copy_reads_the_converted_frames():
    _run(34, 18, "420", pad=(8, 10, 50, 38), plane=0)


def test_the_stage_runs_inside_the_scale_interval():
    with MjpegEncoder(0, 33, 17, qscale=5, max_batch=NF, chroma="444", timing=True, cmat=C_79) as enc:
        enc.encode(_frames(33, 17, "444"))
        ms, n = enc.kernel_times()
    assert n == 1 and ms["scale"] > 0


# ------------------------------------------------------------------------- nothing changed for others
def test_no_matrix_and_the_identity_open_a_context_without_the_stage():
    frames = _frames(130, 66, "420")
    for extra in (dict(), dict(dst_w=70, dst_h=38), dict(lut_in=T_IN)):
        out = []
        for cm in (None, ref.IDENTITY):
            with MjpegEncoder(0, 130, 66, qscale=5, max_batch=NF, chroma="420", cmat=cm, **extra) as enc:
                assert enc.debug_cmat() is None
                jp = enc.encode(frames)
                with pytest.raises(_lib.MjgError) as e:
                    enc.debug_cmat_out(0)
                assert e.value.code == _lib.MJG_E_STATE
                out.append((jp, enc.scale_path(0), enc.scale_path(1), enc.encode_path()))
        _check(out[1][0], out[0][0])
        assert out[1][1:] == out[0][1:]


def test_a_bad_matrix_is_refused():
    with pytest.raises(ValueError):
        MjpegEncoder(0, 33, 17, chroma="444", cmat=(1, 2, 3))
    with pytest.raises(_lib.MjgError) as e:
        MjpegEncoder(0, 33, 17, chroma="444", cmat=(0, 0, 65536, 0, 262145, 65536))
    assert e.value.code == _lib.MJG_E_INVALID and str(e.value).count("cmatrix vu 262145")


# ------------------------------------------------------------------------- the worker
def _y4m420(frames, w, h, field="p", extra=""):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 I{field} A1:1 C420jpeg{extra}\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def test_worker_yadif_colormatrix_eq_scale_pad_across_three_halo_submits():
    w, h, c = 130, 66, "420"
    frames = _frames(w, h, c, 5)
    vf = "yadif,colormatrix=bt709:bt601,eq=1.1,scale=70:38,pad=80:48"
    args = ["-vf", vf] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, w, h, "t")), stdout=out, stderr=err,
                    opts=worker.Options(batch=2))      # submits of 2 + 2 + 1
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue(), err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets, info = [d for _, d in r.frames(1)], r.info(1)
    assert (info.width, info.height, info.codec) == (80, 48, "V_MJPEG")
    assert profile.colormatrix_coefs("bt709", "bt601") == C_79
    tabs = profile.eq_tables(dict(contrast=1.1))
    assert (tabs == eq_ref.tables(dict(contrast=1.1))).all()
    d = deint_frames(frames, w, h, c, 0, 1)
    sar = profile.scaled_sar((1, 1), (w, h), (70, 38))
    pad = profile.resolve_pad({"w": 80, "h": 48, "x": None, "y": None}, 70, 38, c)
    refs = [chain_ref(f, w, h, c, C_79, tabs, dw=70, dh=38, pad=pad, qscale=profile.effective_qscale(5), sar=sar) for f in d]
    _clipped(refs)
    _check(packets, [r["jpeg"] for r in refs], "worker")


def test_worker_sends_a_full_range_source_to_ffmpeg(tmp_path):
    log = tmp_path / "shim.log"
    env = dict(os.environ, PATH=os.path.join(HERE, "shims") + os.pathsep + os.environ["PATH"],
               SHIM_LOG=str(log), PYTHONPATH=ROOT)
    w, h = 16, 8
    fr = np.full((3, w * h + 2 * 8 * 4), 0x41, np.uint8)      # ASCII-safe: the shim reads text
    args = ["-vf", "colormatrix=bt709:bt601,scale=8:4"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    p = subprocess.run([sys.executable, "-m", "ffmpeg_distributed_amd.worker", "--device", "0", *args],
                       input=_y4m420(fr, w, h, extra=" XCOLORRANGE=FULL"), capture_output=True, env=env, timeout=60)
    assert p.returncode == 0, p.stderr
    assert b"colormatrix on a full-range (yuvj) input: the filter takes yuv420p / yuv422p / yuv444p" in p.stderr
    assert b"running ffmpeg on the CPU" in p.stderr
    calls = [json.loads(l) for l in open(log)]
    assert calls == [{"prog": "ffmpeg", "argv": ["-f", "yuv4mpegpipe", "-i", "pipe:", *args, "-f", "matroska", "pipe:"],
                      "host": "localhost"}]
