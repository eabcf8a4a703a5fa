"""`-vf yadif` without a GPU: the reference itself (tests/yadif_ref.py: the loop form against the
numpy form, and the properties a GPU test relies on), the profile parser, the container's field
order, the worker's parity resolution and its batch schedule."""
import io
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from yadif_ref import deint_frames, yadif_plane_loop, yadif_plane_vec
from ffmpeg_distributed_amd import container, profile, worker
from ffmpeg_distributed_amd.encoder import i420_frame_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAIL = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()

SIZES = [(3, 3), (10, 4), (35, 19), (130, 66)]


def _noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3))


# ------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_loop_and_numpy_forms_agree(w, h):
    p, c, n = _noise(w, h, 7 * w + h)
    for tff in (1, 0):
        for mode in (0, 2):
            a, b = yadif_plane_loop(p, c, n, mode, tff), yadif_plane_vec(p, c, n, mode, tff)
            bad = np.argwhere(a != b)
            assert bad.size == 0, (tff, mode, bad[:4].tolist())


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_kept_rows_are_cur(w, h):
    p, c, n = _noise(w, h, 3 * w + h)
    for tff in (1, 0):
        out = yadif_plane_vec(p, c, n, 0, tff)
        kept = [y for y in range(h) if not ((y ^ tff ^ 1) & 1)]
        assert kept and (out[kept] == c[kept]).all()
        assert kept[0] == (0 if tff else 1)      # tff: the odd rows are interpolated


def test_static_vertical_ramp_comes_back_in_the_interior():
    """prev = cur = next, a ramp down the rows: d = cur[y], every temporal difference is 0 and the
    mode-0 check gives diff = 0 in rows 2..h-3, so out = d there whatever the spatial prediction."""
    w, h = 35, 19
    ramp = np.repeat((np.arange(h, dtype=np.uint8) * 9)[:, None], w, axis=1)
    for tff in (1, 0):
        for fn in (yadif_plane_loop, yadif_plane_vec):
            out = fn(ramp, ramp, ramp, 0, tff)
            assert (out[2:h - 2] == ramp[2:h - 2]).all()


def test_every_argument_changes_the_output_on_the_test_noise():
    """No GPU test can pass while ignoring the mode, the parity or a neighbour frame: on 130 x 66
    noise each of them changes the reference."""
    w, h, c = 130, 66, "420"
    fb = i420_frame_bytes(w, h, c)
    fr = np.random.default_rng(130066).integers(0, 256, (4, fb), dtype=np.uint8)
    base = deint_frames(fr[:3], w, h, c, 0, 1)
    assert (deint_frames(fr[:3], w, h, c, 2, 1) != base).sum() >= 12      # modes 0 and 2: the clip differs
    assert (deint_frames(fr[:3], w, h, c, 0, 0) != base).any()            # tff / bff
    # the first frame's prev (itself) and the last frame's next (itself) replaced by another frame
    longer = deint_frames(np.concatenate([fr[3:4], fr[:3], fr[3:4]]), w, h, c, 0, 1)[1:4]
    assert (longer[0] != base[0]).any() and (longer[2] != base[2]).any()
    assert (longer[1] == base[1]).all()
    # and within a sequence: prev and next are different frames
    swapped = deint_frames(fr[[2, 1, 0]], w, h, c, 0, 1)
    assert (swapped[1] != base[1]).any()


def test_one_frame_is_its_own_neighbours():
    w, h, c = 33, 17, "444"
    f = np.random.default_rng(5).integers(0, 256, (1, i420_frame_bytes(w, h, c)), dtype=np.uint8)
    one = deint_frames(f, w, h, c, 0, 1)
    assert (one[0] == deint_frames(np.repeat(f, 3, axis=0), w, h, c, 0, 1)[1]).all()


# ------------------------------------------------------------------------- the parser
ACCEPTED = [
    ("yadif", {"mode": 0, "parity": -1}),
    ("yadif=0", {"mode": 0, "parity": -1}),
    ("yadif=2", {"mode": 2, "parity": -1}),
    ("yadif=0:0", {"mode": 0, "parity": 0}),
    ("yadif=2:1", {"mode": 2, "parity": 1}),
    ("yadif=0:-1:0", {"mode": 0, "parity": -1}),
    ("yadif=send_frame", {"mode": 0, "parity": -1}),
    ("yadif=send_frame_nospatial:bff", {"mode": 2, "parity": 1}),
    ("yadif=mode=send_frame:parity=tff:deint=all", {"mode": 0, "parity": 0}),
    ("yadif=mode=2", {"mode": 2, "parity": -1}),
    ("yadif=parity=auto", {"mode": 0, "parity": -1}),
    ("yadif=parity=bff:mode=0", {"mode": 0, "parity": 1}),
    ("yadif=0:tff:all", {"mode": 0, "parity": 0}),
    ("yadif=deint=0", {"mode": 0, "parity": -1}),
]


@pytest.mark.parametrize("vf,want", ACCEPTED, ids=[a for a, _ in ACCEPTED])
def test_parser_accepts(vf, want):
    p = profile.parse(["-vf", vf] + TAIL)
    assert p.deint == want
    assert (p.crop, p.scale, p.pad, p.orient) == (None, None, None, 0)


REJECTED = [
    ("yadif=1", "mode=1"),
    ("yadif=3", "mode=3"),
    ("yadif=send_field", "mode=1"),
    ("yadif=mode=send_field_nospatial", "mode=3"),
    ("yadif=0:0:1", "deint=interlaced"),
    ("yadif=deint=interlaced", "deint=interlaced"),
    ("yadif=0:0:0:0", "positional"),
    ("yadif=mode=4", "mode=4"),
    ("yadif=parity=2", "parity=2"),
    ("yadif=field=1", "'field'"),
    ("scale=64:32,yadif", "yadif after scale"),
    ("vflip,yadif", "yadif after vflip"),
    ("yadif,yadif", "yadif after yadif"),
    ("crop=64:32,yadif=0,scale=32:16", "yadif after crop"),
    ("bwdif", "bwdif"),
    ("bwdif=0,scale=64:32", "bwdif"),
    ("yadif,w3fdif", "w3fdif"),
    ("estdif", "estdif"),
]


@pytest.mark.parametrize("vf,reason", REJECTED, ids=[a for a, _ in REJECTED])
def test_parser_rejects_with_a_reason_that_names_it(vf, reason):
    with pytest.raises(profile.Unsupported) as e:
        profile.parse(["-vf", vf] + TAIL)
    assert reason in str(e.value), str(e.value)
    assert profile.try_parse(["-vf", vf] + TAIL)[0] is None


def test_parser_without_yadif_has_no_deint():
    assert profile.parse(TAIL).deint is None
    assert profile.parse(["-vf", "scale=64:32"] + TAIL).deint is None


def test_yadif_in_front_of_the_whole_chain():
    p = profile.parse(["-vf", "yadif=0:1,transpose=1,crop=62:126:2:2,scale=32:64,pad=48:80:8:8"] + TAIL)
    assert p.deint == {"mode": 0, "parity": 1}
    assert p.orient == 3 and p.scale == (32, 64)
    assert p.crop == {"w": 62, "h": 126, "x": 2, "y": 2} and p.pad == {"w": 48, "h": 80, "x": 8, "y": 8}
    q = profile.parse(["-vf", "transpose=1,crop=62:126:2:2,scale=32:64,pad=48:80:8:8"] + TAIL)
    p.deint = None
    assert p == q
    r = profile.parse(["-vf", "yadif,scale=1280:720"] + TAIL)
    assert r.deint == {"mode": 0, "parity": -1} and r.scale == (1280, 720) and r.orient == 0


# ------------------------------------------------------------------------- the containers
def _y4m(frames, w, h, tags):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1{tags}\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + bytes(f))
    return b.getvalue()


@pytest.mark.parametrize("tags,field", [(" It A1:1 C420jpeg", "t"), (" Ib A1:1 C420jpeg", "b"), (" Im A1:1 C420jpeg", "m"),
                                        (" A1:1 C420jpeg", "p"), (" Ip A1:1 C420jpeg", "p"), (" I? C420jpeg", "p")])
def test_y4m_reader_parses_the_field_order(tags, field):
    rd = container.Y4MReader(io.BytesIO(_y4m([], 16, 8, tags)))
    assert rd.info.field == field and (rd.info.width, rd.info.height) == (16, 8)


def test_stream_info_field_is_the_last_field_and_defaults_to_progressive():
    import dataclasses
    assert [f.name for f in dataclasses.fields(container.StreamInfo)][-1] == "field"
    assert container.StreamInfo(16, 8).field == "p"


def test_y4m_header_round_trip():
    info = container.StreamInfo(16, 8, Fraction(30000, 1001), (4, 3), True, chroma="422")
    assert container.y4m_header(info) == b"YUV4MPEG2 W16 H8 F30000:1001 Ip A4:3 C422 XCOLORRANGE=FULL\n"
    assert container.y4m_header(container.StreamInfo(16, 8)) == b"YUV4MPEG2 W16 H8 F25:1 Ip A0:0 C420jpeg\n"
    for fld in "tbm":
        info = container.StreamInfo(16, 8, sar=(1, 1), field=fld)
        hdr = container.y4m_header(info)
        assert f" I{fld} ".encode() in hdr
        assert container.Y4MReader(io.BytesIO(hdr)).info == info


def _mkv_with(video_extra: bytes) -> bytes:
    """A Matroska segment with one V_UNCOMPRESSED I420 track of 16 x 8 and no clusters, the Video
    master extended by `video_extra` (a small local EBML writer: container.element / uint_el)."""
    E, U, S = container.element, container.uint_el, container.str_el
    ebml = E(container.EBML, U(0x4286, 1) + U(0x42F7, 1) + U(0x42F2, 4) + U(0x42F3, 8) + S(0x4282, "matroska")
             + U(0x4287, 4) + U(0x4285, 2))
    video = U(0xB0, 16) + U(0xBA, 8) + E(0x2EB524, b"I420") + video_extra
    track = E(container.TRACK_ENTRY, U(0xD7, 1) + U(0x73C5, 1) + U(0x83, 1) + S(0x86, "V_UNCOMPRESSED")
              + U(0x23E383, 40000000) + E(container.VIDEO, video))
    body = E(container.INFO, U(0x2AD7B1, 1000000)) + E(container.TRACKS, track)
    return ebml + E(container.SEGMENT, body)


@pytest.mark.parametrize("extra,field", [
    (b"", "p"),
    (container.uint_el(0x9A, 0), "p"),
    (container.uint_el(0x9A, 2), "p"),
    (container.uint_el(0x9A, 2) + container.uint_el(0x9D, 6), "p"),       # FlagInterlaced != 1: the order is not read
    (container.uint_el(0x9A, 1) + container.uint_el(0x9D, 1), "t"),
    (container.uint_el(0x9A, 1) + container.uint_el(0x9D, 6), "b"),
    (container.uint_el(0x9A, 1), "m"),
    (container.uint_el(0x9A, 1) + container.uint_el(0x9D, 0), "m"),
    (container.uint_el(0x9A, 1) + container.uint_el(0x9D, 2), "m"),
    (container.uint_el(0x9A, 1) + container.uint_el(0x9D, 9), "m"),
    (container.uint_el(0x9A, 1) + container.uint_el(0x9D, 14), "m"),
], ids=lambda v: v if isinstance(v, str) else v.hex() or "none")
def test_mkv_reader_parses_flag_interlaced_and_field_order(extra, field):
    r = container.MkvReader(io.BytesIO(_mkv_with(extra)))
    info = r.info(1)
    assert (info.width, info.height, info.chroma, info.field) == (16, 8, "420", field)


# ------------------------------------------------------------------------- the worker's decisions
def test_resolve_deint():
    I = container.StreamInfo
    y, ns, bff = 1, 2, 4
    assert worker.resolve_deint(None, I(16, 8)) == 0
    auto0, auto2 = {"mode": 0, "parity": -1}, {"mode": 2, "parity": -1}
    assert worker.resolve_deint(auto0, I(16, 8)) == y
    assert worker.resolve_deint(auto0, I(16, 8, field="t")) == y
    assert worker.resolve_deint(auto0, I(16, 8, field="b")) == y | bff
    assert worker.resolve_deint(auto2, I(16, 8, field="b")) == y | ns | bff
    why = worker.resolve_deint(auto0, I(16, 8, field="m"))
    assert isinstance(why, str) and "Im" in why and "yadif" in why
    # a given parity is used as given
    assert worker.resolve_deint({"mode": 0, "parity": 1}, I(16, 8, field="t")) == y | bff
    assert worker.resolve_deint({"mode": 2, "parity": 0}, I(16, 8, field="m")) == y | ns
    # planes below 3 x 3 (4 x 2 luma; 4 x 4 4:2:0 has 2 x 2 chroma)
    for info in (I(4, 2, chroma="444"), I(4, 4, chroma="420"), I(2, 16, chroma="444")):
        why = worker.resolve_deint(auto0, info)
        assert isinstance(why, str) and "3x3" in why
    assert worker.resolve_deint(auto0, I(6, 6, chroma="420")) == y
    assert worker.resolve_deint(auto0, I(3, 3, chroma="444")) == y


def test_encoder_key_depends_on_the_deinterlacer():
    info = container.StreamInfo(130, 66, chroma="420")
    prof = profile.parse(["-vf", "yadif"] + TAIL)
    k = [worker.encoder_key(prof, info, 130, 66, (1, 1), False, 8, deint=d) for d in (0, 1, 3, 5, 7)]
    assert len(set(k)) == 5
    assert k[0] == worker.encoder_key(prof, info, 130, 66, (1, 1), False, 8)


@pytest.mark.parametrize("batch", [1, 2, 4])
def test_batch_schedule(batch):
    """Frames 0..N-1 once each and in order; each submit's neighbours are the frames next to it,
    present exactly when they exist in the segment."""
    for n in range(1, 3 * batch + 2):
        sched = worker.deint_schedule(n, batch)
        enc = [f for first, k, _, _ in sched for f in range(first, first + k)]
        assert enc == list(range(n)), (n, batch, sched)
        for first, k, hp, hn in sched:
            assert 1 <= k <= batch
            assert bool(hp) == (first > 0) and bool(hn) == (first + k < n), (n, batch, sched)
        assert not sched[-1][3]
        assert all(k == batch for _, k, _, _ in sched[:-1])
    assert worker.deint_schedule(1, batch) == [(0, 1, False, False)]
    assert worker.deint_schedule(0, batch) == []


def test_deint_step_keeps_one_frame_of_look_ahead():
    assert worker.deint_step(0, 5, 4, False) == (0, 4, False, True)
    assert worker.deint_step(0, 4, 4, True) == (0, 4, False, False)
    assert worker.deint_step(4, 6, 4, True) == (4, 2, True, False)
    assert worker.deint_step(4, 5, 4, True) == (4, 1, True, False)
    assert worker.deint_step(0, 0, 4, True) == (0, 0, False, False)


def test_worker_sends_a_mixed_field_order_to_ffmpeg_with_its_tag(tmp_path):
    """y4m `Im` with -vf yadif (parity auto): the CPU ffmpeg gets the frames, the unchanged
    remote_args and the source's own I tag (not `Ip`)."""
    log = tmp_path / "shim.log"
    env = dict(os.environ, PATH=os.path.join(HERE, "shims") + os.pathsep + os.environ["PATH"],
               SHIM_LOG=str(log), PYTHONPATH=ROOT)
    w, h = 16, 8
    fr = np.full((3, w * h + 2 * 8 * 4), 0x41, np.uint8)      # ASCII-safe: the shim reads text
    fr[:, :7] = np.arange(3)[:, None] + 0x30
    args = ["-vf", "yadif"] + TAIL
    p = subprocess.run([sys.executable, "-m", "ffmpeg_distributed_amd.worker", "--device", "0", *args],
                       input=_y4m(fr, w, h, " Im A1:1 C420jpeg"), capture_output=True, env=env, timeout=60)
    assert p.returncode == 0, p.stderr
    assert b"Im" in p.stderr and b"running ffmpeg on the CPU" in p.stderr
    calls = [json.loads(l) for l in open(log)]
    assert calls == [{"prog": "ffmpeg", "argv": ["-f", "yuv4mpegpipe", "-i", "pipe:", *args, "-f", "matroska", "pipe:"],
                      "host": "localhost"}]
    body = p.stdout[len(b"ENC["):-1]
    assert body.startswith(b"YUV4MPEG2 W16 H8 F25:1 Im A1:1 C420jpeg\n")
    rd = container.Y4MReader(io.BytesIO(body))
    assert rd.info.field == "m"
    buf = np.zeros_like(fr)
    assert rd.read_into(buf, 3) == 3
    np.testing.assert_array_equal(buf, fr)
