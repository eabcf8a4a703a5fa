"""`-vf tile` on the GPU (MjpegEncoder(sheet=...): k_tile_plane behind the sws stage and the sharpen, mjg_open_sheet),
byte for byte against tests/tile_ref.py.  Every case compares debug_cell() first (the kernel's input, what
the composed references of the chain in front give), then debug_planes() (the sheets, the encoder's
input), then the JPEGs, so a failure names the stage and the first differing sample.
tools/tile_host_check.py walks the launches of every geometry here (tile_ref.GPU_GEOMETRY) on the CPU under
AddressSanitizer (profiles/tile/host_check.txt)."""
import io

import numpy as np
import pytest

import colormatrix_ref
import eq_ref
import tile_ref
from chroma_resample_ref import composed_planes, source_frames
from crop_ref import crop_frame
from orient_ref import orient_frame, oriented_size
from unsharp_ref import DEFAULT, kernel_constant, unsharp_planes
from yadif_ref import deint_frames
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, split_i420

pytestmark = pytest.mark.gpu


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


def _frames(w, h, c, n):
    """n frames per shape and format, made once and left unchanged."""
    if (w, h, c, n) not in _SRC:
        f = source_frames(w, h, n, 7 * w + h + n, c)
        f.setflags(write=False)
        _SRC[(w, h, c, n)] = f
    return _SRC[(w, h, c, n)]


def _same_planes(what, i, got, want):
    for name, a, b in zip("YUV", got, want):
        bad = np.argwhere(a != b)
        if bad.size:
            y, x = bad[0]
            print(f"{what}: frame {i} plane {name}: first difference at y={y} x={x}: got {a[y, x]}, want {b[y, x]}, "
                  f"{len(bad)} of {a.size} differ")
            pytest.fail(f"{what}: frame {i} plane {name} differs first at (y={y}, x={x})")


_REF = {}


def _ref(key, cells, cw, ch, dst, sheet, **enc_kw):
    """(sheet planes, JPEGs) of one sequence of cells, computed once per key."""
    key = (key, cw, ch, dst, sheet, tuple(sorted(enc_kw.items())))
    if key not in _REF:
        sheets = tile_ref.sheets_numpy(cells, cw, ch, dst, sheet)
        _REF[key] = (sheets, [tile_ref.sheet_jpeg(s, dst, **enc_kw) for s in sheets])
    return _REF[key]


def _check_stages(enc, cells, sheets, dst, first_cell=0):
    """debug_cell for every input frame of the last submit, then debug_planes for every sheet."""
    for i, want in enumerate(cells):
        _same_planes("cell (k_tile_plane's input)", first_cell + i, split_i420(enc.debug_cell(i), enc.dst_w, enc.dst_h, dst), want)
    for j, want in enumerate(sheets):
        _same_planes("sheet (k_tile_plane's output)", j, split_i420(enc.debug_planes(j), enc.enc_w, enc.enc_h, dst), want)
    for bad in (len(cells), -1):
        with pytest.raises(_lib.MjgError):
            enc.debug_cell(bad)
    with pytest.raises(_lib.MjgError):
        enc.debug_planes(len(sheets))


def _cells(frames, w, h, c, us=None, full=False, dw=None, dh=None, dst=None):
    return [tile_ref.cell_planes(f, w, h, c, us, dst=dst, full=full, dw=dw, dh=dh) for f in frames]


def test_the_geometry_list_is_what_the_cases_below_encode():
    """tools/tile_host_check.py walks tile_ref.GPU_GEOMETRY: keep it in step with the cases."""
    assert tile_ref.GPU_GEOMETRY == [
        (8, 8, "420", (5, 3, 0, 0, 0), (17,)), (33, 17, "444", (2, 2, 0, 3, 5), (4,)), (33, 17, "444", (2, 2, 0, 3, 5), (5,)),
        (208, 120, "422", (2, 2, 3, 0, 0), (7,)), (64, 32, "420", (3, 2, 0, 0, 0), (6,)), (64, 32, "420", (3, 2, 0, 0, 0), (7,)),
        (16, 16, "420", (2, 2, 0, 0, 0), (4, 1, 6)), (16, 16, "420", (2, 2, 0, 0, 0), (4,)), (16, 16, "420", (2, 2, 0, 0, 0), (1,)),
        (16, 16, "420", (2, 2, 0, 0, 0), (6,)), (32, 16, "420", (2, 1, 0, 0, 0), (5,)), (32, 16, "420", (2, 1, 0, 0, 0), (4,)),
        (32, 48, "420", (2, 2, 0, 0, 0), (3,)), (32, 24, "420", (3, 2, 0, 0, 0), (6,))]


# ------------------------------------------------------------------------- 1. cells narrower than a piece
def test_cells_narrower_than_a_piece_and_a_partial_last_sheet():
    """16x16 4:2:0 tv -> scale=8:8,tile=5x3, 17 frames in one host submit: two 40x24 sheets; the chroma cell rows are 4
    bytes, so every piece is put together byte by byte; the second sheet has 2 cells and 13 blank."""
    w, h, c, sheet, n = 16, 16, "420", (5, 3, 0, 0, 0), 17
    frames = _frames(w, h, c, n)
    sar = profile.scaled_sar((1, 1), (w, h), (8, 8))
    cells = _cells(frames, w, h, c, dw=8, dh=8)
    sheets, jp = _ref("t1", cells, 8, 8, c, sheet, sar=sar)
    assert len(sheets) == 2 and sheets[0][0].shape == (24, 40)
    with MjpegEncoder(0, w, h, 8, 8, qscale=5, sar=sar, max_batch=n, chroma=c, sheet=sheet) as enc:
        assert enc.debug_sheet() == (5, 3, 15, 0, 0) and (enc.enc_w, enc.enc_h) == (40, 24)
        assert enc.frames_out(17) == 2 and enc.frames_out(15) == 1 and enc.frames_out(16) == 2
        enc.submit(frames)
        assert len(enc.sync()) == 2
        got = enc.fetch()
        _check_stages(enc, cells, sheets, c)
    _check(got, jp)


# ------------------------------------------------------------------------- 2. no scale, odd byte counts
def test_no_scale_odd_bytes_margin_and_padding_from_a_device_pointer_at_byte_1():
    """33x17 4:4:4 full range, tile=2x2:margin=3:padding=5 -> 77x45: 4 frames as a device submit from byte 1 of its
    allocation, then 5 frames (a second sheet with one cell)."""
    import torch
    w, h, c, sheet = 33, 17, "444", (2, 2, 0, 3, 5)
    frames = _frames(w, h, c, 5)
    cells = _cells(frames, w, h, c, full=True)
    with MjpegEncoder(0, w, h, full_range=True, qscale=5, max_batch=5, chroma=c, sheet=sheet) as enc:
        assert (enc.enc_w, enc.enc_h) == (77, 45) and enc.scale_path(0) != 0      # the sws stage always runs with a sheet
        for n in (4, 5):
            sheets, jp = _ref(("t2", n), cells[:n], w, h, c, sheet)
            pool = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device="cuda:0")
            pool[1:] = torch.from_numpy(frames[:n].reshape(-1).copy()).to("cuda:0")
            torch.cuda.synchronize()
            enc.submit(device_ptr=pool.data_ptr() + 1, nframes=n)
            got = enc.fetch()
            _check_stages(enc, cells[:n], sheets, c)
            assert (pool[1:].cpu().numpy() == frames[:n].reshape(-1)).all()      # the caller's frames are never written
            _check(got, jp, f"{n} frames")


# ------------------------------------------------------------------------- 3. past one workgroup, N < cols * rows
def test_past_one_workgroup_and_fewer_frames_than_cells():
    """416x240 4:2:2 tv -> scale=208:120,tile=2x2:nb_frames=3, 7 frames: three 416x240 sheets of 3, 3 and 1 frames, cell 3
    blank in all."""
    w, h, c, sheet, n = 416, 240, "422", (2, 2, 3, 0, 0), 7
    per_wg = 16 * kernel_constant("kCopyThreads") * kernel_constant("kCopyVecs")
    assert 416 * 240 > per_wg and 208 * 240 > per_wg      # luma and chroma: more than one workgroup per (plane, sheet)
    frames = _frames(w, h, c, n)
    sar = profile.scaled_sar((1, 1), (w, h), (208, 120))
    cells = _cells(frames, w, h, c, dw=208, dh=120)
    sheets, jp = _ref("t3", cells, 208, 120, c, sheet, sar=sar)
    assert len(sheets) == 3
    for s in sheets:
        assert (s[0][120:, 208:] == 0).all() and (s[1][120:, 104:] == 128).all()
    with MjpegEncoder(0, w, h, 208, 120, qscale=5, sar=sar, max_batch=8, chroma=c, sheet=sheet) as enc:
        assert enc.debug_sheet() == (2, 2, 3, 0, 0)
        got = enc.encode(frames)      # 6 + 1: max_batch 8 holds two sheets of 3
        _check_stages(enc, cells[6:], sheets[2:], c, first_cell=6)
    _check(got, jp)
    with MjpegEncoder(0, w, h, 208, 120, qscale=5, sar=sar, max_batch=7, chroma=c, sheet=sheet) as enc:
        enc.submit(frames)
        got = enc.fetch()
        _check_stages(enc, cells, sheets, c)
    _check(got, jp, "one submit")


# ------------------------------------------------------------------------- 4. behind the sharpen, RST, optimal
@pytest.mark.parametrize("enc_kw", [{}, {"rst": True}, {"huffman": "optimal"}], ids=["plain", "rst", "optimal"])
def test_behind_the_sharpen(enc_kw):
    """130x66 4:2:0 -> scale=64:32,unsharp,tile=3x2: 6 frames (one full 192x64 sheet) and 7 (a second with one cell)."""
    w, h, c, sheet = 130, 66, "420", (3, 2, 0, 0, 0)
    frames = _frames(w, h, c, 7)
    sar = profile.scaled_sar((1, 1), (w, h), (64, 32))
    cells = _cells(frames, w, h, c, us=DEFAULT, dw=64, dh=32)
    with MjpegEncoder(0, w, h, 64, 32, qscale=5, sar=sar, max_batch=7, chroma=c, unsharp=DEFAULT, sheet=sheet, **enc_kw) as enc:
        for n in (6, 7):
            sheets, jp = _ref(("t4", n), cells[:n], 64, 32, c, sheet, sar=sar, **enc_kw)
            enc.submit(frames[:n])
            got = enc.fetch()
            _check_stages(enc, cells[:n], sheets, c)
            pre = tile_ref.cell_planes(frames[0], w, h, c, dw=64, dh=32)
            _same_planes("presharp", 0, split_i420(enc.debug_presharp(0), 64, 32, c), pre)
            _check(got, jp, f"{n} frames")


# ------------------------------------------------------------------------- 5. segments
def test_segments_are_sequences_of_their_own():
    """mjg_submit_segments of 4 + 1 + 6 frames of 32x32 4:2:0, scale=16:16,tile=2x2: 1 + 1 + 2 sheets, equal byte for byte
    to three single submits, each segment from byte 1 of its own allocation."""
    import torch
    w, h, c, sheet, split = 32, 32, "420", (2, 2, 0, 0, 0), (4, 1, 6)
    frames = _frames(w, h, c, 11)
    sar = profile.scaled_sar((1, 1), (w, h), (16, 16))
    cells = _cells(frames, w, h, c, dw=16, dh=16)
    segs, at, want_sheets, want = [], 0, [], []
    for n in split:
        t = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device="cuda:0")
        t[1:] = torch.from_numpy(frames[at:at + n].reshape(-1).copy()).to("cuda:0")
        segs.append((t, n))
        sh, jp = _ref(("t5", at, n), cells[at:at + n], 16, 16, c, sheet, sar=sar)
        want_sheets += sh
        want += jp
        at += n
    torch.cuda.synchronize()
    assert len(want) == 4
    with MjpegEncoder(0, w, h, 16, 16, qscale=5, sar=sar, max_batch=11, chroma=c, sheet=sheet) as enc:
        assert [enc.frames_out(n) for n in range(1, 10)] == [1, 1, 1, 1, 2, 2, 2, 2, 3]
        enc.submit_segments([(t.data_ptr() + 1, n) for t, n in segs])
        assert len(enc.sync()) == 4
        got = enc.fetch()
        _check_stages(enc, cells, want_sheets, c)
        single = []
        for t, n in segs:
            enc.submit(device_ptr=t.data_ptr() + 1, nframes=n)
            single += enc.fetch()
    _check(got, want, "segments")
    _check(single, want, "single submits")


# ------------------------------------------------------------------------- 6. behind a deinterlacer, the whole chain
def test_behind_a_deinterlacer_in_one_submit_and_as_a_halo_submit():
    """yadif,scale=32:16,tile=2x1 on 64x32 4:2:0: 5 frames in one submit (3 sheets), then frames 1..4 of 6 as a halo submit:
    the sheets hold the frames deinterlaced with their neighbours, two sheets of two."""
    w, h, c, sheet = 64, 32, "420", (2, 1, 0, 0, 0)
    frames = _frames(w, h, c, 6)
    sar = profile.scaled_sar((1, 1), (w, h), (32, 16))
    with MjpegEncoder(0, w, h, 32, 16, qscale=5, sar=sar, max_batch=5, chroma=c, deint=_lib.MJG_DEINT_YADIF, sheet=sheet) as enc:
        d = deint_frames(frames[:5], w, h, c, 0, 1)
        cells = _cells(d, w, h, c, dw=32, dh=16)
        sheets, jp = _ref("t6a", cells, 32, 16, c, sheet, sar=sar)
        enc.submit(frames[:5])
        got = enc.fetch()
        assert len(got) == 3
        _check_stages(enc, cells, sheets, c)
        _check(got, jp, "one submit")
        d = deint_frames(frames, w, h, c, 0, 1)[1:5]
        cells = _cells(d, w, h, c, dw=32, dh=16)
        sheets, jp = _ref("t6b", cells, 32, 16, c, sheet, sar=sar)
        enc.submit(frames, 4, halo=3)
        got = enc.fetch()
        assert len(got) == 2
        _check_stages(enc, cells, sheets, c)
        _check(got, jp, "halo submit")


def test_behind_the_whole_chain():
    """An orientation with a transpose, a colour matrix, a crop, the scale, a table behind it, the sharpen, tile=2x2, on
    130x66 4:2:0: three frames on one 64x96 sheet."""
    w, h, c, sheet, orient = 130, 66, "420", (2, 2, 0, 0, 0), 3
    cm = colormatrix_ref.coefs("bt709", "bt601")
    tabs = eq_ref.tables(dict(contrast=1.2))
    rect, dw, dh = (2, 4, 60, 120), 32, 48
    frames = _frames(w, h, c, 3)
    ow, oh = oriented_size(w, h, orient)
    sar = profile.scaled_sar((1, 1), rect[2:], (dw, dh))
    cells = []
    for f in frames:
        o = colormatrix_ref.convert_frames(orient_frame(f, w, h, c, orient), ow, oh, c, cm)
        pl = composed_planes(crop_frame(o, ow, oh, c, rect), rect[2], rect[3], c, c, False, dw, dh)
        cells.append(unsharp_planes(*[tabs[p][pl[p]] for p in range(3)], DEFAULT))
    sheets, jp = _ref("t6c", cells, dw, dh, c, sheet, sar=sar)
    with MjpegEncoder(0, w, h, dw, dh, qscale=5, sar=sar, max_batch=3, chroma=c, orient=orient, cmat=cm, crop=rect,
                      lut_out=tabs, unsharp=DEFAULT, sheet=sheet) as enc:
        got = enc.encode(frames)
        _check_stages(enc, cells, sheets, c)
    _check(got, jp)


# ------------------------------------------------------------------------- 7. the trivial sheet
def test_the_trivial_sheet_is_no_sheet():
    w, h, c = 130, 66, "420"
    frames = _frames(w, h, c, 3)
    out = []
    for sheet in (None, (1, 1, 0, 0, 0), (1, 1, 1, 0, 7)):
        with MjpegEncoder(0, w, h, 64, 32, qscale=5, max_batch=3, chroma=c, sheet=sheet) as enc:
            assert enc.debug_sheet() is None and (enc.enc_w, enc.enc_h) == (64, 32) and enc.frames_out(3) == 3
            out.append(enc.encode(frames))
            with pytest.raises(_lib.MjgError) as e:
                enc.debug_cell(0)
            assert e.value.code == _lib.MJG_E_STATE
    _check(out[1], out[0])
    _check(out[2], out[0])
    with MjpegEncoder(0, w, h, qscale=5, max_batch=3, chroma=c, sheet=(1, 1, 0, 0, 0)) as enc:      # and no sws stage either
        assert enc.encode_path() & 1 and enc.scale_path(0) == 0


def test_the_tile_runs_inside_the_scale_interval():
    with MjpegEncoder(0, 33, 17, full_range=True, qscale=5, max_batch=4, chroma="444", timing=True, sheet=(2, 2, 0, 3, 5)) as enc:
        enc.encode(_frames(33, 17, "444", 5)[:4])
        ms, n = enc.kernel_times()
    assert n == 1 and ms["scale"] > 0


# ------------------------------------------------------------------------- 8. the worker
def _y4m420(frames, w, h, fps="25:1"):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F{fps} Ip A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def test_worker_framestep_scale_tile_end_to_end(monkeypatch):
    """A 23-frame 64x48 y4m at 25 fps, -vf framestep=2,scale=32:24,tile=3x2, MJG_WORKER_BATCH=6: 12 kept frames in two
    submits give two 96x48 JPEGs in a Matroska at 25 / 12 fps: default duration 480 ms, frame times 0 and 480 ms."""
    w, h, c = 64, 48, "420"
    frames = _frames(w, h, c, 23)
    monkeypatch.setenv("MJG_WORKER_BATCH", "6")
    args = ["-vf", "framestep=2,scale=32:24,tile=3x2"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, w, h)), stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue(), err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    pk, info = list(r.frames(1)), r.info(1)
    assert (info.width, info.height, info.codec) == (96, 48, "V_MJPEG")
    assert r.tracks[0].default_duration == 480_000_000
    assert [t for t, _ in pk] == [0, 480]
    kept = frames[::2]
    assert len(kept) == 12
    sar = profile.scaled_sar((1, 1), (w, h), (32, 24))
    cells = _cells(kept, w, h, c, dw=32, dh=24)
    sheets, jp = _ref("t8", cells, 32, 24, c, (3, 2, 0, 0, 0), qscale=profile.effective_qscale(5), sar=sar)
    _check([d for _, d in pk], jp, "worker")
    last = [l for l in err.getvalue().splitlines() if l.startswith("frame=")][-1]
    assert last.startswith("frame=    2 ") and "time=00:00:00.96" in last, last
