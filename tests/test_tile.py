"""`-vf tile` / `-vf framestep` without a GPU: the parser (profile._take_sheet, SheetProfile), the plan
(worker.SheetPlan, tile_fallthrough_reason, sheet_batch), mjg_open_sheet's refusals (all in front of the
first HIP call), the two forms of tests/tile_ref.py, Source.skip and the muxer at fps / N.  The kernel
itself: tests/test_gpu_tile.py and tools/tile_host_check.py."""
import ctypes as C
import dataclasses
import io
from fractions import Fraction

import numpy as np
import pytest

import open_chain_calls as oc
import tile_ref
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.container import StreamInfo
from ffmpeg_distributed_amd.encoder import split_i420

TAIL = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact"


def _parse(vf, *extra):
    return profile.try_parse(["-vf", vf] + TAIL.split() + list(extra))


def _tile(cols, rows, nb=0, margin=0, padding=0):
    return {"cols": cols, "rows": rows, "nb_frames": nb, "margin": margin, "padding": padding}


# ------------------------------------------------------------------------------------ the parser
ACCEPTED = [
    ("tile", _tile(6, 5), 1, None),
    ("scale=160:90,tile=6x5", _tile(6, 5), 1, (160, 90)),
    ("scale=160:90,tile=layout=3x2", _tile(3, 2), 1, (160, 90)),
    ("tile=3x2:5", _tile(3, 2, 5), 1, None),
    ("tile=3x2:nb_frames=5", _tile(3, 2, 5), 1, None),
    ("tile=2x2:0:4:6", _tile(2, 2, 0, 4, 6), 1, None),
    ("tile=2x2:margin=4:padding=6", _tile(2, 2, 0, 4, 6), 1, None),
    ("tile=2x2:padding=6:margin=4:layout=4x3", _tile(4, 3, 0, 4, 6), 1, None),
    ("tile=2x2:color=black", _tile(2, 2), 1, None),
    ("tile=2x2:0:0:0:black:0:0", _tile(2, 2), 1, None),
    ("framestep=step=3", None, 3, None),
    ("framestep=3,scale=8:8", None, 3, (8, 8)),
    ("framestep=25,scale=160:90,tile=6x5", _tile(6, 5), 25, (160, 90)),
    ("framestep=1,scale=8:8,tile", _tile(6, 5), 1, (8, 8)),
    ("crop=64:32,scale=32:16,unsharp,tile=3x2", _tile(3, 2), 1, (32, 16)),
    ("yadif,transpose=1,colormatrix=bt709:bt601,eq=1.2,scale=32:16,tile=2x1", _tile(2, 1), 1, (32, 16)),
]


@pytest.mark.parametrize("vf,tile,step,scale", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_accepted_graphs(vf, tile, step, scale):
    p, why = _parse(vf)
    assert why is None and type(p) is profile.SheetProfile
    assert (p.tile, p.framestep, p.scale) == (tile, step, scale)


REJECTED = [
    ("tile=2x2:color=red", "tile color 'red'"),
    ("tile=2x2:0:0:0:white", "tile color 'white'"),
    ("tile=2x2:overlap=1", "tile overlap 1"),
    ("tile=2x2:init_padding=2", "tile init_padding 2"),
    ("tile=2x2,scale=8:8", "tile is not the last filter"),
    ("scale=8:8,tile,tile", "a second tile"),
    ("scale=8:8,pad=16:16,tile", "tile in a graph with pad"),
    ("scale=8:8,framestep=2", "framestep after scale"),
    ("framestep=2,framestep=3,scale=8:8", "a second framestep"),
    ("framestep=2,yadif,scale=8:8", "framestep together with yadif"),
    ("framestep=n/2", "framestep 'n/2': not a decimal integer (expressions"),
    ("tile=2x2:margin=iw/8", "tile margin 'iw/8': not a decimal integer of 0 or more (expressions"),
    ("tile=ax2", "tile layout 'ax2'"),
    ("tile=2x2:nb_frames=5", "tile nb_frames 5: FFmpeg rejects"),
    ("tile=0x2", "tile layout 0x2: FFmpeg rejects"),
    ("tile=2x2:padding=-2", "tile padding '-2'"),
    ("framestep=0", "framestep 0: FFmpeg rejects"),
    ("tile=2x2:frames=3", "tile option 'frames'"),
]


@pytest.mark.parametrize("vf,text", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_graphs_name_their_reason(vf, text):
    p, why = _parse(vf)
    assert p is None and text in why, why


@pytest.mark.parametrize("vf", [None, "scale=8:8", "framestep=1,scale=8:8", "framestep=1", "crop=64:32,scale=32:16,unsharp,pad=40:24",
                                "yadif,scale=8:8"])
def test_a_graph_without_the_two_filters_is_a_plain_profile(vf):
    p = profile.parse((["-vf", vf] if vf else []) + TAIL.split())
    assert type(p) is profile.Profile
    assert "tile" not in dataclasses.asdict(p) and "framestep" not in dataclasses.asdict(p)
    if vf and vf.startswith("framestep=1,"):
        assert p == profile.parse(["-vf", vf.split(",", 1)[1]] + TAIL.split())


def test_parse_graph_adds_its_keys_only_when_set():
    assert profile.parse_graph("scale=8:8") == {"scale": (8, 8), "sws_flags": ("bicubic",)}
    assert set(profile.parse_graph("framestep=2,scale=8:8")) == {"scale", "sws_flags", "framestep"}
    assert set(profile.parse_graph("framestep=1,scale=8:8,tile")) == {"scale", "sws_flags", "tile"}
    assert profile.GRAPH_STAGES[0] is profile._take_sheet


def test_of_two_vf_options_the_last_wins_both_ways():
    p = profile.parse(["-vf", "scale=8:8,tile=2x2", "-vf", "scale=16:16"] + TAIL.split())
    assert type(p) is profile.Profile and p.scale == (16, 16)
    p = profile.parse(["-vf", "scale=16:16", "-vf", "framestep=2,scale=8:8,tile=2x2"] + TAIL.split())
    assert type(p) is profile.SheetProfile and (p.scale, p.framestep, p.tile) == ((8, 8), 2, _tile(2, 2))
    _, why = profile.try_parse(["-vf", "tile=2x2:color=red", "-vf", "scale=16:16"] + TAIL.split())
    assert "tile color 'red'" in why      # an earlier graph outside the profile still refuses the arguments


# ------------------------------------------------------------------------------------ the plan
def _plan(vf, info=None, *extra):
    return worker.plan_segment(profile.parse(["-vf", vf] + TAIL.split() + list(extra)), info or StreamInfo(130, 66, sar=(1, 1), chroma="420"))


def test_the_sheet_size_with_margin_and_padding():
    plan = _plan("scale=64:32,tile=3x2:margin=4:padding=6")
    assert type(plan) is worker.SheetPlan
    assert (plan.dst_w, plan.dst_h, plan.enc_w, plan.enc_h) == (64, 32, 3 * 64 + 2 * 6 + 8, 2 * 32 + 6 + 8)
    assert plan.sheet == (3, 2, 6, 4, 6) and plan.framestep == 1 and plan.pad is None
    assert plan.sar == profile.scaled_sar((1, 1), (130, 66), (64, 32))      # the cell's
    assert plan.encoder_kwargs()["sheet"] == (3, 2, 6, 4, 6)
    assert type(_plan("scale=64:32")) is worker.SegmentPlan and "sheet" not in _plan("scale=64:32").encoder_kwargs()


def test_out_fps():
    info = StreamInfo(130, 66, Fraction(30000, 1001), chroma="420")
    assert _plan("framestep=2,scale=64:32,tile=3x2", info).out_fps == Fraction(30000, 1001) / 12
    assert _plan("framestep=2,scale=64:32,tile=3x2:nb_frames=5", info).out_fps == Fraction(30000, 1001) / 10
    plan = _plan("framestep=2,scale=64:32", info)
    assert type(plan) is worker.SheetPlan and plan.sheet is None and plan.out_fps == Fraction(15000, 1001)
    assert (plan.enc_w, plan.enc_h) == (64, 32) and plan.encoder_kwargs()["sheet"] is None


def test_the_batch_rule():
    assert [worker.sheet_batch(10, n) for n in (4, 6, 30)] == [8, 6, 30]
    opts = worker.Options.from_env({"MJG_WORKER_BATCH": "3"})
    assert worker.batch_frames(opts, 1 << 20) == 3 and worker.sheet_batch(3, 4) == 4 and worker.sheet_batch(3, 1) == 3


FALLTHROUGH = [
    ("tile=2x2", StreamInfo(130, 66, chroma="444"), ("-pix_fmt", "yuvj420p"), "tile before the 444 -> 420 -pix_fmt conversion"),
    ("tile=2x2", StreamInfo(131, 66, chroma="420"), (), "tile of 131x66 cells in 420: the size is no multiple"),
    ("scale=64:33,tile=2x2", None, (), "tile of 64x33 cells in 420"),
    ("scale=64:32,tile=2x2:margin=3", None, (), "tile margin 3 / padding 0 in 420: no multiple"),
    ("scale=64:32,tile=2x2:padding=5", None, (), "tile margin 0 / padding 5 in 420: no multiple"),
    ("scale=4096:32,tile=5x1", None, (), "a 20480x32 sheet, a side beyond 16384"),
    ("scale=16:16,tile=6x6", None, (), "tile of 36 frames a sheet: more than the 32 frames a submit holds"),
]


@pytest.mark.parametrize("vf,info,extra,text", FALLTHROUGH, ids=[f[3][:40] for f in FALLTHROUGH])
def test_each_fallthrough_reason(vf, info, extra, text):
    with pytest.raises(worker.Fallthrough) as e:
        _plan(vf, info, *extra)
    assert text in str(e.value)


def test_accepted_at_the_limits():
    assert _plan("scale=16:16,tile=6x6:nb_frames=32").sheet == (6, 6, 32, 0, 0)
    assert _plan("tile=2x2:margin=3:padding=5", StreamInfo(33, 17, chroma="444", full_range=True)).enc_w == 77
    assert _plan("scale=64:32,tile=2x2", StreamInfo(130, 66, chroma="444"), "-pix_fmt", "yuvj420p").dst_chroma == "420"


def test_the_key_changes_in_exactly_one_element_with_the_sheet():
    info = StreamInfo(130, 66, chroma="420")
    pa, pb, p0 = (profile.parse(["-vf", vf] + TAIL.split()) for vf in
                  ("scale=64:32,tile=3x2", "scale=64:32,tile=3x2:nb_frames=5", "scale=64:32"))
    ka, kb, k0 = (worker.plan_segment(p, info).key(p, info, False, 6) for p in (pa, pb, p0))
    assert len(ka) == len(kb) == len(k0) + 1 and ka[:-1] == k0 and kb[:-1] == k0
    assert ka[-1] == ("sheet", (3, 2, 6, 0, 0)) and kb[-1] == ("sheet", (3, 2, 5, 0, 0))
    assert [a != b for a, b in zip(ka, kb)].count(True) == 1


# ------------------------------------------------------------------------------------ mjg_open_sheet, no GPU
DEVICE = 7      # no refusal gets as far as the device


def _open_sheet(sheet, device=DEVICE, cfg=None, **fields):
    L = _lib.load()
    cfg, ch, hnd = cfg or oc.config(), oc.make_chain(**fields), C.c_void_p()
    sh = None if sheet is None else C.byref(_lib.MjgSheet(*sheet))
    rc = L.mjg_open_sheet(device, C.byref(cfg), C.byref(ch), sh, C.byref(hnd))
    msg = L.mjg_last_error().decode()
    oc.close(hnd.value)
    return rc, msg, hnd.value


NO_PAD = {k: v for k, v in oc.BASE.items() if k != "pad"}      # 24x40 cells, 4:2:0
SHEET_REFUSALS = [
    ((0, 2, 0, 0, 0), "sheet 0x2: cols or rows below 1"),
    ((2, -1, 0, 0, 0), "sheet 2x-1: cols or rows below 1"),
    ((2, 2, -1, 0, 0), "sheet 2x2: nb_frames -1 not in 0..4"),
    ((2, 2, 5, 0, 0), "sheet 2x2: nb_frames 5 not in 0..4"),
    ((2, 2, 0, -2, 0), "sheet 2x2: margin -2 or padding 0 is negative"),
    ((2, 2, 0, 0, -4), "sheet 2x2: margin 0 or padding -4 is negative"),
    ((683, 1, 0, 0, 0), "sheet 683x1 of 24x40 cells, margin 0, padding 0: 16392x40, a side is beyond 16384"),
    ((1, 2, 0, 8180, 0), "sheet 1x2 of 24x40 cells, margin 8180, padding 0: 16384x16440, a side is beyond 16384"),
    ((2, 2, 0, 3, 0), "sheet 2x2 of 24x40 cells, margin 3, padding 0: not multiples of the encoded format's chroma sub-sampling (2x2)"),
    ((2, 2, 0, 0, 5), "sheet 2x2 of 24x40 cells, margin 0, padding 5: not multiples"),
]


@pytest.mark.parametrize("sheet,message", SHEET_REFUSALS, ids=[m[:36] for _, m in SHEET_REFUSALS])
def test_open_sheet_refuses_before_any_hip_call(sheet, message):
    rc, msg, hnd = _open_sheet(sheet, **NO_PAD)
    assert rc == _lib.MJG_E_INVALID and msg.startswith(message) and not hnd, (rc, msg)


def test_open_sheet_refuses_a_pad_and_an_odd_cell():
    rc, msg, _ = _open_sheet((2, 2, 0, 0, 0), **oc.BASE)
    assert rc == _lib.MJG_E_INVALID and msg.startswith("sheet 2x2 behind a pad"), msg
    rc, msg, _ = _open_sheet((2, 2, 0, 0, 0), cfg=oc.config((24, 41)), **NO_PAD)
    assert rc == _lib.MJG_E_INVALID and msg.startswith("sheet 2x2 of 24x41 cells"), msg
    # (a pad that is the trivial rectangle is no pad)
    rc, msg, _ = _open_sheet((2, 2, 0, 0, 0), device=0, **dict(NO_PAD, pad=(0, 0, 24, 40)))
    assert rc in (_lib.MJG_OK, _lib.MJG_E_HIP), (rc, msg)


@pytest.mark.parametrize("sheet", [None, (1, 1, 0, 0, 0), (1, 1, 1, 0, 6)], ids=["null", "1x1", "1x1_nb1_padding"])
def test_the_null_and_the_trivial_sheet_take_open_chains_path(sheet):
    for change in (dict(orient=9), dict(crop=(2, 4, 64, 60)), dict(pad=(4, 2, 16, 48)), dict(deint=8)):
        fields = dict(oc.BASE, **change)
        rc, msg, _ = _open_sheet(sheet, **fields)
        rc0, msg0, hnd = oc.open_chain(DEVICE, **fields)
        oc.close(hnd)
        assert (rc, msg) == (rc0, msg0) and rc == _lib.MJG_E_INVALID, (change, msg, msg0)
    rc, msg, _ = _open_sheet(sheet, device=0, **oc.BASE)      # a good chain, with its pad: past validation
    assert rc in (_lib.MJG_OK, _lib.MJG_E_HIP), (rc, msg)


def test_a_good_sheet_gets_past_validation_and_null_arguments_do_not():
    rc, msg, _ = _open_sheet((3, 2, 5, 2, 4), device=0, **NO_PAD)
    assert rc in (_lib.MJG_OK, _lib.MJG_E_HIP), (rc, msg)
    L = _lib.load()
    assert L.mjg_open_sheet(0, None, None, None, None) == _lib.MJG_E_INVALID
    assert L.mjg_frames_out(None, 5) == 0 and L.mjg_version() == 105


def test_the_exports_and_the_encoder_without_the_symbol(monkeypatch):
    for name in ("mjg_open_sheet", "mjg_frames_out", "mjg_debug_sheet", "mjg_debug_cell"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert [f[0] for f in _lib.MjgSheet._fields_] == ["cols", "rows", "nb_frames", "margin", "padding"]
    from ffmpeg_distributed_amd.encoder import MjpegEncoder

    class Old:
        def mjg_open_chain(self, *a):
            raise AssertionError("not reached")

    monkeypatch.setattr(_lib, "load", lambda: Old())
    with pytest.raises(_lib.MjgError, match="library lacks mjg_open_sheet") as e:
        MjpegEncoder(0, 70, 38, 32, 16, sheet=(2, 2, 0, 0, 0))
    assert e.value.code == _lib.MJG_E_STATE
    with pytest.raises(ValueError):
        MjpegEncoder(0, 70, 38, sheet=(2, 2))


# ------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("w,h,c,sheet,n", [(8, 8, "420", (5, 3, 0, 0, 0), 17), (33, 17, "444", (2, 2, 0, 3, 5), 5),
                                           (16, 6, "422", (3, 2, 4, 2, 4), 9), (4, 4, "420", (1, 3, 0, 0, 2), 2)])
def test_the_two_forms_of_the_reference_agree(w, h, c, sheet, n):
    rng = np.random.default_rng(w + h + n)
    from ffmpeg_distributed_amd.encoder import i420_frame_bytes
    cells = [split_i420(rng.integers(1, 255, i420_frame_bytes(w, h, c), dtype=np.uint8), w, h, c) for _ in range(n)]
    a, b = tile_ref.sheets_loop(cells, w, h, c, sheet), tile_ref.sheets_numpy(cells, w, h, c, sheet)
    assert len(a) == len(b) == tile_ref.frames_out(n, sheet)
    W, H = tile_ref.sheet_size(w, h, sheet)
    for s, t in zip(a, b):
        assert s[0].shape == (H, W)
        for p, q in zip(s, t):
            assert (p == q).all()
    N = tile_ref.resolve(sheet)[2]
    last, held = b[-1], n - (len(b) - 1) * N
    if held < sheet[0] * sheet[1]:      # the first blank cell of the last sheet is black
        x0, y0 = sheet[3] + (w + sheet[4]) * (held % sheet[0]), sheet[3] + (h + sheet[4]) * (held // sheet[0])
        assert (last[0][y0:y0 + h, x0:x0 + w] == 0).all()
    assert (b[0][0][sheet[3]:sheet[3] + h, sheet[3]:sheet[3] + w] == cells[0][0]).all()


# ------------------------------------------------------------------------------------ Source.skip
def _kept(src, step, fb):
    out, buf = [], np.zeros(fb, np.uint8)
    while src.read_into(buf, 1) == 1:
        out.append(buf.copy())
        src.skip(step - 1)
    return out


@pytest.mark.parametrize("step", [2, 3, 7])
def test_source_skip_on_a_y4m_pipe_and_on_a_regular_file_matroska(step, tmp_path):
    w, h, n = 16, 8, 11
    frames = [np.random.default_rng(i).integers(0, 256, w * h * 3 // 2, dtype=np.uint8) for i in range(n)]
    y4m = f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg\n".encode() + b"".join(b"FRAME\n" + f.tobytes() for f in frames)
    src = worker.Source(io.BytesIO(y4m))
    got = _kept(src, step, src.info.frame_bytes)
    assert len(got) == len(frames[::step]) and all((a == b).all() for a, b in zip(got, frames[::step]))
    assert src.skip(3) == 0 and src.skip(0) == 0
    path = tmp_path / "seg.mkv"
    with open(path, "wb") as f:
        wr = container.MkvWriter(f, w, h, Fraction(3), codec="V_UNCOMPRESSED", colour_space=b"I420")      # several clusters
        for fr in frames:
            wr.write_frame(fr.tobytes())
        wr.close()
    for as_file in (True, False):
        raw = open(path, "rb") if as_file else io.BytesIO(path.read_bytes())
        src = worker.Source(raw)
        assert (getattr(src, "_fd", None) is not None) == as_file
        got = _kept(src, step, src.info.frame_bytes)
        assert len(got) == len(frames[::step]) and all((a == b).all() for a, b in zip(got, frames[::step])), as_file
        src.close()
        raw.close()


def test_skip_on_a_regular_file_issues_no_read(tmp_path):
    w, h = 16, 8
    frames = [np.full(w * h * 3 // 2, i, np.uint8) for i in range(6)]
    path = tmp_path / "seg.mkv"
    with open(path, "wb") as f:
        wr = container.MkvWriter(f, w, h, Fraction(25), codec="V_UNCOMPRESSED", colour_space=b"I420")
        for fr in frames:
            wr.write_frame(fr.tobytes())
        wr.close()
    with open(path, "rb") as raw:
        src = worker.Source(raw)
        calls = []
        src._pool = type("P", (), {"submit": lambda self, *a: calls.append(a), "shutdown": lambda self, wait=True: None})()
        assert src.skip(4) == 4 and calls == []
        buf = np.zeros(w * h * 3 // 2, np.uint8)
        assert src.skip(5) == 2      # frames 4 and 5 were left
        src.close()


# ------------------------------------------------------------------------------------ the muxer
def test_mkv_writer_at_fps_over_n():
    buf = io.BytesIO()
    wr = container.MkvWriter(buf, 96, 48, Fraction(25) / 12, (1, 1))
    for i in range(3):
        wr.write_frame(bytes([0xFF, 0xD8, i, 0xFF, 0xD9]))
    wr.close()
    r = container.MkvReader(io.BytesIO(buf.getvalue()))
    assert [t for t, _ in r.frames(1)] == [0, 480, 960]
    assert r.tracks[0].default_duration == 480_000_000
    buf = io.BytesIO()
    wr = container.MkvWriter(buf, 96, 48, Fraction(30000, 1001) / 12, (1, 1))
    for i in range(3):
        wr.write_frame(bytes([0xFF, 0xD8, i, 0xFF, 0xD9]))
    wr.close()
    r = container.MkvReader(io.BytesIO(buf.getvalue()))
    assert [t for t, _ in r.frames(1)] == [0, 400, 801] and r.tracks[0].default_duration == 400_400_000
