"""k_unsharp_plane past one tile row and column, k_yadif_plane in front of every reader of d_deint,
and both in a seeded sweep of the chain: byte for byte against tests/unsharp_ref.py and
tests/yadif_ref.py followed by the composed crop / scale / pad oracle.  tests/test_gpu_unsharp.py
and tests/test_gpu_yadif.py run toy planes (at most two tile columns, the picture's left edge on a
quad boundary, every tile of a padded canvas touching the picture; two readers of d_deint, one
split into segments); the shapes here are the smallest that reach the rest.  Every case asserts
with tests/chain_geom.py, *before* it opens a context, that its shape reaches what it names
(sharp_cells, deint_span, predict_paths), and on the context that the kernels it means ran
(scale_path / encode_path).  A sharpen case compares debug_presharp(), debug_planes() and then the
JPEGs; a deinterlacer case debug_deint(), debug_planes() where a sws stage runs, then the JPEGs; a
difference names the stage and the first differing sample.  tools/unsharp_host_check.py and
tools/yadif_host_check.py walk the launches of these geometries and splits on the CPU first."""
import io

import numpy as np
import pytest

import chain_geom as cg
import test_gpu_chain as chain
import test_gpu_unsharp as gu
import test_gpu_yadif as gy
from chain_geom import COPY, IN_PLACE, NONE, PADCOPY, STREAM, TILE, UA
from chroma_resample_ref import source_frames
from orient_ref import oriented_planes
from test_gpu_orient import _check_oriented
from unsharp_ref import (DEFAULT, GPU_GEOMETRY_CHAIN, US_13, US_23, US_422, US_55, US_73, US_LUMA0, WIDE, sharp_planes,
                         sharp_ref)
from yadif_ref import deint_frames, deint_planes
from ffmpeg_distributed_amd import container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes

pytestmark = pytest.mark.gpu

_check = gu._check


# ================================================================= 1. the sharpen past one tile row and column
def _cells(W, H, c, px, py, w, h, us):
    """sharp_cells of the luma and of a chroma plane of an encoded W x H frame; the geometry must be
    one that tools/unsharp_host_check.py walks."""
    assert (W, H, c, px, py, w, h, us) in GPU_GEOMETRY_CHAIN
    return tuple(cg.sharp_cells(*g) for g in cg.sharp_plane_geoms(W, H, c, px, py, w, h, us))


def _sharp_run(w, h, c, us, paths, full=False, dw=None, dh=None, dst=None, pad=None, q=5, **enc_kw):
    """One encoder on the three frames of test_gpu_unsharp._frames(w, h, c): the paths, then the sws
    stage's output, the sharpened planes and the JPEGs against the reference."""
    frames = gu._frames(w, h, c)
    sar = profile.scaled_sar((1, 1), (w, h), (dw or w, dh or h))
    pre, post, jp = gu._ref((w, h, c, None), frames, w, h, c, us, orient=0, rect=None, dst=dst or c, full=full, dw=dw,
                            dh=dh, pad=pad, qscale=q, sar=sar, **enc_kw)
    with MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, sar=sar, max_batch=gu.NF, chroma=dst or c,
                      src_chroma=c, pad=pad, unsharp=us, **enc_kw) as enc:
        assert (enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))) == (0, paths)
        got = enc.encode(frames)
        gu._check_stage(enc, "presharp (the sws stage's output)", enc.debug_presharp, pre, dst or c)
        gu._check_stage(enc, "planes (k_unsharp_plane's output)", enc.debug_planes, post, dst or c)
    _check(got, jp)


def _wide_cells(us):
    """197 x 70 4:4:4: four tile columns by three tile rows, every tile filtering, the last column
    5 wide (one short quad a row)."""
    luma, chroma = _cells(*WIDE, "444", 0, 0, *WIDE, us)
    for cells in (luma, chroma):
        assert (cells.tx, cells.ty, cells.short) == (4, 3, 70)
    return luma, chroma


@pytest.mark.parametrize("us", [US_23, US_13, US_55], ids=["23x3_3x23", "13x13_9x15", "5x5_all_planes"])
def test_sharpen_across_three_tile_seams_each_way(us):
    """197 x 70 4:4:4 full range without a scale (k_plane_copy in front).  23:3 / 3:23: aprons of 11
    across three column seams (luma) and two row seams (chroma), sx + sy = 12, and the staging
    loop's third iteration (86 x 34 and 66 x 54 staged bytes are 748 and 918 quads).  13:13 / 9:15
    at -1.0: the 32-bit limit on tiles with neighbours, a blur on the chroma.  5:5 on all three
    planes: the unrolled <5, 5> for luma and for the paired U + V launch of 2 x 3 x 12 tiles."""
    luma, chroma = _wide_cells(us)
    assert (luma.filt, luma.copy, chroma.filt, chroma.copy) == (12, 0, 12, 0)
    assert luma.masks == chroma.masks == {1: 70, 15: 3430}
    if us == US_23:
        assert (us[0] // 2, us[4] // 2) == (11, 11) and us[0] // 2 + us[1] // 2 == 12
    _sharp_run(*WIDE, "444", us, (COPY, COPY), full=True)


def test_sharpen_behind_the_tile_scale_kernel():
    """The same plane out of a 260 x 100 4:4:4 tv source through k_scale (under 4:1 both ways)."""
    _wide_cells(US_23)
    assert cg.scale_variant(260, 100, *WIDE)[0] == "tile"
    _sharp_run(260, 100, "444", US_23, (TILE, TILE), dw=WIDE[0], dh=WIDE[1])


STREAM_SRC = (208, 562)      # the smallest source (by area) whose 197 x 70 tile needs more than 64 KiB of LDS


def test_sharpen_behind_the_stream_kernel():
    """The same plane out of k_scale_stream: 208 x 562 -> 197 x 70, 8:1 down the columns."""
    _wide_cells(US_13)
    assert cg.scale_variant(*STREAM_SRC, *WIDE)[0] == "stream" and cg.tile_lds(*STREAM_SRC, *WIDE) > 64 * 1024
    assert cg.tile_lds(STREAM_SRC[0], STREAM_SRC[1] - 1, *WIDE) <= 64 * 1024      # one row less stays on the tile kernel
    _sharp_run(*STREAM_SRC, "444", US_13, (STREAM, STREAM), dw=WIDE[0], dh=WIDE[1])


def test_padded_picture_cuts_quads_on_both_sides_among_copying_tiles():
    """4:4:4, the pad copy in front.  201 x 99 with a 70 x 34 picture at (67, 33), 5:5 everywhere:
    the picture starts at the last sample of a quad (pic 8) and ends after the first of another
    (pic 1); 203 x 101 with 66 x 33 at (69, 35), 7:3 / 3:7: pic 14 and 7.  Either way four
    filtering tiles in the middle of twelve that only copy, and every clamp of the filter at a
    picture edge that is not the plane's."""
    for (W, H, px, py, w, h, us, masks) in ((201, 99, 67, 33, 70, 34, US_55, {0: 1402, 1: 34, 8: 34, 15: 578}),
                                            (203, 101, 69, 35, 66, 33, US_73, {0: 1487, 7: 33, 14: 33, 15: 495})):
        for cells in _cells(W, H, "444", px, py, w, h, us):
            assert (cells.tx, cells.ty, cells.filt, cells.copy) == (4, 4, 4, 12) and cells.masks == masks
        assert px > us[0] // 2 and py > us[1] // 2 and px + w + us[0] // 2 < W and py + h + us[1] // 2 < H
        _sharp_run(w, h, "444", us, (PADCOPY, PADCOPY), full=True, pad=(px, py, W, H))


PAD420 = dict(w=260, h=132, dw=130, dh=66, pad=(70, 38, 264, 136))


def _pad420_cells():
    luma, chroma = _cells(264, 136, "420", 70, 38, 130, 66, US_55)
    assert (luma.tx, luma.ty, luma.filt, luma.copy) == (5, 5, 9, 16) and luma.masks == {0: 2430, 12: 66, 15: 2112}
    assert (chroma.tx, chroma.ty, chroma.filt, chroma.copy) == (3, 3, 4, 5) and chroma.masks == {0: 1487, 8: 33, 15: 528}


@pytest.mark.parametrize("kw", [dict(), dict(huffman="optimal"), dict(rst=True)], ids=["default", "optimal", "rst"])
def test_padded_420_picture_at_an_odd_chroma_offset(kw):
    """4:2:0, 260 x 132 scaled to 130 x 66 at (70, 38) of a 264 x 136 canvas, 5:5 everywhere: luma
    pic 12, the chroma picture at (35, 19) with pic 8, copying tiles in both launches.  Then
    k_encode's other forms on d_sharp: -huffman optimal (15 chunks a frame: work units start at
    chunks 12, 9 and 6) and RST (two chunks an MCU row and an even kBatch: every unit starts at
    chunk 0, but in restart segments 6, 3 and 6 of their frames)."""
    _pad420_cells()
    if kw.get("rst"):
        assert cg.mid_segment_units(264, 136, "420", True, gu.NF) == []
        assert [u[:2] for u in cg.unit_starts(264, 136, "420", True, gu.NF)] == [(0, 0), (0, 6), (1, 3), (2, 0), (2, 6)]
    else:
        assert [u[2] for u in cg.mid_segment_units(264, 136, "420", False, gu.NF)] == [12, 9, 6]
    p = PAD420
    _sharp_run(p["w"], p["h"], "420", US_55, (TILE, TILE), dw=p["dw"], dh=p["dh"], pad=p["pad"], **kw)


@pytest.mark.parametrize("src", ["422", "444"], ids=["from_422", "pix_fmt_from_444_with_a_scale"])
def test_sharpen_422(src):
    """A 134 x 70 4:2:2 frame, 7:5 luma and <5, 5> on the 67 x 70 chroma planes (pic 7 at their
    edge): from a 4:2:2 source of that size through the plane copy, and as -pix_fmt from 268 x 140
    4:4:4 through the tile kernel."""
    luma, chroma = _cells(134, 70, "422", 0, 0, 134, 70, US_422)
    assert (luma.tx, luma.ty, luma.masks) == (3, 3, {3: 70, 15: 2310})
    assert (chroma.tx, chroma.ty, chroma.filt, chroma.masks) == (2, 3, 6, {7: 70, 15: 1120})
    if src == "422":
        _sharp_run(134, 70, "422", US_422, (COPY, COPY))
    else:
        _sharp_run(268, 140, "444", US_422, (TILE, TILE), dw=134, dh=70, dst="422")


def test_amount_zero_copies_a_plane_of_twelve_tiles():
    """197 x 70 4:4:4 with 5:5:0.0:3:3:1.0: the luma goes through twelve copying tiles, the chroma
    planes are filtered."""
    luma, chroma = _wide_cells(US_LUMA0)
    assert (luma.filt, luma.copy, luma.masks) == (0, 12, {}) and (chroma.filt, chroma.copy) == (12, 0)
    _sharp_run(*WIDE, "444", US_LUMA0, (COPY, COPY), full=True)


# ================================================================= 2. the deinterlacer's consumers and segments
NF = gy.NF


def _deint_case(w, h, c, mode, tff, rect=None, dst=None, dw=None, dh=None, pad=None, full=False, orient=0,
                unaligned_fetch=True, q=5, **enc_kw):
    """One context on the five frames of test_gpu_yadif._frames(w, h, c): the paths predict_paths
    gives (the deinterlacer in front changes none of them), debug_deint(), the oriented frames and
    the planes where those stages run, then the JPEGs.  Returns (encode_path, scale paths)."""
    dst = dst or c
    want = cg.predict_paths(w, h, c, rect, dst, dw, dh, pad, unaligned_fetch, orient=orient)
    frames, d = gy._frames(w, h, c), gy._deint(w, h, c, mode, tff)
    what = f"mode {mode} tff {tff}"
    with MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, max_batch=NF, chroma=dst, src_chroma=c, crop=rect,
                      pad=pad, orient=orient, deint=gy.flags(mode, tff), **enc_kw) as enc:
        assert enc.frame_bytes == i420_frame_bytes(w, h, c)
        assert enc._L.mjg_debug_deint_flags(enc._h) == gy.flags(mode, tff)
        assert (enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))) == want[:2]
        got = enc.encode(frames)
        gy._check_deint(enc, d, w, h, c, what)
        if orient:
            _check_oriented(enc, d, w, h, c, orient)
        if not want[0] & IN_PLACE:
            gu._check_stage(enc, "planes (the sws stage's output)", enc.debug_planes,
                            [deint_planes(f, w, h, c, orient, rect, dst, full, dw, dh, pad) for f in d], dst)
    _check(got, gy._ref(w, h, c, mode, tff, 0, NF, orient, rect, dst, full, dw, dh, pad, qscale=q, **enc_kw))
    return want[:2]


CROPS = [("aligned", 1, dict(rst=True)), ("aligned", 0, dict()), ("ua", 1, dict(huffman="optimal")), ("ua", 0, dict())]


@pytest.mark.parametrize("kind,tff,kw", CROPS, ids=[f"{k}_{'tff' if t else 'bff'}_{'_'.join(kw) or 'default'}"
                                                    for k, t, kw in CROPS])
def test_yadif_then_a_crop_read_in_place(kind, tff, kw, monkeypatch):
    """256 x 160 4:2:0: k_encode on a 224 x 128 window of d_deint, src_off[0] added to the slot's
    own pointer.  At x = 16 with MJG_UNALIGNED_FETCH=0 every offset and stride is a multiple of 8:
    the plain kernel and its 8-byte loads; at x = 6 the chroma planes start at x = 3: k_encode<UA>.
    11 chunks a frame, so work units start at chunks 1, 2, 3 and 4 of frames 1 to 4 and carry_row
    reads deinterlaced rows (with RST: in restart segments 6, 4, 2, 0, 6 and 4)."""
    w, h, c = 256, 160, "420"
    assert cg.deint_span(w, h).wgs == 10 and cg.deint_span(w // 2, h // 2).wgs == 3
    rect = (16, 16, 224, 128) if kind == "aligned" else (6, 16, 224, 128)
    if kw.get("rst"):
        assert [u[:2] for u in cg.unit_starts(224, 128, c, True, NF)][1:] == [(0, 6), (1, 4), (2, 2), (3, 0), (3, 6), (4, 4)]
    else:
        assert cg.mid_segment_units(224, 128, c, False, NF) == [(1, 0, 1), (2, 0, 2), (3, 0, 3), (4, 0, 4)]
    if kind == "aligned":
        monkeypatch.setenv("MJG_UNALIGNED_FETCH", "0")
    saw = _deint_case(w, h, c, 0, tff, rect, unaligned_fetch=kind != "aligned", **kw)
    assert saw == ((IN_PLACE if kind == "aligned" else IN_PLACE | UA), (NONE, NONE))


# (source, rectangle, encoded format, size, pad, full range, orientation, flags (mode, tff), expected paths)
CONSUMERS = {
    "rect_copy_pix_fmt": ((256, 160, "444"), (3, 5, 200, 100), "420", None, None, None, True, 0, (2, 0), (0, (COPY, TILE))),
    "pad_copy": ((130, 66, "420"), None, "420", None, None, (26, 28, 180, 120), False, 0, (0, 0), (0, (PADCOPY, PADCOPY))),
    "pix_fmt_420_from_444": ((130, 66, "444"), None, "420", None, None, None, False, 0, (2, 1), (0, (COPY, TILE))),
    "stream": ((256, 160, "420"), None, "420", 32, 20, None, False, 0, (0, 0), (0, (STREAM, TILE))),
    "mirror_orient2": ((301, 203, "420"), None, "420", None, None, None, False, 2, (0, 1), (IN_PLACE, (NONE, NONE))),
    "transpose_orient5": ((301, 203, "420"), None, "420", None, None, None, False, 5, (0, 0), (IN_PLACE, (NONE, NONE))),
}


@pytest.mark.parametrize("name", list(CONSUMERS))
def test_yadif_in_front_of_each_reader_of_d_deint(name):
    """The rectangle copy (full range, 4:4:4 to 4:2:0: the luma rectangle through k_plane_copy's
    RECT form, the chroma through k_scale; mode 2 bff, ten workgroups a plane whose later ones hold
    interior interpolated rows, which the bottom row of 4100 x 5 is not), the pad copy alone, -pix_fmt without a resize,
    k_scale_stream (256 x 160 -> 32 x 20), and both forms of k_orient_plane on 301 x 203 4:2:0
    (odd frame bytes: frames 1.. of d_deint at odd addresses; four workgroups of the mirroring
    copy, twelve tiles of the transposing one, 15 luma workgroups of the deinterlacer)."""
    (w, h, c), rect, dst, dw, dh, pad, full, orient, (mode, tff), want = CONSUMERS[name]
    assert cg.deint_span(w, h).wgs > 1
    if name == "rect_copy_pix_fmt":
        assert cg.predict_paths(w, h, c, rect, dst, dw, dh, pad)[2]      # the rectangle form
    if name == "stream":
        assert cg.scale_variant(w, h, dw, dh)[0] == "stream"
    if orient:
        assert i420_frame_bytes(w, h, c) % 2 == 1 and cg.deint_span(w, h, 15).head == 15
        assert cg.orient_span(w, h, bool(orient & 1))[3 if orient & 1 else 0] > 1
    assert _deint_case(w, h, c, mode, tff, rect, dst, dw, dh, pad, full, orient) == want


@pytest.mark.parametrize("shape", [gy.BIG, (131, 67, "420")], ids=lambda v: "%dx%d_%s" % v)
@pytest.mark.parametrize("tff", [0, 1], ids=["bff", "tff"])
def test_nospatial_past_one_workgroup(shape, tff):
    """Mode 2 with either parity where a plane takes several workgroups: 4100 x 5 4:4:4 (six a
    plane, a row's pieces from two of them, three pieces over a row end) and 131 x 67 4:2:0 (three
    for the luma, odd chroma planes, frames at odd addresses)."""
    w, h, c = shape
    span = cg.deint_span(w, h)
    assert span.wgs == (6 if shape == gy.BIG else 3) and span.over_row_end >= 3
    assert _deint_case(w, h, c, 2, tff, q=4) == (IN_PLACE, (NONE, NONE))


@pytest.mark.parametrize("lens", [(1, 3, 1), (1, 1, 2, 1)], ids=["1+3+1", "1+1+2+1"])
def test_segments_are_sequences_of_their_own(lens):
    """submit_segments on 33 x 17 4:4:4, every segment from byte 1 of its own allocation: a
    one-frame segment between others (its prev, cur and next are itself while its neighbours
    clamp to other bounds) and kMaxSegs segments.  The expected frames are each segment
    deinterlaced alone; a frame at a segment boundary differs from the five-frame sequence's."""
    w, h, c = 33, 17, "444"
    frames = gy._frames(w, h, c)
    cuts = np.cumsum((0,) + lens)
    assert cuts[-1] == NF
    segs = [(chain._device(frames[a:b], 1), int(b - a)) for a, b in zip(cuts, cuts[1:])]
    with MjpegEncoder(0, w, h, full_range=False, qscale=5, max_batch=NF, chroma=c, deint=gy.flags(0, 1)) as enc:
        assert len(lens) <= enc._L.mjg_max_segments()
        enc.submit_segments([(t.data_ptr(), n) for t, n in segs])
        got = enc.fetch()
        want = np.concatenate([gy._deint(w, h, c, 0, 1, int(a), int(b)) for a, b in zip(cuts, cuts[1:])])
        gy._check_deint(enc, want, w, h, c, "segments " + "+".join(map(str, lens)))
    ref = []
    for a, b in zip(cuts, cuts[1:]):
        ref += gy._ref(w, h, c, 0, 1, int(a), int(b), qscale=5)
    _check(got, ref)
    # every frame at a segment boundary sees other neighbours than in the five-frame sequence: its
    # deinterlaced bytes differ (checked above against `want`), the others' do not; the smooth frames
    # 1 and 3 differ in 14 bytes only, which q = 5 may round away, so of the JPEGs only "some differ"
    whole_d, whole = gy._deint(w, h, c, 0, 1), gy._ref(w, h, c, 0, 1, qscale=5)
    boundary = [(i in cuts and i > 0) or (i + 1 in cuts and i + 1 < NF) for i in range(NF)]
    assert [bool((want[i] != whole_d[i]).any()) for i in range(NF)] == boundary
    assert all(got[i] == whole[i] for i in range(NF) if not boundary[i])
    assert got[0] != whole[0] and got[4] != whole[4]


def test_worker_yadif_scale_unsharp_pad_across_batch_boundaries():
    """-vf yadif,scale=70:38,unsharp,pad=80:48:6:4 on five bff frames in batches of 2: three halo
    submits through slots with d_deint, d_scaled and d_sharp; the packets of the bff sequence."""
    W, H = gy.W, gy.H
    frames = gy._frames(W, H, "420")
    args = ["-vf", "yadif,scale=70:38,unsharp,pad=80:48:6:4"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    opts = worker.Options.from_env({"MJG_WORKER_BATCH": "2"})
    rc = worker.run(0, args, stdin=io.BytesIO(gy._y4m420(frames, W, H, "b")), stdout=out, stderr=err, opts=opts)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    packets = [d for _, d in r.frames(1)]
    info = r.info(1)
    assert (info.width, info.height, info.codec) == (80, 48, "V_MJPEG")
    sar = profile.scaled_sar((1, 1), (W, H), (70, 38))
    want = [sharp_ref(f, W, H, "420", DEFAULT, dw=70, dh=38, pad=(6, 4, 80, 48), qscale=profile.effective_qscale(5), sar=sar)
            for f in gy._deint(W, H, "420", 0, 0)]
    _check(packets, want)


# ================================================================= 3. the seeded sweep with a filter
SWEEP_SEED, SWEEP_COUNT, SWEEP_PARTS = cg.FILTER_SWEEP_SEED, 120, 4


def _filter_reference(cfg):
    """(source frames, deinterlaced frames, the sws stage's planes in front of a sharpen or None,
    the encoder's input planes, JPEGs) of one configuration, on the CPU."""
    w, h = cg.source_size(cfg)
    frames = source_frames(w, h, 3, cfg.fseed, cfg.src)[:cfg.nframes]
    d = frames
    if cfg.deint:
        mode, tff = (2 if "nospatial" in cfg.deint else 0), int(cfg.deint.startswith("tff"))
        parts = [frames[:2], frames[2:]] if cfg.submit == "segments" else [frames]      # a segment is a sequence of its own
        d = np.concatenate([deint_frames(p, w, h, cfg.src, mode, tff) for p in parts])
    huffman, rst = cfg.kw.get("huffman", "default"), cfg.kw.get("rst", False)
    pre = None
    if cfg.unsharp:
        pl = [sharp_planes(f, w, h, cfg.src, cfg.unsharp, cfg.orient, cfg.rect, cfg.dst, cfg.full, cfg.dw, cfg.dh, cfg.pad)
              for f in d]
        pre, planes = [p[0] for p in pl], [p[1] for p in pl]
    else:
        planes = [oriented_planes(f, w, h, cfg.src, cfg.orient, cfg.rect, cfg.dst, cfg.full, cfg.dw, cfg.dh, cfg.pad) for f in d]
    return frames, d, pre, planes, [chain.ref_jpeg(p, cfg.dst, cfg.q, huffman, rst) for p in planes]


def _run_filter_config(cfg):
    """One configuration against the reference; its feature set and paths, as the context reports."""
    w, h = cg.source_size(cfg)
    frames, d, pre, planes, ref = _filter_reference(cfg)
    split = (2, 1) if cfg.deint else (1, 1)
    mode = {"host": "host", "dev_odd": "dev", "segments": "segments", "merged": "merged"}[cfg.submit]
    with MjpegEncoder(0, w, h, cfg.dw, cfg.dh, full_range=cfg.full, qscale=cfg.q, max_batch=cfg.nframes, chroma=cfg.dst,
                      src_chroma=cfg.src, crop=cfg.rect, pad=cfg.pad, merge=cfg.submit == "merged", orient=cfg.orient,
                      deint=cg.DEINT_FLAGS[cfg.deint] or None, unsharp=cfg.unsharp, **cfg.kw) as enc:
        assert enc._L.mjg_debug_deint_flags(enc._h) == cg.DEINT_FLAGS[cfg.deint]
        assert (enc.debug_unsharp() is not None) == (cfg.unsharp is not None)
        enc_path, paths = enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))
        got, first = chain.submit(enc, frames, mode, offset=1 + 2 * (cfg.fseed % 8), split=split)
        if cfg.deint:
            assert first == 0
            gy._check_deint(enc, d, w, h, cfg.src, str(cfg.deint))
        if cfg.orient:
            _check_oriented(enc, d[first:], w, h, cfg.src, cfg.orient)
        if pre is not None:
            gu._check_stage(enc, "presharp (the sws stage's output)", enc.debug_presharp, pre[first:], cfg.dst)
        if not enc_path & IN_PLACE:
            gu._check_stage(enc, "planes (the encoder's input)", enc.debug_planes, planes[first:], cfg.dst)
    _check(got, ref)
    return cg.filter_features(cfg, enc_path, paths), (enc_path, paths)


@pytest.mark.parametrize("part", range(SWEEP_PARTS))
def test_seeded_sweep_with_a_filter(part):
    """The 120 configurations chain_geom.filter_sweep_configs draws for seed 2451, 30 per part:
    those of sweep_configs, each with a deinterlacer (none, tff, bff, either without the spatial
    check), a sharpen (none or one of five) or both, and in one of three an orientation.  A
    deinterlaced configuration has three frames through a host submit, a device pointer at an odd
    byte or submit_segments of 2 + 1 (each segment deinterlaced alone).  Every configuration must
    pass: the deinterlaced and the oriented bytes, the sws stage's output in front of a sharpen,
    the encoder's input wherever it is not read in place, then the JPEGs.  After the loop the part
    asserts how many of its configurations carried each feature, as the contexts reported it,
    against chain_geom.FILTER_SWEEP_FLOORS: the counts filter_predict and sharp_cells give for
    this seed on the CPU (tests/test_chain_geom.py pins them), every one at least 1: each
    deinterlacer kind, each sharpen kind (<5, 5> on the luma alone, on all planes, sizes at run
    time, the luma copied), each reader of d_deint (k_encode in place with and without UA, the
    rectangle copy, the pad copy, the tile and the stream kernel, both forms of the orientation),
    each feeder of the sharpen (tile, stream, plane copy, pad copy, a pad around a scaled picture),
    three tile columns, a copying tile beside a filtering one, a picture edge that cuts a quad on
    its left and on its right, every submit mode, and default / optimal / RST."""
    cfgs = cg.filter_sweep_configs(SWEEP_SEED, SWEEP_COUNT)[part * 30:(part + 1) * 30]
    sets = []
    for i, cfg in enumerate(cfgs):
        want = cg.filter_predict(cfg)[:2]
        print(part, i, tuple(cfg))
        try:
            f, saw = _run_filter_config(cfg)
        except AssertionError as e:
            raise AssertionError((part, i, tuple(cfg)) + e.args) from e
        assert saw == want, (part, i, tuple(cfg), saw, want)
        sets.append(f)
    counts = cg.count_filter_features(sets)
    print(part, counts)
    assert set(cg.FILTER_SWEEP_FLOORS[part]) == set(cg.FILTER_FEATURES)
    for k, floor in cg.FILTER_SWEEP_FLOORS[part].items():
        assert floor >= 1 and counts[k] >= floor, (part, k, counts[k], floor)
