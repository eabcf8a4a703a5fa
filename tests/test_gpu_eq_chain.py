"""k_lut_plane past one workgroup and over row ends, the table slots in front of and behind every
other stage, and both in a seeded sweep of the chain: byte for byte against tests/eq_ref.py inside
the composed reference of test_gpu_eq.chain_ref (orientation, slot "in", crop, sws stage, slot
"out", unsharp, pad, oracle).  tests/test_gpu_eq.py runs toy planes: its padded canvases are 80 x 48
(spans of 159 pieces, where a workgroup covers kCopyThreads x kCopyVecs = 1024), its largest slot-"out"
picture is 64 x 32, and d_lut, the identity copy, d_deint in place and the merged submits run on
130 x 66 only, one workgroup a plane; the shapes here are the smallest that reach the rest.  Every
case asserts with chain_geom.lut_span, *before* it opens a context, that its shape reaches what it
names (workgroups, pieces over a row end and skipped pieces of workgroups blk >= 1, head and tail
bytes), and on the context that the kernels it means ran (scale_path / encode_path).  It then
compares debug_lut_in(), debug_presharp() where a sharpen runs, debug_planes() and the JPEGs, in
that order; a difference names the stage and the first differing sample.  tools/lut_host_check.py
walks the launches of these shapes and canvases on the CPU first."""
import numpy as np
import pytest

import chain_geom as cg
import eq_ref
import test_gpu_chain as chain
import test_gpu_eq as ge
import test_gpu_unsharp as gu
import test_gpu_yadif as gy
from chain_geom import COPY, IN_PLACE, PADCOPY, STREAM, TILE, UA
from chroma_resample_ref import source_frames
from orient_ref import orient_frame, oriented_size
from test_gpu_eq import T_IN, T_OUT, _check, _frames, _run, _same, chain_ref
from test_gpu_filter_chain import PAD420, STREAM_SRC
from test_gpu_orient import _check_oriented
from unsharp_ref import GPU_GEOMETRY_CHAIN, US_55, WIDE
from yadif_ref import deint_frames
from ffmpeg_distributed_amd import profile
from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes

pytestmark = pytest.mark.gpu

TABLES = {"perm": (), "identity_Y": (0,), "identity_U": (1,), "identity_V": (2,)}


def _tab(t, name):
    return ge._with_identity(t, TABLES[name])


def _out_spans(W, H, c, px, py, w, h, n=ge.NF):
    """[luma, U, V] LutSpan of frame 0 and all of them per (plane, frame) of slot "out"."""
    spans = cg.lut_out_spans(W, H, c, px, py, w, h, n)
    return [spans[(p, 0)] for p in range(3)], spans


# ================================================================= 1. slot "out" at the canvas stride
def test_lut_out_strided_two_workgroups_row_ends_8_bytes_apart():
    """200 x 100 4:4:4 full range at (5, 7) of 208 x 120, the pad copy in front: every plane a span of
    20792 bytes, two workgroups, head 11, no skipped piece (the gap of 8 is below 16), 198 pieces over
    a row end of which 42 lie in workgroup 1.  The border keeps 0 / 128 / 128."""
    first, _ = _out_spans(208, 120, "444", 5, 7, 200, 100)
    for sp in first:
        assert (sp.wgs, sp.head, sp.skipped, sp.whole + sp.over_row_end) == (2, 11, 0, 1298) and sp.late_over >= 1
    r = chain_ref(_frames(200, 100, "444")[0], 200, 100, "444", None, T_OUT, full=True, pad=(5, 7, 208, 120))
    yy, uu, vv = r["planes"]
    assert (yy[0, 0], uu[0, 0], vv[0, 0], yy[119, 207]) == (0, 128, 128, 0)
    assert all(T_OUT[p][0] != 0 and T_OUT[p][128] != 128 for p in range(3))
    _run(200, 100, "444", lut_out=T_OUT, full=True, pad=(5, 7, 208, 120), want_paths=(PADCOPY, PADCOPY, 0))


@pytest.mark.parametrize("kw", [dict(), dict(huffman="optimal"), dict(rst=True)], ids=["default", "optimal", "rst"])
def test_lut_out_strided_skipped_pieces_odd_chroma_place_and_a_sharpen_behind(kw):
    """tests/test_gpu_filter_chain.py's PAD420: 260 x 132 4:2:0 scaled to 130 x 66 at (70, 38) of 264 x
    136, 5:5 everywhere behind the tables.  Luma: a span of 17290 bytes, two workgroups, head 10,
    skipped pieces in workgroup 1; chroma: 65 x 33 at (35, 19) of 132 x 68, head 1, one workgroup."""
    assert (264, 136, "420", 70, 38, 130, 66, US_55) in GPU_GEOMETRY_CHAIN
    (luma, u, v), _ = _out_spans(264, 136, "420", 70, 38, 130, 66)
    assert cg.lut_plane_geoms(264, 136, "420", 70, 38, 130, 66)[1][:3] == (65, 33, 132)
    assert 65 * 264 + 130 == 17290 and (luma.wgs, luma.head) == (2, 10) and luma.late_skipped >= 1 and luma.late_over >= 1
    assert (u.wgs, u.head, v.wgs, v.head) == (1, 1, 1, 1) and u.skipped and u.over_row_end
    p = PAD420
    _run(p["w"], p["h"], "420", lut_out=T_OUT, dw=p["dw"], dh=p["dh"], us=US_55, pad=p["pad"], want_paths=(TILE, TILE, 0), **kw)


CHROMA_CANVASES = {"gap_10": (12, 14, 520, 300), "gap_20": (20, 14, 540, 300)}


@pytest.mark.parametrize("canvas,name", [("gap_10", n) for n in TABLES] + [("gap_20", "perm")])
def test_lut_out_strided_chroma_past_one_workgroup(canvas, name):
    """500 x 280 4:2:0 without a resize under a pad.  At (12, 14) of 520 x 300: nine luma workgroups
    with skipped pieces (a gap of 20); the chroma 250 x 140 of 260 x 150, three workgroups a plane
    in the paired U + V launch (a V workgroup's blk is not its blockIdx), pieces over a row end in
    blk >= 1, none skipped: its gap of 10 is below 16.  At (20, 14) of 540 x 300 the chroma gap is
    20 and workgroups blk >= 1 of U and V skip pieces too (ten luma workgroups).  With an identity Y, U or V the paired
    launch holds one plane that is left alone and one that is mapped."""
    pad = CHROMA_CANVASES[canvas]
    (luma, u, v), _ = _out_spans(pad[2], pad[3], "420", pad[0], pad[1], 500, 280)
    assert luma.wgs == (9 if canvas == "gap_10" else 10) and luma.late_over >= 1 and luma.late_skipped >= 1
    for sp in (u, v):
        assert sp.wgs == 3 and sp.late_over >= 1 and (sp.late_skipped >= 1) == (canvas == "gap_20")
    _run(500, 280, "420", lut_out=_tab(T_OUT, name), pad=pad, want_paths=(PADCOPY, PADCOPY, 0))


# ================================================================= 2. slot "out", flat
def test_lut_out_flat_past_one_workgroup():
    """256 x 160 4:4:4 without a resize: slot "out" forces the plane copy, three workgroups a plane."""
    first, _ = _out_spans(256, 160, "444", 0, 0, 256, 160)
    assert [(sp.wgs, sp.head, sp.tail, sp.over_row_end + sp.skipped) for sp in first] == [(3, 0, 0, 0)] * 3
    _run(256, 160, "444", lut_out=T_OUT, want_paths=(COPY, COPY, 0))


def test_lut_out_flat_on_frames_at_odd_addresses():
    """301 x 203 4:2:0 without a resize: odd enc_frame_bytes, so frames 1 and 2 of d_scaled lie at odd
    addresses: four luma workgroups with heads 0, 13, 10 and tails 15, 2, 5."""
    assert i420_frame_bytes(301, 203, "420") % 2 == 1
    _, spans = _out_spans(301, 203, "420", 0, 0, 301, 203)
    assert [(spans[(0, f)].wgs, spans[(0, f)].head, spans[(0, f)].tail) for f in range(3)] == [(4, 0, 15), (4, 13, 2), (4, 10, 5)]
    assert all(spans[(p, f)].head and spans[(p, f)].tail for p in (1, 2) for f in range(3))
    _run(301, 203, "420", lut_out=T_OUT, want_paths=(COPY, COPY, 0))


# ================================================================= 3. slot "in" into d_lut in every submit mode
BIG = (301, 203, "420")
_REFS = {}


def _big_refs(name):
    """chain_ref of the five frames of 301 x 203 under slot "in" with the named tables, computed once."""
    if name not in _REFS:
        _REFS[name] = [chain_ref(f, *BIG, _tab(T_IN, name)) for f in _frames(*BIG, 5)]
    return _REFS[name]


def _big_spans():
    """Four luma workgroups, one a chroma plane; frames 1.. at odd addresses in d_lut."""
    w, h, c = BIG
    assert i420_frame_bytes(w, h, c) % 2 == 1 and cg.lut_span(w, h, w).wgs == 4 and cg.lut_span(151, 102, 151).wgs == 1
    assert cg.lut_span(w, h, w, 13).head == 13


@pytest.mark.parametrize("name", ["perm", "identity_Y", "identity_U"])
@pytest.mark.parametrize("mode", ["host", "device+1", "segments_1+3+1", "segments_1+1+2+1", "merged"])
def test_lut_in_into_d_lut_past_one_workgroup(mode, name):
    """301 x 203 4:2:0, odd frame bytes: the luma is four workgroups.  With an identity Y those four copy
    (`id && s != d`); with an identity U the paired launch copies U and maps V.  A host submit, a device
    pointer at byte 1, submit_segments of five frames each segment from byte 1 of its own allocation,
    and two merged device submits."""
    _big_spans()
    w, h, c = BIG
    tabs = _tab(T_IN, name)
    if mode in ("host", "device+1"):      # (three frames: test_gpu_eq._run's own reference)
        _run(w, h, c, lut_in=tabs, device=mode != "host", want_paths=(0, 0, 1))
        return
    frames, refs = _frames(w, h, c, 5), _big_refs(name)
    if mode == "merged":
        parts = [chain._device(frames[lo:lo + n], 0) for lo, n in ((0, 2), (2, 3))]
        got = []
        with MjpegEncoder(0, w, h, qscale=5, max_batch=3, chroma=c, merge=True, lut_in=tabs) as enc:
            assert (enc.scale_path(0), enc.scale_path(1), enc.encode_path() & 3) == (0, 0, 1)
            for t, n in zip(parts, (2, 3)):
                enc.submit(device_ptr=t.data_ptr(), nframes=n)
            for _ in parts:
                enc.sync()
                got += enc.fetch()
            for i in range(3):      # the last job's frames lie behind the first job's two
                _same("lut_in, merged submits", 2 + i, enc.debug_lut_in(i), refs[2 + i]["lut_in"], w, h, c)
        _check(got, [r["jpeg"] for r in refs])
        return
    lens = (1, 3, 1) if mode == "segments_1+3+1" else (1, 1, 2, 1)
    cuts = np.cumsum((0,) + lens)
    segs = [chain._device(frames[a:b], 1) for a, b in zip(cuts, cuts[1:])]
    with MjpegEncoder(0, w, h, qscale=5, max_batch=5, chroma=c, lut_in=tabs) as enc:
        assert len(lens) <= enc._L.mjg_max_segments()
        assert (enc.scale_path(0), enc.scale_path(1), enc.encode_path() & 3) == (0, 0, 1)
        enc.submit_segments([(t.data_ptr(), n) for t, n in zip(segs, lens)])
        got = enc.fetch()
        for i in range(5):
            _same("lut_in, " + mode, i, enc.debug_lut_in(i), refs[i]["lut_in"], w, h, c)
    for t, a, b in zip(segs, cuts, cuts[1:]):      # the caller's frames are never written
        assert (t.cpu().numpy() == frames[a:b].reshape(-1)).all()
    _check(got, [r["jpeg"] for r in refs])


# ================================================================= 4. slot "in" in place in d_deint
@pytest.mark.parametrize("kind", ["whole", "crop_aligned", "crop_ua"])
def test_lut_in_in_place_in_d_deint_past_one_workgroup(kind, monkeypatch):
    """256 x 160 4:2:0, yadif mode 2 bff, five frames in two halo submits: three luma workgroups of the
    table stage on d_deint in place.  Then a 224 x 128 crop read in place behind it (x = 16 with
    MJG_UNALIGNED_FETCH=0: the plain kernel; x = 6: k_encode<UA>): k_encode reads mapped,
    deinterlaced rows through src_off."""
    w, h, c = 256, 160, "420"
    assert cg.lut_span(w, h, w).wgs == 3 and cg.deint_span(w, h).wgs == 10
    rect = {"whole": None, "crop_aligned": (16, 16, 224, 128), "crop_ua": (6, 16, 224, 128)}[kind]
    if kind == "crop_aligned":
        monkeypatch.setenv("MJG_UNALIGNED_FETCH", "0")
    want = cg.predict_paths(w, h, c, rect, c, None, None, None, kind != "crop_aligned")
    assert want[:2] == ((IN_PLACE | UA if kind == "crop_ua" else IN_PLACE), (0, 0))
    frames = _frames(w, h, c, 5)
    d = deint_frames(frames, w, h, c, 2, 0)
    refs = [chain_ref(f, w, h, c, T_IN, rect=rect) for f in d]
    got = []
    with MjpegEncoder(0, w, h, qscale=5, max_batch=ge.NF, chroma=c, crop=rect, deint=gy.flags(2, 0), lut_in=T_IN) as enc:
        assert (enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))) == want[:2]
        for lo, n, halo in ((0, 3, 2), (3, 2, 1)):
            first = lo - (halo & 1)
            enc.submit(frames[first:lo + n + (halo >> 1 & 1)], n, halo=halo)
            got += enc.fetch()
            for i in range(n):
                _same(f"lut_in in place in d_deint, halo {halo}", lo + i, enc.debug_lut_in(i), refs[lo + i]["lut_in"], w, h, c)
    _check(got, [r["jpeg"] for r in refs])


# ================================================================= 5. both slots around the stream kernel
def test_both_slots_with_the_stream_kernel_between_them():
    """208 x 562 4:4:4 -> 197 x 70: d_lut (eight workgroups a plane) in front of k_scale_stream, slot
    "out" flat on 13790 bytes a plane behind it, U and V at heads 2 and 4."""
    assert cg.scale_variant(*STREAM_SRC, *WIDE)[0] == "stream"
    assert cg.lut_span(*STREAM_SRC, STREAM_SRC[0]).wgs == 8
    first, _ = _out_spans(*WIDE, "444", 0, 0, *WIDE)
    assert [(sp.wgs, sp.head) for sp in first] == [(1, 0), (1, 2), (1, 4)]
    _run(*STREAM_SRC, "444", lut_in=T_IN, lut_out=T_OUT, dw=WIDE[0], dh=WIDE[1], want_paths=(STREAM, STREAM, 0))


# ================================================================= 6. the worker
WORKER = [("yadif,eq=gamma=1.3:saturation=0.8,scale=130:66,pad=264:136:70:38", dict(gamma=1.3, saturation=0.8), "in", "b"),
          ("scale=130:66,eq=contrast=1.3:brightness=0.05,unsharp,pad=264:136:70:38", dict(contrast=1.3, brightness=0.05),
           "out", "p")]


@pytest.mark.parametrize("vf,spec,slot,field", WORKER, ids=["yadif_eq_scale_pad", "scale_eq_unsharp_pad"])
def test_worker_eq_graphs_on_the_padded_420_geometry(vf, spec, slot, field):
    """260 x 132 frames in batches of 2 to 130 x 66 at (70, 38) of 264 x 136, with real eq tables, which
    clip and so are not injective.  Behind yadif the tables run in place in d_deint (three luma
    workgroups); behind the scale they run under the pad (two strided luma workgroups, the sharpen
    behind them)."""
    w, h, c = 260, 132, "420"
    frames = _frames(w, h, c, 5)
    tabs = profile.eq_tables(spec)
    assert (tabs == eq_ref.tables(spec)).all()
    assert any(len(set(t.tolist())) < 256 for t in tabs)
    pad = profile.resolve_pad({"w": 264, "h": 136, "x": 70, "y": 38}, 130, 66, c)
    assert pad == PAD420["pad"] and cg.lut_span(w, h, w).wgs == 3
    packets, info = ge._worker(vf, frames, w, h, field=field, batch=2)
    assert (info.width, info.height, info.codec) == (264, 136, "V_MJPEG")
    sar = profile.scaled_sar((1, 1), (w, h), (130, 66))
    d = deint_frames(frames, w, h, c, 0, 0) if slot == "in" else frames
    refs = [chain_ref(f, w, h, c, tabs if slot == "in" else None, tabs if slot == "out" else None, dw=130, dh=66,
                      us=(5, 5, 1.0, 5, 5, 0.0) if slot == "out" else None, pad=pad, qscale=profile.effective_qscale(5),
                      sar=sar)["jpeg"] for f in d]
    _check(packets, refs, "worker, slot " + slot)


# ================================================================= 7. the seeded sweep with a table
SWEEP_SEED, SWEEP_COUNT, SWEEP_PARTS = cg.EQ_SWEEP_SEED, cg.EQ_SWEEP_COUNT, 4
PER_PART = SWEEP_COUNT // SWEEP_PARTS


def _sweep_tables(cfg):
    """The (3, 256) tables of the two slots: eq_ref.perm_tables seeded from fseed, with the kind's identity planes."""
    out = []
    for kind, seed in ((cfg.lut_in, cfg.fseed), (cfg.lut_out, cfg.fseed ^ 0x5a5a5a)):
        out.append(None if kind is None else ge._with_identity(eq_ref.perm_tables(seed), cg.LUT_IDENT[kind]))
    return out


def _run_eq_config(cfg):
    """One configuration against the reference; its feature set and paths, as the context reports."""
    w, h = cg.source_size(cfg)
    ow, oh = oriented_size(w, h, cfg.orient)
    frames = source_frames(w, h, 3, cfg.fseed, cfg.src)[:cfg.nframes]
    d = frames
    if cfg.deint:
        mode, tff = (2 if "nospatial" in cfg.deint else 0), int(cfg.deint.startswith("tff"))
        parts = [frames[:2], frames[2:]] if cfg.submit == "segments" else [frames]      # a segment is a sequence of its own
        d = np.concatenate([deint_frames(p, w, h, cfg.src, mode, tff) for p in parts])
    tin, tout = _sweep_tables(cfg)
    refs = [chain_ref(f, w, h, cfg.src, tin, tout, cfg.orient, cfg.rect, cfg.dst, cfg.full, cfg.dw, cfg.dh, cfg.unsharp,
                      cfg.pad, cfg.q, (1, 1), cfg.kw.get("huffman", "default"), cfg.kw.get("rst", False)) for f in d]
    split = (2, 1) if cfg.deint else (1, 1)
    mode = {"host": "host", "dev_odd": "dev", "segments": "segments", "merged": "merged"}[cfg.submit]
    with MjpegEncoder(0, w, h, cfg.dw, cfg.dh, full_range=cfg.full, qscale=cfg.q, max_batch=cfg.nframes, chroma=cfg.dst,
                      src_chroma=cfg.src, crop=cfg.rect, pad=cfg.pad, merge=cfg.submit == "merged", orient=cfg.orient,
                      deint=cg.DEINT_FLAGS[cfg.deint] or None, unsharp=cfg.unsharp, lut_in=tin, lut_out=tout, **cfg.kw) as enc:
        assert enc._L.mjg_debug_deint_flags(enc._h) == cg.DEINT_FLAGS[cfg.deint]
        for slot, t in (("in", tin), ("out", tout)):
            got_t = enc.debug_lut(slot)
            assert (got_t is None) == (t is None) and (t is None or (got_t == t).all()), slot
        enc_path, paths = enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))
        got, first = chain.submit(enc, frames, mode, offset=1 + 2 * (cfg.fseed % 8), split=split)
        # slot "in" runs in place in the buffer of the stage in front of it: d_orient, else d_deint, then
        # holds the mapped frames, which debug_lut_in reads; the stages in front keep theirs
        if cfg.deint:
            assert first == 0
            if cfg.orient or tin is None:
                gy._check_deint(enc, d, w, h, cfg.src, str(cfg.deint))
        if cfg.orient and tin is None:
            _check_oriented(enc, d[first:], w, h, cfg.src, cfg.orient)
        if tin is not None:
            for i, r in enumerate(refs[first:]):
                if cfg.orient:      # the oriented bytes, through the tables
                    assert (r["lut_in"] == eq_ref.map_frames(orient_frame(d[first + i], w, h, cfg.src, cfg.orient), ow, oh,
                                                             cfg.src, tin)).all()
                _same("lut_in (k_lut_plane's slot-in output)", first + i, enc.debug_lut_in(i), r["lut_in"], ow, oh, cfg.src)
        if cfg.unsharp is not None:
            gu._check_stage(enc, "presharp (the mapped sws output)", enc.debug_presharp, [r["presharp"] for r in refs[first:]],
                            cfg.dst)
        if not enc_path & IN_PLACE:
            gu._check_stage(enc, "planes (the encoder's input)", enc.debug_planes, [r["planes"] for r in refs[first:]], cfg.dst)
    _check(got, [r["jpeg"] for r in refs])
    return cg.eq_features(cfg, enc_path, paths), (enc_path, paths)


@pytest.mark.parametrize("part", range(SWEEP_PARTS))
def test_seeded_sweep_with_a_table(part):
    """The configurations chain_geom.eq_sweep_configs draws for the committed seed, in four parts:
    those of sweep_configs, each with a table kind per slot (none, permutations, those with an
    identity Y, with an identity U and V), at least one slot set, in one of four a deinterlacer, in
    one of four an orientation, in one of three a sharpen.  Every configuration must pass: the
    deinterlaced and the oriented bytes where a buffer still holds them (slot "in" maps the last of
    them in place), debug_lut_in, the mapped sws output in front of a sharpen, the encoder's input
    wherever it is not read in place, then the JPEGs.  After the loop the part asserts how many of
    its configurations carried each feature, as the contexts reported paths, against
    chain_geom.EQ_SWEEP_FLOORS: the counts eq_predict and lut_span give for this seed on the CPU
    (tests/test_chain_geom.py pins them), every one at least 1: each table kind per slot, both
    slots at once, slot "in" into d_lut, in place in d_deint and in d_orient, d_lut under each
    submit mode, each reader of the mapped frames (k_encode in place on a crop aligned and UA, the
    rectangle copy, the pad copy, k_plane_copy, k_scale, k_scale_stream), slot "out" flat and
    strided, each past one workgroup, with pieces over a row end and skipped pieces in workgroups
    blk >= 1, a sharpen behind slot "out", every submit mode, and default / optimal / RST; and three that a
    mutation run asked for (profiles/eq_chain/mutations.txt): an identity plane copied into d_lut by
    three workgroups or more, a mapped V plane of three or more (in either slot), and a whole V piece
    in a loop slot i >= 1 at the canvas stride.  The seed is the one of 1..3000 whose sorted counts
    are largest, compared from the smallest up (chain_geom.EQ_SWEEP_SEED)."""
    cfgs = cg.eq_sweep_configs(SWEEP_SEED, SWEEP_COUNT)[part * PER_PART:(part + 1) * PER_PART]
    sets = []
    for i, cfg in enumerate(cfgs):
        want = cg.eq_predict(cfg)[:2]
        print(part, i, tuple(cfg))
        try:
            f, saw = _run_eq_config(cfg)
        except AssertionError as e:
            raise AssertionError((part, i, tuple(cfg)) + e.args) from e
        assert saw == want, (part, i, tuple(cfg), saw, want)
        sets.append(f)
    counts = cg.count_eq_features(sets)
    print(part, counts)
    assert set(cg.EQ_SWEEP_FLOORS[part]) == set(cg.EQ_FEATURES)
    for k, floor in cg.EQ_SWEEP_FLOORS[part].items():
        assert floor >= 1 and counts[k] >= floor, (part, k, counts[k], floor)
