"""k_orient_plane past one workgroup, and the orientation in front of the rest of the chain: byte
for byte against numpy indexing (tests/orient_ref.py) followed by the composed crop / scale / pad
oracle.  tests/test_gpu_orient.py runs toy frames, one workgroup per (plane, frame) in both forms
of the kernel; the shapes here are the smallest that reach the other paths (blk > 0, gxy > 1,
idle waves beside working ones, partial blocks in later tiles, tx == 1 over two workgroups), and
behind the orientation the readers of d_orient that had no test: k_encode reading a crop in place
with work units that start mid-segment, the rectangle copy, the pad copy and k_scale_stream.
Every test asserts with tests/chain_geom.py, *before* it opens a context, that its shape reaches
the path it means, and on the context that the kernels it means ran (encode_path / scale_path).
debug_oriented() is compared first, then debug_planes() where a sws stage runs, then the JPEGs."""
import numpy as np
import pytest

import chain_geom as cg
import test_gpu_chain as chain
from chain_geom import COPY, IN_PLACE, NONE, PADCOPY, STREAM, TILE, UA
from chroma_resample_ref import source_frames
from crop_ref import same_inside
from orient_ref import orient_frame, oriented_planes, oriented_ref, oriented_size
from test_chain_geom import ORIENT_INVERSE, ORIENT_SHAPES
from test_gpu_orient import _check, _check_oriented
from ffmpeg_distributed_amd.encoder import MjpegEncoder, chroma_size, i420_frame_bytes

pytestmark = pytest.mark.gpu

NF = 3
_SRC = {}


def _frames(w, h, c):
    """3 frames (two noise, one smooth) per source shape and format, made once."""
    if (w, h, c) not in _SRC:
        f = source_frames(w, h, NF, 100 * w + h + 17, c)
        f.setflags(write=False)
        _SRC[(w, h, c)] = f
    return _SRC[(w, h, c)]


_REF = {}


def _ref(w, h, src, orient, rect=None, full=False, **kw):
    """The expected JPEGs of _frames(w, h, src), computed once per configuration."""
    key = (w, h, src, orient, rect, full, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = [oriented_ref(f, w, h, src, orient, rect, src, full, **kw) for f in _frames(w, h, src)]
    return _REF[key]


def _turned_back(oriented, ow, oh, c, orient):
    """The source frames whose oriented frames are `oriented` (ow x oh): the inverse map of each."""
    return np.stack([orient_frame(f, ow, oh, c, ORIENT_INVERSE[orient]) for f in oriented])


def _open(w, h, src, orient, rect=None, dst=None, dw=None, dh=None, pad=None, full=False, q=5, unaligned_fetch=True,
          nf=NF, **kw):
    """A context on w x h source frames, after asserting that it reports the orientation and the
    paths chain_geom predicts."""
    dst = dst or src
    want = cg.predict_paths(w, h, src, rect, dst, dw, dh, pad, unaligned_fetch, orient=orient)
    enc = MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, max_batch=nf, chroma=dst, src_chroma=src,
                       crop=rect, pad=pad, orient=orient, **kw)
    try:
        assert enc.frame_bytes == i420_frame_bytes(w, h, src)
        assert enc._L.mjg_debug_orient(enc._h) == orient
        assert (enc.or_w, enc.or_h) == oriented_size(w, h, orient)
        assert (enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))) == want[:2]
    except BaseException:
        enc.close()
        raise
    return enc


def _past_one_workgroup(w, h, c, orient, chroma_too=False):
    """The precondition of 2a, from the table of tests/test_chain_geom.py: the form this map takes
    runs more than one workgroup on the luma plane (and on each chroma plane)."""
    t = cg.orient_cells(orient)[0]
    l0, l1, csize, c0, c1 = ORIENT_SHAPES[(w, h, c)]
    assert chroma_size(w, h, c) == csize
    span, cspan = cg.orient_span(w, h, t), cg.orient_span(*csize, t)
    assert tuple(span[:4]) == (l1 if t else l0) and tuple(cspan[:4]) == (c1 if t else c0)
    assert span[3 if t else 0] > 1
    if chroma_too:
        assert cspan[3 if t else 0] > 1
    return span


# ---------------------------------------------------------------- a: the orientation alone past one workgroup
ALONE_SHAPES = [(300, 200, "444"), (301, 203, "420"), (301, 203, "444"), (40, 600, "420"), (600, 40, "444")]
ALONE = ([(w, h, c, o) for (w, h, c) in ALONE_SHAPES for o in range(1, 8)]
         + [(300, 200, "422", o) for o in (2, 4, 6)])


def _full_too(w, h, c, orient):
    """Full range on one shape per map (and on one map of the 4:2:2 shape)."""
    return (c == "422" and orient == 4) or (c != "422" and ALONE_SHAPES.index((w, h, c)) == orient % len(ALONE_SHAPES))


@pytest.mark.parametrize("w,h,c,orient", ALONE, ids=lambda v: str(v))
def test_orientation_alone_past_one_workgroup(w, h, c, orient):
    """All seven maps on planes of 2 to 4 workgroups in both forms.  300x200 4:4:4: luma and the
    U + V launch past one workgroup, 10 tiles (the third workgroup has two idle waves), a 12-wide
    partial block in tiles 4 and 9.  301x203: 13-wide and 3-row partial blocks in tiles of the
    second and third workgroup, and an odd frame size, so frames 1 and 2 lie at odd bytes of
    d_orient (T = 0: head != 0; T = 1: dword pairs stored at odd addresses).  40x600: tx == 1 (the
    div_magic shortcut) with five tile rows over two workgroups, and 40-byte rows, of whose 16-byte
    pieces 2 in 5 are gathered over a row end.  600x40: one tile row, the lanes of rows 40.. idle
    in every tile.  300x200 4:2:2: the mirroring maps on a 150-wide chroma plane of 2 workgroups.
    The oriented bytes of all three frames (two of noise: a permuted or repeated 16-byte piece
    shows), then the JPEGs k_encode makes of d_orient read in place."""
    span = _past_one_workgroup(w, h, c, orient)
    if orient & 1:
        assert span.partial_past_first and span.idle > 0  # working and idle waves in the last workgroup
    if (w, h) == (40, 600) and orient & 1:
        assert span.tx == 1 and span.ty > cg.ORIENT_WAVES
    frames = _frames(w, h, c)
    for full in ((False, True) if _full_too(w, h, c, orient) else (False,)):
        with _open(w, h, c, orient, full=full, q=4) as enc:
            assert (enc.encode_path(), enc.scale_path(0), enc.scale_path(1)) == (IN_PLACE, NONE, NONE)
            got = enc.encode(frames)
            _check_oriented(enc, frames, w, h, c, orient)
        _check(got, _ref(w, h, c, orient, full=full, qscale=4))


assert {o for (w, h, c, o) in ALONE if c != "422" and _full_too(w, h, c, o)} == set(range(1, 8))  # every map in full range


@pytest.mark.parametrize("mode", ["dev", "segments"])
@pytest.mark.parametrize("orient", [6, 3], ids=["T0_orient6", "T1_orient3"])
def test_orientation_from_an_odd_device_pointer_and_from_two_segments(orient, mode):
    """One case per form on 301x203 4:4:4 (every plane past one workgroup): the frames at byte 1 of
    their allocation in one device submit, and as submit_segments of 2 + 1 frames from separate
    allocations, so that seg_frame picks the second segment in a launch with gxy > 1."""
    w, h, c = 301, 203, "444"
    _past_one_workgroup(w, h, c, orient, chroma_too=True)
    frames = _frames(w, h, c)
    with _open(w, h, c, orient, q=4) as enc:
        got, first = chain.submit(enc, frames, mode, offset=1, split=(2, 1))
        assert first == 0
        _check_oriented(enc, frames, w, h, c, orient)
    _check(got, _ref(w, h, c, orient, qscale=4))


# ---------------------------------------------------------------- b: a crop read in place out of d_orient
def _crop_out_of_orient(w, h, c, orient, rect, path, mode="default", monkeypatch=None, rst=False, seed=84):
    """k_encode on a window of the oriented frames: a host submit (the oriented bytes first), a device
    submit from byte 1, submit_segments of 2 + 1, and the frames whose bytes outside the
    rectangle's pre-image are other noise, through one context, each against the reference."""
    kw = dict(huffman="optimal") if mode == "optimal" else {}
    if mode == "fetch_off":
        monkeypatch.setenv("MJG_UNALIGNED_FETCH", "0")
    ow, oh = oriented_size(w, h, orient)
    frames = _frames(w, h, c)
    ref = _ref(w, h, c, orient, rect, qscale=5, rst=rst, **kw)
    oriented = np.stack([orient_frame(f, w, h, c, orient) for f in frames])
    other = _turned_back(same_inside(oriented, ow, oh, c, rect, seed), ow, oh, c, orient)
    assert other.shape == frames.shape and (frames != other).mean() > 0.2
    with _open(w, h, c, orient, rect, unaligned_fetch=mode != "fetch_off", rst=rst, **kw) as enc:
        assert enc.encode_path() == path and enc.scale_path(0) == NONE
        for m in ("host", "dev", "segments"):
            got = chain.submit(enc, frames, m, split=(2, 1))[0]
            if m == "host":
                _check_oriented(enc, frames, w, h, c, orient)
            _check(got, ref)
        _check(enc.encode(other), ref)


TURNED = [(o, rect, interior, mode) for o in (3, 5) for rect, interior in (((2, 6, 250, 150), False), ((2, 6, 234, 150), True))
          for mode in ("default", "optimal")] + [(3, (2, 6, 234, 150), True, "fetch_off")]


@pytest.mark.parametrize("orient,rect,interior,mode", TURNED, ids=[f"orient{t[0]}_{t[1][2]}_{t[3]}" for t in TURNED])
def test_crop_in_place_out_of_a_quarter_turn_units_start_mid_segment(orient, rect, interior, mode, monkeypatch):
    """200x300 4:2:0 turned to 300x200 (12 tiles in 3 workgroups; T = 0 does not apply), then
    k_encode<UA> on a window of d_orient's 300-byte rows: src_off[0] is added to the slot's own
    pointer, the work units start at chunks 12, 9 and 6, so carry_row recomputes their DC
    predictors from oriented pixel rows: at 250 wide from the partial MCU at the window's edge, at
    234 wide from interior blocks (tests/test_gpu_chain.py MID_SEGMENT, on the caller's frames).
    MJG_UNALIGNED_FETCH=0: the plain kernel on the same geometry."""
    w, h, c = 200, 300, "420"
    assert tuple(cg.orient_span(w, h, True)[:4]) == ORIENT_SHAPES[(w, h, c)][1]
    assert [u[2] for u in cg.mid_segment_units(rect[2], rect[3], c, False, NF)] == [12, 9, 6]
    preds = [p[3].values() for p in cg.carry_preds(rect[2], rect[3], c, False, NF)]
    assert all(all(p) for p in preds) if interior else not any(any(p) for p in preds)
    _crop_out_of_orient(w, h, c, orient, rect, IN_PLACE if mode == "fetch_off" else IN_PLACE | UA, mode, monkeypatch)


def test_crop_in_place_out_of_a_half_turn():
    """300x200 4:4:4 under orient 6 (no size change, the T = 0 form at 4 workgroups a plane), the
    window (3, 5, 250, 150): 30 chunks a frame, units start at chunks 12, 24, 6, 18, 12, 24."""
    w, h, c, rect = 300, 200, "444", (3, 5, 250, 150)
    assert cg.orient_span(w, h, False) == ORIENT_SHAPES[(w, h, c)][0]
    assert [u[2] for u in cg.mid_segment_units(250, 150, c, False, NF)] == [12, 24, 6, 18, 12, 24]
    _crop_out_of_orient(w, h, c, 6, rect, IN_PLACE | UA)


def test_crop_in_place_out_of_a_transpose_with_rst():
    """64x400 4:4:4 transposed to 400x64, the window (3, 5, 350, 40) with RST: 5 chunks per MCU
    row, units start at row 2 chunk 2, row 1 chunk 4 and row 1 chunk 1, so carry_row<UA> runs on
    d_orient with a segment base != 0."""
    w, h, c, rect = 64, 400, "444", (3, 5, 350, 40)
    assert cg.orient_span(w, h, True).wgs == 1 and cg.orient_span(w, h, True).ntiles == 4  # a small plane: k_encode is the subject
    assert cg.unit_starts(350, 40, c, True, NF) == [(0, 0, 0), (0, 2, 2), (1, 1, 4), (2, 1, 1)]
    _crop_out_of_orient(w, h, c, 1, rect, IN_PLACE | UA, rst=True)


@pytest.mark.parametrize("rect,path", [((16, 16, 224, 128), IN_PLACE), ((8, 16, 224, 128), IN_PLACE | UA)],
                         ids=["x16_aligned", "x8_ua"])
def test_aligned_crop_in_place_out_of_a_transpose(rect, path):
    """160x256 4:2:0 under orient 7 gives 256x160 (6 tiles, 2 workgroups): with the window at
    x % 16 == 0 every offset and stride is a multiple of 8 and the context launches k_encode<UA =
    false> on d_orient (256-aligned, so its 8-byte fast path runs); x = 8 puts the chroma planes
    at x = 4 and sets UA.  11 chunks a frame: units start at chunk 1 of frame 1, chunk 2 of frame 2."""
    w, h, c = 160, 256, "420"
    assert tuple(cg.orient_span(w, h, True)[:4]) == ORIENT_SHAPES[(w, h, c)][1]
    assert cg.unit_starts(224, 128, c, False, NF) == [(0, 0, 0), (1, 0, 1), (2, 0, 2)]
    _crop_out_of_orient(w, h, c, 7, rect, path, seed=85)


# ---------------------------------------------------------------- c: the sws stage reading d_orient
# (oriented frame and format, rectangle, encoded format, size, pad, q, paths): the shapes of
# tests/test_gpu_chain.py, whose frames, planes and JPEGs (chain._frames, chain._ref) are reused
SWS = {
    "rect_copy": ((300, 200, "444"), (3, 5, 251, 151), "420", None, None, None, 4, (COPY, TILE)),
    "pad_copy": ((200, 84, "420"), None, "420", None, None, (26, 28, 250, 140), 4, (PADCOPY, PADCOPY)),
    "stream_border": ((1100, 700, "420"), None, "420", 200, 100, (28, 22, 256, 144), 5, (STREAM, STREAM)),
}
SWS_CASES = [("rect_copy", 5), ("rect_copy", 6), ("pad_copy", 1), ("pad_copy", 4), ("stream_border", 7), ("stream_border", 2)]


@pytest.mark.parametrize("name,orient", SWS_CASES, ids=[f"{n}_orient{o}" for n, o in SWS_CASES])
def test_sws_stage_reads_the_oriented_frames(name, orient):
    """k_plane_copy's rectangle form, k_pad_plane's copy and k_scale_stream (with k_pad_plane's
    border around its picture) reading d_orient, each past one workgroup, under one transposing
    and one mirroring map.  The source is the inverse orientation of the frames of
    tests/test_gpu_chain.py, so the oriented frames, the planes and the bytes are those that test
    expects of the caller's frames; oriented_planes of the first source frame ties the two."""
    (ow, oh, c), rect, dst, dw, dh, pad, q, paths = SWS[name]
    pic = (dw or (rect[2] if rect else ow), dh or (rect[3] if rect else oh))
    canvas = pad[2:] if pad else pic
    assert cg.copy_span(canvas[0] * canvas[1])[0] >= 3
    w, h = oriented_size(ow, oh, orient)
    want = cg.predict_paths(w, h, c, rect, dst, dw, dh, pad, orient=orient)
    assert want[:2] == (0, paths) and want[2] == (name == "rect_copy")
    oriented = chain._frames(ow, oh, c)
    frames = _turned_back(oriented, ow, oh, c, orient)
    planes, ref = chain._ref(ow, oh, c, rect, dst, False, dw, dh, pad, q)
    for a, b in zip(oriented_planes(frames[0], w, h, c, orient, rect, dst, False, dw, dh, pad), planes[0]):
        assert a.shape == b.shape and (a == b).all()
    with _open(w, h, c, orient, rect, dst, dw, dh, pad, q=q) as enc:
        got = enc.encode(frames)
        _check_oriented(enc, frames, w, h, c, orient)
        assert all((enc.debug_oriented(i) == oriented[i]).all() for i in range(NF))
        chain.check_planes(enc, planes, dst, pad=pad, pic=pic if pad else None)
    _check(got, ref)


# ---------------------------------------------------------------- d: the seeded sweep with an orientation
SWEEP_SEED, SWEEP_COUNT, SWEEP_PARTS = cg.ORIENT_SWEEP_SEED, 120, 4


def _run_orient_config(cfg):
    """One configuration against the reference; its feature set and paths, as the context reports."""
    w, h = cg.source_size(cfg)
    frames = source_frames(w, h, 2, cfg.fseed, cfg.src)[:cfg.nframes]
    oriented = [orient_frame(f, w, h, cfg.src, cfg.orient) for f in frames]
    huffman, rst = cfg.kw.get("huffman", "default"), cfg.kw.get("rst", False)
    planes = [chain.ref_planes(f, cfg.w, cfg.h, cfg.src, cfg.rect, cfg.dst, cfg.full, cfg.dw, cfg.dh, cfg.pad)
              for f in oriented]
    ref = [chain.ref_jpeg(p, cfg.dst, cfg.q, huffman, rst) for p in planes]
    mode = {"host": "host", "dev_odd": "dev", "segments": "segments", "merged": "merged"}[cfg.submit]
    with MjpegEncoder(0, w, h, cfg.dw, cfg.dh, full_range=cfg.full, qscale=cfg.q, max_batch=cfg.nframes,
                      chroma=cfg.dst, src_chroma=cfg.src, crop=cfg.rect, pad=cfg.pad, merge=cfg.submit == "merged",
                      orient=cfg.orient, **cfg.kw) as enc:
        assert enc._L.mjg_debug_orient(enc._h) == cfg.orient
        enc_path, paths = enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))
        got, first = chain.submit(enc, frames, mode, offset=1 + 2 * (cfg.fseed % 8), split=(1, 1))
        _check_oriented(enc, frames[first:], w, h, cfg.src, cfg.orient)
        if not enc_path & IN_PLACE:
            pic = (cfg.dw or (cfg.rect[2] if cfg.rect else cfg.w), cfg.dh or (cfg.rect[3] if cfg.rect else cfg.h))
            chain.check_planes(enc, planes, cfg.dst, first=first, pad=cfg.pad, pic=pic)
    _check(got, ref)
    return cg.orient_features(cfg, enc_path, paths), (enc_path, paths)


@pytest.mark.parametrize("part", range(SWEEP_PARTS))
def test_seeded_sweep_with_an_orientation(part):
    """The 120 configurations chain_geom.sweep_configs draws for seed 2901, 30 per part, each with
    one of the seven maps (a mirroring one where the source is 4:2:2) in front: the drawn frame is
    the oriented one, the source h x w under a transposing map.  Every configuration must pass:
    the oriented bytes, the planes wherever the encoder does not read in place, then the JPEGs.
    After the loop the part asserts how many of its configurations carried each feature, as the
    contexts reported it, against chain_geom.ORIENT_SWEEP_FLOORS: the counts predict_paths and
    orient_span give for this seed on the CPU (tests/test_chain_geom.py pins them), seed 2901
    chosen among 1..3000 for the largest smallest counts.  Per part:
      maps 1..7: 4 5 4 4 6 6 1; 3 5 4 6 2 4 6; 2 4 4 7 3 8 2; 3 8 3 3 4 5 4;
      luma past one workgroup in T = 0 11, 13, 14, 13, in T = 1 10, 10, 7, 10;
      orientation alone read in place 2, 2, 3, 2; crop in place out of d_orient with UA 2, 3, 4, 2,
      aligned 2, 2, 2, 5; a sws stage reading d_orient 24, 23, 21, 21;
      host 8, 8, 8, 7; device pointer at an odd byte 8, 7, 14, 7; submit_segments 4, 5, 5, 11;
      merged single submits 10, 10, 3, 5."""
    cfgs = cg.orient_sweep_configs(SWEEP_SEED, SWEEP_COUNT)[part * 30:(part + 1) * 30]
    sets = []
    for i, cfg in enumerate(cfgs):
        want = cg.orient_predict(cfg)[:2]
        print(part, i, tuple(cfg))
        try:
            f, saw = _run_orient_config(cfg)
        except AssertionError as e:
            raise AssertionError((part, i, tuple(cfg)) + e.args) from e
        assert saw == want, (part, i, tuple(cfg), saw, want)
        sets.append(f)
    counts = cg.count_orient_features(sets)
    print(part, counts)
    for k, floor in cg.ORIENT_SWEEP_FLOORS[part].items():
        assert counts[k] >= floor, (part, k, counts[k], floor)
