"""crop, pad and the plane copy past one workgroup and one work unit, and a seeded sweep of the
whole filter chain (crop -> -pix_fmt / scale -> pad -> encode), byte for byte against the CPU
oracle composed as in tests/pad_ref.py (crop_frame, composed_planes, pad_planes,
oracle.encode_frame).  tests/test_gpu_crop.py, test_gpu_pad.py and test_gpu_chroma_resample.py
run toy sizes: one copy workgroup, one or two k_encode work units that start at chunk 0.  The
shapes here are the smallest that reach the other paths; every test asserts that *before* it
opens a context with tests/chain_geom.py (so a change of kBatch or kCopyVecs fails it loudly),
and on the context through encode_path() / scale_path() that the kernel it means ran.
debug_planes() is compared first wherever the sws stage runs, then the JPEG bytes."""
import numpy as np
import pytest

import chain_geom as cg
import oracle
import test_gpu_scale_stream as scale_stream
from chain_geom import COPY, IN_PLACE, NONE, PADCOPY, STREAM, TILE, UA
from chroma_resample_ref import composed_planes, source_frames
from crop_ref import crop_frame, same_inside
from pad_ref import BORDER, pad_planes
from test_chain_geom import ARM_SHAPES, CHROMA_COPY_RECTS, CHROMA_COPY_SIZE
from ffmpeg_distributed_amd.encoder import CHROMA_SHIFTS, MjpegEncoder, chroma_size, i420_frame_bytes, split_i420

pytestmark = pytest.mark.gpu


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
    """3 frames (two noise, one smooth) per source shape and format, made once."""
    if (w, h, c) not in _SRC:
        f = source_frames(w, h, 3, 100 * w + h + 11, c)
        f.setflags(write=False)
        _SRC[(w, h, c)] = f
    return _SRC[(w, h, c)]


def ref_planes(frame, w, h, src, rect, dst, full, dw, dh, pad):
    """pad_ref.padded_planes, with pad = None for no pad (pad_planes refuses the odd picture sizes
    an unpadded sub-sampled frame may have)."""
    r = rect or (0, 0, w, h)
    p = composed_planes(crop_frame(frame, w, h, src, r), r[2], r[3], src, dst, full, dw, dh)
    return p if pad is None else pad_planes(*p, dst, *pad)


def ref_jpeg(planes, dst, q, huffman="default", rst=False):
    """pad_ref.padded_ref's second half: the planes are the encoder's full-range input."""
    return oracle.encode_frame(*planes, full_range=True, qscale=q, sar=(1, 1), huffman=huffman, chroma=dst, rst=rst)


_REF = {}


def _ref(w, h, src, rect, dst, full, dw, dh, pad, q, huffman="default", rst=False):
    """(planes, JPEGs) of _frames(w, h, src), computed once per configuration."""
    pk = (w, h, src, rect, dst, full, dw, dh, pad)
    if pk not in _REF:
        _REF[pk] = [ref_planes(f, w, h, src, rect, dst, full, dw, dh, pad) for f in _frames(w, h, src)]
    jk = pk + (q, huffman, rst)
    if jk not in _REF:
        _REF[jk] = [ref_jpeg(p, dst, q, huffman, rst) for p in _REF[pk]]
    return _REF[pk], _REF[jk]


def check_planes(enc, planes, dst, first=0, pad=None, pic=None):
    """debug_planes() of the last synced submit (frames first.. of `planes`); under a pad also,
    explicitly, every byte outside the picture (pic = its size)."""
    ew, eh = enc.enc_w, enc.enc_h
    hs, vs = CHROMA_SHIFTS[dst]
    for i, want in enumerate(planes[first:]):
        got = split_i420(enc.debug_planes(i), ew, eh, dst)
        for p, (name, a, b) in enumerate(zip("YUV", got, want)):
            bad = np.argwhere(a != b)
            assert bad.size == 0, (first + i, name, len(bad), bad[:4].tolist())
            if pad is not None:
                border = np.ones(a.shape, bool)
                sx, sy = (0, 0) if p == 0 else (hs, vs)
                x, y = pad[0] >> sx, pad[1] >> sy
                border[y:y + ((pic[1] + (1 << sy) - 1) >> sy), x:x + ((pic[0] + (1 << sx) - 1) >> sx)] = False
                assert border.any() and (a[border] == BORDER[p]).all(), (first + i, name)


def _device(frames, offset):
    """The frames on the GPU at byte `offset` of their allocation (the tensor keeps it alive)."""
    import torch
    flat = np.ascontiguousarray(frames).reshape(-1)
    pool = torch.zeros(flat.size + offset, dtype=torch.uint8, device="cuda:0")
    pool[offset:] = torch.from_numpy(flat.copy()).to("cuda:0")
    torch.cuda.synchronize()
    t = pool[offset:]
    assert t.data_ptr() % 256 == offset % 256  # allocations are 256-aligned: the offset is the misalignment
    return t


def submit(enc, frames, mode, offset=1, split=None):
    """Encode `frames` through one submit mode; (JPEGs, first frame of the last synced submit).
    host; dev: one device submit from byte `offset` of its allocation; segments: one
    submit_segments of split = (a, b) frames, each from byte 1 of its allocation; merged: one
    single device submit per part of split on a merge=True context."""
    n = len(frames)
    if mode == "host":
        return enc.encode(frames), 0
    if mode == "dev":
        t = _device(frames, offset)
        enc.submit(device_ptr=t.data_ptr(), nframes=n)
        return enc.fetch(), 0
    a, b = split or (n - 1, 1)
    assert a + b == n
    segs = [_device(frames[:a], 1), _device(frames[a:], 1)]
    if mode == "segments":
        enc.submit_segments([(segs[0].data_ptr(), a), (segs[1].data_ptr(), b)])
        return enc.fetch(), 0
    assert mode == "merged"
    for t, k in zip(segs, (a, b)):
        enc.submit(device_ptr=t.data_ptr(), nframes=k)
    got = []
    for _ in segs:
        enc.sync()
        got += enc.fetch()
    return got, a


def _open(w, h, src, rect=None, dst=None, dw=None, dh=None, pad=None, full=False, q=5, unaligned_fetch=True,
          plane_copy=True, **kw):
    """A context, after asserting that it reports the paths chain_geom predicts."""
    dst = dst or src
    want = cg.predict_paths(w, h, src, rect, dst, dw, dh, pad, unaligned_fetch, plane_copy)
    enc = MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, max_batch=3, chroma=dst, src_chroma=src,
                       crop=rect, pad=pad, **kw)
    try:
        assert enc.frame_bytes == i420_frame_bytes(w, h, src)
        assert (enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))) == want[:2]
    except BaseException:
        enc.close()
        raise
    return enc


# ---------------------------------------------------------------- 3a / 3b: crop in place, UA
def _crop_in_place(w, h, c, rect, full, mode, monkeypatch, rst=False):
    """Host submit, a device submit from byte 1, submit_segments of 2 + 1 and the frames with other
    noise outside the rectangle, through one context, each against the oracle."""
    kw = dict(huffman="optimal") if mode == "optimal" else {}
    if mode == "fetch_off":
        monkeypatch.setenv("MJG_UNALIGNED_FETCH", "0")
    frames = _frames(w, h, c)
    _, ref = _ref(w, h, c, rect, c, full, None, None, None, 5, kw.get("huffman", "default"), rst)
    other = same_inside(frames, w, h, c, rect, 79)
    assert (frames != other).mean() > 0.2
    with _open(w, h, c, rect, full=full, unaligned_fetch=mode != "fetch_off", rst=rst, **kw) as enc:
        assert enc.encode_path() == (IN_PLACE if mode == "fetch_off" else IN_PLACE | UA)
        for m in ("host", "dev", "segments"):
            _check(submit(enc, frames, m, split=(2, 1))[0], ref)
        _check(enc.encode(other), ref)


# (format, rectangle of the 300x200 source, chunks at which units start, the predecessor blocks are interior)
MID_SEGMENT = [
    ("420", (2, 6, 250, 150), [12, 9, 6], False), ("420", (2, 6, 234, 150), [12, 9, 6], True),
    ("422", (2, 6, 250, 150), [12, 4, 16, 8], False), ("422", (2, 6, 234, 150), [12, 5, 17, 10], True),
    ("444", (3, 5, 250, 150), [12, 24, 6, 18, 12, 24], False), ("444", (3, 5, 234, 150), [12, 24, 7, 19, 2, 14, 26], True),
]


@pytest.mark.parametrize("mode", ["default", "optimal", "fetch_off"])
@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
@pytest.mark.parametrize("c,rect,chunks,interior", MID_SEGMENT, ids=[f"{m[0]}_{m[1][2]}" for m in MID_SEGMENT])
def test_crop_in_place_units_start_mid_segment(c, rect, chunks, interior, full, mode, monkeypatch):
    """k_encode<UA> reading a window of 300-byte rows (stride % 8 == 4) in place, 3 frames of 15 to
    30 chunks: work units of 12 tasks start at the chunks listed, so carry_row<UA> recomputes the
    DC predictors from the window's pixel rows (chunk != 0), in the emitting kernel, in -huffman
    optimal's counting one, and (MJG_UNALIGNED_FETCH=0: the plain kernel, every block through
    fetch_rows_edge) in carry_row's byte loads on a crop geometry.  At 250 wide (16 / 32 MCUs a
    row) every unit starts at the first MCU of an MCU row, so the blocks whose DC it needs are the
    last, partial MCU of the row before: carry_row's byte loop with the clamp to the window's
    edge.  At 234 wide (15 / 30 MCUs) they lie inside the window: carry_row<UA>'s 8-byte loads at
    any alignment."""
    assert [u[2] for u in cg.mid_segment_units(rect[2], rect[3], c, False, 3)] == chunks
    preds = [p[3].values() for p in cg.carry_preds(rect[2], rect[3], c, False, 3)]
    assert any(all(p) for p in preds) if interior else not any(any(p) for p in preds)
    _crop_in_place(300, 200, c, rect, full, mode, monkeypatch)


@pytest.mark.parametrize("mode", ["default", "fetch_off"])
@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
def test_crop_in_place_rst_units_start_inside_an_mcu_row(full, mode, monkeypatch):
    """RST with 5 chunks per MCU row (4:4:4, 350x40 of a 400x64 source at (3, 5): 44 MCUs, 264
    blocks a row, 3 rows): units start at row 2 chunk 2 of frame 0, row 1 chunk 4 of frame 1 and
    row 1 chunk 1 of frame 2, so carry_row<UA> runs with a segment base (bbase) != 0."""
    rect = (3, 5, 350, 40)
    assert cg.unit_starts(350, 40, "444", True, 3) == [(0, 0, 0), (0, 2, 2), (1, 1, 4), (2, 1, 1)]
    assert all(all(p[3].values()) for p in cg.carry_preds(350, 40, "444", True, 3))  # the 8-byte loads
    _crop_in_place(400, 64, "444", rect, full, mode, monkeypatch, rst=True)


# ---------------------------------------------------------------- 3c: aligned crop in place
ALIGNED = [((16, 16, 224, 128), IN_PLACE), ((0, 16, 256, 128), IN_PLACE), ((16, 16, 200, 100), IN_PLACE),
           ((8, 16, 224, 128), IN_PLACE | UA)]


@pytest.mark.parametrize("kw", [dict(), dict(full=True), dict(huffman="optimal"), dict(rst=True)],
                         ids=["tv", "full", "optimal", "rst"])
@pytest.mark.parametrize("rect,path", ALIGNED, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_aligned_crop_in_place(rect, path, kw):
    """4:2:0 256x160, the rectangle at x % 16 == 0: every plane offset and stride is a multiple of
    8, so the context launches k_encode<UA = false> on the crop geometry (stride != width, plane
    offsets from the rectangle's first byte) and its 8-byte fast path.  224x128 has 11 chunks a
    frame (units start at chunk 1 of frame 1 and chunk 2 of frame 2); (0, 16, 256, 128) is the
    letterbox crop; 200x100 ends inside a block both ways: the edge blocks replicate the crop's
    edge, not the source pixels beside it (the frames with other noise outside give the same
    bytes).  x = 8 puts the chroma planes at x = 4: the UA bit must be set."""
    w, h, c = 256, 160, "420"
    if rect == (16, 16, 224, 128) and not kw.get("rst"):
        assert cg.unit_starts(224, 128, c, False, 3) == [(0, 0, 0), (1, 0, 1), (2, 0, 2)]
    if rect == (16, 16, 200, 100) and not kw.get("rst"):
        assert cg.unit_starts(200, 100, c, False, 3) == [(0, 0, 0), (1, 0, 3), (2, 0, 6)]
    if rect[2] != 256 and not kw.get("rst"):  # those units' predecessors are interior: carry_row's aligned 8-byte loads
        assert all(all(p[3].values()) for p in cg.carry_preds(rect[2], rect[3], c, False, 3))
    full = kw.get("full", False)
    ekw = {k: v for k, v in kw.items() if k != "full"}
    frames = _frames(w, h, c)
    _, ref = _ref(w, h, c, rect, c, full, None, None, None, 5, **ekw)
    with _open(w, h, c, rect, full=full, **ekw) as enc:
        assert enc.encode_path() == path
        _check(enc.encode(frames), ref)
        _check(submit(enc, frames, "dev", offset=256)[0], ref)  # an aligned device pointer
        _check(enc.encode(same_inside(frames, w, h, c, rect, 80)), ref)


@pytest.mark.parametrize("offset", [1, 4])
def test_aligned_crop_from_a_device_pointer_that_is_not_8_aligned(offset):
    """The plain kernel with a frame base that fails its alignment test: every block takes
    fetch_rows_edge, and carry_row its byte loads, on the crop geometry."""
    w, h, c, rect = 256, 160, "420", (16, 16, 224, 128)
    assert cg.mid_segment_units(224, 128, c, False, 3)
    frames = _frames(w, h, c)
    _, ref = _ref(w, h, c, rect, c, False, None, None, None, 5)
    with _open(w, h, c, rect) as enc:
        assert enc.encode_path() == IN_PLACE
        _check(submit(enc, frames, "dev", offset=offset)[0], ref)


# ---------------------------------------------------------------- 3d: pad only past one workgroup
# (source size, format, rectangle, pad, luma workgroups, chroma (workgroups, slots))
PAD_COPY = [
    ((200, 84), "420", None, (26, 28, 250, 140), 3, (1, 3)),   # luma 35,000 B, mixed pieces in every row; chroma 8,750 B
    ((200, 84), "444", None, (26, 28, 250, 140), 3, (3, 4)),
    ((320, 136), "420", None, (0, 22, 320, 180), 4, (1, 4)),   # full-width rows of 20 pieces: none mixed
    ((33, 17), "444", None, (107, 59, 251, 141), 3, (3, 4)),   # odd everything: head and tail bytes
    ((300, 200), "420", (2, 6, 200, 84), (26, 28, 250, 140), 3, (1, 3)),  # the picture from a crop
]


@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
@pytest.mark.parametrize("size,c,rect,pad,lwg,cspan", PAD_COPY,
                         ids=["200x84_420", "200x84_444", "320x136_full_width", "33x17_444_odd", "crop_200x84_420"])
def test_pad_only_past_one_workgroup(size, c, rect, pad, lwg, cspan, full):
    """k_pad_plane<.., COPY = true> on canvas planes of 3 and 4 workgroups (blk > 0, every vector
    slot, every thread), tv range through its byte table and full range; every border byte is
    checked explicitly."""
    w, h = size
    ccw, cch = chroma_size(pad[2], pad[3], c)
    assert cg.copy_span(pad[2] * pad[3]) == (lwg, 4) and lwg >= 3
    assert cg.copy_span(ccw * cch) == cspan
    pic = rect[2:] if rect else size
    frames = _frames(w, h, c)
    planes, ref = _ref(w, h, c, rect, c, full, None, None, pad, 4)
    with _open(w, h, c, rect, pad=pad, full=full, q=4) as enc:
        assert (enc.scale_path(0), enc.scale_path(1)) == (PADCOPY, PADCOPY) and enc.encode_path() == 0
        got = enc.encode(frames)
        check_planes(enc, planes, c, pad=pad, pic=pic)
        _check(got, ref)
        if rect:
            _check(enc.encode(same_inside(frames, w, h, c, rect, 81)), ref)
            check_planes(enc, planes, c, pad=pad, pic=pic)


# ---------------------------------------------------------------- 3e: the rectangle copy past one workgroup
@pytest.mark.parametrize("copy_kernel", [True, False], ids=["k_plane_copy", "k_scale_identity"])
@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
@pytest.mark.parametrize("dst", ["420", "422"])
def test_crop_with_pix_fmt_rect_copy_past_one_workgroup(dst, full, copy_kernel, monkeypatch):
    """k_plane_copy<.., RECT = true>: the 251x151 luma (37,901 B, 3 workgroups, every slot) out of
    300-byte rows at (3, 5): the div_magic row split and the gathered pieces at row ends past the
    first workgroup; tv range reads the byte table.  MJG_PLANE_COPY=0 sends the same plane
    through k_scale's identity filters: both must equal the oracle."""
    w, h, src, rect = 300, 200, "444", (3, 5, 251, 151)
    assert cg.copy_span(251 * 151) == (3, 4)
    assert cg.predict_paths(w, h, src, rect, dst, None, None, None)[2]  # the rectangle form
    if not copy_kernel:
        monkeypatch.setenv("MJG_PLANE_COPY", "0")
    frames = _frames(w, h, src)
    planes, ref = _ref(w, h, src, rect, dst, full, None, None, None, 4)
    with _open(w, h, src, rect, dst, full=full, q=4, plane_copy=copy_kernel) as enc:
        assert enc.scale_path(0) == (COPY if copy_kernel else TILE) and enc.encode_path() == 0
        got = enc.encode(frames)
        check_planes(enc, planes, dst)
        _check(got, ref)
        _check(enc.encode(same_inside(frames, w, h, src, rect, 82)), ref)
        check_planes(enc, planes, dst)


@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
@pytest.mark.parametrize("rect", CHROMA_COPY_RECTS, ids=["whole_frames", "crop"])
def test_chroma_plane_copy_beside_a_scaled_luma(rect, full):
    """k_plane_copy<2, ..> (tv range: the chroma byte table) and its RECT form on a chroma plane:
    4:2:0 to 4:4:4 at half size, so luma is scaled 2:1 and the chroma planes keep their size; under
    the crop they are 125 bytes out of 150-byte rows."""
    w, h, src, dst = 300, 200, "420", "444"
    dw, dh = CHROMA_COPY_SIZE[rect]
    assert cg.copy_pad_cells(w, h, src, rect, dst, dw, dh, None, full) == {("copy", 0 if full else 2, rect is not None)}
    frames = _frames(w, h, src)
    planes, ref = _ref(w, h, src, rect, dst, full, dw, dh, None, 4)
    with _open(w, h, src, rect, dst, dw, dh, full=full, q=4) as enc:
        assert (enc.scale_path(0), enc.scale_path(1)) == (TILE, COPY) and enc.encode_path() == 0
        got = enc.encode(frames)
        check_planes(enc, planes, dst)
        _check(got, ref)
        if rect:
            _check(enc.encode(same_inside(frames, w, h, src, rect, 83)), ref)


# ---------------------------------------------------------------- 3f: border only around the stream kernel's picture
def test_border_only_around_a_picture_written_by_the_stream_kernel():
    """k_pad_plane<.., COPY = false> on a 256x144 canvas (luma 36,864 B: 3 workgroups) around the
    200x100 picture k_scale_stream writes at (28, 22) from 1100x700: the planes show that neither
    kernel touched the other's bytes."""
    w, h, c, dw, dh, pad = 1100, 700, "420", 200, 100, (28, 22, 256, 144)
    assert cg.copy_span(256 * 144)[0] >= 3
    frames = _frames(w, h, c)
    planes, ref = _ref(w, h, c, None, c, False, dw, dh, pad, 5)
    with _open(w, h, c, None, c, dw, dh, pad) as enc:
        assert enc.scale_path(0) == STREAM and enc.encode_path() == 0
        got = enc.encode(frames)
        check_planes(enc, planes, c, pad=pad, pic=(dw, dh))
    _check(got, ref)


# ---------------------------------------------------------------- 3g: every arm of the scale kernels' selection
@pytest.mark.parametrize("full", [False, True], ids=["tv", "full"])
@pytest.mark.parametrize("shape,arm", ARM_SHAPES, ids=["%dx%d_%dx%d" % s for s, _ in ARM_SHAPES])
def test_every_scale_arm_matches_reference(shape, arm, full):
    """One plane shape per [tile shape or stream form][d4] arm of build_plan, 4:4:4 in and out (luma
    and chroma the same size: both planes take the arm), two frames in one host submit: tv range
    runs the arm's range 1 and range 2 instantiations, full range its range 0 one.  The paths, the
    planes and then the bytes, as tests/test_gpu_scale_stream.py checks them."""
    sw, sh, dw, dh = shape
    assert cg.scale_variant(*shape) == arm
    path = STREAM if arm[0] == "stream" else TILE
    scale_stream._run(scale_stream._frames(sw, sh, "444", 2), sw, sh, dw, dh, "444", full=full, paths=(path, path))


# ---------------------------------------------------------------- 4: the seeded sweep
SWEEP_SEED, SWEEP_COUNT, SWEEP_PARTS = cg.SWEEP_SEED, 120, 4


def _run_config(cfg):
    """One configuration against the oracle; the feature set it carried, as the context reports."""
    frames = source_frames(cfg.w, cfg.h, 2, cfg.fseed, cfg.src)[:cfg.nframes]
    huffman, rst = cfg.kw.get("huffman", "default"), cfg.kw.get("rst", False)
    planes = [ref_planes(f, cfg.w, cfg.h, cfg.src, cfg.rect, cfg.dst, cfg.full, cfg.dw, cfg.dh, cfg.pad) for f in frames]
    ref = [ref_jpeg(p, cfg.dst, cfg.q, huffman, rst) for p in planes]
    mode = {"host": "host", "dev_odd": "dev", "segments": "segments", "merged": "merged"}[cfg.submit]
    with MjpegEncoder(0, cfg.w, cfg.h, cfg.dw, cfg.dh, full_range=cfg.full, qscale=cfg.q, max_batch=cfg.nframes,
                      chroma=cfg.dst, src_chroma=cfg.src, crop=cfg.rect, pad=cfg.pad, merge=cfg.submit == "merged",
                      **cfg.kw) as enc:
        enc_path, paths = enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))
        got, first = submit(enc, frames, mode, offset=1 + 2 * (cfg.fseed % 8), split=(1, 1))
        if not enc_path & IN_PLACE:
            pic = (cfg.dw or (cfg.rect[2] if cfg.rect else cfg.w), cfg.dh or (cfg.rect[3] if cfg.rect else cfg.h))
            check_planes(enc, planes, cfg.dst, first=first, pad=cfg.pad, pic=pic)
    _check(got, ref)
    return cg.features(cfg, enc_path, paths), (enc_path, paths)


@pytest.mark.parametrize("part", range(SWEEP_PARTS))
def test_seeded_sweep_of_the_chain(part):
    """120 drawn configurations (chain_geom.sweep_configs), 30 per part, one or two frames each:
    source size and format, encoded format, crop, resize, pad, range, q, tables and the submit
    mode.  After the loop the part asserts how many of its configurations carried each feature, as
    the contexts reported it, against chain_geom.SWEEP_FLOORS: the counts predict_paths gives
    for this seed on the CPU (tests/test_chain_geom.py pins them there), seed 93 chosen among
    1..3000 for the largest smallest counts.  The floors are those counts themselves, per part:
      crop in place UA 5, 2, 4, 3; crop in place aligned 2, 2, 3, 2; rectangle copy 4, 2, 2, 1;
      pad copy 4, 4, 2, 3; pad with scale 4, 11, 6, 9; stream kernel 2, 2, 2, 1;
      host 7, 7, 11, 6; device pointer at an odd byte 7, 9, 12, 11; submit_segments 10, 6, 5, 7;
      merged single submits 6, 8, 2, 6
    (of the 120: 14, 9, 9, 13, 30, 7 and 31, 39, 28, 22)."""
    cfgs = cg.sweep_configs(SWEEP_SEED, SWEEP_COUNT)[part * 30:(part + 1) * 30]
    sets = []
    for i, cfg in enumerate(cfgs):
        want = cg.predict_paths(cfg.w, cfg.h, cfg.src, cfg.rect, cfg.dst, cfg.dw, cfg.dh, cfg.pad)[:2]
        try:
            f, saw = _run_config(cfg)
        except AssertionError as e:
            raise AssertionError((part, i, tuple(cfg)) + e.args) from e
        assert saw == want, (part, i, tuple(cfg), saw, want)
        sets.append(f)
    counts = cg.count_features(sets)
    print(part, counts)
    for k, floor in cg.SWEEP_FLOORS[part].items():
        assert counts[k] >= floor, (part, k, counts[k], floor)
