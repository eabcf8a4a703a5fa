"""tests/chain_geom.py against values computed by hand for the shapes of tests/test_gpu_chain.py,
tests/test_gpu_orient_chain.py and tests/test_gpu_filter_chain.py (no GPU).  The hand values assume kBatch = 12 and 256 x 4 pieces per copy workgroup; the first
test says so, so that a change of those constants points here before it fails a sum below."""
import os
import re

import numpy as np
import pytest

import chain_geom as cg
from chain_geom import COPY, NONE, PADCOPY, STREAM, TILE, IN_PLACE, UA
from orient_ref import orient_frame, orient_plane, oriented_size
from ffmpeg_distributed_amd.encoder import chroma_size, i420_frame_bytes


def test_constants_parsed_from_the_kernel_sources():
    assert (cg.K_BATCH, cg.COPY_THREADS, cg.COPY_VECS) == (12, 256, 4)
    assert (cg.SCALE_TILE_W, cg.SCALE_LOAD_ROWS, cg.SCALE_ALIAS_WORDS) == (64, 7, 36)


@pytest.mark.parametrize("w,h,c,rst,n,want", [
    # 250x150 4:2:0: 16 x 10 MCUs of 6 blocks = 960 blocks = 15 chunks
    (250, 150, "420", False, 3, (16, 10, 1, 960, 15, 45)),
    # 4:2:2: 8 blocks per MCU = 1280 blocks = 20 chunks
    (250, 150, "422", False, 3, (16, 10, 1, 1280, 20, 60)),
    # 4:4:4: MCUs 8 wide, 32 x 10 of 6 blocks = 1920 blocks = 30 chunks
    (250, 150, "444", False, 3, (32, 10, 1, 1920, 30, 90)),
    # RST 350x40 4:4:4: 44 MCUs per row = 264 blocks = 5 chunks, 3 rows
    (350, 40, "444", True, 3, (44, 3, 3, 264, 5, 45)),
    # 224x128 4:2:0: 14 x 8 MCUs = 672 blocks = 10.5 -> 11 chunks
    (224, 128, "420", False, 3, (14, 8, 1, 672, 11, 33)),
    (224, 128, "420", True, 3, (14, 8, 8, 84, 2, 48)),
    # one MCU row: RST has nothing to restart
    (72, 16, "420", True, 2, (5, 1, 1, 30, 1, 2)),
    (72, 40, "420", False, 3, (5, 3, 1, 90, 2, 6)),
])
def test_enc_geom(w, h, c, rst, n, want):
    assert tuple(cg.enc_geom(w, h, c, rst, n)) == want


@pytest.mark.parametrize("w,h,c,rst,n,want", [
    (250, 150, "420", False, 3, [(0, 0, 0), (0, 0, 12), (1, 0, 9), (2, 0, 6)]),
    (250, 150, "422", False, 3, [(0, 0, 0), (0, 0, 12), (1, 0, 4), (1, 0, 16), (2, 0, 8)]),
    (250, 150, "444", False, 3, [(0, 0, 0), (0, 0, 12), (0, 0, 24), (1, 0, 6), (1, 0, 18), (2, 0, 0),
                                 (2, 0, 12), (2, 0, 24)]),
    # 15 tasks per frame: task 12 = row 2 chunk 2, task 24 = frame 1 task 9 = row 1 chunk 4,
    # task 36 = frame 2 task 6 = row 1 chunk 1
    (350, 40, "444", True, 3, [(0, 0, 0), (0, 2, 2), (1, 1, 4), (2, 1, 1)]),
    (224, 128, "420", False, 3, [(0, 0, 0), (1, 0, 1), (2, 0, 2)]),
    (256, 128, "420", False, 3, [(0, 0, 0), (1, 0, 0), (2, 0, 0)]),   # 12 chunks: every unit a whole frame
    (200, 100, "420", False, 3, [(0, 0, 0), (1, 0, 3), (2, 0, 6)]),   # 13 x 7 x 6 = 546 blocks = 9 chunks
])
def test_unit_starts(w, h, c, rst, n, want):
    assert cg.unit_starts(w, h, c, rst, n) == want
    assert cg.mid_segment_units(w, h, c, rst, n) == [u for u in want if u[2]]


@pytest.mark.parametrize("w,h,c,b,want", [
    (250, 150, "420", 0, (0, 0, 0, 250, 150)), (250, 150, "420", 3, (0, 8, 8, 250, 150)),
    (250, 150, "420", 4, (1, 0, 0, 125, 75)), (250, 150, "420", 5, (2, 0, 0, 125, 75)),
    # block 765: Y3 of MCU 127 = the last MCU (15) of MCU row 7: x0 = 240 + 8, y0 = 112 + 8
    (250, 150, "420", 765, (0, 248, 120, 250, 150)), (250, 150, "420", 766, (1, 120, 56, 125, 75)),
    # 4:2:2: Cb above Cb, 16 chroma rows per MCU; block 8 * 17 + 5 = MCU 17 = (1, 1), the lower Cb
    (250, 150, "422", 141, (1, 8, 24, 125, 150)),
    # 4:4:4: MCUs 8 wide; block 6 * 33 + 1 = MCU 33 = (1, 1), the lower Y
    (250, 150, "444", 199, (0, 8, 24, 250, 150)), (250, 150, "444", 203, (2, 8, 24, 250, 150)),
])
def test_block_pos(w, h, c, b, want):
    assert cg.block_pos(w, h, c, b) == want


def test_carry_preds():
    """250 wide: 16 (32) MCUs a row, units start at the first MCU of a row and need the DCs of
    the last, partial MCU before it (x0 = 248 luma, 120 chroma: past pw - 8).  234 wide: 15 MCUs,
    chunk 12 starts at MCU 128 = row 8, MCU 8: its predecessors are interior."""
    for c in ("420", "422", "444"):
        assert not any(any(p[3].values()) for p in cg.carry_preds(250, 150, c, False, 3))
    assert cg.carry_preds(234, 150, "420", False, 3) == [(0, 0, 12, {0: True, 1: True, 2: True}),
                                                         (1, 0, 9, {0: True, 1: True, 2: True}),
                                                         (2, 0, 6, {0: True, 1: True, 2: True})]
    assert [(p[2], all(p[3].values())) for p in cg.carry_preds(234, 150, "444", False, 3)] == [
        (12, True), (24, True), (7, True), (19, True), (2, True), (14, False), (26, True)]
    assert all(all(p[3].values()) for p in cg.carry_preds(350, 40, "444", True, 3))
    assert all(all(p[3].values()) for p in cg.carry_preds(224, 128, "420", False, 3))


@pytest.mark.parametrize("nbytes,want", [
    (64 * 48, (1, 1)),         # 192 pieces: the largest pad-only plane of tests/test_gpu_pad.py
    (101 * 57, (1, 2)),        # 359 pieces: the largest rectangle of tests/test_gpu_crop.py
    (250 * 140, (3, 4)),       # 2187 pieces
    (125 * 70, (1, 3)),        # 546 pieces: slots 0 to 2
    (320 * 180, (4, 4)),       # 3600 pieces
    (251 * 141, (3, 4)),       # 2211 pieces
    (251 * 151, (3, 4)),       # 2368 pieces
    (256 * 144, (3, 4)),       # 2304 pieces
    (16384, (1, 4)), (16384 + 16, (2, 4)), (15, (1, 1)), (4096, (1, 1)), (4096 + 16, (1, 2)),
])
def test_copy_span(nbytes, want):
    assert cg.copy_span(nbytes) == want


def test_orient_constants_parsed_from_the_kernel_source():
    """The hand values below assume tiles of 64 columns x 128 rows, 4 to a workgroup; kOrientWaves
    is an expression in scale.hip, so chain_geom restates it and this checks that it still reads so."""
    assert (cg.ORIENT_TILE, cg.ORIENT_TILE_H, cg.ORIENT_WAVES) == (64, 128, 4)
    with open(os.path.join(cg._CSRC, "scale.hip")) as f:
        assert re.search(r"constexpr\s+int\s+kOrientWaves\s*=\s*kCopyThreads\s*/\s*64\s*;", f.read())


# The shapes of tests/test_gpu_orient_chain.py: (source, format) -> luma T = 0 (workgroups, slots),
# luma T = 1 (tx, ty, tiles, workgroups), the chroma plane, and the same two for it; None: 4:2:2
# is not transposed.  Workgroups of 16,384 bytes (T = 0) and of 4 tiles (T = 1).
ORIENT_SHAPES = {
    (300, 200, "444"): ((4, 4), (5, 2, 10, 3), (300, 200), (4, 4), (5, 2, 10, 3)),
    (301, 203, "420"): ((4, 4), (5, 2, 10, 3), (151, 102), (1, 4), (3, 1, 3, 1)),
    (301, 203, "444"): ((4, 4), (5, 2, 10, 3), (301, 203), (4, 4), (5, 2, 10, 3)),
    (300, 200, "422"): ((4, 4), None, (150, 200), (2, 4), None),
    (40, 600, "420"): ((2, 4), (1, 5, 5, 2), (20, 300), (1, 2), (1, 3, 3, 1)),
    (600, 40, "444"): ((2, 4), (10, 1, 10, 3), (600, 40), (2, 4), (10, 1, 10, 3)),
    (200, 300, "420"): ((4, 4), (4, 3, 12, 3), (100, 150), (1, 4), (2, 2, 4, 1)),
    (160, 256, "420"): ((3, 4), (3, 2, 6, 2), (80, 128), (1, 3), (2, 1, 2, 1)),
}


@pytest.mark.parametrize("shape", list(ORIENT_SHAPES), ids=lambda s: "%dx%d_%s" % s)
def test_orient_span(shape):
    w, h, c = shape
    l0, l1, csize, c0, c1 = ORIENT_SHAPES[shape]
    assert chroma_size(w, h, c) == csize
    assert cg.orient_span(w, h, False) == l0 == cg.copy_span(w * h)
    assert cg.orient_span(*csize, False) == c0
    if l1 is not None:
        assert tuple(cg.orient_span(w, h, True)[:4]) == l1
        assert tuple(cg.orient_span(*csize, True)[:4]) == c1


def test_orient_span_edges():
    """The idle waves and the partial blocks of the shapes above, by hand.  300 = 4 x 64 + 44: the
    last tile column has two whole lane columns, a 12-wide partial one and one outside; 200 = 128 +
    72 = 9 x 8: no partial rows; tiles 4 and 9 (the last column) lie past the first workgroup.
    301 x 203: 13-wide and 3-row partial blocks.  40 x 600: one tile column (its tx_magic is 0: the
    shortcut), 40 = 2 x 16 + 8.  600 x 40: 600 = 9 x 64 + 24, one tile row of 40 rows, 5 lane rows."""
    assert cg.orient_span(300, 200, True) == (5, 2, 10, 3, 2, True, False, True)
    assert cg.orient_span(301, 203, True) == (5, 2, 10, 3, 2, True, True, True)
    assert cg.orient_span(151, 102, True) == (3, 1, 3, 1, 1, True, True, False)
    assert cg.orient_span(40, 600, True) == (1, 5, 5, 2, 3, True, False, True)
    assert cg.orient_span(600, 40, True) == (10, 1, 10, 3, 2, True, False, True)
    assert cg.orient_span(200, 300, True) == (4, 3, 12, 3, 0, True, True, True)
    assert cg.orient_span(160, 256, True) == (3, 2, 6, 2, 2, False, False, False)
    assert cg.orient_span(64, 128, True) == (1, 1, 1, 1, 3, False, False, False)
    assert cg.orient_span(130, 66, True)[:4] == (3, 1, 3, 1)   # the largest planes of tests/test_gpu_orient.py:
    assert cg.orient_span(70, 150, True)[:4] == (2, 2, 4, 1)   # one workgroup
    assert cg.orient_span(130, 66, False) == (1, 3) and cg.orient_span(70, 150, False) == (1, 3)
    # 301 x 203: an odd frame size, so frames 1 and 2 start at an odd byte of the oriented buffer
    assert (301 * 203 + 2 * 151 * 102) % 2 == 1 and (301 * 203 * 3) % 2 == 1


def test_orient_cells_are_reached_by_the_gpu_tests():
    """k_orient_plane<T, FX> with fy 0 and 1: the seven maps are every cell but <0, 0> with fy 0,
    which is orient 0 and launches nothing.  tests/test_gpu_orient_chain.py runs all seven on
    300x200 4:4:4, whose luma plane and whose chroma planes (the U + V launch) take more than one
    workgroup in both forms; the 4:2:2 case adds the non-transposing maps on a chroma plane half
    as wide."""
    cells = {cg.orient_cells(o) for o in range(1, 8)}
    assert cells == {(t, fx, fy) for t in (False, True) for fx in (False, True) for fy in (0, 1)} - {(False, False, 0)}
    assert cg.orient_cells(0) == (False, False, 0)
    assert [cg.orient_cells(o) for o in (1, 2, 4)] == [(True, False, 0), (False, True, 0), (False, False, 1)]
    w, h, c = 300, 200, "444"
    for o in range(1, 8):
        t = cg.orient_cells(o)[0]
        for plane in ((w, h), chroma_size(w, h, c)):
            assert cg.orient_span(*plane, t)[3 if t else 0] > 1
    assert all(cg.orient_span(*chroma_size(300, 200, "422"), False)[0] > 1 for o in (2, 4, 6))


def test_the_inverse_of_every_orientation():
    """orient o undoes itself, except the two quarter turns 3 and 5, which undo each other: what
    tests/test_gpu_orient_chain.py uses to build a source whose oriented frame is a given one."""
    p = (np.arange(5 * 7, dtype=np.int64) * 37 % 251).astype(np.uint8).reshape(5, 7)
    for o, inv in ORIENT_INVERSE.items():
        assert (orient_plane(orient_plane(p, o), inv) == p).all()
        assert (orient_plane(orient_plane(p, inv), o) == p).all()
    assert not (orient_plane(orient_plane(p, 3), 3).shape == p.shape and (orient_plane(orient_plane(p, 3), 3) == p).all())
    f = (np.arange(i420_frame_bytes(7, 5, "420"), dtype=np.int64) * 41 % 253).astype(np.uint8)
    for o, inv in ORIENT_INVERSE.items():
        ow, oh = oriented_size(7, 5, o)
        assert (orient_frame(orient_frame(f, 7, 5, "420", o), ow, oh, "420", inv) == f).all()


ORIENT_INVERSE = {1: 1, 2: 2, 3: 5, 4: 4, 5: 3, 6: 6, 7: 7}


@pytest.mark.parametrize("args,want", [
    # crop in place from 300-byte rows: UA; MJG_UNALIGNED_FETCH=0: the plain kernel
    ((300, 200, "420", (2, 6, 250, 150), "420", None, None, None), (IN_PLACE | UA, (NONE, NONE), False)),
    ((300, 200, "444", (3, 5, 250, 150), "444", None, None, None), (IN_PLACE | UA, (NONE, NONE), False)),
    # 256x160 4:2:0: offsets 16 * 256 + 16, 40960 + 8 * 128 + 8, + 10240; strides 256, 128; 61440 a frame
    ((256, 160, "420", (16, 16, 224, 128), "420", None, None, None), (IN_PLACE, (NONE, NONE), False)),
    ((256, 160, "420", (0, 16, 256, 128), "420", None, None, None), (IN_PLACE, (NONE, NONE), False)),
    ((256, 160, "420", (16, 16, 200, 100), "420", None, None, None), (IN_PLACE, (NONE, NONE), False)),
    ((256, 160, "420", (8, 16, 224, 128), "420", None, None, None), (IN_PLACE | UA, (NONE, NONE), False)),  # chroma x = 4
    ((256, 160, "420", None, "420", None, None, None), (IN_PLACE, (NONE, NONE), False)),
    ((130, 66, "420", (0, 0, 130, 66), "420", None, None, None), (IN_PLACE, (NONE, NONE), False)),  # no crop: never UA
    # pad only, from whole frames and from a crop
    ((200, 84, "420", None, "420", None, None, (26, 28, 250, 140)), (0, (PADCOPY, PADCOPY), False)),
    ((300, 200, "420", (2, 6, 200, 84), "420", None, None, (26, 28, 250, 140)), (0, (PADCOPY, PADCOPY), False)),
    ((200, 84, "420", None, "420", None, None, (0, 0, 200, 84)), (IN_PLACE, (NONE, NONE), False)),  # the trivial pad
    # -pix_fmt under a crop: luma by the rectangle copy
    ((300, 200, "444", (3, 5, 251, 151), "420", None, None, None), (0, (COPY, TILE), True)),
    ((300, 200, "444", None, "422", None, None, None), (0, (COPY, TILE), False)),
    # the shapes of tests/test_gpu_scale_stream.py and tests/test_gpu_pad.py, as they run there
    ((256, 160, "420", None, "420", 32, 20, (6, 10, 48, 36)), (0, (STREAM, TILE), False)),
    ((1100, 700, "420", None, "420", 200, 100, (28, 22, 256, 144)), (0, (STREAM, STREAM), False)),  # chroma 5.5:1
    ((384, 240, "444", None, "420", 128, 80, None), (0, (TILE, STREAM), False)),
    ((320, 200, "420", (30, 20, 262, 151), "420", 49, 28, None), (0, (TILE, TILE), False)),
    ((640, 400, "420", (30, 20, 523, 301), "420", 97, 55, None), (0, (STREAM, TILE), False)),
    ((1000, 600, "420", None, "420", 500, 300, (6, 10, 512, 320)), (0, (TILE, TILE), False)),
])
def test_predict_paths(args, want):
    assert cg.predict_paths(*args) == want


def test_predict_paths_switches():
    a = (300, 200, "420", (2, 6, 250, 150), "420", None, None, None)
    assert cg.predict_paths(*a, unaligned_fetch=False) == (IN_PLACE, (NONE, NONE), False)
    b = (300, 200, "444", (3, 5, 251, 151), "420", None, None, None)
    assert cg.predict_paths(*b, plane_copy=False) == (0, (TILE, TILE), False)


PREDICT_ROWS = test_predict_paths.pytestmark[0].args[1]


@pytest.mark.parametrize("args,want", PREDICT_ROWS)
def test_predict_paths_with_an_orientation(args, want):
    """orient = 0 is the function as it was; a mirroring map changes nothing downstream; under a
    transposing map the same oriented frame comes from an h x w source (4:2:2 is not transposed)."""
    w, h, src = args[:3]
    for o in (0, 2, 4, 6):
        assert cg.predict_paths(*args, orient=o) == want
    if src != "422":
        for o in (1, 3, 5, 7):
            assert cg.predict_paths(h, w, *args[2:], orient=o) == want


def test_predict_paths_of_the_oriented_shapes():
    """tests/test_gpu_orient_chain.py: an orientation alone is read in place and is no crop (never
    UA, whatever the sizes); the crops out of the oriented 300x200, 400x64 and 256x160."""
    for (w, h, c) in ORIENT_SHAPES:
        for o in ((2, 4, 6) if c == "422" else range(1, 8)):
            assert cg.predict_paths(w, h, c, None, c, None, None, None, orient=o) == (IN_PLACE, (NONE, NONE), False)
    for o in (3, 5):
        for rect in ((2, 6, 250, 150), (2, 6, 234, 150)):
            a = (200, 300, "420", rect, "420", None, None, None)
            assert cg.predict_paths(*a, orient=o) == (IN_PLACE | UA, (NONE, NONE), False)
            assert cg.predict_paths(*a, unaligned_fetch=False, orient=o) == (IN_PLACE, (NONE, NONE), False)
    assert cg.predict_paths(300, 200, "444", (3, 5, 250, 150), "444", None, None, None, orient=6)[0] == IN_PLACE | UA
    assert cg.predict_paths(64, 400, "444", (3, 5, 350, 40), "444", None, None, None, orient=1)[0] == IN_PLACE | UA
    assert cg.predict_paths(160, 256, "420", (16, 16, 224, 128), "420", None, None, None, orient=7)[0] == IN_PLACE
    assert cg.predict_paths(160, 256, "420", (8, 16, 224, 128), "420", None, None, None, orient=7)[0] == IN_PLACE | UA
    # the sws stage behind an orientation: the source is the oriented frame turned back
    assert cg.predict_paths(200, 300, "444", (3, 5, 251, 151), "420", None, None, None, orient=5) == (0, (COPY, TILE), True)
    assert cg.predict_paths(84, 200, "420", None, "420", None, None, (26, 28, 250, 140), orient=1)[1] == (PADCOPY, PADCOPY)
    assert cg.predict_paths(700, 1100, "420", None, "420", 200, 100, (28, 22, 256, 144), orient=7)[1] == (STREAM, STREAM)


def test_orient_sweep_draw_and_its_floors():
    """The sweep of tests/test_gpu_orient_chain.py, counted without a GPU: the configurations of
    sweep_configs for its seed, each with a map (a mirroring one on 4:2:2), and per part of 30
    exactly the feature counts the GPU test uses as floors, every one at least 1."""
    seed = cg.ORIENT_SWEEP_SEED
    cfgs = cg.orient_sweep_configs(seed, 120)
    assert len(cfgs) == 120 and cfgs == cg.orient_sweep_configs(seed, 120)
    assert [tuple(c[:-1]) for c in cfgs] == [tuple(c) for c in cg.sweep_configs(seed, 120)]
    for c in cfgs:
        assert 1 <= c.orient <= 7 and not (c.src == "422" and c.orient & 1)
        assert cg.source_size(c) == ((c.h, c.w) if c.orient & 1 else (c.w, c.h))
    parts = [cg.orient_predicted_counts(cfgs[i * 30:(i + 1) * 30]) for i in range(4)]
    assert parts == cg.ORIENT_SWEEP_FLOORS
    assert all(set(p) == set(cg.ORIENT_FEATURES) and min(p.values()) >= 1 for p in parts)
    total = {k: sum(p[k] for p in parts) for k in cg.ORIENT_FEATURES}
    assert total == {"map1": 12, "map2": 22, "map3": 15, "map4": 20, "map5": 15, "map6": 23, "map7": 13,
                     "luma_t0_past_one_wg": 51, "luma_t1_past_one_wg": 37, "orient_alone_in_place": 9,
                     "crop_in_place_ua": 11, "crop_in_place_aligned": 11, "sws_reads_orient": 89,
                     "host": 31, "dev_odd": 36, "segments": 25, "merged": 28}


def test_tile_lds_of_a_shape_the_suite_names():
    """tests/test_gpu_scale_stream.py: 262x151 -> 49x28 is one tile of 62,464 B."""
    assert cg.tile_lds(262, 151, 49, 28) == 62464
    assert cg.tile_lds(256, 160, 32, 20) > 64 * 1024


def test_sweep_draw_and_its_floors():
    """The sweep of tests/test_gpu_chain.py, counted without a GPU: 120 configurations that keep
    the rules (no up-sampling, the crop inside the frame at the source's sub-sampling, a padded
    picture at the encoded format's), and per part of 30 exactly the feature counts the GPU tests
    use as floors."""
    cfgs = cg.sweep_configs(cg.SWEEP_SEED, 120)
    assert len(cfgs) == 120 and cfgs == cg.sweep_configs(cg.SWEEP_SEED, 120)
    for c in cfgs:
        assert 64 <= c.w <= 420 and 48 <= c.h <= 260 and c.dst in cg.DOWN[c.src]
        iw, ih = c.w, c.h
        if c.rect:
            x, y, iw, ih = c.rect
            shs, svs = cg.CHROMA_SHIFTS[c.src]
            assert 0 <= x <= c.w - iw and 0 <= y <= c.h - ih and x % (1 << shs) == 0 and y % (1 << svs) == 0
        if c.dw:
            assert 2 * c.dw <= iw + 1 and 6 * c.dw >= iw - 3 or c.dw == 8
            assert 2 * c.dh <= ih + 1 and 6 * c.dh >= ih - 3 or c.dh == 8
        if c.pad:
            hs, vs = cg.CHROMA_SHIFTS[c.dst]
            pw, ph = c.dw or iw, c.dh or ih
            assert not ((c.pad[0] | c.pad[2] | pw) & ((1 << hs) - 1) or (c.pad[1] | c.pad[3] | ph) & ((1 << vs) - 1))
            assert c.pad[0] + pw <= c.pad[2] and c.pad[1] + ph <= c.pad[3] and c.pad[2:] != (pw, ph)
        assert c.nframes in (1, 2) and (c.nframes == 2 or c.submit in ("host", "dev_odd"))
    parts = [cg.predicted_counts(cfgs[i * 30:(i + 1) * 30]) for i in range(4)]
    assert parts == cg.SWEEP_FLOORS
    assert all(v >= 1 for p in parts for v in p.values())
    total = {k: sum(p[k] for p in parts) for k in cg.FEATURES}
    assert total == {"crop_in_place_ua": 14, "crop_in_place_aligned": 9, "rect_copy": 9, "pad_copy": 13,
                     "pad_with_scale": 30, "stream": 7, "host": 31, "dev_odd": 39, "segments": 28, "merged": 22}


# One plane shape (source -> destination) per kernel instantiation family that build_plan can pick
# for a resized plane and that some filter reaches: tests/test_gpu_chain.py runs each as 4:4:4 in
# and out (luma and chroma the same plane size, so both take the arm), tv range (the arm's range 1
# and range 2 instantiations) and full range (its range 0 one).
ARM_SHAPES = [
    ((64, 48, 32, 24), ("tile", (8, 5, 64), True)),      # 2:1, the 64-row tile
    ((12, 24, 6, 12), ("tile", (8, 5, 32), True)),       # 2:1 from a source narrower than 16
    ((64, 48, 128, 96), ("tile", (4, 3, 32), False)),    # 1:2 up: the full-weight edge tap is no D4 coefficient
    ((64, 24, 63, 48), ("tile", (4, 3, 32), True)),      # h 64:63 down (4 taps, none of full weight), v 1:2 up
    ((96, 72, 32, 24), ("tile", (0, 0, 32), True)),      # 3:1: 12 h taps, the run-time tap counts
    ((64, 48, 64, 24), ("tile", (0, 0, 32), False)),     # h identity (one tap of 16384), v 2:1
    ((256, 160, 32, 20), ("stream", True, True)),        # 8:1
    ((40, 1000, 80, 17), ("stream", False, True)),       # h 1:2 up, 234 v taps
    ((3968, 64, 65, 16), ("stream", True, False)),       # 244 h taps: the strip's h coefficients do not fit LDS
]
# The arms build_plan can name that no filter reaches, and why.  Of all h filters between widths
# 1..399 (mjg_sws_filter) only 4-tap ones hold a coefficient outside D4's range (16384: an
# upscale's full-weight edge tap, the identity); a filter of more taps spreads its weight.
ARMS_NOT_REACHED = {
    ("tile", (8, 5, 64), False): "an 8-tap h filter has no coefficient past D4's range",
    ("tile", (8, 5, 32), False): "the same filters",
    ("stream", False, False): "coefficients past D4's range come with 4 h taps, whose 512 B of rows always fit LDS",
}


def test_arm_shapes_cover_every_reachable_arm():
    """Each shape of ARM_SHAPES reaches the arm it is listed for (scale_variant, from the library's
    own filters), and with ARMS_NOT_REACHED they are every [tile shape or hcl][d4] cell of the host's
    selection: 4 tile shapes and 2 stream forms, each with and without D4."""
    for shape, arm in ARM_SHAPES:
        assert cg.scale_variant(*shape) == arm, shape
        assert cg.plane_path(*shape, False) == (STREAM if arm[0] == "stream" else TILE)
    every = {("tile", t, d4) for t in ((8, 5, 64), (8, 5, 32), (4, 3, 32), (0, 0, 32)) for d4 in (False, True)}
    every |= {("stream", d4, hcl) for d4 in (False, True) for hcl in (False, True)}
    reached = {arm for _, arm in ARM_SHAPES}
    assert len(reached) == len(ARM_SHAPES) and not reached & set(ARMS_NOT_REACHED)
    assert reached | set(ARMS_NOT_REACHED) == every
    assert cg.scale_variant(64, 48, 64, 48) == ("copy",)
    assert cg.scale_variant(64, 48, 32, 24, force_stream=True)[0] == "stream"
    # everything a case moves stays small: at most a few hundred KB of source planes
    assert max(3 * s[0] * s[1] for s, _ in ARM_SHAPES) <= 800 * 1024


def test_copy_and_pad_cells_are_reached_by_the_gpu_tests():
    """The ten instantiations k_plane_copy<RANGE, RECT> and k_pad_plane<RANGE, COPY> (+ <0, false>),
    and a configuration of the GPU tests that launches each (restated from those tests)."""
    pad = (26, 28, 250, 140)
    reached = set()
    for full in (False, True):
        # tests/test_gpu_chain.py: PAD_COPY's first row, the rectangle copy, the border around a scaled picture
        reached |= cg.copy_pad_cells(200, 84, "420", None, "420", None, None, pad, full)
        reached |= cg.copy_pad_cells(300, 200, "444", (3, 5, 251, 151), "420", None, None, None, full)
        reached |= cg.copy_pad_cells(1100, 700, "420", None, "420", 200, 100, (28, 22, 256, 144), full)
        # tests/test_gpu_chroma_resample.py: a down-sampling pair without a resize (luma: the plain copy)
        reached |= cg.copy_pad_cells(33, 17, "444", None, "420", None, None, None, full)
        # tests/test_gpu_chain.py CHROMA_COPY: 4:2:0 -> 4:4:4 at half size, chroma keeps its size
        for rect in CHROMA_COPY_RECTS:
            reached |= cg.copy_pad_cells(300, 200, "420", rect, "444", *CHROMA_COPY_SIZE[rect], None, full)
    assert reached == ({("copy", r, rect) for r in (0, 1, 2) for rect in (False, True)}
                       | {("pad", r, True) for r in (0, 1, 2)} | {("pad", 0, False)})
    # without the CHROMA_COPY cases no GPU test reaches k_plane_copy<2, ..>: the up-sampling pair of
    # tests/test_gpu_chroma_resample.py keeps the frame size, so its chroma planes are scaled 1:2
    assert cg.copy_pad_cells(34, 18, "420", None, "444", None, None, None, False) == {("copy", 1, False)}


# tests/test_gpu_chain.py CHROMA_COPY: the rectangles of the 300x200 4:2:0 source (None: whole
# frames) and the 4:4:4 size at which the chroma planes keep theirs
CHROMA_COPY_RECTS = (None, (2, 6, 250, 150))
CHROMA_COPY_SIZE = {None: (150, 100), (2, 6, 250, 150): (125, 75)}


# ------------------------------------------------------------------ the deinterlacer's and the sharpen's launches
def test_filter_constants_parsed_from_the_kernel_source():
    """The hand values below assume 256 pieces of 16 bytes a deinterlacer workgroup and 64 x 32 tiles."""
    assert (cg.DEINT_THREADS, cg.SHARP_TILE_W, cg.SHARP_TILE_H) == (256, 64, 32)


@pytest.mark.parametrize("args,want", [
    # 130 x 66 = 8580 B: 536 pieces and 4 bytes, 3 workgroups (256 + 256 + 24).  16 and 130 share the factor 2: over 65
    # pieces (8 rows) the piece's column takes every even value once, and it runs over the row end from column 116 on
    # (116..128: 7 of 65); 536 = 8 * 65 + 16, and of the last 16 pieces (from row 64, column 0) the one at column 128
    ((130, 66), (3, 536, 8 * 7 + 1, 0, 4)),
    # 4100 x 5 = 20500 B: 1281 pieces and 4 bytes, 6 workgroups (the sixth holds one piece); 4100 = 16 * 256 + 4, so the
    # ends of rows 0, 1 and 2 (4100, 8200, 12300) fall inside a piece and the end of row 3 (16400 = 16 * 1025) between two
    ((4100, 5), (6, 1281, 3, 0, 4)),
    # 33 x 17 = 561 B at an odd address (15 bytes to the boundary, as frame 1 of a 4:4:4 sequence has): 34 pieces after
    # the head and 2 bytes; a piece at column c of a 33-byte row runs over its end from c = 18 on.  16 and 33 are coprime,
    # so pieces 0..32 (columns (15 + 16 k) % 33) take every column once, 15 of them in 18..32; piece 33 is at column 15 again
    ((33, 17, 15), (1, 34, 15, 15, 2)),
    ((33, 17), (1, 35, 15, 0, 1)),
    ((3, 3, 7), (1, 0, 0, 7, 2)),       # smaller than a piece: threads 0..15 of the one workgroup make every byte
])
def test_deint_span(args, want):
    span = cg.deint_span(*args)
    assert tuple(span) == want
    # the same by walking every byte of the plane's string once (yadif_work: head, nv pieces of 16, the rest)
    w, h, head = args[0], args[1], (args[2] if len(args) > 2 else 0)
    head = min(head, w * h)
    over = sum(1 for j in range(head, w * h - 15, 16) if j // w != (j + 15) // w)
    assert span.over_row_end == over and span.head + 16 * span.pieces + span.tail == w * h and 0 <= span.tail < 16
    assert (span.wgs - 1) * cg.DEINT_THREADS < max(1, (w * h) >> 4) <= span.wgs * cg.DEINT_THREADS


def _cells_by_sharp_store(cw, ch, px, py, w, h, amount):
    """sharp_cells again, quad by quad as k_unsharp_plane's threads see them (sharp_tile and sharp_store)."""
    tw, th = cg.SHARP_TILE_W, cg.SHARP_TILE_H
    tx, ty = -(-cw // tw), -(-ch // th)
    filt = copy = short = 0
    masks = {}
    for blk in range(tx * ty):
        x0, y0 = blk % tx * tw, blk // tx * th
        f = amount != 0 and x0 < px + w and x0 + tw > px and y0 < py + h and y0 + th > py
        filt, copy = filt + f, copy + (not f)
        for idx in range(tw * th // 4):
            x, y = x0 + 4 * (idx % (tw // 4)), y0 + idx // (tw // 4)
            if x >= cw or y >= ch:
                continue
            n = min(4, cw - x)
            pic = sum(1 << k for k in range(n) if py <= y < py + h and px <= x + k < px + w)
            short += n < 4
            if f:
                masks[pic] = masks.get(pic, 0) + 1
    return cg.SharpCells(tx, ty, filt, copy, dict(sorted(masks.items())), short)


# (plane, picture, amount) -> (tx, ty, filtering tiles, copying tiles, pic masks of the filtering tiles' quads)
SHARP_CELLS = [
    # 197 = 3 * 64 + 5 columns: 49 whole quads and one of a single sample per row, 70 rows over three tile rows
    ((197, 70, 0, 0, 197, 70, 65536), (4, 3, 12, 0, {1: 70, 15: 49 * 70})),
    # the picture's columns 67..136 and rows 33..66 touch tile columns 1, 2 and tile rows 1, 2; those tiles hold
    # 128 x 64 samples = 32 quads x 64 rows = 2048 quads; per picture row (34 of them): 67 = 4 * 16 + 3 starts with the
    # last sample of a quad (8), 137 = 4 * 34 + 1 ends with the first of one (1), 17 whole quads between (68..135)
    ((201, 99, 67, 33, 70, 34, 65536), (4, 4, 4, 12, {0: 2048 - 19 * 34, 1: 34, 8: 34, 15: 17 * 34})),
    # columns 69..134 (69 = 4 * 17 + 1: samples 1..3 of a quad, 14; 135 = 4 * 33 + 3: samples 0..2, 7; 15 whole quads
    # 72..131), rows 35..67 (33 rows) in the same four tiles
    ((203, 101, 69, 35, 66, 33, 98304), (4, 4, 4, 12, {0: 2048 - 17 * 33, 7: 33, 14: 33, 15: 15 * 33})),
    # the chroma plane of 134 x 70 4:2:2: 67 = 64 + 3 columns, 16 whole quads and one of three samples per row
    ((67, 70, 0, 0, 67, 70, 32768), (2, 3, 6, 0, {7: 70, 15: 16 * 70})),
    # the chroma of the next: columns 35..99 and rows 19..51 touch tile columns 0, 1 and tile rows 0, 1 (2048 quads);
    # 35 = 4 * 8 + 3 (8), 100 = 4 * 25: the right edge falls between quads, 16 whole quads 36..99; five more tiles copy
    ((132, 68, 35, 19, 65, 33, 65536), (3, 3, 4, 5, {0: 2048 - 17 * 33, 8: 33, 15: 16 * 33})),
    # columns 70..199, rows 38..103: tile columns 1..3, tile rows 1..3, nine tiles of 512 quads; 70 = 4 * 17 + 2 (12),
    # 200 = 4 * 50, 32 whole quads 72..199, 66 rows
    ((264, 136, 70, 38, 130, 66, 65536), (5, 5, 9, 16, {0: 9 * 512 - 33 * 66, 12: 66, 15: 32 * 66})),
]


@pytest.mark.parametrize("geom,want", SHARP_CELLS, ids=["%dx%d_%dx%d+%d+%d" % (g[0], g[1], g[4], g[5], g[2], g[3])
                                                       for g, _ in SHARP_CELLS])
def test_sharp_cells(geom, want):
    """The six planes of tests/test_gpu_filter_chain.py, by hand and by walking every thread's quads."""
    cells = cg.sharp_cells(*geom)
    assert tuple(cells[:5]) == want
    assert cells == _cells_by_sharp_store(*geom)
    assert cg.sharp_cells(*geom[:6], 0)[2:5] == (0, cells.tx * cells.ty, {})      # amount 0: every tile copies


def test_sharp_cells_of_the_geometries_the_gpu_tests_encode():
    """Every plane of unsharp_ref.GPU_GEOMETRY_CHAIN is one of the table above (or the 134 x 70 luma);
    and the claim the new cases rest on: no geometry of unsharp_ref.GPU_GEOMETRY (tests/test_gpu_unsharp.py)
    has a picture edge that cuts a quad on its left (pic masks are 0, 15, or 1, 3, 7 on the right) or three
    tile columns, and one alone has a copying tile in a launch that also filters: the luma of 50 x 38 with
    the picture's rows 10..27, whose second tile row (rows 32..37) lies under the picture in a single tile
    column.  None has a copying tile to the left or right of a filtering one."""
    import unsharp_ref
    table = {g[:6] for g, _ in SHARP_CELLS} | {(134, 70, 0, 0, 134, 70)}
    for (W, H, c, px, py, w, h, us) in unsharp_ref.GPU_GEOMETRY_CHAIN:
        for g in cg.sharp_plane_geoms(W, H, c, px, py, w, h, us):
            assert g[:6] in table, g
    assert unsharp_ref.WIDE == (197, 70)
    seen = set()
    for (W, H, c, px, py, w, h, us) in unsharp_ref.GPU_GEOMETRY:
        for g in cg.sharp_plane_geoms(W, H, c, px, py, w, h, us):
            cells = cg.sharp_cells(*g)
            assert cells == _cells_by_sharp_store(*g)
            assert cells.tx <= 2
            assert not (cells.filt and cells.copy) or (g[:6] == (50, 38, 8, 10, 34, 18) and cells[:4] == (1, 2, 1, 1)), g
            assert all(m == 0 or m & 1 for m in cells.masks), (g, cells.masks)
            seen |= set(cells.masks)
    assert seen <= {0, 1, 3, 7, 15}
    new = set()
    for g, _ in SHARP_CELLS:
        new |= set(cg.sharp_cells(*g).masks)
    assert {8, 12, 14} <= new


# ------------------------------------------------------------------ the seeded sweep with a filter
def test_filter_predict_and_features():
    base = cg.Config(300, 200, "420", (6, 16, 224, 128), "420", None, None, None, False, 5, {}, "host", 3, 1)
    cfg = cg.FilterConfig(*base, 0, "bff", None)
    assert cg.filter_predict(cfg)[:2] == (IN_PLACE | UA, (NONE, NONE))
    assert cg.filter_features(cfg, *cg.filter_predict(cfg)[:2]) == {"host", "default", "deint_bff", "deint_to_in_place_ua"}
    # a sharpen runs the sws stage: the rectangle goes through k_plane_copy's RECT form, 224 = 3.5 tile columns
    cfg = cfg._replace(unsharp=cg.SHARPS[1])
    assert cg.filter_predict(cfg) == (0, (COPY, COPY), True)
    assert cg.filter_features(cfg, 0, (COPY, COPY)) == {"host", "default", "deint_bff", "deint_to_rect_copy", "sharp55_luma_only",
                                                        "sharp_from_plane_copy", "sharp_three_tile_columns"}
    # the 4:2:0 pad case of tests/test_gpu_filter_chain.py behind an orientation
    cfg = cg.FilterConfig(260, 132, "420", None, "420", 130, 66, (70, 38, 264, 136), False, 5, {"rst": True}, "segments", 3, 1,
                          5, "tff_nospatial", cg.SHARPS[2])
    assert cg.source_size(cfg) == (132, 260) and cg.encoded_geometry(cfg) == (264, 136, 70, 38, 130, 66)
    assert cg.filter_features(cfg, *cg.filter_predict(cfg)[:2]) == {
        "segments", "rst", "deint_tff_nospatial", "deint_to_orient_t1", "sharp55_all_planes", "sharp_from_pad_with_scale",
        "sharp_three_tile_columns", "sharp_copy_tile_beside_filter", "sharp_left_partial_mask"}


def test_filter_sweep_draw_and_its_floors():
    """The sweep of tests/test_gpu_filter_chain.py, counted without a GPU: the configurations of
    sweep_configs for its seed, each with a deinterlacer, a sharpen or both, and per part of 30
    exactly the feature counts the GPU test uses as floors, every one at least 1."""
    seed = cg.FILTER_SWEEP_SEED
    assert seed == 2451
    cfgs = cg.filter_sweep_configs(seed, 120)
    assert len(cfgs) == 120 and cfgs == cg.filter_sweep_configs(seed, 120)
    for c, b in zip(cfgs, cg.sweep_configs(seed, 120)):
        assert tuple(c[:11]) == tuple(b[:11]) and c.fseed == b.fseed
        assert c.deint in cg.DEINTS and c.unsharp in cg.SHARPS and (c.deint or c.unsharp)
        assert 0 <= c.orient <= 7 and not (c.src == "422" and c.orient & 1)
        if c.deint:
            assert c.nframes == 3 and c.submit in ("host", "dev_odd", "segments")
            assert c.submit == b.submit or b.submit == "merged"
        else:
            assert (c.submit, c.nframes) == (b.submit, b.nframes)
        sw, sh = cg.source_size(c)
        assert min(chroma_size(sw, sh, c.src)) >= 24      # every plane far above the deinterlacer's 3 x 3
    assert sum(1 for c in cfgs if c.orient) == 31          # about one in three of those not on a rare path
    parts = [cg.filter_predicted_counts(cfgs[i * 30:(i + 1) * 30]) for i in range(4)]
    assert parts == cg.FILTER_SWEEP_FLOORS
    assert all(set(p) == set(cg.FILTER_FEATURES) and min(p.values()) >= 1 for p in parts)
    total = {k: sum(p[k] for p in parts) for k in cg.FILTER_FEATURES}
    assert total == {"deint_None": 19, "deint_tff": 23, "deint_bff": 25, "deint_tff_nospatial": 26, "deint_bff_nospatial": 27,
                     "sharp55_luma_only": 12, "sharp55_all_planes": 16, "sharp_runtime_sizes": 34, "sharp_luma_copied": 22,
                     "deint_to_in_place_ua": 6, "deint_to_in_place_aligned": 12, "deint_to_rect_copy": 7, "deint_to_pad_copy": 9,
                     "deint_to_tile_scale": 45, "deint_to_stream": 8, "deint_to_orient_t0": 15, "deint_to_orient_t1": 9,
                     "sharp_from_tile_scale": 54, "sharp_from_stream": 8, "sharp_from_plane_copy": 14, "sharp_from_pad_copy": 9,
                     "sharp_from_pad_with_scale": 23, "sharp_three_tile_columns": 14, "sharp_copy_tile_beside_filter": 20,
                     "sharp_left_partial_mask": 23, "sharp_right_partial_mask": 21, "host": 43, "dev_odd": 36, "segments": 36,
                     "merged": 5, "default": 35, "optimal": 50, "rst": 35}


# ------------------------------------------------------------------ long submits: V in a launch of its own
def test_plane_launches_at_the_grid_limit():
    """submit_impl's launches per plane stage, by hand: U and V share a grid while 2 n <= 65535
    (n <= 32767); from 32768 frames on U and V get a launch each, of n in z."""
    assert (cg.UV_LIMIT, cg.LONG, cg.MAX_BATCH) == (65535, 32768, 65535)
    assert cg.plane_launches(1) == [("Y", 1), ("UV", 2)]
    assert cg.plane_launches(32767) == [("Y", 32767), ("UV", 65534)]
    assert cg.plane_launches(32768) == [("Y", 32768), ("U", 32768), ("V", 32768)]
    assert cg.plane_launches(65535) == [("Y", 65535), ("U", 65535), ("V", 65535)]
    assert cg.plane_launches(39999) == [("Y", 39999), ("U", 39999), ("V", 39999)]
    assert all(nz <= cg.UV_LIMIT for n in (1, 32767, 32768, 39999, 65535) for _, nz in cg.plane_launches(n))


def test_merged_frames_is_capped_as_open_caps_it():
    """slot_B = max_batch * merge: two jobs a launch (kMerge = 2 of kMaxSegs = 4), so two submits
    below the limit make one launch above it; never with a deinterlacer, without MJG_F_MERGE, past a
    quarter of free memory or where k_encode's task magic would overflow."""
    assert (cg.MERGE, cg.MAX_SEGS, cg.SLOTS, cg.SLOT_WORDS) == (2, 4, 2, 3328)
    assert cg.merged_frames(20000) == 40000 and len(cg.plane_launches(20000)) == 2 and len(cg.plane_launches(39999)) == 3
    assert cg.merged_frames(20000, merge=False) == 20000
    assert cg.merged_frames(20000, deint=True) == 20000
    assert cg.merged_frames(65535) == 131070
    assert cg.merged_frames(65535, nseg=2, nchunks=2048) == 131070       # 65535 * 2 * 2 * 2048^2 = 2^40 - 2^24
    assert cg.merged_frames(65535, nseg=2, nchunks=2049) == 65535
    # the 16 x 16 -> 8 x 8 4:2:0 context with a sharpen: one chunk a frame, 96-byte encoded frames
    per = cg.slot_frame_bytes(1, 1, 96, 384, sharp=True)
    assert per == 2 * 3328 * 4 + 3 * 96
    assert cg.merged_frames(20000, per_frame_bytes=per, free_bytes=16 << 30) == 40000      # 2.2 GB of 4 GB
    assert cg.merged_frames(20000, per_frame_bytes=per, free_bytes=8 << 30) == 20000


def test_long_frame_index_tells_the_frames_at_the_limit_apart():
    """Frame i of a long submit is base (7 i + i // 1000) % 61: frames 0, 32767, 32768 and the last
    frame are four different base frames at every frame count the GPU file uses, neighbours always
    differ, and all 61 occur on both sides of frame 32768."""
    assert cg.LONG_K == 61
    idx = cg.long_frame_index(65535)
    assert [int(idx[i]) for i in (0, 1, 999, 1000, 32767, 32768)] == [0, 7, 39, 47, 41, 48]      # 7001 = 114 * 61 + 47
    for n in (32770, 38000, 39999, 65535):
        assert len({int(idx[i]) for i in (0, 32767, 32768, n - 1)}) == 4, n
    assert int(idx[0]) != int(idx[32766]) != int(idx[32767])       # the n = 32768 and 32767 submits' ends
    assert (idx[1:] != idx[:-1]).all() and (idx[2:] != idx[:-2]).all()
    assert set(idx[:32768].tolist()) == set(idx[32768:39999].tolist()) == set(range(61))


LONG_PATHS = {
    "in_place": (IN_PLACE, (NONE, NONE)), "optimal": (IN_PLACE, (NONE, NONE)), "rst": (IN_PLACE, (NONE, NONE)),
    "scale_tv": (0, (TILE, TILE)), "scale_pc": (0, (TILE, TILE)), "scale_up_444": (0, (TILE, TILE)),
    "scale_stream": (0, (TILE, TILE)),      # (without MJG_SCALE_STREAM; with it both planes stream)
    "pix_fmt_copy": (0, (COPY, TILE)), "rect_copy": (0, (COPY, TILE)),
    "pad_copy": (0, (PADCOPY, PADCOPY)), "pad_scale": (0, (TILE, TILE)),
    "hflip": (IN_PLACE, (NONE, NONE)), "transpose": (IN_PLACE, (NONE, NONE)),
    "yadif": (IN_PLACE, (NONE, NONE)), "yadif_nospatial": (IN_PLACE, (NONE, NONE)),
    "unsharp55": (0, (COPY, COPY)), "unsharp_chroma": (0, (COPY, COPY)),
    "chain": (0, (TILE, TILE)), "scale_sharp": (0, (TILE, TILE)),
}


def test_long_cases_reach_the_paths_they_are_listed_for():
    """The shapes of tests/test_gpu_long_submit.py, each the smallest on which its stage exists: the
    kernel family of either plane, the three tile instantiations, the stream form, the rectangle
    form of the copy, both forms of the pad with a V offset that is no plane start, the
    deinterlacer's 3 x 3 floor, and the sharpen's two cells."""
    assert set(cg.LONG_CASES) == set(LONG_PATHS)
    for name, c in cg.LONG_CASES.items():
        enc_path, paths, rect_form = cg.long_predict(c)
        assert (enc_path, paths) == LONG_PATHS[name], name
        assert rect_form == (name == "rect_copy"), name
        if c.pad:
            assert c.pad[1] >> 1 != 0 and c.pad[0] >> 1 != 0
        if c.deint:
            assert min(chroma_size(c.w, c.h, c.src)) > 3
    variants = {n: [cg.scale_variant(*s, *d, force_stream=c.stream) for s, d in cg.long_plane_sizes(c)]
                for n, c in cg.LONG_CASES.items() if not cg.long_predict(c)[0] & IN_PLACE}
    assert variants["scale_tv"] == variants["scale_pc"] == variants["pad_scale"] == variants["scale_sharp"] \
        == [("tile", (8, 5, 64), True), ("tile", (0, 0, 32), True)]
    assert variants["scale_up_444"] == [("tile", (4, 3, 32), False)] * 2
    assert variants["scale_stream"] == [("stream", True, True)] * 2
    assert variants["pix_fmt_copy"] == variants["rect_copy"] == [("copy",), ("tile", (0, 0, 32), True)]
    assert variants["pad_copy"] == variants["unsharp55"] == variants["unsharp_chroma"] == [("copy",), ("copy",)]
    assert variants["chain"] == [("tile", (8, 5, 32), True), ("tile", (0, 0, 32), True)]
    assert cg.LONG_CASES["hflip"].orient == 2 and cg.orient_cells(2)[:2] == (False, True)
    assert cg.LONG_CASES["transpose"].orient == 1 and cg.orient_cells(1)[0] is True
    assert chroma_size(24, 8, "420") == (12, 4)
    # the sharpen's cells: <5, 5> filtering every plane; 5:5 at amount 0 copying the luma, 3:5 on U and V
    for name, want in (("unsharp55", (1, 1)), ("unsharp_chroma", (0, 1))):
        us = cg.LONG_CASES[name].unsharp
        luma, chroma = (cg.sharp_cells(*g) for g in cg.sharp_plane_geoms(8, 8, "420", 0, 0, 8, 8, us))
        assert (luma.filt, luma.copy, chroma.filt, chroma.copy) == (want[0], 1 - want[0], want[1], 1 - want[1]), name
    assert cg.LONG_CASES["unsharp55"].unsharp[:2] == cg.LONG_CASES["unsharp55"].unsharp[3:5] == (5, 5)
    assert cg.LONG_CASES["unsharp_chroma"].unsharp == (5, 5, 0.0, 3, 5, 0.7)
    assert cg.enc_geom(8, 32, "420", True).nseg == 2 and cg.enc_geom(8, 32, "420", True, cg.LONG).ntasks == 65536


LONG_STAGE_PATHS = {
    "dn": (IN_PLACE, (NONE, NONE)), "dn_yadif_segs": (IN_PLACE, (NONE, NONE)),
    "tile_a": (0, (COPY, COPY)), "tile_b": (0, (TILE, TILE)), "tile_c": (0, (COPY, COPY)), "tile_segs": (0, (COPY, COPY)),
    "lut_out": (0, (TILE, TILE)), "cmat_chain": (0, (TILE, TILE)), "full_chain": (0, (TILE, TILE)),
}


def test_long_stage_cases_split_u_and_v_and_reach_their_paths():
    """The shapes of tests/test_gpu_long_stages.py: every submit has three launches a plane stage, the
    tile's launch is split or paired by its sheets (32,768 and 32,769 split, 20,000 paired), the paths
    are what the context must report, and the pads put V's offset off a plane start."""
    assert set(cg.LONG_STAGE_CASES) == set(LONG_STAGE_PATHS)
    for name, c in cg.LONG_STAGE_CASES.items():
        assert [p for p, _ in cg.plane_launches(c.n)] == ["Y", "U", "V"], name
        assert c.n <= cg.MAX_BATCH and (c.segs is None or (sum(c.segs) == c.n and len(c.segs) == cg.MAX_SEGS)), name
        assert cg.long_stage_predict(c) == LONG_STAGE_PATHS[name], name
        if c.geom.pad:
            assert c.geom.pad[1] >> 1 == 3 and c.geom.pad[0] >> 1 != 0
        if c.geom.deint:
            assert min(chroma_size(c.geom.w, c.geom.h, c.geom.src)) > 3
        assert not (c.sheet and c.denoise)      # open refuses a denoiser in front of a sheet
    m = {name: cg.sheets_out(c) for name, c in cg.LONG_STAGE_CASES.items() if c.sheet}
    assert m == {"tile_a": 32768, "tile_b": 20000, "tile_c": 32768, "tile_segs": 32769}
    assert {name: len(cg.plane_launches(v)) for name, v in m.items()} == {"tile_a": 3, "tile_b": 2, "tile_c": 3, "tile_segs": 3}
    a = cg.LONG_STAGE_CASES["tile_a"]
    assert cg.sheets_out(a, cg.LONG - 1) == cg.LONG - 1 and len(cg.plane_launches(cg.LONG - 1)) == 2      # the paired run beside it
    assert cg.LONG_STAGE_CASES["tile_c"].n % 2 == 1      # the last sheet is partial
    s = cg.LONG_STAGE_CASES["tile_segs"]
    firsts = [sum((k + 1) // 2 for k in s.segs[:i]) for i in range(len(s.segs))]
    assert sum(k % 2 for k in s.segs) >= 2 and firsts[3] == cg.LONG - 1
    y = cg.LONG_STAGE_CASES["dn_yadif_segs"]
    assert y.segs == (12345, 20422, 3000, 2233) and sum(y.segs[:2]) == cg.LONG - 1      # test_gpu_long_submit's yadif split
    variants = {n: [cg.scale_variant(*sz, *d) for sz, d in cg.long_plane_sizes(c.geom)]
                for n, c in cg.LONG_STAGE_CASES.items() if LONG_STAGE_PATHS[n][1] == (TILE, TILE)}
    assert all(v == [("tile", (8, 5, 64), True), ("tile", (0, 0, 32), True)] for v in variants.values()) and len(variants) == 4


# ------------------------------------------------------------------ the table stage's launches
def test_lut_span_by_hand():
    """200 x 100 at (5, 7) of a 208 x 120 4:4:4 canvas: rows 208 apart, a gap of 8 between a row's end
    and the next one's start, so no piece lies between two rows; the span is 99 * 208 + 200 bytes."""
    luma, chroma = cg.lut_plane_geoms(208, 120, "444", 5, 7, 200, 100)
    assert luma == (200, 100, 208, 7 * 208 + 5) == (200, 100, 208, 1461)
    assert chroma == (200, 100, 208, 208 * 120 + 1461)
    assert (-1461) & 15 == 11 and (208 * 120) % 16 == 0 and (3 * 208 * 120) % 16 == 0
    nb = 99 * 208 + 200
    assert nb == 20792 and nb >> 4 == 1299 and (nb - 11) >> 4 == 1298
    sp = cg.lut_span(200, 100, 208, 11)
    assert cg.LUT_PER_WG == 1024 and (sp.wgs, sp.head, sp.tail) == (2, 11, nb - 11 - 16 * 1298) == (2, 11, 13)
    assert sp.whole + sp.over_row_end == 1298 and sp.skipped == sp.late_skipped == 0
    # 208 = 13 pieces: every row end (span bytes 200..207 of a row) lies inside one piece or on the seam of two,
    # counted here from the rows instead of from the pieces
    over = set()
    for r in range(100):
        for j in range(r * 208 + 200, r * 208 + 208):      # the gap behind row r; the pieces that hold a byte of it
            if j - 11 >= 0 and (j - 11) // 16 < 1298:
                over.add((j - 11) // 16)
    assert len(over) == sp.over_row_end == 198 and sum(1 for k in over if k >= 1024) == sp.late_over == 42
    assert sp.whole == 1100
    # flat: rows fold into one; the kernel's own piece count is one less behind a head
    assert cg.lut_span(130, 66, 130) == cg.LutSpan(1, 536, 0, 0, 0, 0, 0, 4)
    assert cg.lut_span(256, 160, 256) == cg.LutSpan(3, 2560, 0, 0, 0, 0, 0, 0)
    assert cg.lut_span(301, 203, 301, 13) == cg.LutSpan(4, 3818, 0, 0, 0, 0, 13, 2)
    assert cg.lut_span(3, 3, 3, 15) == cg.LutSpan(1, 0, 0, 0, 0, 0, 9, 0)      # all head
    # the largest canvas of tests/test_gpu_eq.py: 159 pieces, one workgroup
    assert (31 * 80 + 64) >> 4 == 159 and cg.lut_span(64, 32, 80).wgs == 1 and cg.lut_span(64, 32, 80).late_over == 0


def test_lut_span_of_the_canvases_the_gpu_tests_encode():
    """Cases 1 to 4 of tests/test_gpu_eq_chain.py."""
    # the 4:2:0 pad geometry: 130 x 66 at (70, 38) of 264 x 136; chroma 65 x 33 at (35, 19) of 132 x 68
    luma, chroma = cg.lut_plane_geoms(264, 136, "420", 70, 38, 130, 66)
    assert luma == (130, 66, 264, 38 * 264 + 70) and chroma == (65, 33, 132, 264 * 136 + 19 * 132 + 35)
    sp = cg.lut_out_spans(264, 136, "420", 70, 38, 130, 66)
    assert sp[(0, 0)] == cg.LutSpan(2, 495, 98, 487, 5, 22, 10, 0) and 65 * 264 + 130 == 17290
    assert sp[(1, 0)] == sp[(2, 0)] == cg.LutSpan(1, 108, 56, 104, 0, 0, 1, 0)
    # 500 x 280 at (12, 14) of 520 x 300: the chroma gap of 10 skips nothing; at (20, 14) of 540 x 300 it does
    sp = cg.lut_out_spans(520, 300, "420", 12, 14, 500, 280)
    assert sp[(0, 0)] == cg.LutSpan(9, 8540, 418, 140, 372, 124, 4, 8)
    assert sp[(1, 0)] == cg.LutSpan(3, 2065, 208, 0, 114, 0, 14, 8) and sp[(2, 0)] == cg.LutSpan(3, 2065, 209, 0, 114, 0, 6, 0)
    sp = cg.lut_out_spans(540, 300, "420", 20, 14, 500, 280)
    assert all(sp[(p, 0)].wgs == 3 and sp[(p, 0)].late_skipped >= 1 and sp[(p, 0)].late_over >= 1 for p in (1, 2))
    # flat, and flat on odd frame bytes
    assert set(cg.lut_out_spans(256, 160, "444", 0, 0, 256, 160, 3).values()) == {cg.LutSpan(3, 2560, 0, 0, 0, 0, 0, 0)}
    sp = cg.lut_out_spans(301, 203, "420", 0, 0, 301, 203, 3)
    assert [sp[(0, f)][-2:] for f in range(3)] == [(0, 15), (13, 2), (10, 5)] and sp[(1, 1)].whole == 961
    # a pad with rows as wide as the picture is flat
    assert cg.lut_plane_geoms(64, 48, "420", 0, 8, 64, 32)[0][:3] == (64, 32, 64) and cg.lut_span(64, 32, 64).over_row_end == 0


# ------------------------------------------------------------------ the seeded sweep with a table
def test_eq_predict_and_features():
    base = cg.Config(300, 200, "420", (6, 16, 224, 128), "420", None, None, None, False, 5, {}, "host", 3, 1)
    cfg = cg.EqConfig(*base, 0, "bff", None, "perm", None)
    assert cg.eq_predict(cfg)[:2] == (IN_PLACE | UA, (NONE, NONE))
    assert cg.eq_features(cfg, *cg.eq_predict(cfg)[:2]) == {"host", "default", "in_perm", "in_place_d_deint", "read_in_place_ua"}
    # slot "out" runs the sws stage as a sharpen does: the rectangle goes through k_plane_copy's RECT form
    cfg = cfg._replace(lut_out="perm_id_y", deint=None)
    assert cg.eq_predict(cfg) == (0, (COPY, COPY), True)
    assert cg.eq_features(cfg, 0, (COPY, COPY)) == {"host", "default", "in_perm", "out_perm_id_y", "both_slots", "in_to_d_lut",
                                                    "d_lut_host", "read_rect_copy", "read_plane_copy", "out_flat"}
    # the 4:2:0 pad case behind an orientation, a sharpen behind slot "out"; with an identity Y only the chroma counts
    cfg = cg.EqConfig(260, 132, "420", None, "420", 130, 66, (70, 38, 264, 136), False, 5, {"rst": True}, "segments", 3, 1,
                      5, "tff_nospatial", cg.SHARPS[2], "perm_id_uv", "perm")
    assert cg.eq_features(cfg, *cg.eq_predict(cfg)[:2]) == {
        "segments", "rst", "in_perm_id_uv", "out_perm", "both_slots", "in_place_d_orient", "read_k_scale", "out_strided",
        "out_strided_past_one_wg", "out_late_over", "out_late_skipped", "out_sharp_behind", "out_strided_v_second_slot"}
    # (65 x 33 at a stride of 132 behind a head of 1: 268 pieces, piece 256 at column 5 of row 31 is whole)
    assert (1 + 16 * 256) % 132 == 5 and (33 * 132 - 67 - 1) >> 4 == 268
    assert "out_strided_past_one_wg" not in cg.eq_features(cfg._replace(lut_out="perm_id_y"), *cg.eq_predict(cfg)[:2])


def test_eq_sweep_draw_and_its_floors():
    """The sweep of tests/test_gpu_eq_chain.py, counted without a GPU: the configurations of sweep_configs
    for its seed, each with a table in at least one slot, and per part exactly the feature counts the GPU
    test uses as floors, every one at least 1."""
    seed, count = cg.EQ_SWEEP_SEED, cg.EQ_SWEEP_COUNT
    assert seed == 168 and count % 4 == 0
    cfgs = cg.eq_sweep_configs(seed, count)
    assert len(cfgs) == count and cfgs == cg.eq_sweep_configs(seed, count)
    for c, b in zip(cfgs, cg.sweep_configs(seed, count)):
        assert tuple(c[:11]) == tuple(b[:11]) and c.fseed == b.fseed
        assert c.lut_in in cg.LUT_KINDS and c.lut_out in cg.LUT_KINDS and (c.lut_in or c.lut_out)
        assert c.deint in cg.DEINTS and c.unsharp in cg.SHARPS
        assert 0 <= c.orient <= 7 and not (c.src == "422" and c.orient & 1)
        if c.deint:
            assert c.nframes == 3 and c.submit in ("host", "dev_odd", "segments")
        else:
            assert (c.submit, c.nframes) == (b.submit, b.nframes)
        enc_path = cg.eq_predict(c)[0]
        assert not (enc_path & IN_PLACE and (c.lut_out or c.unsharp))      # what k_encode reads in place has slot "in" only
    per = count // 4
    parts = [cg.eq_predicted_counts(cfgs[i * per:(i + 1) * per]) for i in range(4)]
    assert parts == cg.EQ_SWEEP_FLOORS
    assert all(set(p) == set(cg.EQ_FEATURES) and min(p.values()) >= 1 for p in parts)
    assert len(cg.EQ_FEATURES) == 38 and len(set(cg.EQ_FEATURES)) == 38
