"""Device-free geometry of the encoder for the GPU tests of the filter chain
(tests/test_chain_geom.py, tests/test_gpu_chain.py): a restatement, from the sizes alone, of what
open_ctx (csrc/api.hip) derives, so that a test can assert *before* it opens a context that its
shape reaches the path it means to check.

  - enc_geom / unit_starts: k_encode's segments, chunks and tasks, and the (frame, segment,
    chunk) at which each work unit of kBatch tasks starts (a unit that starts at chunk != 0
    recomputes its DC predictors from pixel rows: carry_row);
  - copy_span: workgroups and vector slots a plane of n bytes takes in k_plane_copy / k_pad_plane;
  - orient_span / orient_cells: the tiles and workgroups k_orient_plane takes for a source plane, and
    its instantiation (plan_orient), for tests/test_gpu_orient_chain.py;
  - scale_variant / copy_pad_cells: the kernel instantiation build_plan picks for a plane;
  - deint_span / sharp_cells: the workgroups, pieces and head / tail bytes k_yadif_plane takes for a
    plane, and the tiles, `pic` masks and short quads of k_unsharp_plane's launch, for
    tests/test_gpu_filter_chain.py; filter_sweep_configs and its family: that file's seeded sweep;
  - lut_span / lut_plane_geoms / lut_out_spans: the workgroups, the whole pieces, those over a row end
    and those skipped between two rows (and how many of each lie in workgroups blk >= 1), head and
    tail bytes of one (plane, frame) of k_lut_plane, and slot "out"'s rectangles as plan_lut sets
    them, for tests/test_gpu_eq_chain.py; eq_sweep_configs and its family: that file's seeded sweep;
  - plane_launches / merged_frames: the launches submit_impl makes per plane stage for a launch of
    n frames (U and V apart past 2 n <= 65535) and the frames a merged launch may carry;
    LONG_CASES and its family: the shapes of tests/test_gpu_long_submit.py; LONG_STAGE_CASES: those of
    tests/test_gpu_long_stages.py;
  - predict_paths: what mjg_debug_encode_path and mjg_debug_scale_path will report for an
    orient / crop / -pix_fmt / scale / pad configuration (the rules of plan_geometry and
    plan_plane_scale; the filters come from the library's own device-free mjg_sws_filter).

kBatch, kCopyThreads, kCopyVecs, kDeintThreads, the orientation's and the sharpen's tile and the tile kernel's constants are parsed from the kernel
sources, so a change there moves these values and a hollowed-out test fails its precondition."""
import os
import re
from collections import namedtuple

from ffmpeg_distributed_amd import _lib
from ffmpeg_distributed_amd.encoder import CHROMA_SHIFTS, chroma_size

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ffmpeg_distributed_amd", "csrc")


def _const(path, name):
    with open(os.path.join(_CSRC, path)) as f:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", f.read())
    assert m, (path, name)
    return int(m.group(1))


K_BATCH = _const("kernels.hip", "kBatch")
COPY_THREADS = _const("scale.hip", "kCopyThreads")
COPY_VECS = _const("scale.hip", "kCopyVecs")
SCALE_TILE_W = _const("scale.hip", "kScaleTileW")
SCALE_LOAD_ROWS = _const("scale.hip", "kScaleLoadRows")
SCALE_ALIAS_WORDS = _const("scale.hip", "kScaleAliasWords")
STREAM_THREADS = _const("scale.hip", "kStreamThreads")
STREAM_MAX_PIECES = _const("scale.hip", "kStreamMaxPieces")
STREAM_BAND = _const("scale.hip", "kStreamBand")
ORIENT_TILE = _const("scale.hip", "kOrientTile")
ORIENT_TILE_H = _const("scale.hip", "kOrientTileH")
ORIENT_WAVES = COPY_THREADS // 64  # scale.hip: kCopyThreads / 64 (tests/test_chain_geom.py checks that it still says so)

EncGeom = namedtuple("EncGeom", "mbw mbh nseg seg_blocks nchunks ntasks")


def enc_geom(w, h, chroma, rst=False, nframes=1):
    """plan_geometry's values for an encoded w x h frame in `chroma` (under a pad: the canvas)."""
    bpm = 8 if chroma == "422" else 6
    lmw = 8 if chroma == "444" else 16
    mbw, mbh = (w + lmw - 1) // lmw, (h + 15) // 16
    rst = bool(rst) and mbh > 1
    nseg = mbh if rst else 1
    seg_blocks = (mbw if rst else mbw * mbh) * bpm
    nchunks = (seg_blocks + 63) // 64
    return EncGeom(mbw, mbh, nseg, seg_blocks, nchunks, nchunks * nseg * nframes)


def unit_starts(w, h, chroma, rst=False, nframes=1):
    """[(frame, segment, chunk)] of the first task of every work unit: task t is chunk
    t % nchunks of segment (t / nchunks) % nseg of frame t / (nchunks nseg); unit u starts at
    task u kBatch (k_encode, task_pos)."""
    g = enc_geom(w, h, chroma, rst, nframes)
    out = []
    for t in range(0, g.ntasks, K_BATCH):
        seg = t // g.nchunks
        out.append((seg // g.nseg, seg % g.nseg, t % g.nchunks))
    return out


def mid_segment_units(w, h, chroma, rst=False, nframes=1):
    """The units that start inside a segment (chunk != 0)."""
    return [u for u in unit_starts(w, h, chroma, rst, nframes) if u[2] != 0]


def _mcu_tables():
    """build_tabs's kPlane / kDx / kDy: per format, the plane and the 8x8 position in its MCU of every
    block of an MCU in coding order."""
    with open(os.path.join(_CSRC, "api.hip")) as f:
        src = f.read()
    out = {}
    for name in ("kPlane", "kDx", "kDy"):
        m = re.search(name + r"\[3\]\[8\]\s*=\s*\{(.*?)\};", src)
        assert m, name
        rows = re.findall(r"\{([^{}]*)\}", m.group(1))
        assert len(rows) == 3, name
        out[name] = [[int(v) for v in r.split(",")] for r in rows]
    return out


_MCU = _mcu_tables()
_FMT = {"420": 0, "422": 1, "444": 2}


def block_pos(w, h, chroma, b):
    """(plane, x0, y0, plane width, plane height) of block b of a frame in coding order
    (kernels.hip block_pos with build_tabs's descriptors)."""
    f = _FMT[chroma]
    bpm = 8 if chroma == "422" else 6
    lmw, cmh = (8 if chroma == "444" else 16), (8 if chroma == "420" else 16)
    mbw = (w + lmw - 1) // lmw
    m, i = divmod(b, bpm)
    my, mx = divmod(m, mbw)
    pl = _MCU["kPlane"][f][i]
    xs, ys = (lmw, 16) if pl == 0 else (8, cmh)
    pw, ph = (w, h) if pl == 0 else chroma_size(w, h, chroma)
    return pl, mx * xs + 8 * _MCU["kDx"][f][i], my * ys + 8 * _MCU["kDy"][f][i], pw, ph


def carry_preds(w, h, chroma, rst=False, nframes=1):
    """For every unit that starts inside a segment, (frame, segment, chunk, {plane: interior}): of
    the 8 blocks before the unit's first one, whose pixel rows carry_row loads, the last block of
    each plane (the DC predictor of that plane's first block in the chunk), and whether it lies
    inside the picture (x0 + 8 <= plane width: carry_row's one 8-byte load per row, at any
    alignment under UA) or on its right edge (the byte loop with the clamp)."""
    g = enc_geom(w, h, chroma, rst, nframes)
    out = []
    for fr, seg, chunk in mid_segment_units(w, h, chroma, rst, nframes):
        last = {}
        for b in range(seg * g.seg_blocks + chunk * 64 - 8, seg * g.seg_blocks + chunk * 64):
            pl, x0, _, pw, _ = block_pos(w, h, chroma, b)
            last[pl] = x0 + 8 <= pw
        out.append((fr, seg, chunk, last))
    return out


def copy_span(nbytes):
    """(workgroups, vector slots in use) for one (plane, frame) of nbytes in the copy kernels:
    16-byte pieces, kCopyThreads x kCopyVecs of them per workgroup, slot i of thread tid holding
    piece tid + i kCopyThreads (the launch sizes its grid from nbytes >> 4; an unaligned head can
    make the kernel's own piece count one less)."""
    pieces = nbytes >> 4
    per = COPY_THREADS * COPY_VECS
    wgs = max(1, (pieces + per - 1) // per)
    slots = COPY_VECS if wgs > 1 else min(COPY_VECS, max(1, (pieces + COPY_THREADS - 1) // COPY_THREADS))
    return wgs, slots


OrientSpan = namedtuple("OrientSpan", "tx ty ntiles wgs idle right bottom partial_past_first")


def orient_cells(orient):
    """(T, FX, fy) of k_orient_plane<T, FX> with OrientGeom::fy for orient = T | FX << 1 | FY << 2."""
    return bool(orient & 1), bool(orient & 2), (orient >> 2) & 1


def orient_span(sw, sh, transposing):
    """What plan_orient and k_orient_plane derive for one source plane of sw x sh.
    T = 0: copy_span(sw sh), the mirrored streaming copy's (workgroups, vector slots in use).
    T = 1: tile columns and rows (kOrientTile columns x kOrientTileH rows a tile, one wave each),
    tiles, workgroups of kOrientWaves tiles and the idle waves of the last one (tile >= ntiles);
    whether some lane's 16-column x 8-row block is cut by the plane's right edge (sw % 16) / its
    bottom edge (sh % 8) and so moves byte by byte, and whether a tile past the first workgroup
    holds such a lane."""
    if not transposing:
        return copy_span(sw * sh)
    tx, ty = (sw + ORIENT_TILE - 1) // ORIENT_TILE, (sh + ORIENT_TILE_H - 1) // ORIENT_TILE_H
    ntiles = tx * ty
    wgs = (ntiles + ORIENT_WAVES - 1) // ORIENT_WAVES
    right, bottom = sw % 16 != 0, sh % 8 != 0
    past = any((right and t % tx == tx - 1) or (bottom and t // tx == ty - 1) for t in range(ORIENT_WAVES, ntiles))
    return OrientSpan(tx, ty, ntiles, wgs, wgs * ORIENT_WAVES - ntiles, right, bottom, past)


# mjg_debug_scale_path's values
NONE, COPY, TILE, STREAM, PADCOPY = 0, 1, 2, 3, 4
IN_PLACE, UA = 1, 2  # mjg_debug_encode_path's bits


def taps_ok(sw, sh, dw, dh):
    """Both filters of one plane stay below 256 taps (else swscale cascades: open refuses)."""
    try:
        _lib.sws_filter(sw, dw, 1 << 14, 4)
        _lib.sws_filter(sh, dh, 1 << 12, 2)
        return True
    except _lib.MjgError:
        return False


def _tile_plan(sw, sh, dw, dh):
    """(ht, npv, th, max_nw, LDS bytes, d4) of k_scale's tile for a sw x sh -> dw x dh plane
    (plan_plane_scale).  Every plane's filter positions are 128 (sws_local_pos with the default
    chroma siting), mjg_sws_filter's default.  d4: every h coefficient splits into the hi / lo
    bytes of the v_dot4 layout."""
    hc, hpos = _lib.sws_filter(sw, dw, 1 << 14, 4)
    vc, vpos = _lib.sws_filter(sh, dh, 1 << 12, 2)
    ht, vt = (hc.shape[1] + 3) & ~3, vc.shape[1]
    npv = vt // 2 + 1
    vps = [int(p) >> 1 for p in vpos]
    max_nw = 0
    for x0 in range(0, dw, SCALE_TILE_W):
        xe, cb = min(x0 + SCALE_TILE_W, dw), int(hpos[x0]) & ~3
        max_nw = max(max_nw, ((((int(hpos[xe - 1]) + ht - cb + 3) >> 2) + 1) + 3) & ~3)

    def tile_pairs(th):
        return max(vps[min(y0 + th, dh) - 1] + npv - vps[y0] for y0 in range(0, dh, th))

    # scale_waves(64) = 4, scale_loads_per_wave(64) = 5
    th = 64 if (ht == 8 and npv == 5 and max_nw <= SCALE_ALIAS_WORDS and sw >= 16
                and 2 * tile_pairs(64) <= 4 * 5 * SCALE_LOAD_ROWS) else 32
    mp = tile_pairs(th)
    if th >= 64:
        lds = 2 * mp * SCALE_ALIAS_WORDS * 4 + 64
    else:
        lds = (2 * mp * max_nw + mp * SCALE_TILE_W + th * (npv + 1)) * 4
    d4 = bool(int(hc.min()) >= -128 * 128 - 64 and int(hc.max()) < 127 * 128 + 64)
    return ht, npv, th, max_nw, lds, d4


def tile_lds(sw, sh, dw, dh):
    """Bytes of LDS k_scale would need for one tile of a sw x sh -> dw x dh plane
    (plan_plane_scale: past 64 KiB the plane goes to k_scale_stream)."""
    return _tile_plan(sw, sh, dw, dh)[4]


def stream_hcl(max_nw, ht, npv):
    """plan_scale_stream's choice for a plane whose widest strip window is max_nw dwords: whether
    the first plan that fits 64 KiB (chunk rows R from 16 down by halving, staging 3 down to 0)
    stages the strip's h coefficients in LDS; None when nothing fits."""
    npc = max_nw // 4
    R = 16
    while R >= 2:
        for stage in (3, 2, 1, 0):
            need = (2 * R * max_nw + (npv + R) * SCALE_TILE_W + (SCALE_TILE_W * (ht // 2) if stage & 2 else 0)
                    + (STREAM_BAND * npv if stage & 1 else 0)) * 4
            if need <= 64 * 1024 and R * npc <= STREAM_THREADS * STREAM_MAX_PIECES:
                return bool(stage & 2)
        R >>= 1
    return None


def scale_variant(sw, sh, dw, dh, force_stream=False):
    """The kernel family and template key build_plan selects for a sw x sh -> dw x dh plane (with
    MJG_PLANE_COPY unset; force_stream: MJG_SCALE_STREAM=1): ("copy",), ("stream", d4, hcl) or
    ("tile", (HT, NPV, TH), d4).  Each family has one instantiation per range beside."""
    if (sw, sh) == (dw, dh):
        return ("copy",)
    ht, npv, th, max_nw, lds, d4 = _tile_plan(sw, sh, dw, dh)
    if lds > 64 * 1024 or force_stream:
        return ("stream", d4, stream_hcl(max_nw, ht, npv))
    if (ht, npv) == (8, 5):
        return ("tile", (8, 5, th), d4)
    return ("tile", (4, 3, 32) if (ht, npv) == (4, 3) else (0, 0, 32), d4)


def plane_path(sw, sh, dw, dh, has_pad, plane_copy=True):
    if plane_copy and (sw, sh) == (dw, dh):
        return PADCOPY if has_pad else COPY
    return STREAM if tile_lds(sw, sh, dw, dh) > 64 * 1024 else TILE


def predict_paths(w, h, src, rect, dst, dw, dh, pad, unaligned_fetch=True, plane_copy=True, orient=0):
    """(encode_path, (luma scale_path, chroma scale_path), RECT) of a context on w x h frames in
    `src`, cropped to rect (None: whole frames), encoded in `dst` at dw x dh (None: the
    rectangle's size) on the canvas pad = (x, y, W, H) (None: no pad).  RECT: the luma copy is
    k_plane_copy's rectangle form.  unaligned_fetch / plane_copy: MJG_UNALIGNED_FETCH /
    MJG_PLANE_COPY not 0 at open.  orient (T | FX << 1 | FY << 2): everything after the
    orientation is derived from the oriented frame as if it were the source (plan_geometry: fw =
    lay.ow), h x w under T, and the rectangle lies in it; an orientation alone is no crop."""
    if orient & 1:
        assert src != "422"
        w, h = h, w
    x, y, rw, rh = rect or (0, 0, w, h)
    dw, dh = dw or rw, dh or rh
    has_pad = pad is not None and tuple(pad) != (0, 0, dw, dh)
    scale = (rw, rh) != (dw, dh) or src != dst or has_pad
    shs, svs = CHROMA_SHIFTS[src]
    scw, sch = chroma_size(w, h, src)
    if not scale:
        off0 = y * w + x
        off1 = w * h + (y >> svs) * scw + (x >> shs)
        off2 = off1 + scw * sch
        is_crop = (x, y, rw, rh) != (0, 0, w, h)
        bits = off0 | off1 | off2 | w | scw | (w * h + 2 * scw * sch)
        return IN_PLACE | (UA if is_crop and (bits & 7) and unaligned_fetch else 0), (NONE, NONE), False
    ccw, cch = chroma_size(rw, rh, src)
    pcw, pch = chroma_size(dw, dh, dst)
    luma = plane_path(rw, rh, dw, dh, has_pad, plane_copy)
    chroma = plane_path(ccw, cch, pcw, pch, has_pad, plane_copy)
    return 0, (luma, chroma), luma == COPY and rw != w


def copy_pad_cells(w, h, src, rect, dst, dw, dh, pad, full):
    """The instantiations of the copy and pad kernels a configuration launches, as build_plan picks
    them: ("copy", RANGE, RECT) for k_plane_copy, ("pad", RANGE, COPY) for k_pad_plane.  RANGE is 0
    for full-range input, else 1 for luma and 2 for chroma; RECT: the plane's source rows are wider
    than the rectangle's; a border around a scaled picture is k_pad_plane<0, false>."""
    _, _, rw, _ = rect or (0, 0, w, h)
    _, paths, _ = predict_paths(w, h, src, rect, dst, dw, dh, pad)
    wide = (rw != w, chroma_size(rw, 2, src)[0] != chroma_size(w, 2, src)[0])
    out = set()
    for p in (0, 1):
        rng = 0 if full else 1 + p
        if paths[p] == COPY:
            out.add(("copy", rng, wide[p]))
        elif paths[p] == PADCOPY:
            out.add(("pad", rng, True))
        elif paths[p] in (TILE, STREAM) and pad is not None and tuple(pad) != (0, 0, dw, dh):
            out.add(("pad", 0, False))
    return out


# ------------------------------------------------------------------ the seeded sweep of the chain
DOWN = {"444": ("444", "422", "420"), "422": ("422", "420"), "420": ("420",)}  # never up-sampling
SUBMITS = ("host", "dev_odd", "segments", "merged")
MODES = ({}, {"huffman": "optimal"}, {"rst": True})
FEATURES = ("crop_in_place_ua", "crop_in_place_aligned", "rect_copy", "pad_copy", "pad_with_scale", "stream") + SUBMITS

Config = namedtuple("Config", "w h src rect dst dw dh pad full q kw submit nframes fseed")


def sweep_configs(seed, count):
    """`count` drawn configurations of crop -> convert / scale -> pad -> encode.  Source 64..420 x
    48..260 in any format; the encoded format the source's or a down-sampling of it; a crop in 2
    of 3 (the rectangle at least half the frame each way; for one crop in 2 the frame width and
    the rectangle's x are cut to multiples of 16, which is what the aligned read in place needs);
    a resize in 1 of 2, 2:1 to 6:1 down per direction; a pad in 1 of 2 with margins of 0..40;
    range, q, default / optimal / rst and the submit mode.  Every value is drawn before the
    rules are tested; a draw whose padded picture breaks the encoded format's sub-sampling, or
    whose filters reach 256 taps, is dropped and drawn again."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        w, h = int(rng.integers(64, 421)), int(rng.integers(48, 261))
        src = ("420", "422", "444")[int(rng.integers(3))]
        dst = DOWN[src][int(rng.integers(len(DOWN[src])))]
        crop, snap = int(rng.integers(3)) < 2, bool(rng.integers(2))
        fr = rng.uniform(0.5, 1.0, 2)
        fo = rng.uniform(0.0, 1.0, 2)
        resize = bool(rng.integers(2))
        rx, ry = rng.uniform(2.0, 6.0, 2)
        padded = bool(rng.integers(2))
        ml, mr, mt, mb = (int(v) for v in rng.integers(0, 41, 4))
        full = bool(rng.integers(2))
        q = (2, 5, 31)[int(rng.integers(3))]
        kw = MODES[int(rng.integers(3))]
        submit = SUBMITS[int(rng.integers(4))]
        nframes = 2 if submit in ("segments", "merged") else 1 + int(rng.integers(2))
        fseed = int(rng.integers(1 << 30))
        shs, svs = CHROMA_SHIFTS[src]
        rect = None
        if crop:
            if snap:
                w &= ~15
            rw, rh = max(8, int(w * fr[0])), max(8, int(h * fr[1]))
            x, y = int((w - rw) * fo[0]), int((h - rh) * fo[1])
            if snap:
                x &= ~15
            rect = (x & ~((1 << shs) - 1), y & ~((1 << svs) - 1), rw, rh)
        iw, ih = rect[2:] if rect else (w, h)
        dw, dh = (max(8, int(round(iw / rx))), max(8, int(round(ih / ry)))) if resize else (None, None)
        pw, ph = dw or iw, dh or ih
        hs, vs = CHROMA_SHIFTS[dst]  # the margins are cut to the encoded format's sub-sampling
        ml, mr, mt, mb = ml & ~((1 << hs) - 1), mr & ~((1 << hs) - 1), mt & ~((1 << vs) - 1), mb & ~((1 << vs) - 1)
        pad = (ml, mt, pw + ml + mr, ph + mt + mb) if padded and (ml or mr or mt or mb) else None
        if pad is not None and ((pw & ((1 << hs) - 1)) or (ph & ((1 << vs) - 1))):
            continue  # a picture of odd size cannot be padded in a sub-sampled format
        if (iw, ih) != (pw, ph) or src != dst or pad is not None:  # the sws stage runs: its filters
            ccw, cch = chroma_size(iw, ih, src)
            pcw, pch = chroma_size(pw, ph, dst)
            if not (taps_ok(iw, ih, pw, ph) and taps_ok(ccw, cch, pcw, pch)):
                continue
        out.append(Config(w, h, src, rect, dst, dw, dh, pad, full, q, kw, submit, nframes, fseed))
    return out


def features(cfg, enc_path, paths):
    """The FEATURES a configuration carries, from its encode path and scale paths (predicted by
    predict_paths, or as the context reports them)."""
    crop = cfg.rect is not None and tuple(cfg.rect) != (0, 0, cfg.w, cfg.h)
    f = {cfg.submit}
    if crop and enc_path == (IN_PLACE | UA):
        f.add("crop_in_place_ua")
    if crop and enc_path == IN_PLACE:
        f.add("crop_in_place_aligned")
    if paths[0] == COPY and crop and cfg.rect[2] != cfg.w:
        f.add("rect_copy")
    if PADCOPY in paths:
        f.add("pad_copy")
    if cfg.pad is not None and (TILE in paths or STREAM in paths):
        f.add("pad_with_scale")
    if STREAM in paths:
        f.add("stream")
    return f


def count_features(sets):
    return {k: sum(k in s for s in sets) for k in FEATURES}


def predicted_counts(cfgs):
    sets = []
    for c in cfgs:
        enc_path, paths, _ = predict_paths(c.w, c.h, c.src, c.rect, c.dst, c.dw, c.dh, c.pad)
        sets.append(features(c, enc_path, paths))
    return count_features(sets)


# The sweep of tests/test_gpu_chain.py: the seed, and per part of 30 configurations the number
# that carry each feature, counted by predicted_counts (tests/test_chain_geom.py checks that).
SWEEP_SEED = 93  # of seeds 1..3000 the one whose eight smallest counts below are largest
SWEEP_FLOORS = [
    {"crop_in_place_ua": 5, "crop_in_place_aligned": 2, "rect_copy": 4, "pad_copy": 4, "pad_with_scale": 4, "stream": 2,
     "host": 7, "dev_odd": 7, "segments": 10, "merged": 6},
    {"crop_in_place_ua": 2, "crop_in_place_aligned": 2, "rect_copy": 2, "pad_copy": 4, "pad_with_scale": 11, "stream": 2,
     "host": 7, "dev_odd": 9, "segments": 6, "merged": 8},
    {"crop_in_place_ua": 4, "crop_in_place_aligned": 3, "rect_copy": 2, "pad_copy": 2, "pad_with_scale": 6, "stream": 2,
     "host": 11, "dev_odd": 12, "segments": 5, "merged": 2},
    {"crop_in_place_ua": 3, "crop_in_place_aligned": 2, "rect_copy": 1, "pad_copy": 3, "pad_with_scale": 9, "stream": 1,
     "host": 6, "dev_odd": 11, "segments": 7, "merged": 6},
]


# ------------------------------------------------------------------ the seeded sweep with an orientation
ORIENT_FEATURES = (tuple("map%d" % o for o in range(1, 8))
                   + ("luma_t0_past_one_wg", "luma_t1_past_one_wg", "orient_alone_in_place", "crop_in_place_ua",
                      "crop_in_place_aligned", "sws_reads_orient") + SUBMITS)

OrientConfig = namedtuple("OrientConfig", Config._fields + ("orient",))


def orient_sweep_configs(seed, count):
    """sweep_configs(seed, count), each with an orientation from a generator of its own: 1..7, or
    one of 2, 4, 6 where the source is 4:2:2 (no transpose of it).  The drawn w x h is the
    oriented frame, which the rectangle, the size and the pad refer to: the source frames are
    source_size(cfg), h x w under a transposing map."""
    import numpy as np
    rng = np.random.default_rng([seed, 0x6f72])
    out = []
    for c in sweep_configs(seed, count):
        o = (2, 4, 6)[int(rng.integers(3))] if c.src == "422" else 1 + int(rng.integers(7))
        out.append(OrientConfig(*c, o))
    return out


def source_size(cfg):
    return (cfg.h, cfg.w) if cfg.orient & 1 else (cfg.w, cfg.h)


def orient_predict(cfg):
    """predict_paths of an OrientConfig (from its source size, as a context is opened)."""
    sw, sh = source_size(cfg)
    return predict_paths(sw, sh, cfg.src, cfg.rect, cfg.dst, cfg.dw, cfg.dh, cfg.pad, orient=cfg.orient)


def orient_features(cfg, enc_path, paths):
    """The ORIENT_FEATURES an OrientConfig carries, from its encode path and scale paths (predicted,
    or as the context reports them) and orient_span of its source's luma plane."""
    crop = cfg.rect is not None and tuple(cfg.rect) != (0, 0, cfg.w, cfg.h)
    sw, sh = source_size(cfg)
    t = bool(cfg.orient & 1)
    f = {cfg.submit, "map%d" % cfg.orient}
    if orient_span(sw, sh, t)[3 if t else 0] > 1:
        f.add("luma_t1_past_one_wg" if t else "luma_t0_past_one_wg")
    if enc_path & IN_PLACE:
        f.add("orient_alone_in_place" if not crop else
              "crop_in_place_ua" if enc_path & UA else "crop_in_place_aligned")
    else:
        assert paths[0] != NONE
        f.add("sws_reads_orient")
    return f


def orient_predicted_counts(cfgs):
    sets = []
    for c in cfgs:
        enc_path, paths, _ = orient_predict(c)
        sets.append(orient_features(c, enc_path, paths))
    return count_orient_features(sets)


def count_orient_features(sets):
    return {k: sum(k in s for s in sets) for k in ORIENT_FEATURES}


# The sweep of tests/test_gpu_orient_chain.py: the seed, and per part of 30 configurations the
# number that carry each feature, counted by orient_predicted_counts (tests/test_chain_geom.py
# checks that).  Of seeds 1..3000 the one whose sorted counts (68: 17 features x 4 parts) are
# largest, compared from the smallest up; every count is at least 1 at 30 per part.
ORIENT_SWEEP_SEED = 2901
ORIENT_SWEEP_FLOORS = [dict(zip(ORIENT_FEATURES, v)) for v in (
    (4, 5, 4, 4, 6, 6, 1, 11, 10, 2, 2, 2, 24, 8, 8, 4, 10),
    (3, 5, 4, 6, 2, 4, 6, 13, 10, 2, 3, 2, 23, 8, 7, 5, 10),
    (2, 4, 4, 7, 3, 8, 2, 14, 7, 3, 4, 2, 21, 8, 14, 5, 3),
    (3, 8, 3, 3, 4, 5, 4, 13, 10, 2, 2, 5, 21, 7, 7, 11, 5),
)]


# ------------------------------------------------------------------ the deinterlacer's and the sharpen's launches
DEINT_THREADS = _const("scale.hip", "kDeintThreads")
SHARP_TILE_W = _const("scale.hip", "kSharpTileW")
SHARP_TILE_H = _const("scale.hip", "kSharpTileH")

DeintSpan = namedtuple("DeintSpan", "wgs pieces over_row_end head tail")


def deint_span(w, h, head=0):
    """What plan_deint and yadif_work derive for one (plane, frame) of w x h whose first output
    byte lies `head` bytes in front of a 16-byte boundary: the workgroups of kDeintThreads pieces
    (the launch sizes its grid from w h >> 4), the whole 16-byte pieces nv = (w h - head) >> 4, how
    many of them run over a row end (col + 16 > w: gathered byte by byte), and the bytes in front
    of the first and behind the last piece, which the first workgroup's threads 0..15 make."""
    nb = w * h
    wgs = max(1, ((nb >> 4) + DEINT_THREADS - 1) // DEINT_THREADS)
    head = min(head, nb)
    nv = (nb - head) >> 4
    over = sum(1 for k in range(nv) if (head + 16 * k) % w + 16 > w)
    return DeintSpan(wgs, nv, over, head, nb - head - 16 * nv)


SharpCells = namedtuple("SharpCells", "tx ty filt copy masks short")


def _row_quads(cw, px, w):
    """[(x, n, pic)] of the output quads of one picture row of a cw-wide plane (sharp_store: quads
    start at multiples of 4 of the plane, a tile is a multiple of 4 wide): n samples inside the
    plane, bit k of pic: sample k inside the picture columns [px, px + w)."""
    out = []
    for x in range(0, cw, 4):
        n = min(4, cw - x)
        out.append((x, n, sum(1 << k for k in range(n) if px <= x + k < px + w)))
    return out


def sharp_cells(cw, ch, px, py, w, h, amount):
    """What sharp_geom, sharp_tile and sharp_store derive for one cw x ch plane with the w x h
    picture at (px, py) and the plane's amount: tile columns and rows, the tiles that filter
    (amount != 0 and the tile holds a picture sample) and those that only copy, the histogram of
    `pic` over the output quads of the filtering tiles (0: a quad of such a tile outside the
    picture, copied; 15: one dword store; anything else byte by byte), and the quads of the whole
    plane with fewer than four samples inside it (n < 4, at the plane's right edge)."""
    tw, th = SHARP_TILE_W, SHARP_TILE_H
    tx, ty = (cw + tw - 1) // tw, (ch + th - 1) // th
    quads = _row_quads(cw, px, w)
    filt = copy = 0
    masks = {}
    for r in range(ty):
        y0 = r * th
        rows = min(th, ch - y0)
        rows_in = max(0, min(y0 + rows, py + h) - max(y0, py))
        for c in range(tx):
            x0 = c * tw
            if not (amount != 0 and x0 < px + w and x0 + tw > px and y0 < py + h and y0 + th > py):
                copy += 1
                continue
            filt += 1
            for x, n, pic in quads:
                if x0 <= x < x0 + tw:
                    if rows_in:
                        masks[pic] = masks.get(pic, 0) + rows_in
                    if rows - rows_in:
                        masks[0] = masks.get(0, 0) + rows - rows_in
    short = ch * sum(1 for _, n, _ in quads if n < 4)
    return SharpCells(tx, ty, filt, copy, dict(sorted(masks.items())), short)


def sharp_plane_geoms(W, H, c, px, py, w, h, us):
    """The two launches' (cw, ch, px, py, w, h, amount_i) of an encoded W x H frame in `c` whose
    w x h picture sits at (px, py) (plan_sharp: luma, then the chroma planes), for sharp_cells."""
    hs, vs = CHROMA_SHIFTS[c]
    la, ca = int(float(us[2]) * 65536.0), int(float(us[5]) * 65536.0)
    return ((W, H, px, py, w, h, la),
            ((W + hs) >> hs, (H + vs) >> vs, px >> hs, py >> vs, (w + hs) >> hs, (h + vs) >> vs, ca))


# ------------------------------------------------------------------ the seeded sweep with a filter
DEINTS = (None, "tff", "bff", "tff_nospatial", "bff_nospatial")
DEINT_FLAGS = {None: 0, "tff": 1, "bff": 1 | 4, "tff_nospatial": 1 | 2, "bff_nospatial": 1 | 2 | 4}  # MJG_DEINT_*
SHARPS = (None, (5, 5, 1.0, 5, 5, 0.0), (5, 5, 1.0, 5, 5, 1.0), (3, 7, 1.5, 7, 3, -0.5), (9, 15, -1.0, 3, 3, 0.8),
          (5, 5, 0.0, 3, 5, 0.7))
SHARP_KINDS = {SHARPS[1]: "sharp55_luma_only", SHARPS[2]: "sharp55_all_planes", SHARPS[3]: "sharp_runtime_sizes",
               SHARPS[4]: "sharp_runtime_sizes", SHARPS[5]: "sharp_luma_copied"}
FILTER_FEATURES = (tuple("deint_" + str(d) for d in DEINTS)
                   + ("sharp55_luma_only", "sharp55_all_planes", "sharp_runtime_sizes", "sharp_luma_copied")
                   + ("deint_to_in_place_ua", "deint_to_in_place_aligned", "deint_to_rect_copy", "deint_to_pad_copy",
                      "deint_to_tile_scale", "deint_to_stream", "deint_to_orient_t0", "deint_to_orient_t1")
                   + ("sharp_from_tile_scale", "sharp_from_stream", "sharp_from_plane_copy", "sharp_from_pad_copy",
                      "sharp_from_pad_with_scale")
                   + ("sharp_three_tile_columns", "sharp_copy_tile_beside_filter", "sharp_left_partial_mask",
                      "sharp_right_partial_mask")
                   + SUBMITS + ("default", "optimal", "rst"))

FilterConfig = namedtuple("FilterConfig", Config._fields + ("orient", "deint", "unsharp"))

def filter_sweep_configs(seed, count):
    """sweep_configs(seed, count), each with values from a generator of its own (seeded [seed,
    tag]): a deinterlacer out of DEINTS, a sharpen out of SHARPS, in one draw of three an
    orientation (1..7; 2, 4 or 6 where the source is 4:2:2), and a submit mode for the case below.
    Every value is drawn before the rules are tested; a draw with neither a deinterlacer nor a
    sharpen is drawn again.  As in orient_sweep_configs the drawn w x h is the oriented frame and
    the source frames are source_size(cfg).  A deinterlaced configuration has three frames (the
    middle one has two distinct neighbours) and, a deint context never merging, one of the other
    three submit modes in place of "merged"; its segments are 2 + 1 frames.
    The odds are not those of a uniform draw.  sweep_configs gives a part of 30 about one
    configuration on the stream kernel, one or two crops read in place of either kind and two
    rectangle copies (of seeds 1..800, 13% have a stream kernel in every part, 64% each kind of
    crop in place, 80% a rectangle copy, 4% all of them), so with uniform odds no seed of 1..3000
    gave every feature in every part.  Hence: "no deinterlacer" counts twice among six
    deinterlacer values (merged submits are for sharpen-only draws), and a base draw on one of
    those rare paths always gets one of the four deinterlacers; one that is read in place gets no
    sharpen (a sharpen runs the sws stage: nothing would read d_deint in place) and no
    orientation; one with a plane on the stream kernel always gets a sharpen and no orientation
    (so the one configuration has d_deint in front of the stream kernel and d_sharp behind it)."""
    import numpy as np
    rng = np.random.default_rng([seed, 0x6669])
    out = []
    for c in sweep_configs(seed, count):
        enc_path, paths, rect_form = predict_paths(c.w, c.h, c.src, c.rect, c.dst, c.dw, c.dh, c.pad)
        in_place, stream = bool(enc_path & IN_PLACE), STREAM in paths
        while True:
            d6, d4 = int(rng.integers(6)), 1 + int(rng.integers(4))
            s6, s5 = int(rng.integers(6)), 1 + int(rng.integers(5))
            turned = int(rng.integers(3)) == 0
            o, om = 1 + int(rng.integers(7)), (2, 4, 6)[int(rng.integers(3))]
            sub = SUBMITS[int(rng.integers(3))]
            d = d4 if in_place or stream or rect_form else max(0, d6 - 1)
            s = 0 if in_place else s5 if stream else s6
            if d or s:
                break
        orient = 0 if not turned or in_place or stream else om if c.src == "422" else o
        submit, nframes = c.submit, c.nframes
        if d:
            submit, nframes = (sub if submit == "merged" else submit), 3
        out.append(FilterConfig(*c._replace(submit=submit, nframes=nframes), orient, DEINTS[d], SHARPS[s]))
    return out


def filter_predict(cfg):
    """(encode_path, (luma, chroma) scale_path, RECT) of a FilterConfig: predict_paths from its
    source size; a sharpen always runs the sws stage (plan_geometry: scale |= sharp), so what
    would be read in place goes through the plane copy first."""
    sw, sh = source_size(cfg)
    enc_path, paths, rect_form = predict_paths(sw, sh, cfg.src, cfg.rect, cfg.dst, cfg.dw, cfg.dh, cfg.pad,
                                               orient=cfg.orient)
    if cfg.unsharp is not None and enc_path & IN_PLACE:
        assert paths == (NONE, NONE)
        return 0, (COPY, COPY), cfg.rect is not None and cfg.rect[2] != cfg.w
    return enc_path, paths, rect_form


def encoded_geometry(cfg):
    """(canvas W, H, picture x, y, w, h) of the frames a configuration encodes."""
    pw = cfg.dw or (cfg.rect[2] if cfg.rect else cfg.w)
    ph = cfg.dh or (cfg.rect[3] if cfg.rect else cfg.h)
    return (cfg.pad[2], cfg.pad[3], cfg.pad[0], cfg.pad[1], pw, ph) if cfg.pad is not None else (pw, ph, 0, 0, pw, ph)


def filter_features(cfg, enc_path, paths):
    """The FILTER_FEATURES a FilterConfig carries, from its encode path and scale paths (predicted
    by filter_predict, or as the context reports them), its own values and sharp_cells of its
    encoded planes."""
    crop = cfg.rect is not None and tuple(cfg.rect) != (0, 0, cfg.w, cfg.h)
    f = {cfg.submit, "deint_" + str(cfg.deint),
         "optimal" if cfg.kw.get("huffman") == "optimal" else "rst" if cfg.kw.get("rst") else "default"}
    if cfg.deint is not None:  # who reads d_deint
        if cfg.orient:
            f.add("deint_to_orient_t1" if cfg.orient & 1 else "deint_to_orient_t0")
        elif enc_path & IN_PLACE:
            if crop:
                f.add("deint_to_in_place_ua" if enc_path & UA else "deint_to_in_place_aligned")
        else:
            if paths[0] == COPY and crop and cfg.rect[2] != cfg.w:
                f.add("deint_to_rect_copy")
            if PADCOPY in paths:
                f.add("deint_to_pad_copy")
            if TILE in paths:
                f.add("deint_to_tile_scale")
            if STREAM in paths:
                f.add("deint_to_stream")
    if cfg.unsharp is not None:
        assert not enc_path & IN_PLACE
        f.add(SHARP_KINDS[cfg.unsharp])
        if cfg.pad is not None and (TILE in paths or STREAM in paths):
            f.add("sharp_from_pad_with_scale")
        if PADCOPY in paths:
            f.add("sharp_from_pad_copy")
        if COPY in paths:
            f.add("sharp_from_plane_copy")
        if TILE in paths and cfg.pad is None:
            f.add("sharp_from_tile_scale")
        if STREAM in paths:
            f.add("sharp_from_stream")
        for cw, ch, px, py, w, h, amount in sharp_plane_geoms(*encoded_geometry(cfg)[:2], cfg.dst,
                                                              *encoded_geometry(cfg)[2:], cfg.unsharp):
            if not amount:
                continue
            cells = sharp_cells(cw, ch, px, py, w, h, amount)
            if cells.tx >= 3:
                f.add("sharp_three_tile_columns")
            if cells.filt and cells.copy:
                f.add("sharp_copy_tile_beside_filter")
            for x, n, pic in _row_quads(cw, px, w):
                if pic and not pic & 1:
                    f.add("sharp_left_partial_mask")
                if n == 4 and pic & 1 and pic != 15:
                    f.add("sharp_right_partial_mask")  # (the picture's right edge cuts a whole quad of the canvas)
    return f


def count_filter_features(sets):
    return {k: sum(k in s for s in sets) for k in FILTER_FEATURES}


def filter_predicted_counts(cfgs):
    return count_filter_features([filter_features(c, *filter_predict(c)[:2]) for c in cfgs])


# The sweep of tests/test_gpu_filter_chain.py: the seed, and per part of 30 configurations the
# number that carry each feature, counted by filter_predicted_counts (tests/test_chain_geom.py
# checks that).  Of seeds 1..3000 the one whose sorted counts (132: 33 features x 4 parts) are
# largest, compared from the smallest up; five seeds have every count at least 1, which the GPU
# test requires of every feature in every part.
FILTER_SWEEP_SEED = 2451
FILTER_SWEEP_FLOORS = [dict(zip(FILTER_FEATURES, v)) for v in (
    (6, 7, 6, 6, 5, 4, 6, 6, 6, 1, 4, 2, 3, 12, 1, 3, 1, 16, 1, 3, 2, 4, 4, 4, 2, 3, 12, 9, 8, 1, 9, 11, 10),
    (6, 6, 8, 6, 4, 1, 4, 11, 4, 3, 1, 2, 2, 8, 2, 4, 3, 13, 2, 5, 2, 5, 2, 4, 6, 4, 6, 10, 12, 2, 7, 11, 12),
    (3, 5, 6, 8, 8, 3, 3, 9, 6, 1, 2, 1, 2, 12, 4, 5, 2, 10, 4, 3, 4, 8, 5, 8, 9, 8, 14, 8, 7, 1, 10, 14, 6),
    (4, 5, 5, 6, 10, 4, 3, 8, 6, 1, 5, 2, 2, 13, 1, 3, 3, 15, 1, 3, 1, 6, 3, 4, 6, 6, 11, 9, 9, 1, 9, 14, 7),
)]


# ------------------------------------------------------------------ the plane stages' launches of a long submit
def _uv_limit():
    """The largest grid z submit_impl gives a plane stage: every `uv1 = 2 * n <= LIMIT` of api.hip (the
    deinterlacer, the orientation, the sws stage with the sharpen) must state the same one."""
    with open(os.path.join(_CSRC, "api.hip")) as f:
        found = re.findall(r"const bool uv1 = 2 \* n <= (\d+);", f.read())
    assert len(found) == 3 and len(set(found)) == 1, found
    return int(found[0])


def _api_const(name):
    with open(os.path.join(_CSRC, "api.hip")) as f:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", f.read())
    assert m, name
    return int(m.group(1))


UV_LIMIT = _uv_limit()
MAX_BATCH = 65535      # check_config: max_batch in 1..65535
MAX_SEGS = _const("kernels.hip", "kMaxSegs")
MERGE = _api_const("kMerge")
SLOTS = _api_const("kSlots")
SLOT_WORDS = (64 * _const("kernels.hip", "kMaxBlockBits") + 31) // 32      # kSlotWords: one chunk's scratch / stream words
LONG = UV_LIMIT // 2 + 1      # the fewest frames of one launch whose V plane gets a launch of its own


def plane_launches(n):
    """[(planes, grid z)] of the launches submit_impl makes per plane stage (deinterlacer, orientation,
    every pass of the sws stage, sharpen) for a launch of n frames: luma, then U and V together
    (blockIdx.z >= n is V, through poff) while 2 n fits the grid's z range; past that U alone (poff
    0, nz = n) and V alone (`p == 2`: the plane offset added on the host)."""
    if 2 * n <= UV_LIMIT:
        return [("Y", n), ("UV", 2 * n)]
    return [("Y", n), ("U", n), ("V", n)]


def merged_frames(max_batch, merge=True, deint=False, nseg=1, nchunks=1, per_frame_bytes=0, free_bytes=None):
    """The frames one launch may carry (open_device: slot_B = max_batch * merge) on a context opened
    with max_batch and MJG_F_MERGE (`merge`), capped as open caps it: kMerge jobs a launch (at most
    kMaxSegs; MJG_MERGE unset), none with a deinterlacer, none when kSlots slots of merge x max_batch
    frames of per_frame_bytes would take more than a quarter of free_bytes (given: the device's
    free memory; None: not tested), none when max_batch merge nseg nchunks^2 reaches 2^40
    (k_encode's task magic)."""
    assert 1 <= max_batch <= MAX_BATCH
    m = max(1, min(MAX_SEGS, MERGE)) if merge else 1
    if deint:
        m = 1
    if m > 1 and free_bytes is not None and SLOTS * m * max_batch * per_frame_bytes > 0.25 * free_bytes:
        m = 1
    if max_batch * m * nseg * nchunks * nchunks >= 1 << 40:
        m = 1
    return m * max_batch


def slot_frame_bytes(nchunks, nseg, enc_frame_bytes, in_frame_bytes=0, orient=False, sharp=False):
    """open_device's per_frame: scratch and stream words of a frame's chunks, the scaled frame twice
    (d_scaled, d_out's share), the oriented and the sharpened frame where those stages run."""
    return (2 * nchunks * nseg * SLOT_WORDS * 4 + 2 * enc_frame_bytes + (in_frame_bytes if orient else 0)
            + (enc_frame_bytes if sharp else 0))


LONG_K = 61      # distinct base frames of tests/test_gpu_long_submit.py: prime, so no period lines up with 64, 256 or a grid


def long_frame_index(n):
    """Base frame of every frame of a long submit: frame i is base[(7 i + i // 1000) % 61]."""
    import numpy as np
    i = np.arange(n, dtype=np.int64)
    return ((i * 7 + i // 1000) % LONG_K).astype(np.int64)


LongCase = namedtuple("LongCase", "w h src dst rect dw dh pad full orient deint unsharp kw stream")


def _lc(w, h, src="420", dst=None, rect=None, dw=None, dh=None, pad=None, full=False, orient=0, deint=None, unsharp=None,
        kw=None, stream=False):
    return LongCase(w, h, src, dst or src, rect, dw, dh, pad, full, orient, deint, unsharp, kw or {}, stream)


# The configurations of tests/test_gpu_long_submit.py: per plane stage the smallest frames on which it
# exists (w x h source frames; the rectangle, the size and the pad refer to the oriented frame; deint
# out of DEINTS; stream: MJG_SCALE_STREAM=1).  The pads sit at (4, 6): py >> 1 = 3, so the V launch's
# d_off is no plane start.  tests/test_chain_geom.py pins the paths of each.
LONG_CASES = {
    "in_place": _lc(8, 8),
    "optimal": _lc(8, 8, kw={"huffman": "optimal"}),
    "rst": _lc(8, 32, kw={"rst": True}),
    "scale_tv": _lc(16, 16, dw=8, dh=8),
    "scale_pc": _lc(16, 16, dw=8, dh=8, full=True),
    "scale_up_444": _lc(8, 8, "444", dw=12, dh=12),
    "scale_stream": _lc(16, 16, dw=8, dh=8, stream=True),
    "pix_fmt_copy": _lc(8, 8, "444", "420"),
    "rect_copy": _lc(16, 8, "444", "420", rect=(4, 0, 8, 8)),
    "pad_copy": _lc(8, 8, pad=(4, 6, 16, 16)),
    "pad_scale": _lc(16, 16, dw=8, dh=8, pad=(4, 6, 16, 16)),
    "hflip": _lc(24, 8, orient=2),
    "transpose": _lc(24, 8, orient=1),
    "yadif": _lc(8, 8, deint="tff"),
    "yadif_nospatial": _lc(8, 8, deint="tff_nospatial"),
    "unsharp55": _lc(8, 8, full=True, unsharp=SHARPS[2]),
    "unsharp_chroma": _lc(8, 8, full=True, unsharp=SHARPS[5]),
    "chain": _lc(24, 16, deint="tff", orient=1, rect=(2, 2, 12, 20), dw=8, dh=12, unsharp=SHARPS[2], pad=(4, 6, 16, 24)),
    "scale_sharp": _lc(16, 16, dw=8, dh=8, unsharp=SHARPS[2]),
}


def long_predict(c):
    """(encode_path, (luma, chroma) scale_path, RECT) of a LongCase: predict_paths from its source
    size; a sharpen always runs the sws stage (filter_predict)."""
    enc_path, paths, rect_form = predict_paths(c.w, c.h, c.src, c.rect, c.dst, c.dw, c.dh, c.pad, orient=c.orient)
    if c.unsharp is not None and enc_path & IN_PLACE:
        assert paths == (NONE, NONE)
        ow = c.h if c.orient & 1 else c.w
        return 0, (COPY, COPY), c.rect is not None and c.rect[2] != ow
    return enc_path, paths, rect_form


def long_plane_sizes(c):
    """((source w, h), (encoded w, h)) of the luma and of a chroma plane of the sws stage of a LongCase."""
    ow, oh = (c.h, c.w) if c.orient & 1 else (c.w, c.h)
    rw, rh = c.rect[2:] if c.rect else (ow, oh)
    dw, dh = c.dw or rw, c.dh or rh
    return (((rw, rh), (dw, dh)), (chroma_size(rw, rh, c.src), chroma_size(dw, dh, c.dst)))


# The configurations of tests/test_gpu_long_stages.py: the stages that came after LONG_CASES (the denoiser, the
# tile, slot "out" of the table stage, the colour matrix).  geom: a LongCase; n: the frames of the submit, segs
# their split into device segments (None: one submit); sheet: the tile's (cols, rows, nb_frames, margin,
# padding); denoise / cmat / lut_in / lut_out: whether the stage is there (the test file holds the tables;
# a case with the denoiser gets low-contrast noise, so that the temporal table acts).
StageCase = namedtuple("StageCase", "geom n segs sheet denoise cmat lut_in lut_out")
_PAD = (4, 6, 16, 16)
LONG_STAGE_CASES = {
    "dn": StageCase(_lc(8, 8, full=True), LONG, None, None, True, False, False, False),
    "dn_yadif_segs": StageCase(_lc(8, 8, full=True, deint="tff"), 38000, (12345, 20422, 3000, 2233), None, True, False, False, False),
    "tile_a": StageCase(_lc(8, 8, full=True, unsharp=SHARPS[2]), LONG, None, (2, 1, 1, 0, 0), False, False, False, False),
    "tile_b": StageCase(_lc(16, 16, dw=8, dh=8, unsharp=SHARPS[2]), 40000, None, (2, 1, 0, 0, 0), False, False, False, False),
    "tile_c": StageCase(_lc(8, 8), MAX_BATCH, None, (2, 1, 0, 0, 0), False, False, False, False),
    "tile_segs": StageCase(_lc(8, 8), 65534, (12345, 20421, 32765, 3), (2, 1, 0, 0, 0), False, False, False, False),
    "lut_out": StageCase(_lc(16, 16, dw=8, dh=8, pad=_PAD), LONG, None, None, False, False, False, True),
    "cmat_chain": StageCase(_lc(16, 16, dw=8, dh=8, pad=_PAD, unsharp=SHARPS[2]), LONG, None, None, False, True, True, True),
    "full_chain": StageCase(_lc(16, 16, dw=8, dh=8, pad=_PAD, unsharp=SHARPS[2], deint="tff"), LONG, None, None, True, True, True,
                            True),
}


def long_stage_predict(c):
    """(encode_path, (luma, chroma) scale_path) of a StageCase: long_predict of its geometry; a sheet and a
    slot-"out" table always run the sws stage, as a sharpen does (a plane that keeps its size: the copy)."""
    enc_path, paths, _ = long_predict(c.geom)
    if enc_path & IN_PLACE and (c.sheet is not None or c.lut_out):
        assert paths == (NONE, NONE)
        return 0, (COPY, COPY)
    return enc_path, paths


def sheets_out(c, n=None):
    """The frames k_encode codes for a StageCase (sheet_split): ceil(count / N) sheets for every segment."""
    counts = c.segs or (c.n if n is None else n,)
    if c.sheet is None:
        return sum(counts)
    per = c.sheet[2] or c.sheet[0] * c.sheet[1]
    return sum((k + per - 1) // per for k in counts)


# ------------------------------------------------------------------ the table stage's launches
LutSpan = namedtuple("LutSpan", "wgs whole over_row_end skipped late_over late_skipped head tail")
LUT_PER_WG = COPY_THREADS * COPY_VECS      # the 16-byte pieces of one workgroup of k_lut_plane


def lut_span(w, h, stride, head=0):
    """What lut_geom_rect and lut_work derive for one (plane, frame) of a table launch: a w x h
    rectangle whose rows lie `stride` bytes apart on both sides (slot "in": stride = w; slot "out":
    the canvas stride) and whose first destination byte lies `head` bytes in front of a 16-byte
    boundary.  Rows that are contiguous fold into one row of w h bytes.  The span is nb = (h - 1)
    stride + w bytes; the launch sizes its grid from nb >> 4 pieces, kCopyThreads x kCopyVecs a
    workgroup; the kernel's own count is nv = (nb - head) >> 4, piece k at span bytes [head + 16 k,
    + 16), column col = (head + 16 k) % stride: whole (one 16-byte load and store) when col + 16 <=
    w, over a row end (byte by byte) when col < w or col + 16 > stride, else between two rows and
    skipped.  late_*: those of pieces k >= kCopyThreads kCopyVecs, which workgroups blk >= 1 hold.
    head, tail: the bytes in front of the first and behind the last piece (workgroup 0, threads
    0..15)."""
    if stride == w:
        w, h, stride = w * h, 1, w * h
    nb = (h - 1) * stride + w
    pieces = nb >> 4
    wgs = (pieces + LUT_PER_WG - 1) // LUT_PER_WG if pieces else 1
    head = min(head, nb)
    nv = (nb - head) >> 4
    tail = nb - head - 16 * nv
    if h == 1:
        return LutSpan(wgs, nv, 0, 0, 0, 0, head, tail)
    whole = over = skipped = late_over = late_skipped = 0
    for k in range(nv):
        col = (head + 16 * k) % stride
        if col + 16 <= w:
            whole += 1
        elif col < w or col + 16 > stride:
            over += 1
            late_over += k >= LUT_PER_WG
        else:
            skipped += 1
            late_skipped += k >= LUT_PER_WG
    return LutSpan(wgs, whole, over, skipped, late_over, late_skipped, head, tail)


def lut_plane_geoms(W, H, c, px, py, w, h):
    """The luma and the chroma (w, h, stride, d_off) of slot "out" as plan_lut sets them for an
    encoded W x H frame in `c` whose w x h picture sits at (px, py): the picture's planes in
    d_scaled at the canvas stride, d_off the rectangle's first byte inside a frame (the chroma
    one is U's; V's lies a chroma plane of the canvas further, lut_plane_heads).  A 16-aligned
    d_scaled and frame bytes that are a multiple of 16 make head = (-d_off) & 15 in every frame."""
    hs, vs = CHROMA_SHIFTS[c]
    cw, ch = (W + hs) >> hs, (H + vs) >> vs
    return ((w, h, W, py * W + px),
            ((w + hs) >> hs, (h + vs) >> vs, cw, W * H + (py >> vs) * cw + (px >> hs)))


def lut_out_spans(W, H, c, px, py, w, h, nframes=1):
    """{(plane, frame): LutSpan} of slot "out" for nframes frames of d_scaled (16-aligned; frames
    enc_frame_bytes apart, so at any address where that is odd)."""
    hs, vs = CHROMA_SHIFTS[c]
    cplane = ((W + hs) >> hs) * ((H + vs) >> vs)
    fb = W * H + 2 * cplane
    luma, chroma = lut_plane_geoms(W, H, c, px, py, w, h)
    out = {}
    for f in range(nframes):
        for p, (gw, gh, gs, off) in enumerate((luma, chroma, chroma)):
            out[(p, f)] = lut_span(gw, gh, gs, -(f * fb + off + (cplane if p == 2 else 0)) & 15)
    return out


# ------------------------------------------------------------------ the seeded sweep with a table
LUT_KINDS = (None, "perm", "perm_id_y", "perm_id_uv")      # a slot's tables: none, eq_ref.perm_tables, with identity planes
LUT_IDENT = {None: (0, 1, 2), "perm": (), "perm_id_y": (0,), "perm_id_uv": (1, 2)}
EQ_FEATURES = (tuple("in_" + k for k in LUT_KINDS[1:]) + tuple("out_" + k for k in LUT_KINDS[1:]) + ("both_slots",)
               + ("in_to_d_lut", "in_place_d_deint", "in_place_d_orient")
               + tuple("d_lut_" + s for s in SUBMITS) + ("d_lut_identity_copy_three_wgs",)
               + ("read_in_place_aligned", "read_in_place_ua", "read_rect_copy", "read_pad_copy", "read_plane_copy",
                  "read_k_scale", "read_k_scale_stream")
               + ("out_flat", "out_strided", "out_flat_past_one_wg", "out_strided_past_one_wg", "out_late_over",
                  "out_late_skipped", "out_strided_v_second_slot", "out_sharp_behind", "v_mapped_three_wgs")
               + SUBMITS + ("default", "optimal", "rst"))

EqConfig = namedtuple("EqConfig", FilterConfig._fields + ("lut_in", "lut_out"))


def eq_sweep_configs(seed, count):
    """sweep_configs(seed, count), each with values from a generator of its own (seeded [seed,
    tag]): a table kind out of LUT_KINDS per slot, in one draw of four a deinterlacer, in one of
    four an orientation (1..7; 2, 4 or 6 where the source is 4:2:2), in one of three a sharpen, and
    a submit mode for a deinterlaced draw.  Every value is drawn before the rules are tested; a
    draw with no table is drawn again.  The drawn w x h is the oriented frame (source_size); a
    deinterlaced configuration has three frames, never "merged", segments of 2 + 1.
    The odds: slot "in" writes d_lut only on a caller's frames (no deinterlacer, no orientation),
    and that has to meet each of four submit modes in every part of 30, so both are rarer than in
    filter_sweep_configs.  The rules: a base draw whose crop k_encode reads in place keeps that
    (the rare path): slot "in" only, no sharpen, no orientation; one on the stream kernel or the
    rectangle copy always gets slot "in" and no orientation, so those readers see mapped frames.
    Anything else that would be read in place and draws slot "out" goes through the sws stage
    (eq_predict).  With these odds 22 seeds of 1..3000 give every feature of EQ_FEATURES in every
    part of 30; EQ_SWEEP_SEED is the one whose sorted counts are largest, compared from the
    smallest up."""
    import numpy as np
    rng = np.random.default_rng([seed, 0x6571])
    out = []
    for c in sweep_configs(seed, count):
        enc_path, paths, rect_form = predict_paths(c.w, c.h, c.src, c.rect, c.dst, c.dw, c.dh, c.pad)
        crop = c.rect is not None and tuple(c.rect) != (0, 0, c.w, c.h)
        keep, rare = bool(enc_path & IN_PLACE) and crop, STREAM in paths or rect_form
        while True:
            li, li3, lo = int(rng.integers(4)), 1 + int(rng.integers(3)), int(rng.integers(4))
            d4, d = int(rng.integers(4)) == 0, 1 + int(rng.integers(4))
            turned = int(rng.integers(4)) == 0
            o, om = 1 + int(rng.integers(7)), (2, 4, 6)[int(rng.integers(3))]
            s3, s5 = int(rng.integers(3)) == 0, 1 + int(rng.integers(5))
            sub = SUBMITS[int(rng.integers(3))]
            li = li3 if keep or rare else li
            lo = 0 if keep else lo
            if li or lo:
                break
        orient = 0 if not turned or keep or rare else om if c.src == "422" else o
        sharp = SHARPS[s5] if s3 and not keep else None
        submit, nframes = c.submit, c.nframes
        if d4:
            submit, nframes = (sub if submit == "merged" else submit), 3
        out.append(EqConfig(*c._replace(submit=submit, nframes=nframes), orient, DEINTS[d] if d4 else None, sharp,
                            LUT_KINDS[li], LUT_KINDS[lo]))
    return out


def eq_predict(cfg):
    """(encode_path, (luma, chroma) scale_path, RECT) of an EqConfig: filter_predict's rule with
    slot "out" beside the sharpen (plan_geometry: either runs the sws stage), so what would be
    read in place goes through the plane copy first."""
    sw, sh = source_size(cfg)
    enc_path, paths, rect_form = predict_paths(sw, sh, cfg.src, cfg.rect, cfg.dst, cfg.dw, cfg.dh, cfg.pad,
                                               orient=cfg.orient)
    if (cfg.unsharp is not None or cfg.lut_out is not None) and enc_path & IN_PLACE:
        assert paths == (NONE, NONE)
        return 0, (COPY, COPY), cfg.rect is not None and cfg.rect[2] != cfg.w
    return enc_path, paths, rect_form


def eq_features(cfg, enc_path, paths):
    """The EQ_FEATURES an EqConfig carries, from its encode path and scale paths (predicted by
    eq_predict, or as the context reports them), its own values and lut_span of every mapped
    (plane, frame) of slot "out" (a plane with the identity table is left alone in d_scaled).  Three
    features are there because a mutation run showed the need (profiles/eq_chain/mutations.txt):
    an identity plane copied into d_lut by three workgroups or more, a mapped V plane of three, and
    a V plane at the canvas stride with pieces past the first kCopyThreads."""
    crop = cfg.rect is not None and tuple(cfg.rect) != (0, 0, cfg.w, cfg.h)
    f = {cfg.submit, "optimal" if cfg.kw.get("huffman") == "optimal" else "rst" if cfg.kw.get("rst") else "default"}
    if cfg.lut_in and cfg.lut_out:
        f.add("both_slots")
    if cfg.lut_in:
        f.add("in_" + cfg.lut_in)
        iw, ih = chroma_size(cfg.w, cfg.h, cfg.src)      # slot "in": the whole planes of the oriented frame, flat
        in_planes = ((cfg.w, cfg.h, cfg.w), (iw, ih, iw))
        if cfg.orient:
            f.add("in_place_d_orient")
        elif cfg.deint:
            f.add("in_place_d_deint")
        else:
            f.update(("in_to_d_lut", "d_lut_" + cfg.submit))
            if any(lut_span(*in_planes[min(p, 1)]).wgs >= 3 for p in LUT_IDENT[cfg.lut_in]):
                f.add("d_lut_identity_copy_three_wgs")      # (`id && s != d` in workgroups blk >= 2)
        if 2 not in LUT_IDENT[cfg.lut_in] and lut_span(*in_planes[1]).wgs >= 3:
            f.add("v_mapped_three_wgs")      # (a V workgroup blk >= 2 of the paired launch, whose blk is not its blockIdx)
        if enc_path & IN_PLACE:
            if crop:
                f.add("read_in_place_ua" if enc_path & UA else "read_in_place_aligned")
        else:
            if paths[0] == COPY and crop and cfg.rect[2] != cfg.w:
                f.add("read_rect_copy")
            for path, name in ((PADCOPY, "read_pad_copy"), (COPY, "read_plane_copy"), (TILE, "read_k_scale"),
                               (STREAM, "read_k_scale_stream")):
                if path in paths:
                    f.add(name)
    if cfg.lut_out:
        assert not enc_path & IN_PLACE
        f.add("out_" + cfg.lut_out)
        if cfg.unsharp is not None:
            f.add("out_sharp_behind")
        W, H, px, py, w, h = encoded_geometry(cfg)
        wide = [g[2] != g[0] for g in lut_plane_geoms(W, H, cfg.dst, px, py, w, h)]      # plan_lut: d_stride = pg.cw > w
        for (p, _), sp in lut_out_spans(W, H, cfg.dst, px, py, w, h, cfg.nframes).items():
            if p in LUT_IDENT[cfg.lut_out]:
                continue
            strided = wide[min(p, 1)]
            f.add("out_strided" if strided else "out_flat")
            if sp.wgs > 1:
                f.add("out_strided_past_one_wg" if strided else "out_flat_past_one_wg")
            if sp.late_over:
                f.add("out_late_over")
            if sp.late_skipped:
                f.add("out_late_skipped")
            gw, _, gs, _ = lut_plane_geoms(W, H, cfg.dst, px, py, w, h)[1]
            if strided and p == 2 and any((sp.head + 16 * k) % gs + 16 <= gw for k in
                                          range(COPY_THREADS, sp.whole + sp.over_row_end + sp.skipped)):
                f.add("out_strided_v_second_slot")      # (a whole V piece of loop iteration i >= 1 at the canvas stride)
            if p == 2 and sp.wgs >= 3:
                f.add("v_mapped_three_wgs")
    return f


def count_eq_features(sets):
    return {k: sum(k in s for s in sets) for k in EQ_FEATURES}


def eq_predicted_counts(cfgs):
    return count_eq_features([eq_features(c, *eq_predict(c)[:2]) for c in cfgs])


# The sweep of tests/test_gpu_eq_chain.py: the seed, the configurations (in four parts) and per part
# the number that carry each feature, counted by eq_predicted_counts (tests/test_chain_geom.py
# checks that).  Of seeds 1..3000 the one whose sorted counts (152: 38 features x 4 parts) are
# largest, compared from the smallest up; 22 seeds have every count at least 1, which the GPU test
# requires of every feature in every part.
EQ_SWEEP_SEED = 168
EQ_SWEEP_COUNT = 120
EQ_SWEEP_FLOORS = [dict(zip(EQ_FEATURES, v)) for v in (
    (8, 5, 13, 8, 6, 6, 16, 18, 5, 3, 6, 6, 4, 2, 5, 6, 1, 2, 3, 5, 15, 1, 13, 7, 4, 3, 3, 3, 3, 7, 5, 10, 11, 7, 2, 17, 8, 5),
    (9, 9, 8, 5, 6, 8, 15, 17, 6, 3, 4, 4, 4, 5, 6, 3, 2, 6, 2, 8, 19, 1, 13, 6, 4, 2, 2, 2, 2, 6, 3, 7, 9, 8, 6, 13, 9, 8),
    (9, 6, 5, 4, 9, 12, 15, 13, 5, 2, 4, 2, 3, 4, 4, 3, 1, 2, 3, 5, 12, 1, 15, 10, 3, 2, 2, 2, 3, 12, 4, 8, 7, 8, 7, 10, 13, 7),
    (10, 6, 10, 8, 8, 4, 16, 13, 5, 8, 3, 4, 5, 1, 2, 3, 2, 1, 4, 4, 14, 1, 10, 10, 3, 4, 4, 4, 2, 6, 5, 10, 7, 10, 3, 11, 11, 8),
)]
