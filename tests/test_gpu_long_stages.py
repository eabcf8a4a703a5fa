"""The stages that came after tests/test_gpu_long_submit.py, in submits of more than 32,767 frames: the
denoiser (k_dn_rows / k_dn_cols / k_dn_time: dn_launch, dn_nz), the tile (k_tile_plane: tile_launch, whose
U + V pairing follows the sheets, not the frames), slot "out" of the table stage (k_lut_plane in place on
d_scaled, under a pad), the colour matrix with slot "in" in place behind it (k_cmat_frame's grid of gxy * n
in x), and k_frame_hist past 32,767 frames a call.  From 32,768 frames on V gets a launch of its own, and
only that launch adds the chroma plane to the stage's offsets on the host (uv_place: `if (p == 2) off +=
cplane`); a wrong offset there faults nothing and gives JPEGs that decode with the wrong chroma, so every
JPEG of every submit is compared byte for byte, and the stages' read-backs at a few marks (frames 0, 32766,
32767, 32768, a segment's ends, the last) name the stage first.

Frames are the smallest on which each stage exists (chain_geom.LONG_STAGE_CASES: 8 x 8 4:2:0, or 16 x 16 ->
8 x 8) and cycle through 61 base frames of seeded noise, frame i being base (7 i + i // 1000) % 61
(chain_geom.long_frame_index); with the denoiser the noise is low-contrast (88..112), so that the temporal
table acts.  The references are the existing ones, made once per distinct input: hqdn3d_ref.denoise_indexed
walks the time scan over the index (its output is eventually periodic, so everything behind the denoiser is
made once per distinct denoised frame: at most 2,000, asserted before a context is opened), tile_ref per
distinct tuple of base frames on a sheet, colormatrix_ref and test_gpu_eq.chain_ref per base frame,
thumbnail_ref.hist_ref per base frame.  Each case asserts from chain_geom, before it opens a context, that
its launches are the ones it is listed for, and on the context that the paths are those the stage's own
tests assert.  One context is open at a time."""
import numpy as np
import pytest

import chain_geom as cg
import colormatrix_ref
import hqdn3d_ref as R
import test_gpu_chain as chain
import test_gpu_eq as eq
import test_gpu_long_submit as ls
import thumbnail_ref
import tile_ref
from test_gpu_hqdn3d import TABS
from unsharp_ref import kernel_constant
from yadif_ref import deint_frame, deint_ref
from ffmpeg_distributed_amd.encoder import FrameHist, MjpegEncoder, i420_frame_bytes, split_i420

pytestmark = pytest.mark.gpu

N = cg.LONG          # 32768: the fewest frames with three launches a stage
K = cg.LONG_K
MAX_DISTINCT = 2000  # distinct denoised frames a case may have: the reference behind the denoiser is made once for each
COEFS = colormatrix_ref.coefs("bt709", "bt601")
T_IN, T_OUT = eq.T_IN, eq.T_OUT      # eq_ref.perm_tables: different for Y, U and V and for the two slots
first_diff = chain.first_diff
_same_planes = ls._same_planes


# ================================================================= inputs
_LOW = {}


def _base(c):
    """The 61 base frames of a StageCase: every byte seeded noise (U, V and Y all differ), full range, or
    88..112 as hqdn3d_ref.make_frames("noise") in front of the denoiser."""
    g = c.geom
    if not c.denoise:
        return ls._base(g.w, g.h, g.src)
    if (g.w, g.h, g.src) not in _LOW:
        f = np.random.default_rng([g.w, g.h, int(g.src), K, 88]).integers(88, 113, (K, i420_frame_bytes(g.w, g.h, g.src)),
                                                                          dtype=np.uint8)
        for fr in f:
            y, u, v = split_i420(fr, g.w, g.h, g.src)
            assert (u != v).any() and (y.reshape(-1)[:u.size] != u.reshape(-1)).any()
        assert len({fr.tobytes() for fr in f}) == K
        f.setflags(write=False)
        _LOW[(g.w, g.h, g.src)] = f
    return _LOW[(g.w, g.h, g.src)]


def _launches(n):
    return [p for p, _ in cg.plane_launches(n)]


def _segs(lens):
    cuts = np.cumsum((0,) + tuple(lens))
    return [(int(a), int(b - a)) for a, b in zip(cuts, cuts[1:])]


# ================================================================= references
class _Cache:
    """fn(key) made once per key."""

    def __init__(self, fn):
        self.fn, self.made = fn, {}

    def __call__(self, key):
        if key not in self.made:
            self.made[key] = self.fn(key)
        return self.made[key]


_DEINT, _DN = {}, {}


def _deinterlaced(name, n, segs):
    """(distinct deinterlaced frames, the index of each of the n frames into them): yadif mode 0, tff, made once per
    distinct (prev, cur, next); a frame's neighbours clamp to its own sequence."""
    if (name, n, tuple(segs)) not in _DEINT:
        c = cg.LONG_STAGE_CASES[name]
        g, base, idx = c.geom, _base(c), cg.long_frame_index(n)
        assert g.deint == "tff"
        j = np.arange(n)
        lo, hi = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for first, count in segs:
            lo[first:first + count], hi[first:first + count] = first, first + count - 1
        keys, inv = np.unique((idx[np.maximum(j - 1, lo)] * K + idx) * K + idx[np.minimum(j + 1, hi)], return_inverse=True)
        d = np.stack([deint_frame(base[k // (K * K)], base[k // K % K], base[k % K], g.w, g.h, g.src, 0, 1) for k in keys.tolist()])
        d.setflags(write=False)
        _DEINT[(name, n, tuple(segs))] = (d, inv.reshape(-1))
    return _DEINT[(name, n, tuple(segs))]


def _denoised(name, n, segs=None, dn_segs="same"):
    """The denoiser's reference of n frames of a StageCase, made once: (want (n, frame_bytes), state, the distinct
    denoised frames, the index of each frame into them).  segs: the submit's sequences (the deinterlacer's and,
    with dn_segs "same", the denoiser's; dn_segs None: the denoiser runs one sequence over all of them).  One
    sequence of 2 x 32768 frames continues the one of 32768 from its state."""
    key = (name, n, None if segs is None else tuple(segs), dn_segs)
    if key not in _DN:
        c = cg.LONG_STAGE_CASES[name]
        g = c.geom
        if g.deint:
            src, sidx = _deinterlaced(name, n, segs or [(0, n)])
        else:
            src, sidx = _base(c), cg.long_frame_index(n)
        if n == 2 * N and segs is None and not g.deint:
            head, hst = _denoised(name, N)[:2]
            tail, st = R.denoise_indexed(src, sidx[N:], g.w, g.h, g.src, TABS, state=hst)
            want = np.concatenate([head, tail])
        else:
            want, st = R.denoise_indexed(src, sidx, g.w, g.h, g.src, TABS, segs if dn_segs == "same" else None)
        uniq, inv = np.unique(want, axis=0, return_inverse=True)
        for a in (want, st, uniq):
            a.setflags(write=False)
        _DN[key] = (want, st, uniq, inv.reshape(-1))
    return _DN[key]


def _assert_denoiser_reference_is_worth_it(name, want, uniq, marks):
    """Before a context is opened: few enough distinct denoised frames, the tables act, U and V differ at the marks."""
    c = cg.LONG_STAGE_CASES[name]
    g = c.geom
    assert K < len(uniq) <= MAX_DISTINCT, (name, len(uniq))      # (more than the inputs: history matters)
    for m in marks:
        _, u, v = split_i420(want[m], g.w, g.h, g.src)
        assert (u != v).any(), (name, m)


_DN_JPEG = _Cache(lambda fr: deint_ref(np.frombuffer(fr, np.uint8), 8, 8, "420", full=True, qscale=5))


def _chain_refs(name):
    """test_gpu_eq.chain_ref behind the colour matrix for a frame (as bytes) in front of it, made once per frame."""
    c = cg.LONG_STAGE_CASES[name]
    g = c.geom

    def make(fr):
        f = np.frombuffer(fr, np.uint8)
        if c.cmat:
            f = colormatrix_ref.convert_frames(f, g.w, g.h, g.src, COEFS)
        return eq.chain_ref(f, g.w, g.h, g.src, T_IN if c.lut_in else None, T_OUT if c.lut_out else None, dst=g.dst, full=g.full,
                            dw=g.dw, dh=g.dh, us=g.unsharp, pad=g.pad)
    return _Cache(make)


class _Sheets:
    """The tile's reference of a StageCase: the cell of a base frame, and a sheet (planes, JPEG) per distinct tuple of
    base frames on it; members[j]: that tuple for sheet j of the submit, every segment a sequence of its own."""

    def __init__(self, name, n=None, segs=None):
        c = cg.LONG_STAGE_CASES[name]
        g, base = c.geom, _base(c)
        self.c, self.n = c, c.n if n is None else n
        self.idx = cg.long_frame_index(self.n)
        per = tile_ref.resolve(c.sheet)[2]
        self.cell = _Cache(lambda b: tile_ref.cell_planes(base[b], g.w, g.h, g.src, g.unsharp, dst=g.dst, full=g.full, dw=g.dw, dh=g.dh))
        self.members = []
        for first, count in (segs or [(0, self.n)]):
            assert tile_ref.frames_out(count, c.sheet) == (count + per - 1) // per
            self.members += [tuple(self.idx[a:min(a + per, first + count)].tolist()) for a in range(first, first + count, per)]
        cw, ch = g.dw or g.w, g.dh or g.h

        def make(t):
            planes, = tile_ref.sheets_numpy([self.cell(b) for b in t], cw, ch, g.dst, c.sheet)
            return planes, tile_ref.sheet_jpeg(planes, g.dst)
        self.sheet = _Cache(make)


# ================================================================= checks
def _check_jpegs(got, want_of, n, what, first=0):
    """Every JPEG against want_of(i); `first`: the sequence's index of got[0]."""
    assert len(got) == n, (what, len(got), n)
    for i, a in enumerate(got):
        b = want_of(i)
        if a != b:
            pytest.fail(f"{what}: JPEG of frame {first + i} ({ls._side(first + i)}) differs: first_diff {first_diff(a, b)}, "
                        f"{len(a)} bytes against {len(b)}")


def _check_frame(what, g_, got, want, c):
    g = c.geom
    _same_planes(what, g_, split_i420(got, g.w, g.h, g.src), split_i420(want, g.w, g.h, g.src))


def _check_state(what, enc, want):
    got = enc.debug_denoise_state()
    assert got.shape == want.shape and got.dtype == np.uint16
    bad = np.flatnonzero(got != want)
    if bad.size:
        pytest.fail(f"{what}: the carried state differs in {len(bad)} of {want.size} samples, first at {int(bad[0])}: got "
                    f"{int(got[bad[0]])}, want {int(want[bad[0]])}")


def _open(name, max_batch=None, **extra):
    """A context on a StageCase, after asserting on the CPU what it must reach, and on the context that it reports
    those paths and holds the stages' tables as their own tests assert."""
    c = cg.LONG_STAGE_CASES[name]
    g = c.geom
    want = cg.long_stage_predict(c)
    enc = MjpegEncoder(0, g.w, g.h, g.dw, g.dh, full_range=g.full, qscale=5, max_batch=max_batch or c.n, chroma=g.dst,
                       src_chroma=g.src, pad=g.pad, deint=cg.DEINT_FLAGS[g.deint] or None, unsharp=g.unsharp, sheet=c.sheet,
                       denoise=TABS if c.denoise else None, cmat=COEFS if c.cmat else None, lut_in=T_IN if c.lut_in else None,
                       lut_out=T_OUT if c.lut_out else None, **extra)
    try:
        assert enc.frame_bytes == i420_frame_bytes(g.w, g.h, g.src)
        assert (enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))) == want, name
        assert enc._L.mjg_debug_deint_flags(enc._h) == cg.DEINT_FLAGS[g.deint]
        assert (enc.debug_unsharp() is not None) == (g.unsharp is not None)
        for slot, t in (("in", T_IN if c.lut_in else None), ("out", T_OUT if c.lut_out else None)):
            held = enc.debug_lut(slot)
            assert (held is None) == (t is None) and (t is None or (held == t).all()), slot
        assert enc.debug_cmat() == (tuple(COEFS) if c.cmat else None)
        if c.sheet:
            assert enc.debug_sheet() == tile_ref.resolve(c.sheet)
            assert (enc.enc_w, enc.enc_h) == tile_ref.sheet_size(enc.dst_w, enc.dst_h, c.sheet) and enc.scale_path(0) != 0
        else:
            assert enc.debug_sheet() is None
    except BaseException:
        enc.close()
        raise
    return enc


# ================================================================= 1. the denoiser alone
def _denoiser_alone(n):
    """One host submit of the first n frames of the "dn" sequence: the marks, then every JPEG.  Returns the JPEGs."""
    name = "dn"
    c = cg.LONG_STAGE_CASES[name]
    want, _, uniq, inv = _denoised(name, N)
    frames = _base(c)[cg.long_frame_index(n)]
    with _open(name, n) as enc:
        enc.submit(frames, n)
        got = enc.fetch()
        for g_ in (0, n - 2, n - 1):
            _check_frame(f"{name}, {n} frames: denoised (k_dn_time's output)", g_, enc.debug_denoise(g_), want[g_], c)
        if n == N:
            _check_state(name, enc, _denoised(name, N)[1])
    _check_jpegs(got, lambda i: _DN_JPEG(uniq[inv[i]].tobytes()), n, f"{name}, {n} frames")
    return got


def test_denoiser_alone_one_host_submit():
    """8 x 8 4:2:0, 32,768 frames: dn_launch's V launches of k_dn_rows and k_dn_cols (the byte side and the uint16
    side), dn_nz(2, ...) = 1 for V alone with `state + po`, and a time scan of 32,768 frames inside a thread."""
    name = "dn"
    c = cg.LONG_STAGE_CASES[name]
    g, base, idx = c.geom, _base(c), cg.long_frame_index(N)
    assert c.n == N and _launches(N) == ["Y", "U", "V"]
    want, _, uniq, _ = _denoised(name, N)
    _assert_denoiser_reference_is_worth_it(name, want, uniq, (0, N - 2, N - 1))
    own, _ = R.denoise(base[idx[N - 1:]], g.w, g.h, g.src, TABS)
    assert (own[0] != want[N - 1]).any()      # history matters at the mark
    swapped, _ = R.denoise(base[idx[:1]], g.w, g.h, g.src, TABS[[0, 0, 2, 2]])
    assert (swapped[0][g.w * g.h:] != want[0][g.w * g.h:]).any()      # and so do the chroma tables, at mark 0 already
    _denoiser_alone(N)


# ================================================================= 2. the denoiser, continued
def test_denoiser_continued_over_two_device_submits():
    """Two device submits of 32,768 frames each from byte 1 of their allocations, the second with cont: one sequence of
    65,536 frames.  Each submit's V launches read the state the other slot's stream left."""
    name = "dn"
    c = cg.LONG_STAGE_CASES[name]
    g, base, n = c.geom, _base(c), 2 * N
    idx = cg.long_frame_index(n)
    assert _launches(N) == ["Y", "U", "V"]
    want, st, uniq, inv = _denoised(name, n)
    _assert_denoiser_reference_is_worth_it(name, want, uniq, (N, n - 2, n - 1))
    own, _ = R.denoise(base[idx[N:N + 1]], g.w, g.h, g.src, TABS)
    assert (own[0] != want[N]).any()      # the second submit as a sequence of its own would show at its frame 0
    jobs = [chain._device(base[idx[:N]], 1), chain._device(base[idx[N:]], 1)]
    got = []
    with _open(name, N) as enc:
        assert enc.depth >= 2
        for k, t in enumerate(jobs):
            enc.submit(device_ptr=t.data_ptr(), nframes=N, cont=k > 0)
        for _ in jobs:
            assert len(enc.sync()) == N
            got.append(enc.fetch())
        for i in (0, N - 2, N - 1):
            _check_frame(f"{name} continued: denoised, second submit", N + i, enc.debug_denoise(i), want[N + i], c)
        _check_state(name + " continued", enc, st)
    for k, part in enumerate(got):
        _check_jpegs(part, lambda i: _DN_JPEG(uniq[inv[k * N + i]].tobytes()), N, f"{name} continued, submit {k}", first=k * N)


# ================================================================= 3. yadif, hqdn3d over four segments
def test_yadif_hqdn3d_four_segments_with_a_boundary_at_the_limit():
    """submit_segments of (12345, 20422, 3000, 2233) = 38,000 frames: seg_starts hands the denoiser four sequences in
    one buffer, segment 3 starts at frame 32767, and `first` is found from src.f0[k] at large f."""
    name = "dn_yadif_segs"
    c = cg.LONG_STAGE_CASES[name]
    n, segs = c.n, _segs(c.segs)
    cuts = [a for a, _ in segs] + [n]
    assert n == 38000 and cuts[2] == N - 1 and cuts[3] == 35767 and len(segs) == cg.MAX_SEGS and _launches(n) == ["Y", "U", "V"]
    marks = sorted({0, N - 2, N - 1, N, n - 1, *cuts[1:4], *(a - 1 for a in cuts[1:4])})
    dsrc, didx = _deinterlaced(name, n, segs)
    want, st, uniq, inv = _denoised(name, n, segs)
    _assert_denoiser_reference_is_worth_it(name, want, uniq, marks)
    joined = _denoised(name, n, segs, dn_segs=None)[0]
    assert (joined[N - 1] != want[N - 1]).any() and (joined[cuts[3]] != want[cuts[3]]).any()      # one sequence over all would show
    frames = _base(c)[cg.long_frame_index(n)]
    pools = [chain._device(frames[a:a + k], 1) for a, k in segs]
    with _open(name, n) as enc:
        assert len(segs) <= enc.max_segments
        enc.submit_segments([(t.data_ptr(), k) for t, (_, k) in zip(pools, segs)])
        got = enc.fetch()
        for g_ in marks:
            _check_frame(f"{name}: deint (k_yadif_plane's output)", g_, enc.debug_deint(g_), dsrc[didx[g_]], c)
            _check_frame(f"{name}: denoised (k_dn_time's output)", g_, enc.debug_denoise(g_), want[g_], c)
        _check_state(name, enc, st)
    _check_jpegs(got, lambda i: _DN_JPEG(uniq[inv[i]].tobytes()), n, name)


# ================================================================= 4. the tile
def _tile_case(name, n=None, device_segs=None):
    """One submit of a tile StageCase (host, or device segments): debug_cell at frames 0, 32767, 32768 and n - 1,
    debug_planes at sheets 0, 32767, 32768 and m - 1, then every JPEG.  Returns the JPEGs."""
    c = cg.LONG_STAGE_CASES[name]
    g = c.geom
    ref = _Sheets(name, n, device_segs)
    n, m = ref.n, len(ref.members)
    assert m == cg.sheets_out(c, n)
    frames = _base(c)[ref.idx]
    with _open(name, n) as enc:
        assert sum(enc.frames_out(k) for _, k in (device_segs or [(0, n)])) == m
        if device_segs is None:
            enc.submit(frames, n)
        else:
            pools = [chain._device(frames[a:a + k], 1) for a, k in device_segs]
            enc.submit_segments([(t.data_ptr(), k) for t, (_, k) in zip(pools, device_segs)])
        assert len(enc.sync()) == m
        got = enc.fetch()
        for g_ in sorted({0, N - 1, N, n - 1}):
            if g_ < n:
                _same_planes(f"{name}: cell (k_tile_plane's input)", g_, split_i420(enc.debug_cell(g_), enc.dst_w, enc.dst_h, g.dst),
                             ref.cell(int(ref.idx[g_])))
        for j in sorted({0, N - 1, N, m - 1}):
            if j < m:
                _same_planes(f"{name}: sheet (k_tile_plane's output)", j, split_i420(enc.debug_planes(j), enc.enc_w, enc.enc_h, g.dst),
                             ref.sheet(ref.members[j])[0])
    _check_jpegs(got, lambda j: ref.sheet(ref.members[j])[1], m, name)
    assert len(ref.sheet.made) <= 2 * K + 8, len(ref.sheet.made)      # consecutive index pairs: the reference stayed small
    return got


def test_tile_one_frame_a_sheet_both_stages_split():
    """Regime A: 8 x 8 behind a 5:5 sharpen, tile=2x1:nb_frames=1 at n = 32768: m = 32768 sheets, cell 1 blank on every
    one; the sharpen and the tile both launch V alone."""
    c = cg.LONG_STAGE_CASES["tile_a"]
    assert (c.n, cg.sheets_out(c)) == (N, N) and _launches(N) == ["Y", "U", "V"]
    _tile_case("tile_a")


def test_tile_paired_behind_a_split_scale_and_sharpen():
    """Regime B: 16 x 16 -> 8 x 8, 5:5 sharpen, tile=2x1 at n = 40,000: the sws stage and the sharpen launch V alone,
    the tile's 20,000 sheets pair U and V (tuv1 is of the sheets)."""
    c = cg.LONG_STAGE_CASES["tile_b"]
    assert (c.n, cg.sheets_out(c)) == (40000, 20000)
    assert _launches(c.n) == ["Y", "U", "V"] and _launches(20000) == ["Y", "UV"]
    _tile_case("tile_b")


def test_tile_split_with_a_partial_last_sheet():
    """Regime C: 8 x 8, tile=2x1 at n = 65,535: m = 32,768, both split, the last sheet holds one frame."""
    c = cg.LONG_STAGE_CASES["tile_c"]
    assert (c.n, cg.sheets_out(c)) == (cg.MAX_BATCH, N) and _launches(c.n) == _launches(N) == ["Y", "U", "V"]
    _tile_case("tile_c")


def test_tile_four_device_segments_with_a_first_sheet_at_the_limit():
    """tile=2x1 over device segments of 12345, 20421, 32765 and 3 frames: 6173 + 10211 + 16383 + 2 = 32,769 sheets,
    three segments end in a partial sheet, and the last one's first sheet is sheet 32767."""
    name = "tile_segs"
    c = cg.LONG_STAGE_CASES[name]
    out = [tile_ref.frames_out(k, c.sheet) for k in c.segs]
    assert sum(k % 2 for k in c.segs) >= 2 and sum(out) >= N and sum(out[:3]) in (N - 1, N) and sum(c.segs) == c.n <= cg.MAX_BATCH
    assert _launches(c.n) == _launches(sum(out)) == ["Y", "U", "V"]
    _tile_case(name, device_segs=_segs(c.segs))


# ================================================================= 5. slot "out" alone, 6. the colour matrix's chain
def _chain_case(name):
    """One host submit of a StageCase without a denoiser: the stages' read-backs at frames 0 and 32767 in chain order
    (a difference names the first stage that differs), then every JPEG."""
    c = cg.LONG_STAGE_CASES[name]
    g, n, base = c.geom, c.n, _base(c)
    assert n == N and _launches(n) == ["Y", "U", "V"] and g.pad[1] >> cg.CHROMA_SHIFTS[g.dst][1] == 3
    idx = cg.long_frame_index(n)
    assert int(idx[0]) != int(idx[n - 1])
    ref = _chain_refs(name)
    with _open(name, n) as enc:
        enc.submit(base[idx], n)
        got = enc.fetch()
        for g_ in (0, n - 1):
            _check_chain_marks(name, enc, g_, ref(base[idx[g_]].tobytes()))
    _check_jpegs(got, lambda i: ref(base[idx[i]].tobytes())["jpeg"], n, name)


def _check_chain_marks(name, enc, g_, r):
    c = cg.LONG_STAGE_CASES[name]
    g = c.geom
    if c.cmat:
        _check_frame(f"{name}: cmat_out (k_cmat_frame's output, mapped by slot in)", g_, enc.debug_cmat_out(g_), r["lut_in"], c)
    elif c.lut_in:
        _check_frame(f"{name}: lut_in (k_lut_plane's slot-in output)", g_, enc.debug_lut_in(g_), r["lut_in"], c)
    if g.unsharp:
        _same_planes(f"{name}: presharp (the mapped sws output)", g_, split_i420(enc.debug_presharp(g_), enc.enc_w, enc.enc_h, g.dst),
                     r["presharp"])
    _same_planes(f"{name}: planes (the encoder's input)", g_, split_i420(enc.debug_planes(g_), enc.enc_w, enc.enc_h, g.dst), r["planes"])


def test_lut_out_alone_under_a_pad():
    """16 x 16 -> 8 x 8 at (4, 6) of 16 x 16, permutation tables in slot "out": k_lut_plane strided on d_scaled at the
    canvas stride; the chroma picture starts at row 3, so V's offset is no plane start."""
    _chain_case("lut_out")


def test_cmat_lut_in_scale_lut_out_unsharp_pad():
    """k_cmat_frame's grid of gxy * n in x (the frame by a multiply-high division), slot "in" in place behind it with V
    alone, then the scale, slot "out", the sharpen and the pad, every one reading the previous V launch."""
    _chain_case("cmat_chain")


# ================================================================= 7. the same chain behind yadif and hqdn3d
def test_full_chain_behind_yadif_and_hqdn3d():
    """yadif, hqdn3d, colormatrix, slot "in", scale, slot "out", unsharp, pad on 16 x 16 4:2:0, one host submit of 32,768
    frames: the colour matrix and slot "in" run in place in the denoiser's buffer."""
    name = "full_chain"
    c = cg.LONG_STAGE_CASES[name]
    g, n = c.geom, c.n
    assert n == N and _launches(n) == ["Y", "U", "V"]
    dsrc, didx = _deinterlaced(name, n, [(0, n)])
    want, st, uniq, inv = _denoised(name, n, [(0, n)])
    marks = (0, n - 2, n - 1)
    _assert_denoiser_reference_is_worth_it(name, want, uniq, marks)
    ref = _chain_refs(name)
    frames = _base(c)[cg.long_frame_index(n)]
    with _open(name, n) as enc:
        enc.submit(frames, n)
        got = enc.fetch()
        for g_ in marks:
            r = ref(want[g_].tobytes())
            _check_frame(f"{name}: deint (k_yadif_plane's output)", g_, enc.debug_deint(g_), dsrc[didx[g_]], c)
            _check_frame(f"{name}: lut_in (denoised, converted and mapped in place)", g_, enc.debug_lut_in(g_), r["lut_in"], c)
            _check_chain_marks(name, enc, g_, r)
        _check_state(name, enc, st)
    _check_jpegs(got, lambda i: ref(uniq[inv[i]].tobytes())["jpeg"], n, name)


# ================================================================= 8. k_frame_hist
def _same_hist(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint32, (what, got.shape, got.dtype)
    bad = np.argwhere(got != want)
    if bad.size:
        f, j = bad[0]
        pytest.fail(f"{what}: {len(bad)} of {want.size} counters differ, first frame {f} ({ls._side(f)}) plane {j // 256} value "
                    f"{j % 256}: got {got[f, j]}, want {want[f, j]}")


def test_frame_hist_past_32767_frames_a_call():
    """8 x 8 4:2:0, max_frames = 33000: three workgroups a frame, so t reaches 98,999 and hist_block's multiply-high
    division gives frames up to 32,999; calls of 32,768 and 33,000 host frames and one of 33,000 device frames from
    byte 1.  (The pinned result buffer is 33000 * 768 * 4 = 101 MB.)"""
    w, h, c, nmax = 8, 8, "420", 33000
    assert kernel_constant("kHistThreads") * kernel_constant("kHistVecs") * 16 == thumbnail_ref.HIST_WG_BYTES
    assert thumbnail_ref.hist_gpf(w, h, c) == 3 and 3 * nmax - 1 == 98999
    base = ls._base(w, h, c)
    href = thumbnail_ref.hist_ref(base, w, h, c)
    assert len({r.tobytes() for r in href}) == K
    idx = cg.long_frame_index(nmax)
    frames, want = base[idx], href[idx]
    with FrameHist(0, w, h, c, nmax) as hist:
        assert hist.frame_bytes == frames.shape[1]
        for n in (N, nmax):
            _same_hist(hist.count(frames[:n]), want[:n], f"{n} host frames")
        pool = chain._device(frames, 1)
        _same_hist(hist.count(device_ptr=pool.data_ptr(), nframes=nmax), want, f"{nmax} device frames from byte 1")


# ================================================================= 9. the two regimes side by side
def test_denoiser_largest_paired_launch_agrees_with_the_first_split_one():
    """The denoiser alone at n = 32767 (U and V in one launch: two planes of the time scan's grid) and at n = 32768:
    both equal the reference, and the same history gives the same bytes frame for frame."""
    n = N - 1
    assert cg.plane_launches(n) == [("Y", n), ("UV", 2 * n)] and 2 * n == cg.UV_LIMIT - 1
    paired = _denoiser_alone(n)
    split = _denoiser_alone(N)
    for i, (a, b) in enumerate(zip(paired, split)):
        assert a == b, (i, first_diff(a, b))
    assert len(paired) == n and len({bytes(j) for j in paired}) > K


def test_tile_largest_paired_launch_agrees_with_the_first_split_one():
    """Regime A's shape at n = m = 32767 (paired) and at 32768 (split)."""
    n = N - 1
    assert cg.sheets_out(cg.LONG_STAGE_CASES["tile_a"], n) == n and cg.plane_launches(n) == [("Y", n), ("UV", 2 * n)]
    paired = _tile_case("tile_a", n)
    split = _tile_case("tile_a")
    for i, (a, b) in enumerate(zip(paired, split)):
        assert a == b, (i, first_diff(a, b))
    assert len(paired) == n and len({bytes(j) for j in paired}) == K
