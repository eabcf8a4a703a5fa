"""Submits of more than 32,767 frames, where submit_impl (csrc/api.hip) gives V a launch of its own:
past 2 n <= 65535 every plane stage (the deinterlacer, the orientation, each pass of the sws stage,
the sharpen) launches luma, U alone (poff 0, nz = n) and V alone, and only the third launch adds the
chroma plane to the stage's offsets on the host.  A wrong or missing offset there gives JPEGs that
decode, with the wrong chroma, so every JPEG of every submit is compared byte for byte.  The same
submits take seg_frame, the 64-bit frame and plane offsets, k_scan_bits / k_scan_ff / k_write at n
workgroups, k_huff_build at 4 n and k_encode's task magic past 2^15 frames.

Frames are tiny (the smallest on which each stage exists, chain_geom.LONG_CASES) and cycle through
61 base frames of seeded noise, frame i being base (7 i + i // 1000) % 61, so the reference is
computed once per distinct input (for yadif: per distinct (prev, cur, next)) from the existing
references: yadif_ref, orient_ref / pad_ref / chroma_resample_ref (oriented_planes), unsharp_ref
and oracle.encode_frame.  U and V are noise of their own, so a V launch that reads U's plane, or
writes over it, changes bytes.  For the stages that have a debug read-back, frames 0, 32767, 32768
and n - 1 (those the submit has) are compared through debug_deint / debug_oriented /
debug_presharp / debug_planes before the JPEGs, so a failure names the stage.  Each case asserts from
chain_geom, before it opens a context, that its launch has three entries in plane_launches and that
its shape reaches the path it is listed for.  One context is open at a time."""
import numpy as np
import pytest

import chain_geom as cg
import test_gpu_chain as chain
from chain_geom import IN_PLACE, STREAM
from orient_ref import orient_frame, oriented_planes
from unsharp_ref import sharp_planes
from yadif_ref import deint_frame
from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes, split_i420

pytestmark = pytest.mark.gpu

N = cg.LONG          # 32768: the fewest frames with three launches a stage
K = cg.LONG_K
first_diff = chain.first_diff

_BASE = {}


def _base(w, h, c):
    """The 61 base frames of a source shape: every byte seeded noise, so U, V and Y all differ."""
    if (w, h, c) not in _BASE:
        f = np.random.default_rng([w, h, int(c), K]).integers(0, 256, (K, i420_frame_bytes(w, h, c)), dtype=np.uint8)
        for fr in f:
            y, u, v = split_i420(fr, w, h, c)
            assert (u != v).any() and (y.reshape(-1)[:u.size] != u.reshape(-1)).any()
        f.setflags(write=False)
        _BASE[(w, h, c)] = f
    return _BASE[(w, h, c)]


class _Ref:
    """The reference of one LongCase, per distinct input and made once: key b for base frame b, or
    (p 61 + b) 61 + n for base frame b between p and n under a deinterlacer."""

    def __init__(self, case, q=5):
        self.c, self.q, self.base, self.made = case, q, _base(case.w, case.h, case.src), {}

    def keys(self, idx, segs):
        """The key of every frame of a buffer whose frame j is base idx[j]; segs: (first, count) of
        each sequence in it (a frame's neighbours clamp to its own sequence)."""
        idx = np.asarray(idx, np.int64)
        if not self.c.deint:
            return idx.tolist()
        j = np.arange(len(idx))
        lo, hi = np.zeros(len(idx), np.int64), np.zeros(len(idx), np.int64)
        at = 0
        for first, count in segs:
            assert first == at and count >= 1
            lo[first:first + count], hi[first:first + count] = first, first + count - 1
            at += count
        assert at == len(idx)
        return ((idx[np.maximum(j - 1, lo)] * K + idx) * K + idx[np.minimum(j + 1, hi)]).tolist()

    def __call__(self, key):
        if key not in self.made:
            c, out = self.c, {}
            d = self.base[key % K if not c.deint else key // K % K]
            if c.deint:
                mode, tff = (2 if "nospatial" in c.deint else 0), int(c.deint.startswith("tff"))
                d = deint_frame(self.base[key // (K * K)], d, self.base[key % K], c.w, c.h, c.src, mode, tff)
                out["deint"] = d
            if c.orient:
                out["oriented"] = orient_frame(d, c.w, c.h, c.src, c.orient)
            if c.unsharp:
                out["presharp"], planes = sharp_planes(d, c.w, c.h, c.src, c.unsharp, c.orient, c.rect, c.dst, c.full,
                                                       c.dw, c.dh, c.pad)
            else:
                planes = oriented_planes(d, c.w, c.h, c.src, c.orient, c.rect, c.dst, c.full, c.dw, c.dh, c.pad)
            out["planes"] = planes
            out["jpeg"] = chain.ref_jpeg(planes, c.dst, self.q, c.kw.get("huffman", "default"), c.kw.get("rst", False))
            self.made[key] = out
        return self.made[key]


def _side(g):
    return "below 32768" if g < N else "at or above 32768"


def _check_jpegs(got, keys, ref, first=0, what=""):
    """Every JPEG against the reference of its input; `first`: the launch's frame index of got[0]."""
    assert len(got) == len(keys), (what, len(got), len(keys))
    for i, (a, k) in enumerate(zip(got, keys)):
        b = ref(k)["jpeg"]
        if a != b:
            pytest.fail(f"{what}: JPEG of frame {first + i} ({_side(first + i)}; base frame {k % K if not ref.c.deint else k // K % K}) "
                        f"differs: first_diff {first_diff(a, b)}, {len(a)} bytes against {len(b)}")


def _same_planes(what, g, got, want):
    for name, a, b in zip("YUV", got, want):
        bad = np.argwhere(np.asarray(a) != np.asarray(b))
        if bad.size:
            y, x = bad[0]
            pytest.fail(f"{what}: frame {g} ({_side(g)}) plane {name} differs first at (y={y}, x={x}): got {a[y, x]}, "
                        f"want {b[y, x]}, {len(bad)} of {a.size} differ")


def _check_marks(enc, ref, keys, enc_path, n, first=0, more=(), what=""):
    """The stages' read-backs of frames 0, 32767, 32768 and n - 1 of the launch (and `more`), those
    that lie in the last synced job: frames first .. first + len(keys) - 1 of the launch."""
    c = ref.c
    for g in sorted({0, N - 1, N, n - 1, *more}):
        i = g - first
        if not 0 <= i < len(keys):
            continue
        r = ref(keys[i])
        if c.deint:
            _same_planes(f"{what}: deint (k_yadif_plane's output)", g, split_i420(enc.debug_deint(i), c.w, c.h, c.src),
                         split_i420(r["deint"], c.w, c.h, c.src))
        if c.orient:
            _same_planes(f"{what}: oriented (k_orient_plane's output)", g,
                         split_i420(enc.debug_oriented(i), enc.or_w, enc.or_h, c.src),
                         split_i420(r["oriented"], enc.or_w, enc.or_h, c.src))
        if c.unsharp:
            _same_planes(f"{what}: presharp (the sws stage's output)", g,
                         split_i420(enc.debug_presharp(i), enc.enc_w, enc.enc_h, c.dst), r["presharp"])
        if not enc_path & IN_PLACE:
            _same_planes(f"{what}: planes (the encoder's input)", g,
                         split_i420(enc.debug_planes(i), enc.enc_w, enc.enc_h, c.dst), r["planes"])


def _assert_marks_differ(idx, n):
    """Frames 0, 32767, 32768 and n - 1 of a launch are different base frames."""
    marks = sorted({g for g in (0, N - 1, N, n - 1) if g < n})
    assert len({int(idx[g]) for g in marks}) == len(marks), (marks, [int(idx[g]) for g in marks])


def _open(name, max_batch, q=5, **extra):
    """A context on a LongCase, after asserting on the CPU what it must reach and on the context
    that it reports the same paths; (encoder, encode path)."""
    c = cg.LONG_CASES[name]
    want = cg.long_predict(c)[:2]
    if c.stream:
        assert want == (0, (cg.TILE, cg.TILE))
        assert all(cg.scale_variant(*s, *d, force_stream=True)[0] == "stream" for s, d in cg.long_plane_sizes(c))
        want = (0, (STREAM, STREAM))
    enc = MjpegEncoder(0, c.w, c.h, c.dw, c.dh, full_range=c.full, qscale=q, max_batch=max_batch, chroma=c.dst,
                       src_chroma=c.src, crop=c.rect, pad=c.pad, orient=c.orient, deint=cg.DEINT_FLAGS[c.deint] or None,
                       unsharp=c.unsharp, **c.kw, **extra)
    try:
        assert enc.frame_bytes == i420_frame_bytes(c.w, c.h, c.src)
        assert (enc.encode_path(), (enc.scale_path(0), enc.scale_path(1))) == want, name
        assert enc._L.mjg_debug_deint_flags(enc._h) == cg.DEINT_FLAGS[c.deint]
        assert (enc.debug_unsharp() is not None) == (c.unsharp is not None)
    except BaseException:
        enc.close()
        raise
    return enc, want[0]


def _host_case(name, n=N, halo=0, q=5):
    """One host submit of n frames of a LongCase (halo 3: n encoded frames out of n + 2): the marks'
    stages, then every JPEG.  Returns the JPEGs and the base frame of each."""
    c = cg.LONG_CASES[name]
    assert [p for p, _ in cg.plane_launches(n)] == ["Y", "U", "V"] and n <= cg.MAX_BATCH
    hp, hn = halo & 1, (halo >> 1) & 1
    idx = cg.long_frame_index(n + hp + hn)
    _assert_marks_differ(idx[hp:], n)
    ref = _Ref(c, q)
    keys = ref.keys(idx, [(0, n + hp + hn)])[hp:hp + n]
    frames = ref.base[idx]
    enc, enc_path = _open(name, n, q)
    with enc:
        enc.submit(frames, n, halo=halo)
        got = enc.fetch()
        _check_marks(enc, ref, keys, enc_path, n, what=name)
    _check_jpegs(got, keys, ref, what=name)
    return got, idx[hp:hp + n]


# ================================================================= in place: no plane stage (the control)
@pytest.mark.parametrize("n", [N, cg.MAX_BATCH], ids=["32768", "65535"])
def test_in_place_control(n):
    """8 x 8 4:2:0 read in place: k_scan_bits, k_count_ff, k_scan_ff and k_write at n workgroups, the
    last-ticket placement over n frame sizes, the 64-bit frame_offsets; again at max_batch = 65535,
    the most open accepts."""
    assert cg.enc_geom(8, 8, "420", False, n).ntasks == n
    _host_case("in_place", n)


def test_huffman_optimal_every_frame_its_own_tables():
    """k_huff_build at 4 n = 131,072 workgroups; every frame carries its own DHT."""
    assert 4 * N == 131072
    got, idx = _host_case("optimal")
    assert len({bytes(g) for g in got}) == K      # 61 distinct inputs, 61 distinct JPEGs


def test_rst_two_segments_a_frame():
    """8 x 32: two MCU rows, nseg = 2: k_scan_bits_seg and seg_off at 65,536 segments."""
    g = cg.enc_geom(8, 32, "420", True, N)
    assert (g.nseg, g.nseg * N, g.ntasks) == (2, 65536, 65536)
    _host_case("rst")


# ================================================================= the sws stage
@pytest.mark.parametrize("name", ["scale_tv", "scale_pc", "scale_up_444"])
def test_tile_scale_kernel(name):
    """k_scale: 16 x 16 -> 8 x 8 4:2:0 in tv and in pc range (luma <8, 5, 64>, chroma the generic
    tile; range 1, 2 and 0 in luma, U alone and V alone) and 8 x 8 -> 12 x 12 4:4:4 (<4, 3>)."""
    c = cg.LONG_CASES[name]
    assert [cg.scale_variant(*s, *d)[:2] for s, d in cg.long_plane_sizes(c)] == (
        [("tile", (4, 3, 32))] * 2 if name == "scale_up_444" else [("tile", (8, 5, 64)), ("tile", (0, 0, 32))])
    _host_case(name)


def test_stream_scale_kernel(monkeypatch):
    """k_scale_stream on the same 16 x 16 -> 8 x 8 (MJG_SCALE_STREAM=1)."""
    monkeypatch.setenv("MJG_SCALE_STREAM", "1")
    _host_case("scale_stream")


@pytest.mark.parametrize("name", ["pix_fmt_copy", "rect_copy"])
def test_plane_copy(name):
    """k_plane_copy: 4:4:4 -> 4:2:0 at 8 x 8 (the luma copied, the chroma through the 2:1 tile), and its
    rectangle form: 8 x 8 at (4, 0) of 16 x 8."""
    c = cg.LONG_CASES[name]
    assert cg.long_predict(c)[2] == (name == "rect_copy")
    assert cg.copy_pad_cells(c.w, c.h, c.src, c.rect, c.dst, None, None, None, False) == {("copy", 1, name == "rect_copy")}
    _host_case(name)


@pytest.mark.parametrize("name", ["pad_copy", "pad_scale"])
def test_pad(name):
    """k_pad_plane: an 8 x 8 picture copied onto a 16 x 16 canvas, and the border around a 16 x 16 -> 8 x 8
    picture; the picture at (4, 6), so the chroma picture starts at row 3 and the V launch's d_off
    is no plane start."""
    c = cg.LONG_CASES[name]
    assert c.pad[1] >> cg.CHROMA_SHIFTS[c.dst][1] != 0
    cells = cg.copy_pad_cells(c.w, c.h, c.src, c.rect, c.dst, c.dw, c.dh, c.pad, False)
    assert cells == ({("pad", 1, True), ("pad", 2, True)} if name == "pad_copy" else {("pad", 0, False)})
    _host_case(name)


# ================================================================= the orientation, read in place
@pytest.mark.parametrize("name", ["hflip", "transpose"])
def test_orientation_alone(name):
    """k_orient_plane<T = 0> (hflip) and <T = 1> (transpose) on 24 x 8 4:2:0, chroma 12 x 4; k_encode
    reads d_orient in place."""
    c = cg.LONG_CASES[name]
    assert cg.orient_cells(c.orient)[0] == (name == "transpose") and cg.long_predict(c)[0] == IN_PLACE
    _host_case(name)


# ================================================================= the deinterlacer
def test_yadif_one_host_submit():
    """Mode 0, tff, 8 x 8 4:2:0 (chroma 4 x 4, above the 3 x 3 floor): one submit, one sequence."""
    _host_case("yadif")


def test_yadif_halo_submit_without_the_spatial_check():
    """Mode 2, tff: n encoded frames out of n + 2, both halo bits set."""
    _host_case("yadif_nospatial", halo=3)


def test_yadif_four_segments_with_a_boundary_at_the_limit():
    """submit_segments of four device segments, 38,000 frames: segment 3 starts at frame 32767, so
    frames 32766 | 32767 see no neighbour across the boundary and 32768 is a second frame."""
    name, lens = "yadif", (12345, 20422, 3000, 2233)
    c = cg.LONG_CASES[name]
    n = sum(lens)
    cuts = np.cumsum((0,) + lens)
    assert n == 38000 and cuts[2] == N - 1 and len(lens) == cg.MAX_SEGS
    assert [p for p, _ in cg.plane_launches(n)] == ["Y", "U", "V"]
    idx = cg.long_frame_index(n)
    _assert_marks_differ(idx, n)
    ref = _Ref(c)
    keys = ref.keys(idx, [(int(a), int(b - a)) for a, b in zip(cuts, cuts[1:])])
    whole = ref.keys(idx, [(0, n)])
    assert [keys[g] != whole[g] for g in (N - 3, N - 2, N - 1, N)] == [False, True, True, False]
    frames = ref.base[idx]
    segs = [chain._device(frames[a:b], 1) for a, b in zip(cuts, cuts[1:])]
    enc, enc_path = _open(name, n)
    with enc:
        assert len(lens) <= enc.max_segments
        enc.submit_segments([(t.data_ptr(), int(k)) for t, k in zip(segs, lens)])
        got = enc.fetch()
        _check_marks(enc, ref, keys, enc_path, n, more=(N - 2, int(cuts[1]) - 1, int(cuts[1]), int(cuts[3])), what=name)
    _check_jpegs(got, keys, ref, what=name)


# ================================================================= the sharpen
@pytest.mark.parametrize("name", ["unsharp55", "unsharp_chroma"])
def test_unsharp(name):
    """k_unsharp_plane behind the plane copy at 8 x 8: <5, 5> on all planes, and 5:5:0 / 3:5:0.7, where
    the luma launch only copies and U alone, V alone filter with sizes given at run time."""
    _host_case(name)


# ================================================================= the chain
def test_chain_every_stage_reads_the_previous_v_launch():
    """yadif, transpose, crop, scale, unsharp, pad on 24 x 16 4:2:0: 16 x 24 oriented, (2, 2, 12, 20)
    of it to 8 x 12, <5, 5> on all planes, at (4, 6) of 16 x 24."""
    c = cg.LONG_CASES["chain"]
    assert c.deint and c.orient & 1 and c.rect and c.dw and c.unsharp and c.pad
    _host_case("chain")


# ================================================================= two held submits in one launch
def test_merged_launch_of_two_submits_below_the_limit():
    """merge=True, max_batch = 20000, device submits of 20,000 and 19,999 frames behind a scale and a
    sharpen: one launch of 39,999 frames in two segments, 2 n > 65535 although neither submit alone
    is; each job's fetch returns its own frames."""
    name, lens = "scale_sharp", (20000, 19999)
    c = cg.LONG_CASES[name]
    n = sum(lens)
    assert all(len(cg.plane_launches(k)) == 2 for k in lens) and [p for p, _ in cg.plane_launches(n)] == ["Y", "U", "V"]
    assert cg.merged_frames(lens[0]) >= n
    idx = cg.long_frame_index(n)
    _assert_marks_differ(idx, n)
    ref = _Ref(c)
    keys = ref.keys(idx, [(0, n)])
    frames = ref.base[idx]
    jobs = [chain._device(frames[:lens[0]], 1), chain._device(frames[lens[0]:], 1)]
    enc, enc_path = _open(name, lens[0], merge=True, timing=True)
    got = []
    with enc:
        assert enc.depth == cg.SLOTS * cg.MERGE == 2 * enc.host_depth      # open did not cap the merge
        for t, k in zip(jobs, lens):
            enc.submit(device_ptr=t.data_ptr(), nframes=k)
        first = 0
        for k in lens:
            sizes = enc.sync()
            assert len(sizes) == k
            part = enc.fetch()
            if enc.pending == 0:      # (a read-back syncs whatever is pending first: the last job's frames only,
                #                        20000 .. 39998 of the launch, which hold 32767, 32768 and n - 1)
                _check_marks(enc, ref, keys[first:first + k], enc_path, n, first=first, what=name)
            _check_jpegs(part, keys[first:first + k], ref, first=first, what=name)
            got += part
            first += k
        assert first - lens[1] < N - 1 and enc.kernel_times()[1] == 1      # both jobs in one launch
    assert len(got) == n


# ================================================================= the two regimes side by side
def test_the_largest_paired_launch_agrees_with_the_first_split_one():
    """The scale + sharpen shape at n = 32767 (U and V in one grid of 65,534) and at n = 32768 (a
    launch each): both equal the reference, and frame for frame the same base frame gives the same
    bytes in either regime."""
    name = "scale_sharp"
    n = N - 1
    assert cg.plane_launches(n) == [("Y", n), ("UV", 2 * n)] and 2 * n == cg.UV_LIMIT - 1
    c = cg.LONG_CASES[name]
    idx = cg.long_frame_index(n)
    assert len({int(idx[0]), int(idx[n - 1])}) == 2
    ref = _Ref(c)
    keys = ref.keys(idx, [(0, n)])
    enc, enc_path = _open(name, n)
    with enc:
        enc.submit(ref.base[idx], n)
        paired = enc.fetch()
        _check_marks(enc, ref, keys, enc_path, n, what=name + " paired")
    _check_jpegs(paired, keys, ref, what=name + " paired")
    by_base = {}
    for b, jp in zip(idx.tolist(), paired):
        assert by_base.setdefault(b, jp) == jp
    split, idx2 = _host_case(name, N)
    assert len(by_base) == K
    for i, (b, jp) in enumerate(zip(idx2.tolist(), split)):
        assert jp == by_base[b], (i, b, first_diff(jp, by_base[b]))
