"""`-vf hqdn3d` on the GPU (MjpegEncoder(denoise=...): k_dn_rows, k_dn_cols and k_dn_time behind the
deinterlacer), byte for byte against tests/hqdn3d_ref.py: debug_denoise() of every frame and
debug_denoise_state(), then the JPEGs of whatever reads the denoised frames against the existing references
run on the reference's denoised frames."""
import io

import numpy as np
import pytest

import colormatrix_ref
import eq_ref
import hqdn3d_ref as R
from yadif_ref import deint_frames, deint_ref
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes, split_i420

pytestmark = pytest.mark.gpu

NF = R.NFRAMES
TABS = np.stack(R.tables(*R.STRENGTHS))      # four distinct strengths: a swapped table shows
TABS.setflags(write=False)


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


_SRC, _DN = {}, {}


def _frames(kind, w, h, c):
    key = (kind, w, h, c)
    if key not in _SRC:
        f = R.make_frames(kind, w, h, c, NF)
        f.setflags(write=False)
        _SRC[key] = f
    return _SRC[key]


def _dn(kind, w, h, c, lo=0, hi=NF):
    """(denoised frames, state) of the sequence _frames(...)[lo:hi], computed once."""
    key = (kind, w, h, c, lo, hi)
    if key not in _DN:
        out, st = R.denoise(_frames(kind, w, h, c)[lo:hi], w, h, c, TABS)
        out.setflags(write=False), st.setflags(write=False)
        _DN[key] = (out, st)
    return _DN[key]


def _check_frames(enc, want, w, h, c, what=""):
    """debug_denoise() of the last synced submit against the reference, naming the first differing sample."""
    for i, wf in enumerate(want):
        got = enc.debug_denoise(i)
        assert got.size == wf.size
        if (got == wf).all():
            continue
        for name, a, b in zip("YUV", split_i420(got, w, h, c), split_i420(wf, w, h, c)):
            bad = np.argwhere(a != b)
            if bad.size:
                y, x = bad[0]
                print(f"frame {i} plane {name}: first difference at y={y} x={x}: got {a[y, x]}, want {b[y, x]}, "
                      f"{len(bad)} of {a.size} differ")
                pytest.fail(f"hqdn3d {what} {w}x{h} {c}: frame {i} plane {name} differs first at (y={y}, x={x})")


def _check_state(enc, want, w, h, c, what=""):
    got = enc.debug_denoise_state()
    assert got.shape == want.shape and got.dtype == np.uint16
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, w, h, c, len(bad), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def _device(frames):
    """The frames on the GPU, from byte 1 of their allocation."""
    import torch
    pool = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda:0")
    pool[1:] = torch.from_numpy(np.ascontiguousarray(frames).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return pool


def _enc(w, h, c, max_batch=NF, **kw):
    return MjpegEncoder(0, w, h, full_range=kw.pop("full_range", True), qscale=5, max_batch=max_batch, chroma=c,
                        denoise=TABS, **kw)


# ------------------------------------------------------------------------- 1. the denoiser alone
@pytest.mark.parametrize("kind", R.CONTENTS)
@pytest.mark.parametrize("w,h,c", R.GPU_SHAPES, ids=lambda v: str(v))
def test_denoiser_alone_matches_reference(w, h, c, kind):
    """One host submit of five frames: the denoised bytes, the carried state, and the JPEGs (k_encode reads the
    denoised frames in place)."""
    frames = _frames(kind, w, h, c)
    want, st = _dn(kind, w, h, c)
    with _enc(w, h, c) as enc:
        assert enc.frame_bytes == i420_frame_bytes(w, h, c)
        assert (enc.scale_path(0), enc.encode_path() & 1) == (0, 1)
        got = enc.encode(frames)
        _check_frames(enc, want, w, h, c, kind)
        _check_state(enc, st, w, h, c, kind)
    if kind == "noise":
        _check(got, [deint_ref(f, w, h, c, full=True, qscale=5) for f in want])
        assert not (want == frames).all()      # the tables act on this content


@pytest.mark.parametrize("w,h,c", [(33, 17, "444"), (130, 66, "422"), (4100, 5, "420")], ids=lambda v: str(v))
def test_device_frames_from_byte_1(w, h, c):
    frames = _frames("noise", w, h, c)
    want, st = _dn("noise", w, h, c)
    pool = _device(frames)
    with _enc(w, h, c) as enc:
        enc.submit(device_ptr=pool.data_ptr() + 1, nframes=NF)
        got = enc.fetch()
        _check_frames(enc, want, w, h, c, "device")
        _check_state(enc, st, w, h, c, "device")
    _check(got, [deint_ref(f, w, h, c, full=True, qscale=5) for f in want])


# ------------------------------------------------------------------------- 2. sequences
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w,h,c", [(33, 17, "444"), (130, 66, "422")], ids=lambda v: str(v))
def test_continued_submits_equal_one_submit(w, h, c, dev):
    """2 + 3 with cont: the five-frame sequence.  2 + 3 plain: two sequences, which differ from it."""
    frames = _frames("noise", w, h, c)
    fb = frames.shape[1]
    want, st = _dn("noise", w, h, c)
    a, _ = _dn("noise", w, h, c, 0, 2)
    b, bst = _dn("noise", w, h, c, 2, 5)
    assert not (b == want[2:]).all()
    pool = _device(frames) if dev else None

    def submit(enc, lo, hi, **kw):
        if dev:
            enc.submit(device_ptr=pool.data_ptr() + 1 + lo * fb, nframes=hi - lo, **kw)
        else:
            enc.submit(frames[lo:hi], **kw)

    with _enc(w, h, c, max_batch=3) as enc:
        submit(enc, 0, 2)
        enc.sync()
        _check_frames(enc, want[:2], w, h, c, "first piece")
        submit(enc, 2, 5, cont=True)
        enc.sync()
        _check_frames(enc, want[2:], w, h, c, "continued piece")
        _check_state(enc, st, w, h, c, "2 + 3 continued")
        submit(enc, 0, 2)               # a plain submit starts over, whatever the state holds
        enc.sync()
        _check_frames(enc, a, w, h, c, "plain again")
        submit(enc, 2, 5)
        enc.sync()
        _check_frames(enc, b, w, h, c, "a sequence of its own")
        _check_state(enc, bst, w, h, c, "2 + 3 plain")
        assert len(enc.encode(frames)) == NF      # more frames than max_batch: encode() continues by itself
        _check_state(enc, st, w, h, c, "encode()")


def test_each_segment_is_a_sequence_of_its_own():
    w, h, c = 33, 17, "444"
    frames = _frames("noise", w, h, c)
    pools = [_device(frames[:3]), _device(frames[3:])]
    a, _ = _dn("noise", w, h, c, 0, 3)
    b, bst = _dn("noise", w, h, c, 3, 5)
    with _enc(w, h, c) as enc:
        enc.submit_segments([(pools[0].data_ptr() + 1, 3), (pools[1].data_ptr() + 1, 2)])
        got = enc.fetch()
        _check_frames(enc, np.concatenate([a, b]), w, h, c, "segments 3 + 2")
        _check_state(enc, bst, w, h, c, "segments 3 + 2")
    _check(got, [deint_ref(f, w, h, c, full=True, qscale=5) for f in np.concatenate([a, b])])
    assert not (b == _dn("noise", w, h, c)[0][3:]).all()


def test_four_submits_in_a_row_keep_the_state_in_order():
    """Four device submits of five 640 x 360 frames each (the same five, so a sequence of twenty), every one but
    the first continued, the launch queue kept full: two in flight on the two slots' streams, one synced only
    when the queue has no room, which is all the library allows.  While a submit's time scan runs over its
    five frames the next submit's row and column scans are already queued beside it, and its time scan
    follows on the other stream: the state goes from slot to slot by the event alone."""
    w, h, c = 640, 360, "420"
    frames = _frames("noise", w, h, c)
    seq = np.tile(frames, (4, 1))
    want, st = R.denoise(seq, w, h, c, TABS)
    ref = [deint_ref(f, w, h, c, full=True, qscale=5) for f in want]
    pool = _device(frames)
    got = []
    with _enc(w, h, c) as enc:
        assert enc.depth == 2
        for k in range(4):
            if enc.pending == enc.depth:
                enc.sync()
                got += enc.fetch()
            enc.submit(device_ptr=pool.data_ptr() + 1, nframes=NF, cont=k > 0)
        while enc.pending:
            enc.sync()
            got += enc.fetch()
        _check_frames(enc, want[15:], w, h, c, "the last of four")
        _check_state(enc, st, w, h, c, "four submits")
    _check(got, ref)
    assert not (want[15:] == want[:5]).all()      # the fourth pass over the same frames carries the first three


def test_segments_behind_yadif_are_sequences_of_their_own():
    """yadif, hqdn3d through submit_segments (3 + 2): the deinterlacer leaves both segments in one buffer, and
    the denoiser still starts the second from its own samples."""
    w, h, c = 130, 66, "422"
    frames = _frames("noise", w, h, c)
    pools = [_device(frames[:3]), _device(frames[3:])]
    da, db = deint_frames(frames[:3], w, h, c, 0, 1), deint_frames(frames[3:], w, h, c, 0, 1)
    a, _ = R.denoise(da, w, h, c, TABS)
    b, bst = R.denoise(db, w, h, c, TABS)
    joined, _ = R.denoise(np.concatenate([da, db]), w, h, c, TABS)
    assert not (joined[3:] == b).all()           # one sequence over both would show
    want = np.concatenate([a, b])
    with _enc(w, h, c, deint=_lib.MJG_DEINT_YADIF) as enc:
        enc.submit_segments([(pools[0].data_ptr() + 1, 3), (pools[1].data_ptr() + 1, 2)])
        got = enc.fetch()
        _check_frames(enc, want, w, h, c, "yadif, segments 3 + 2")
        _check_state(enc, bst, w, h, c, "yadif, segments 3 + 2")
        single = []
        for t, n in zip(pools, (3, 2)):
            enc.submit(device_ptr=t.data_ptr() + 1, nframes=n)
            single += enc.fetch()
    _check(got, [deint_ref(f, w, h, c, full=True, qscale=5) for f in want])
    _check(got, single)


def test_behind_yadif_with_halo_and_cont():
    """yadif, hqdn3d: 5 frames as 2 + 2 + 1 halo submits, the later ones continued; the denoiser sees the
    deinterlaced frames."""
    w, h, c = 130, 66, "422"
    frames = _frames("noise", w, h, c)
    d = deint_frames(frames, w, h, c, 0, 1)
    want, st = R.denoise(d, w, h, c, TABS)
    got = []
    with _enc(w, h, c, max_batch=2, deint=_lib.MJG_DEINT_YADIF) as enc:
        for k, (lo, hi, n, halo, first) in enumerate([(0, 3, 2, 2, 0), (1, 5, 2, 3, 2), (3, 5, 1, 1, 4)]):
            enc.submit(frames[lo:hi], halo=halo, cont=k > 0)
            got += enc.fetch()
            _check_frames(enc, want[first:first + n], w, h, c, f"halo {halo}")
            for i in range(n):
                assert (enc.debug_deint(i) == d[first + i]).all()      # the caller's frames and yadif's stay as they are
        _check_state(enc, st, w, h, c, "yadif")
        one = enc.encode(frames)
    _check(got, [deint_ref(f, w, h, c, full=True, qscale=5) for f in want])
    _check(one, got)


# ------------------------------------------------------------------------- 3. in front of each reader
def test_in_front_of_the_transposing_orientation():
    w, h, c = 130, 66, "420"
    want, _ = _dn("noise", w, h, c)
    with _enc(w, h, c, orient=3) as enc:
        got = enc.encode(_frames("noise", w, h, c))
        _check_frames(enc, want, w, h, c, "orient")
    _check(got, [deint_ref(f, w, h, c, 3, full=True, qscale=5) for f in want])


def test_in_front_of_the_scale():
    w, h, c = 130, 66, "420"
    want, _ = _dn("noise", w, h, c)
    sar = profile.scaled_sar((1, 1), (w, h), (64, 32))
    with _enc(w, h, c, dst_w=64, dst_h=32, sar=sar, full_range=False) as enc:
        assert enc.scale_path(0) == 2
        got = enc.encode(_frames("noise", w, h, c))
        _check_frames(enc, want, w, h, c, "scale")
    _check(got, [deint_ref(f, w, h, c, 0, None, c, False, 64, 32, qscale=5, sar=sar) for f in want])


def test_cmat_and_lut_in_run_in_place_behind_it():
    w, h, c = 130, 66, "422"
    want, _ = _dn("noise", w, h, c)
    coefs = colormatrix_ref.coefs("bt709", "bt601")
    tabs = eq_ref.perm_tables(3)
    mapped = eq_ref.map_frames(colormatrix_ref.convert_frames(want, w, h, c, coefs), w, h, c, tabs)
    with _enc(w, h, c, cmat=coefs, lut_in=tabs, full_range=False) as enc:
        got = enc.encode(_frames("noise", w, h, c))
        for i in range(NF):
            assert (enc.debug_lut_in(i) == mapped[i]).all()
            assert (enc.debug_denoise(i) == mapped[i]).all()     # in place in the denoiser's buffer
    _check(got, [deint_ref(f, w, h, c, full=False, qscale=5) for f in mapped])


# ------------------------------------------------------------------------- 4. the worker
def _y4m(frames, w, h, field="p"):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 I{field} A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def test_worker_yadif_hqdn3d_scale_across_three_batches():
    w, h, c = 130, 66, "420"
    frames = _frames("noise", w, h, c)
    spec = "2.5:1.5:7:3"
    args = ["-vf", f"yadif,hqdn3d={spec},scale=32:16"] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    opts = worker.Options.from_env({"MJG_WORKER_BATCH": "2"})
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m(frames, w, h, "t")), stdout=out, stderr=err, opts=opts)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue()
    packets = [d for _, d in container.MkvReader(io.BytesIO(out.getvalue())).frames(1)]
    tabs = profile.hqdn3d_tables({"ls": 2.5, "cs": 1.5, "lt": 7.0, "ct": 3.0})
    dn, _ = R.denoise(deint_frames(frames, w, h, c, 0, 1), w, h, c, tabs)
    sar = profile.scaled_sar((1, 1), (w, h), (32, 16))
    want = [deint_ref(f, w, h, c, 0, None, c, False, 32, 16, qscale=profile.effective_qscale(5), sar=sar) for f in dn]
    _check(packets, want)
    one, _ = R.denoise(deint_frames(frames, w, h, c, 0, 1)[2:], w, h, c, tabs)
    assert not (one[0] == dn[2]).all()       # a batch that restarted the sequence would show


# ------------------------------------------------------------------------- 5. errors
def test_cont_is_refused_without_a_denoiser_and_before_any_submit():
    w, h, c = 33, 17, "444"
    frames = _frames("noise", w, h, c)
    with MjpegEncoder(0, w, h, full_range=True, qscale=5, max_batch=NF, chroma=c) as enc:
        with pytest.raises(_lib.MjgError) as e:
            enc.submit(frames[:2], cont=True)
        assert e.value.code == _lib.MJG_E_INVALID and "denoiser" in str(e.value)
        for call in (enc.debug_denoise, enc.debug_denoise_state):
            with pytest.raises(_lib.MjgError) as e:
                call()
            assert e.value.code == _lib.MJG_E_STATE
        assert len(enc.encode(frames[:1])) == 1      # the context is unharmed
    with _enc(w, h, c) as enc:
        with pytest.raises(_lib.MjgError) as e:
            enc.submit(frames[:2], cont=True)
        assert e.value.code == _lib.MJG_E_INVALID and "before any submit" in str(e.value)
        assert enc.pending == 0
        enc.submit(frames[:2])
        enc.submit(frames[2:], cont=True)
        enc.sync(), enc.sync()
        _check_state(enc, _dn("noise", w, h, c)[1], w, h, c, "after the refusal")
