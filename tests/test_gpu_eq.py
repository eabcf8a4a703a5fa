"""The table stage on the GPU (MjpegEncoder(lut_in=, lut_out=): k_lut_plane in front of the sws stage and
on its output), byte for byte.  Library-level cases use seeded random permutation tables, different
for Y, U and V, with t[0] != 0 and t[128] != 128 (eq_ref.perm_tables): a mis-indexed byte, a U table
used for V and a map that spills onto a pad's border all change bytes.  Every case compares
debug_lut_in() first (k_lut_plane's slot-"in" output), then debug_presharp() / debug_planes() where
the sws stage runs, then the JPEGs against the composed reference of the existing stages
(orient_ref, crop_ref, chroma_resample_ref, unsharp_ref, pad_ref, yadif_ref, oracle) on the mapped
frames, so a failure names the stage and the first differing sample.  tools/lut_host_check.py walks
the launches of the shapes here on the CPU under AddressSanitizer."""
import io

import numpy as np
import pytest

import eq_ref
import oracle
from chroma_resample_ref import composed_planes
from crop_ref import crop_frame
from orient_ref import orient_frame, oriented_size
from pad_ref import pad_planes
from unsharp_ref import unsharp_planes
from yadif_ref import deint_frames
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import MjpegEncoder, i420_frame_bytes, split_i420

pytestmark = pytest.mark.gpu

NF = 3
T_IN = eq_ref.perm_tables(101)
T_OUT = eq_ref.perm_tables(202)
ID3 = np.stack([eq_ref.IDENTITY] * 3)


def test_the_tables_are_what_the_cases_need():
    for t in (T_IN, T_OUT):
        assert t.shape == (3, 256) and all(sorted(r.tolist()) == list(range(256)) for r in t)
        assert all(r[0] != 0 and r[128] != 128 for r in t)
        assert (t[0] != t[1]).any() and (t[1] != t[2]).any() and (t[0] != t[2]).any()
    assert (T_IN != T_OUT).any()


def first_diff(a: bytes, b: bytes):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i
    return n if len(a) != len(b) else -1


def _check(got, ref, what=""):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a == b, (what, i, len(a), len(b), first_diff(a, b))


_SRC = {}


def _frames(w, h, c, n=NF):
    """n frames per shape and format, made once: seeded noise in which every plane holds every byte
    value (where it has 256 bytes), U and V noise of their own."""
    if (w, h, c, n) not in _SRC:
        rng = np.random.default_rng([w, h, int(c), n])
        f = rng.integers(0, 256, (n, i420_frame_bytes(w, h, c)), dtype=np.uint8)
        for fr in f:
            at = 0
            for p in split_i420(fr, w, h, c):
                if p.size >= 256:
                    fr[at:at + 256] = rng.permutation(256).astype(np.uint8)
                at += p.size
        f.setflags(write=False)
        _SRC[(w, h, c, n)] = f
    return _SRC[(w, h, c, n)]


def _same(what, i, got, want, w, h, c):
    for name, a, b in zip("YUV", split_i420(got, w, h, c), split_i420(want, w, h, c)):
        bad = np.argwhere(a != b)
        if bad.size:
            y, x = bad[0]
            print(f"{what}: frame {i} plane {name}: first difference at y={y} x={x}: got {a[y, x]}, want {b[y, x]}, "
                  f"{len(bad)} of {a.size} differ")
            pytest.fail(f"{what}: frame {i} plane {name} differs first at (y={y}, x={x})")


def chain_ref(frame, w, h, src, lut_in=None, lut_out=None, orient=0, rect=None, dst=None, full=False, dw=None, dh=None,
              us=None, pad=None, qscale=5, sar=(1, 1), huffman="default", rst=False):
    """One decoded (or deinterlaced) frame through the composed reference: the orientation, the
    slot-"in" tables on the whole oriented frame, the crop, the sws stage, the slot-"out" tables on
    its picture, the unsharp, the pad, the encoder.  Returns {"lut_in": the mapped frame or None,
    "presharp": the planes in front of the unsharp (on the canvas), "planes": the encoder's input,
    "jpeg"}."""
    dst = dst or src
    ow, oh = oriented_size(w, h, orient)
    f = orient_frame(frame, w, h, src, orient)
    out = {"lut_in": None}
    if lut_in is not None:
        f = out["lut_in"] = eq_ref.map_frames(f, ow, oh, src, lut_in)
    rect = rect or (0, 0, ow, oh)
    planes = composed_planes(crop_frame(f, ow, oh, src, rect), rect[2], rect[3], src, dst, full, dw or rect[2], dh or rect[3])
    if lut_out is not None:
        planes = tuple(np.asarray(lut_out[p], np.uint8)[pl] for p, pl in enumerate(planes))
    pre = planes
    if us is not None:
        planes = unsharp_planes(*planes, us)
    if pad is not None:
        pre, planes = pad_planes(*pre, dst, *pad), pad_planes(*planes, dst, *pad)
    out["presharp"], out["planes"] = pre, planes
    out["jpeg"] = oracle.encode_frame(*planes, full_range=True, qscale=qscale, sar=sar, huffman=huffman, chroma=dst, rst=rst)
    return out


def _check_stages(enc, refs, c, dst, us):
    """debug_lut_in, then debug_presharp / debug_planes where they exist, against refs (chain_ref per frame)."""
    for i, r in enumerate(refs):
        if r["lut_in"] is not None:
            _same("lut_in (k_lut_plane's slot-in output)", i, enc.debug_lut_in(i), r["lut_in"], enc.or_w, enc.or_h, c)
    if enc.encode_path() & 1:      # k_encode reads the frames in place: no sws stage to read back
        return
    for i, r in enumerate(refs):
        if us is not None:
            got = split_i420(enc.debug_presharp(i), enc.enc_w, enc.enc_h, dst)
            for name, a, b in zip("YUV", got, r["presharp"]):
                assert (a == b).all(), ("presharp (the mapped sws output)", i, name, np.argwhere(a != b)[0].tolist())
        got = split_i420(enc.debug_planes(i), enc.enc_w, enc.enc_h, dst)
        for name, a, b in zip("YUV", got, r["planes"]):
            assert (a == b).all(), ("planes (the encoder's input)", i, name, np.argwhere(a != b)[0].tolist())


def _run(w, h, c, lut_in=None, lut_out=None, full=False, dw=None, dh=None, dst=None, rect=None, pad=None, orient=0,
         us=None, deint=None, chain=None, device=False, q=5, env=None, monkeypatch=None, want_paths=None, **enc_kw):
    """One encoder, one encode of the shape's frames (from a host buffer, or from a device pointer at
    byte 1 of its allocation): every stage against the reference.  chain: what the stages behind the
    deinterlacer see."""
    src_frames = _frames(w, h, c)
    chain = src_frames if chain is None else chain
    ow, oh = oriented_size(w, h, orient)
    in_size = rect[2:] if rect else (ow, oh)
    sar = profile.scaled_sar((1, 1), in_size, (dw or in_size[0], dh or in_size[1]))
    refs = [chain_ref(f, w, h, c, lut_in, lut_out, orient, rect, dst, full, dw, dh, us, pad, q, sar, **enc_kw) for f in chain]
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    with MjpegEncoder(0, w, h, dw, dh, full_range=full, qscale=q, sar=sar, max_batch=NF, chroma=dst or c, src_chroma=c,
                      crop=rect, pad=pad, orient=orient, deint=deint, unsharp=us, lut_in=lut_in, lut_out=lut_out,
                      **enc_kw) as enc:
        for slot, t in (("in", lut_in), ("out", lut_out)):
            got = enc.debug_lut(slot)
            assert (got is None) == (t is None) and (t is None or (got == t).all()), slot
        if want_paths is not None:
            assert (enc.scale_path(0), enc.scale_path(1), enc.encode_path() & 3) == want_paths
        if device:
            import torch
            pool = torch.zeros(src_frames.size + 1, dtype=torch.uint8, device="cuda:0")
            pool[1:] = torch.from_numpy(src_frames.reshape(-1).copy()).to("cuda:0")
            torch.cuda.synchronize()
            enc.submit(device_ptr=pool.data_ptr() + 1, nframes=len(src_frames))
            got = enc.fetch()
        else:
            got = enc.encode(src_frames)
        _check_stages(enc, refs, c, dst or c, us)
        if device:      # the caller's frames are never written
            assert (pool[1:].cpu().numpy() == src_frames.reshape(-1)).all()
    _check(got, [r["jpeg"] for r in refs])
    return got


# ------------------------------------------------------------------------- slot "in" alone, k_encode in place
ALONE = [(9, 5, "420"), (33, 17, "444"), (130, 66, "420"), (4100, 5, "444")]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device+1"])
@pytest.mark.parametrize("w,h,c", ALONE, ids=[f"{w}x{h}_{c}" for w, h, c in ALONE])
def test_lut_in_alone_k_encode_reads_the_mapped_frames_in_place(w, h, c, device):
    """9x5 4:2:0: chroma planes of 15 bytes, all head and tail; 33x17 4:4:4: odd frame bytes; 130x66: 536 luma
    pieces, so slots i = 0..2 of one workgroup's 1024 (past one workgroup: tests/test_gpu_eq_chain.py); 4100x5:
    long rows, two workgroups a plane."""
    _run(w, h, c, lut_in=T_IN, device=device, want_paths=(0, 0, 1))


def test_lut_in_alone_full_range():
    _run(33, 17, "444", lut_in=T_IN, full=True, want_paths=(0, 0, 1))


# ------------------------------------------------------------------------- a crop read in place
def test_crop_read_in_place_through_the_unaligned_fetch():
    _run(130, 66, "420", lut_in=T_IN, rect=(6, 2, 64, 32), want_paths=(0, 0, 3))


def test_crop_read_in_place_through_the_aligned_fetch(monkeypatch):
    _run(130, 66, "420", lut_in=T_IN, rect=(16, 2, 64, 32), env={"MJG_UNALIGNED_FETCH": "0"}, monkeypatch=monkeypatch,
         want_paths=(0, 0, 1))


# ------------------------------------------------------------------------- every reader of d_lut
def test_k_scale_reads_the_mapped_frames():
    _run(130, 66, "420", lut_in=T_IN, dw=64, dh=32, want_paths=(2, 2, 0))


def test_k_scale_stream_reads_the_mapped_frames(monkeypatch):
    _run(130, 66, "420", lut_in=T_IN, dw=64, dh=32, env={"MJG_SCALE_STREAM": "1"}, monkeypatch=monkeypatch,
         want_paths=(3, 3, 0))


def test_k_plane_copy_reads_the_mapped_frames_table_then_range():
    """tv 4:4:4 -> yuvj420p without a resize: luma through k_plane_copy's tv->pc table behind ours."""
    _run(130, 66, "444", lut_in=T_IN, dst="420", want_paths=(1, 2, 0))


def test_k_pad_plane_reads_the_mapped_frames():
    _run(34, 18, "420", lut_in=T_IN, pad=(8, 10, 50, 38))


# ------------------------------------------------------------------------- every writer in front of it
def test_behind_the_transposing_orientation():
    _run(301, 203, "420", lut_in=T_IN, orient=3, want_paths=(0, 0, 1))


def test_behind_yadif_in_two_halo_submits():
    w, h, c = 130, 66, "420"
    frames = _frames(w, h, c, 5)
    d = deint_frames(frames, w, h, c, 0, 1)
    refs = [chain_ref(f, w, h, c, T_IN) for f in d]
    got = []
    with MjpegEncoder(0, w, h, qscale=5, max_batch=NF, chroma=c, deint=_lib.MJG_DEINT_YADIF, lut_in=T_IN) as enc:
        for lo, n, halo in ((0, 3, 2), (3, 2, 1)):
            first = lo - (halo & 1)
            enc.submit(frames[first:lo + n + (halo >> 1 & 1)], n, halo=halo)
            got += enc.fetch()
            for i in range(n):
                _same(f"lut_in behind yadif, halo {halo}", lo + i, enc.debug_lut_in(i), refs[lo + i]["lut_in"], w, h, c)
    _check(got, [r["jpeg"] for r in refs])


# ------------------------------------------------------------------------- slot "out"
def test_lut_out_behind_k_scale():
    _run(130, 66, "420", lut_out=T_OUT, dw=64, dh=32, want_paths=(2, 2, 0))


def test_lut_out_without_a_resize_forces_the_sws_stage():
    _run(33, 17, "444", lut_out=T_OUT, want_paths=(1, 1, 0))


def test_lut_out_under_a_pad_at_an_odd_canvas_offset_leaves_the_border():
    """The chroma picture starts at canvas column 3, row 5: rows at the canvas stride.  The border stays 0 / 128 / 128."""
    pad = (6, 10, 80, 48)
    _run(130, 66, "420", lut_out=T_OUT, dw=64, dh=32, pad=pad)
    r = chain_ref(_frames(130, 66, "420")[0], 130, 66, "420", None, T_OUT, dw=64, dh=32, pad=pad)
    yy, uu, vv = r["planes"]
    assert yy[0, 0] == 0 and uu[0, 0] == 128 and vv[0, 0] == 128 and T_OUT[0][0] != 0 and T_OUT[1][128] != 128
    _run(130, 66, "444", lut_out=T_OUT, dw=64, dh=32, pad=(3, 5, 80, 48))


def test_lut_out_with_an_unsharp_behind_it():
    _run(130, 66, "420", lut_out=T_OUT, dw=70, dh=38, us=(5, 5, 1.0, 3, 3, 0.5))
    _run(130, 66, "420", lut_out=T_OUT, dw=64, dh=32, us=(5, 5, 1.0, 5, 5, 0.0), pad=(8, 8, 80, 48))


def test_both_slots_at_once_with_different_tables():
    _run(130, 66, "420", lut_in=T_IN, lut_out=T_OUT, dw=64, dh=32)
    _run(130, 66, "420", lut_in=T_IN, lut_out=T_OUT, orient=3, rect=(2, 2, 62, 126), dw=32, dh=64, us=(5, 5, 1.0, 5, 5, 0.0),
         pad=(8, 8, 48, 80))


# ------------------------------------------------------------------------- identity planes
def _with_identity(t, planes):
    t = t.copy()
    for p in planes:
        t[p] = eq_ref.IDENTITY
    return t


@pytest.mark.parametrize("planes", [(0,), (1, 2), (1,), (2,)], ids=["Y", "UV", "U", "V"])
def test_identity_planes_are_copied_or_left_alone(planes):
    tin, tout = _with_identity(T_IN, planes), _with_identity(T_OUT, planes)
    _run(130, 66, "420", lut_in=tin)                                  # copied into d_lut
    _run(130, 66, "420", lut_in=tin, orient=4)                        # in place in d_orient: left alone
    _run(130, 66, "420", lut_out=tout, dw=64, dh=32, pad=(6, 10, 80, 48))      # in place in d_scaled


# ------------------------------------------------------------------------- submit modes
def test_submit_segments_each_from_byte_1_of_its_own_allocation():
    import torch
    w, h, c = 130, 66, "420"
    frames = _frames(w, h, c, 5)
    refs = [chain_ref(f, w, h, c, T_IN) for f in frames]
    segs, at = [], 0
    for n in (1, 3, 1):
        t = torch.zeros(n * frames.shape[1] + 1, dtype=torch.uint8, device="cuda:0")
        t[1:] = torch.from_numpy(frames[at:at + n].reshape(-1).copy()).to("cuda:0")
        segs.append((t, n))
        at += n
    torch.cuda.synchronize()
    with MjpegEncoder(0, w, h, qscale=5, max_batch=5, chroma=c, lut_in=T_IN) as enc:
        enc.submit_segments([(t.data_ptr() + 1, n) for t, n in segs])
        got = enc.fetch()
        for i in range(5):
            _same("lut_in, segments 1+3+1", i, enc.debug_lut_in(i), refs[i]["lut_in"], w, h, c)
    _check(got, [r["jpeg"] for r in refs])


def test_two_merged_device_submits():
    import torch
    w, h, c = 130, 66, "420"
    frames = _frames(w, h, c)
    refs = [chain_ref(f, w, h, c, T_IN, T_OUT, dw=64, dh=32, sar=profile.scaled_sar((1, 1), (w, h), (64, 32))) for f in frames]
    ts = [torch.from_numpy(frames[lo:lo + n].copy()).to("cuda:0") for lo, n in ((0, 2), (2, 1))]
    torch.cuda.synchronize()
    got = []
    with MjpegEncoder(0, w, h, 64, 32, qscale=5, sar=profile.scaled_sar((1, 1), (w, h), (64, 32)), max_batch=NF, chroma=c,
                      merge=True, lut_in=T_IN, lut_out=T_OUT) as enc:
        for t in ts:
            enc.submit(device_ptr=t.data_ptr(), nframes=t.shape[0])
        for t in ts:
            enc.sync()
            got += enc.fetch()
        # (a read-back syncs whatever is queued, so only the last job's: its frame lies behind the first job's two)
        _same("lut_in, merged submits", 2, enc.debug_lut_in(0), refs[2]["lut_in"], w, h, c)
    _check(got, [r["jpeg"] for r in refs])


@pytest.mark.parametrize("kw", [dict(huffman="optimal"), dict(rst=True)], ids=["optimal", "rst"])
def test_huffman_optimal_and_rst(kw):
    _run(130, 66, "420", lut_in=T_IN, **kw)


def test_the_stage_runs_inside_the_scale_interval():
    with MjpegEncoder(0, 33, 17, qscale=5, max_batch=NF, chroma="444", timing=True, lut_in=T_IN) as enc:
        enc.encode(_frames(33, 17, "444"))
        ms, n = enc.kernel_times()
    assert n == 1 and ms["scale"] > 0


# ------------------------------------------------------------------------- V on a launch of its own
def test_v_gets_a_launch_of_its_own_past_32767_frames():
    """8x8 4:2:0, slot "in", one host submit of 32,768 frames that cycle through 61 base frames: the read-back
    at frames 0 and 32,767 (the submit's last: it has no frame 32,768), and every JPEG."""
    w, h, c, n, k = 8, 8, "420", 32768, 61
    base = np.random.default_rng([w, h, k]).integers(0, 256, (k, i420_frame_bytes(w, h, c)), dtype=np.uint8)
    i = np.arange(n, dtype=np.int64)
    idx = (i * 7 + i // 1000) % k
    assert 2 * n > 65535 and len({int(idx[0]), int(idx[n - 2]), int(idx[n - 1])}) == 3
    refs = [chain_ref(f, w, h, c, T_IN) for f in base]
    frames = base[idx]
    with MjpegEncoder(0, w, h, qscale=5, max_batch=n, chroma=c, lut_in=T_IN) as enc:
        enc.submit(frames, n)
        got = enc.fetch()
        for g in (0, n - 1, n):
            if g < n:
                _same("lut_in, U and V apart", g, enc.debug_lut_in(g), refs[idx[g]]["lut_in"], w, h, c)
    assert len(got) == n
    for g, a in enumerate(got):
        b = refs[idx[g]]["jpeg"]
        if a != b:
            pytest.fail(f"JPEG of frame {g} (base frame {idx[g]}) differs: first_diff {first_diff(a, b)}")


# ------------------------------------------------------------------------- nothing changed for others
def test_no_table_and_identity_tables_open_a_context_without_the_stage():
    frames = _frames(130, 66, "420")
    for shape in (dict(dst_w=70, dst_h=38), dict()):
        out = []
        for extra in (dict(unsharp=(5, 5, 1.0, 5, 5, 0.0)) if shape else dict(), dict(lut_in=None, lut_out=None),
                      dict(lut_in=ID3, lut_out=ID3), dict(lut_in=ID3)):
            if shape and "unsharp" not in extra:
                extra = dict(extra, unsharp=(5, 5, 1.0, 5, 5, 0.0))
            with MjpegEncoder(0, 130, 66, qscale=5, max_batch=NF, chroma="420", timing=True, **shape, **extra) as enc:
                assert enc.debug_lut("in") is None and enc.debug_lut("out") is None
                jp = enc.encode(frames)
                with pytest.raises(_lib.MjgError) as e:
                    enc.debug_lut_in(0)
                assert e.value.code == _lib.MJG_E_STATE
                out.append((jp, enc.scale_path(0), enc.scale_path(1), enc.encode_path()))
        for o in out[1:]:
            _check(o[0], out[0][0])
            assert o[1:] == out[0][1:]
    assert out[0][1:] == (0, 0, 1)      # without a scale: k_encode in place, no sws stage


def test_bad_tables_are_refused():
    with pytest.raises(ValueError):
        MjpegEncoder(0, 33, 17, chroma="444", lut_in=np.zeros((3, 255), np.uint8))
    with pytest.raises(ValueError):
        MjpegEncoder(0, 33, 17, chroma="444", lut_out=np.zeros((3, 256), np.int32))


# ------------------------------------------------------------------------- the worker
def _y4m420(frames, w, h, field="p"):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{w} H{h} F25:1 I{field} A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


def _worker(vf, frames, w, h, field="p", batch=0):
    args = ["-vf", vf] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m420(frames, w, h, field)), stdout=out, stderr=err,
                    opts=worker.Options(batch=batch) if batch else None)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue(), err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    return [d for _, d in r.frames(1)], r.info(1)


def test_worker_yadif_crop_eq_scale_unsharp_pad_across_three_batches():
    w, h, c = 40, 24, "420"
    frames = _frames(w, h, c, 5)
    vf = "yadif,crop=36:20:2:2,eq=contrast=1.2:brightness=-0.07:saturation=1.3,scale=24:16,unsharp=3:3:0.8,pad=32:24"
    packets, info = _worker(vf, frames, w, h, field="t", batch=2)      # batches of 2 + 2 + 1
    assert (info.width, info.height, info.codec) == (32, 24, "V_MJPEG")
    tabs = profile.eq_tables(dict(contrast=1.2, brightness=-0.07, saturation=1.3))
    assert (tabs == eq_ref.tables(dict(contrast=1.2, brightness=-0.07, saturation=1.3))).all()
    d = deint_frames(frames, w, h, c, 0, 1)
    sar = profile.scaled_sar((1, 1), (36, 20), (24, 16))
    pad = profile.resolve_pad({"w": 32, "h": 24, "x": None, "y": None}, 24, 16, c)
    refs = [chain_ref(f, w, h, c, tabs, None, rect=(2, 2, 36, 20), dw=24, dh=16, us=(3, 3, 0.8, 5, 5, 0.0), pad=pad,
                      qscale=profile.effective_qscale(5), sar=sar)["jpeg"] for f in d]
    _check(packets, refs, "worker, slot in")


def test_worker_scale_eq_gamma_behind_the_scale():
    w, h, c = 40, 24, "420"
    frames = _frames(w, h, c, 5)
    packets, info = _worker("scale=24:16,eq=gamma=1.1", frames, w, h)
    assert (info.width, info.height) == (24, 16)
    tabs = profile.eq_tables(dict(gamma=1.1))
    sar = profile.scaled_sar((1, 1), (w, h), (24, 16))
    refs = [chain_ref(f, w, h, c, None, tabs, dw=24, dh=16, qscale=profile.effective_qscale(5), sar=sar)["jpeg"] for f in frames]
    _check(packets, refs, "worker, slot out")
