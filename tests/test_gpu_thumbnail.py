"""k_frame_hist and `-vf thumbnail` on the GPU: encoder.FrameHist.count against np.bincount per
plane (tests/thumbnail_ref.py), exactly, on the shapes where the kernel can go wrong, and the worker end to
end against tests/tile_ref.py's sheets of the frames that thumbnail_ref picks.  tools/hist_host_check.py
walks the launches of every shape here (thumbnail_ref.GPU_SHAPES) on the CPU under AddressSanitizer."""
import io

import numpy as np
import pytest

import thumbnail_ref
import tile_ref
from ffmpeg_distributed_amd import _lib, container, profile, worker
from ffmpeg_distributed_amd.encoder import FrameHist, MjpegEncoder

pytestmark = pytest.mark.gpu

_SRC = {}


def _case(kind, w, h, c, n):
    """(frames, histograms) per content and shape, made once and left unchanged."""
    key = (kind, w, h, c, n)
    if key not in _SRC:
        f = thumbnail_ref.make_frames(kind, w, h, c, n, 11)
        want = thumbnail_ref.hist_ref(f, w, h, c)
        f.setflags(write=False)
        want.setflags(write=False)
        _SRC[key] = (f, want)
    return _SRC[key]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint32, (what, got.shape, got.dtype)
    bad = np.argwhere(got != want)
    if bad.size:
        f, j = bad[0]
        pytest.fail(f"{what}: {len(bad)} of {want.size} counters differ, first frame {f} plane {j // 256} value {j % 256}: "
                    f"got {got[f, j]}, want {want[f, j]}")


def test_the_shape_list_is_what_the_issue_names():
    """tools/hist_host_check.py walks thumbnail_ref.GPU_SHAPES: keep it in step with the cases."""
    assert [s[:3] for s in thumbnail_ref.GPU_SHAPES] == [
        (3, 3, "444"), (16, 16, "420"), (33, 17, "444"), (130, 66, "422"), (4100, 5, "420"), (640, 360, "420")]


@pytest.mark.parametrize("kind", thumbnail_ref.CONTENTS)
@pytest.mark.parametrize("w,h,c,n", thumbnail_ref.GPU_SHAPES)
def test_host_frames_count_as_bincount(w, h, c, n, kind):
    frames, want = _case(kind, w, h, c, n)
    sizes = thumbnail_ref.plane_sizes(w, h, c)
    if kind == "noise":      # every byte value occurs where the plane has room for it
        assert all((want[:, 256 * p:256 * p + 256] > 0).all() for p in range(3) if sizes[p] >= 256)
    with FrameHist(0, w, h, c, n) as hist:
        assert hist.frame_bytes == frames.shape[1]
        got = hist.count(frames)                      # nframes = max_frames
        _same(got, want, f"{kind} {w}x{h} {c}, {n} frames")
        if kind == "constant":  # the contention case: one bin holds the plane, 255 are empty
            for f in range(n):
                for p in range(3):
                    row = got[f, 256 * p:256 * p + 256]
                    assert row.max() == sizes[p] and np.count_nonzero(row) == 1, (f, p)
        _same(hist.count(frames[n - 1:]), want[n - 1:], "nframes 1, the last frame")
        _same(hist.count(frames[:1].tobytes()), want[:1], "nframes 1, bytes")


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("w,h,c,n", thumbnail_ref.GPU_SHAPES)
def test_device_frames_at_byte_0_and_byte_1(w, h, c, n, lead):
    import torch
    frames, want = _case("noise", w, h, c, n)
    pool = torch.zeros(frames.size + lead, dtype=torch.uint8, device="cuda:0")
    pool[lead:] = torch.from_numpy(frames.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    with FrameHist(0, w, h, c, n + 2) as hist:        # (fewer frames than max_frames)
        _same(hist.count(device_ptr=pool.data_ptr() + lead, nframes=n), want, f"device frames {lead} byte(s) in")
        _same(hist.count(device_ptr=pool.data_ptr() + lead + frames.shape[1], nframes=1), want[1:2], "one device frame")
    assert (pool[lead:].cpu().numpy() == frames.reshape(-1)).all()   # the caller's frames are never written


def test_a_second_call_starts_from_zero():
    w, h, c, n = 640, 360, "420", 3
    a, wa = _case("noise", w, h, c, n)
    b, wb = _case("checker", w, h, c, n)
    k, wk = _case("constant", w, h, c, n)
    with FrameHist(0, w, h, c, n) as hist:
        _same(hist.count(a), wa, "first call")
        _same(hist.count(b), wb, "second call, other data")
        _same(hist.count(k[:2]), wk[:2], "third call, fewer frames")
        _same(hist.count(a), wa, "fourth call")


def test_nframes_outside_the_object():
    w, h, c, n = 16, 16, "420", 3
    frames, _ = _case("noise", w, h, c, n)
    with FrameHist(0, w, h, c, 2) as hist:
        for bad in (0, 3, -1):
            with pytest.raises(_lib.MjgError, match=r"hist: nframes -?\d+ not in 1\.\.2") as e:
                hist.count(frames, nframes=bad)
            assert e.value.code == _lib.MJG_E_INVALID
        with pytest.raises(ValueError):
            hist.count(frames[0, :-1])
    with pytest.raises(_lib.MjgError, match="hist: device 99"):
        FrameHist(99, w, h, c, 2)


def test_a_count_between_two_submits_leaves_the_encoder_alone():
    """Another context's submits around a count: its JPEGs are those of a run without the count."""
    w, h, c, n = 640, 360, "420", 3
    frames, want = _case("noise", w, h, c, n)
    other, _ = _case("checker", w, h, c, n)

    def run(count):
        got = []
        with MjpegEncoder(0, w, h, 320, 180, qscale=5, max_batch=n, chroma=c) as enc, FrameHist(0, w, h, c, n) as hist:
            enc.submit(frames)
            if count:
                got.append(hist.count(other))
            enc.submit(other)
            if count:
                got.append(hist.count(frames))
            enc.sync()
            jp = enc.fetch()
            enc.sync()
            jp += enc.fetch()
        return jp, got

    plain, _ = run(False)
    mixed, hists = run(True)
    assert len(plain) == 2 * n and mixed == plain
    _same(hists[1], want, "a count behind two queued submits")


# ------------------------------------------------------------------------- the worker
W, H, C_, NF = 64, 32, "420", 23
_E2E = {}


def _segment():
    """23 frames of 64x32 4:2:0: one base picture plus a brightness offset per frame; and their histograms."""
    if not _E2E:
        rng = np.random.default_rng(23)
        fb = thumbnail_ref.frame_bytes(W, H, C_)
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.concatenate([((yy * 3 + xx * 2) % 160 + 30).reshape(-1), rng.integers(90, 170, fb - W * H)]).astype(np.int64)
        off = [(k * 29) % 23 - 11 for k in range(NF)]
        frames = np.stack([np.clip(base + o, 0, 255).astype(np.uint8) for o in off])
        frames.setflags(write=False)
        _E2E["frames"], _E2E["hists"] = frames, thumbnail_ref.hist_ref(frames, W, H, C_)
    return _E2E["frames"], _E2E["hists"]


def _y4m(frames):
    b = io.BytesIO()
    b.write(f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C420jpeg\n".encode())
    for f in frames:
        b.write(b"FRAME\n" + f.tobytes())
    return b.getvalue()


@pytest.mark.parametrize("vf,step,N,orient,sheet", [
    ("thumbnail=5,scale=32:16,tile=2x2", 1, 5, [], (2, 2, 0, 0, 0)),
    ("framestep=2,thumbnail=3,vflip,scale=32:16,tile=2x1", 2, 3, ["vflip"], (2, 1, 0, 0, 0)),
])
def test_worker_thumbnail_scale_tile_end_to_end(monkeypatch, vf, step, N, orient, sheet):
    frames, hists = _segment()
    picks = thumbnail_ref.kept_frames(hists, step, N)
    kept = -(-NF // step)
    assert len(picks) == -(-kept // N) and len({(p // step) % N for p in picks}) > 1   # the picks are not all index 0
    monkeypatch.setenv("MJG_WORKER_BATCH", "4")
    args = ["-vf", vf] + "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact".split()
    out, err = io.BytesIO(), io.StringIO()
    rc = worker.run(0, args, stdin=io.BytesIO(_y4m(frames)), stdout=out, stderr=err)
    assert rc == 0, err.getvalue()
    assert "running ffmpeg on the CPU" not in err.getvalue(), err.getvalue()
    r = container.MkvReader(io.BytesIO(out.getvalue()))
    pk = [bytes(d) for _, d in r.frames(1)]
    cells = [tile_ref.cell_planes(frames[k], W, H, C_, orient=profile.compose_orient(orient), dw=32, dh=16) for k in picks]
    sheets = tile_ref.sheets_numpy(cells, 32, 16, C_, sheet)
    sar = profile.scaled_sar((1, 1), (W, H), (32, 16))
    want = [tile_ref.sheet_jpeg(s, C_, qscale=profile.effective_qscale(5), sar=sar) for s in sheets]
    n_sheet = sheet[0] * sheet[1]
    assert len(want) == -(-len(picks) // n_sheet)
    assert len(pk) == len(want)
    for j, (a, b) in enumerate(zip(pk, want)):
        assert a == b, (vf, j, len(a), len(b))
    # the sheets are numbered as without the thumbnail: out_fps = fps / (framestep * nb_frames)
    assert r.tracks[0].default_duration == 1_000_000_000 * step * n_sheet // 25
