"""`-vf thumbnail` without a GPU: the parser's accept / reject table, profile.thumbnail_pick
against the index-loop restatement of tests/thumbnail_ref.py, the reader strategy of worker.Pipeline with
stand-ins for the encoder, the page-locked buffers and the histogram object (the stand-in counts with
np.bincount), the fallthrough reasons, and the library's argument checks, which make no HIP call."""
import ctypes as C
import io
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

import thumbnail_ref
from ffmpeg_distributed_amd import _lib, container, profile, worker

ARGS = ["-c:v", "mjpeg", "-q:v", "5", "-dct", "int", "-huffman", "default", "-bitexact"]


def parse(vf):
    return profile.try_parse(["-vf", vf] + ARGS)


# ---------------------------------------------------------------------------------- the parser
@pytest.mark.parametrize("vf,step,n", [
    ("thumbnail,tile", 1, 100),
    ("thumbnail=7,tile=2x2", 1, 7),
    ("thumbnail=n=2,scale=64:32,tile", 1, 2),
    ("framestep=2,thumbnail=5,scale=64:32,tile=3x2", 2, 5),
    ("framestep=1,thumbnail=5,tile", 1, 5),
    ("framestep=step=3,thumbnail,vflip,crop=32:16,scale=16:8,unsharp,tile=2x1:2", 3, 100),
])
def test_accepted_graphs(vf, step, n):
    p, why = parse(vf)
    assert why is None and type(p) is profile.ThumbProfile
    assert (p.framestep, p.thumbnail) == (step, n) and p.tile is not None


@pytest.mark.parametrize("vf,names", [
    ("thumbnail=3,thumbnail=4,tile", ("second thumbnail",)),
    ("scale=64:32,thumbnail=5,tile", ("thumbnail after scale",)),
    ("framestep=2,vflip,thumbnail=5,tile", ("thumbnail after vflip",)),
    ("vflip,framestep=2,thumbnail=5,tile", ("thumbnail after framestep", "first filter")),
    ("thumbnail=3,yadif,tile", ("thumbnail together with yadif",)),
    ("yadif,thumbnail=3,tile", ("thumbnail",)),
    ("thumbnail=5,scale=64:32", ("thumbnail without a tile", "sparse timestamps", "MkvWriter")),
    ("thumbnail=5", ("thumbnail without a tile", "MkvWriter")),
    ("thumbnail=5,tile,vflip", ("thumbnail without a tile as the last filter",)),
    ("thumbnail=1,tile", ("thumbnail 1",)),
    ("thumbnail=0,tile", ("thumbnail 0",)),
    ("thumbnail=n=1,tile", ("thumbnail 1",)),
    ("thumbnail=2.5,tile", ("thumbnail '2.5'", "integer")),
    ("thumbnail=-3,tile", ("thumbnail '-3'", "integer")),
    ("thumbnail=n/2,tile", ("thumbnail 'n/2'", "integer")),
    ("thumbnail=n=5:log=info,tile", ("thumbnail option 'log'",)),
    ("thumbnail=m=5,tile", ("thumbnail option 'm'",)),
    ("thumbnail=3:4,tile", ("thumbnail", "positional")),
])
def test_refused_graphs_name_what_they_refuse(vf, names):
    p, why = parse(vf)
    assert p is None
    for name in names:
        assert name in why, why


def test_the_fields_beside_the_thumbnail_are_the_graphs_without_it():
    with_t, _ = parse("framestep=2,thumbnail=5,scale=64:32,tile=3x2")
    without, _ = parse("framestep=2,scale=64:32,tile=3x2")
    assert type(without) is profile.SheetProfile and not hasattr(without, "thumbnail")
    assert (with_t.framestep, with_t.thumbnail) == (2, 5)
    assert with_t.tile == without.tile == {"cols": 3, "rows": 2, "nb_frames": 0, "margin": 0, "padding": 0}
    assert {k: v for k, v in vars(with_t).items() if k != "thumbnail"} == vars(without)
    # and the graph without it is the SheetProfile it was: every field spelled out
    assert without == profile.SheetProfile(qscale=5, q_arg=5.0, scale=(64, 32), sws_flags=("bicubic",), huffman="default",
                                           rst=False, chroma=None, crop=None, pad=None, orient=0, deint=None, unsharp=None,
                                           eq=None, colormatrix=None, tile=with_t.tile, framestep=2)
    plain, _ = parse("scale=64:32")
    assert type(plain) is profile.Profile
    assert [f for f in profile.Profile.__dataclass_fields__] == [f for f in profile.SheetProfile.__dataclass_fields__][:-2]
    assert "thumbnail" not in profile.SheetProfile.__dataclass_fields__


# ---------------------------------------------------------------------------------- the selection
def seeded_hists(n, seed):
    """n histograms of a 64x32 4:2:0 frame's sizes: per plane a multinomial draw around a profile that drifts with
    the frame, so the errors differ."""
    rng = np.random.default_rng([seed, n])
    out = np.zeros((n, 768), np.uint32)
    for i in range(n):
        for p, nb in enumerate((2048, 512, 512)):
            w = rng.random(256) + (np.arange(256) == (40 * p + 3 * i) % 256) * rng.random() * 20
            out[i, 256 * p:256 * p + 256] = rng.multinomial(nb, w / w.sum())
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 7, 100])
def test_pick_is_the_index_loop_restatement(n):
    for seed in range(3 if n < 100 else 1):
        h = seeded_hists(n, seed)
        assert profile.thumbnail_pick(h) == thumbnail_ref.pick_ref(h)
        assert profile.thumbnail_pick([list(map(int, r)) for r in h]) == thumbnail_ref.pick_ref(h)


def test_pick_ties_and_exact_means():
    h = seeded_hists(5, 9)
    assert profile.thumbnail_pick(np.repeat(h[:1], 6, axis=0)) == 0     # identical frames
    for seed in range(4):
        assert profile.thumbnail_pick(seeded_hists(2, seed)) == 0        # two frames: equal errors
    # a group whose mean is frame k exactly: frames k - d and k + d around it, error 0 at k alone
    base = np.full(768, 1000, np.int64)
    d1, d2 = np.arange(768) % 7, (np.arange(768) * 5) % 11
    for k in range(5):
        rows = [base + d1, base - d1, base + d2, base - d2]
        rows.insert(k, base)
        assert profile.thumbnail_pick(np.array(rows, np.uint32)) == k


def test_pick_moves_with_a_permutation():
    h = seeded_hists(7, 4)
    k = thumbnail_ref.pick_ref(h)
    rng = np.random.default_rng(3)
    for _ in range(5):
        perm = rng.permutation(7)
        # (no tie here: the mean of a permuted group is the same sum in another order, and these counts are
        # integers below 2^53 / 7, so every sum is exact and the errors are the same doubles)
        assert profile.thumbnail_pick(h[perm]) == list(perm).index(k)


# ---------------------------------------------------------------------------------- the pipeline
W, H, FB, BATCH = 8, 4, 48, 3


def frame(k: int) -> np.ndarray:
    """Frame k of the segment: a base picture plus a brightness offset that wanders, so the picks are not all 0;
    byte 0 is k itself."""
    base = (np.arange(FB) * 37 + 11) % 200
    f = ((base + (k * 29) % 23) % 256).astype(np.uint8)
    f[0] = k
    return f


def y4m(n: int) -> bytes:
    return f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C420jpeg\n".encode() + b"".join(b"FRAME\n" + frame(k).tobytes() for k in range(n))


class Buf:
    def __init__(self, nbytes):
        self.nbytes, self.array, self.freed = int(nbytes), np.zeros(int(nbytes), np.uint8), 0

    def free(self):
        self.freed += 1


class Enc:
    """encoder.MjpegEncoder's stand-in: remembers the frames it is handed and makes a packet of each sheet's."""
    host_depth = 2
    opened: list = []

    def __init__(self, device, src_w, src_h, dst_w=None, dst_h=None, sheet=None, **kw):
        self.frame_bytes, self.n = src_w * src_h * 3 // 2, (sheet or (1, 1, 1))[2]
        self.pending, self.seen, self.submits, self.closed, self.last_total, self.packets = [], [], [], 0, 0, []
        Enc.opened.append(self)

    def close(self):
        self.closed += 1

    def submit(self, arr, n, halo=0):
        assert len(self.pending) < self.host_depth and not halo and len(arr) == n * self.frame_bytes
        fr = [bytes(arr[i * self.frame_bytes:(i + 1) * self.frame_bytes]) for i in range(n)]
        self.pending.append(fr)
        self.seen += fr
        self.submits.append(n)

    def sync(self):
        fr = self.pending.pop(0)
        self.packets = [b"\xff\xd8" + bytes(f[0] for f in fr[i:i + self.n]) + b"\xff\xd9" for i in range(0, len(fr), self.n)]
        self.last_total = sum(len(p) for p in self.packets)

    def fetch_into(self, buf):
        out, o, mv = [], 0, memoryview(buf.array)
        for p in self.packets:
            buf.array[o:o + len(p)] = np.frombuffer(p, np.uint8)
            out.append(mv[o:o + len(p)])
            o += len(p)
        return out


class Hist:
    """encoder.FrameHist's stand-in: np.bincount per plane, and a record of the calls."""
    opened: list = []

    def __init__(self, device, w, h, chroma="420", max_frames=16):
        self.shape, self.max_frames, self.calls, self.closed = (w, h, chroma), max_frames, [], 0
        Hist.opened.append(self)

    def count(self, frames=None, nframes=None, device_ptr=None):
        assert device_ptr is None and 1 <= nframes <= self.max_frames and len(frames) == nframes * FB
        self.calls.append(nframes)
        return thumbnail_ref.hist_ref(np.array(frames), *self.shape)

    def close(self):
        self.closed += 1


@pytest.fixture
def stand_ins(monkeypatch):
    monkeypatch.setitem(sys.modules, "ffmpeg_distributed_amd.encoder",
                        types.SimpleNamespace(MjpegEncoder=Enc, PinnedBuffer=Buf, FrameHist=Hist))
    monkeypatch.setattr(Enc, "opened", [])
    monkeypatch.setattr(Hist, "opened", [])
    monkeypatch.setenv("MJG_NUMA_BIND", "0")


def run_segment(vf, n, cache=None):
    """One segment through plan_segment, Context.acquire, Pipeline and Context.settle, as worker.run takes it."""
    prof, why = parse(vf)
    assert why is None
    src = worker.Source(io.BytesIO(y4m(n)), 2)
    plan = worker.plan_segment(prof, src.info)
    batch = plan.batch(BATCH)
    ctx = worker.Context.acquire(cache, 0, prof, src.info, plan, batch, False)
    out, err = io.BytesIO(), io.StringIO()
    fps = plan.rate(src.info)
    pipe = worker.Pipeline(ctx.enc, ctx.bufs, ctx.obufs, ctx.new_obuf, src,
                           container.MkvWriter(out, plan.enc_w, plan.enc_h, fps, plan.sar), worker.Progress(err, fps, 5),
                           batch, plan.framestep, bool(plan.deint), ctx.thumb(plan))
    try:
        pipe.run()
    finally:
        rc = pipe.stop()
        ctx.settle(cache, pipe)
    assert rc == 0 and not pipe.failed
    return plan, ctx, pipe, out.getvalue(), batch


@pytest.mark.parametrize("step", [1, 2])
def test_the_reader_hands_on_the_references_picks(stand_ins, step):
    n, N = 23, 5
    vf = ("framestep=2," if step > 1 else "") + f"thumbnail={N},tile=2x1"
    plan, ctx, pipe, out, batch = run_segment(vf, n)
    assert type(plan) is worker.ThumbPlan and plan.thumbnail == N and plan.framestep == step and batch == 2
    frames = np.stack([frame(k) for k in range(n)])
    want = thumbnail_ref.kept_frames(thumbnail_ref.hist_ref(frames, W, H, "420"), step, N)
    kept = -(-n // step)
    assert len(want) == -(-kept // N) and len(set(w % (N * step) for w in want)) > 1   # (the picks are not all index 0)
    assert [f[0] for f in ctx.enc.seen] == want
    assert ctx.enc.seen == [frame(k).tobytes() for k in want]
    # the last group is the remainder: 23 = 4 x 5 + 3, 12 = 2 x 5 + 2
    assert want[-1] in range((kept - kept % N) * step, n, step)
    # the histogram object: the context's, asked for runs of at most a batch, every kept frame once
    hist = Hist.opened[0]
    assert len(Hist.opened) == 1 and hist.max_frames == batch and max(hist.calls) <= batch and sum(hist.calls) == kept
    # sheets: ceil(ceil(kept / N) / nb_frames), at fps / (framestep * nb_frames) whatever N is
    sheets = -(-len(want) // 2)
    r = container.MkvReader(io.BytesIO(out))
    pk = [bytes(d) for _, d in r.frames(1)]
    assert len(pk) == sheets == pipe.frames
    assert b"".join(p[2:-2] for p in pk) == bytes(want)
    assert plan.out_fps == Fraction(25, step * 2) == plan.rate(None)
    assert r.tracks[0].default_duration == 1_000_000_000 * step * 2 // 25
    assert ctx.enc.closed == 1 and hist.closed == 1 and ctx.store.freed == 1 and ctx.store.nbytes == N * FB


def test_groups_that_end_with_the_batch_and_with_the_input(stand_ins):
    for n, N in ((10, 5), (6, 2), (1, 4), (0, 3), (9, 3)):   # whole groups, one short group, no frame
        plan, ctx, pipe, out, batch = run_segment(f"thumbnail={N},tile=2x1", n)
        frames = np.stack([frame(k) for k in range(n)]) if n else np.zeros((0, FB), np.uint8)
        want = thumbnail_ref.kept_frames(thumbnail_ref.hist_ref(frames, W, H, "420"), 1, N) if n else []
        assert [f[0] for f in ctx.enc.seen] == want, (n, N)


def test_the_plan_is_the_sheet_plans_but_for_the_key(stand_ins):
    info = container.StreamInfo(W, H, Fraction(30))
    a = worker.plan_segment(parse("framestep=2,thumbnail=5,tile=2x1")[0], info)
    b = worker.plan_segment(parse("framestep=2,tile=2x1")[0], info)
    assert type(a) is worker.ThumbPlan and type(b) is worker.SheetPlan
    assert (a.rate(info), a.batch(7), a.encoder_kwargs()) == (b.rate(info), b.batch(7), b.encoder_kwargs())
    assert a.rate(info) == Fraction(30, 4)
    prof = parse("framestep=2,thumbnail=5,tile=2x1")[0]
    ka, kb = a.key(prof, info, False, 6), b.key(prof, info, False, 6)
    assert ka[:len(kb)] == kb and ka[len(kb):] == (("thumbnail", 5),)
    c = worker.plan_segment(parse("framestep=2,thumbnail=6,tile=2x1")[0], info)
    assert c.key(prof, info, False, 6) != ka


def test_the_cache_keeps_the_histogram_object_with_the_encoder(stand_ins):
    cache = {}
    _, a, _, _, _ = run_segment("thumbnail=5,tile=2x1", 11, cache)
    _, b, _, _, _ = run_segment("thumbnail=5,tile=2x1", 7, cache)
    assert b is a and len(Hist.opened) == 1 and len(Enc.opened) == 1 and not Hist.opened[0].closed
    _, c, _, _, _ = run_segment("thumbnail=4,tile=2x1", 7, cache)   # another N: another context
    assert c is not a and len(Hist.opened) == 2 and Hist.opened[0].closed == 1 and a.store.freed == 1
    worker.release(cache)
    assert Hist.opened[1].closed == 1 and c.store.freed == 1 and c.enc.closed == 1


# ---------------------------------------------------------------------------------- fallthrough
def test_fallthrough_reasons():
    prof = parse("thumbnail,scale=160:90,tile=6x5")[0]
    k4 = container.StreamInfo(3840, 2160, Fraction(25))
    assert 100 * k4.frame_bytes == 1_244_160_000 and worker.thumbnail_fallthrough_reason(prof, k4) is None
    assert type(worker.plan_segment(prof, k4)) is worker.ThumbPlan
    big = parse("thumbnail=173,scale=160:90,tile=6x5")[0]   # 173 x 12,441,600 > 2^31
    assert worker.thumbnail_fallthrough_reason(parse("thumbnail=172,tile")[0], k4) is None
    why = worker.thumbnail_fallthrough_reason(big, k4)
    assert "thumbnail=173" in why and "page-locked" in why and str(2 << 30) in why
    with pytest.raises(worker.Fallthrough, match="thumbnail=173"):
        worker.plan_segment(big, k4)
    deep = container.StreamInfo(64, 32, Fraction(25), frame_bytes=2 * 64 * 32 * 3 // 2)   # 16-bit samples
    why = worker.thumbnail_fallthrough_reason(prof, deep)
    assert "thumbnail" in why and "more than 8 bits" in why
    with pytest.raises(worker.Fallthrough, match="more than 8 bits"):
        worker.plan_segment(prof, deep)


# ---------------------------------------------------------------------------------- the library's argument checks
def test_hist_arguments_are_checked_before_any_hip_call():
    L = _lib.load()
    assert L.mjg_version() == 105

    def err(rc):
        assert rc == _lib.MJG_E_INVALID
        msg = L.mjg_last_error().decode()
        assert msg.startswith("hist"), msg
        return msg

    h = C.c_void_p()
    assert "null" in err(L.mjg_hist_open(0, 64, 32, 0, 4, None))
    for w, hh in ((0, 32), (64, 0), (16385, 32), (64, 16385), (-1, 32)):
        assert f"{w}x{hh}" in err(L.mjg_hist_open(0, w, hh, 0, 4, C.byref(h)))
        assert h.value is None
    for cf in (-1, 3, 7):
        assert f"chroma_format {cf}" in err(L.mjg_hist_open(0, 64, 32, cf, 4, C.byref(h)))
    for n in (0, -5):
        assert f"max_frames {n}" in err(L.mjg_hist_open(0, 64, 32, 0, n, C.byref(h)))
    assert "2^31" in err(L.mjg_hist_open(0, 16384, 16384, 2, 1 << 20, C.byref(h)))
    out = (C.c_uint32 * 768)()
    buf = (C.c_uint8 * 16)()
    assert "null" in err(L.mjg_hist_frames(None, buf, 1, 0, out))
    L.mjg_hist_close(None)   # as free(NULL)
