"""worker.Pipeline and worker.Context without a GPU: the reader, submit / drain and muxer threads of a
segment driven with stand-ins for the encoder and the page-locked buffers (no library, no torch).
The stand-in encoder makes mistakes visible: it digests what it is handed and checks the digest again at
the sync, refuses a submit beyond host_depth and an output buffer that is too small, writes its packets
into the output buffer it is given and scribbles over the ones the muxer has handed back; both free lists
check every buffer as it comes back.  Frames are 12 bytes (4x2 4:2:0), a batch is 2 frames."""
import hashlib
import io
import queue
import re
import sys
import threading
import time
import types
from collections import deque
from fractions import Fraction

import numpy as np
import pytest

from ffmpeg_distributed_amd import container, profile, worker

W, H, FB, BATCH = 4, 2, 12, 2
ARGS = ["-c:v", "mjpeg", "-q:v", "5", "-dct", "int", "-huffman", "default", "-bitexact"]
BIG = 700_000   # two such packets do not fit the 1 MiB an output buffer starts with


def frame(k: int) -> bytes:
    return bytes([k] + [(k * 13 + j * 7 + 1) % 251 for j in range(1, FB)])


def y4m(n: int) -> bytes:
    return b"YUV4MPEG2 W4 H2 F25:1 Ip A1:1 C420jpeg\n" + b"".join(b"FRAME\n" + frame(k) for k in range(n))


def digest(data) -> bytes:
    return hashlib.blake2b(bytes(data), digest_size=8).digest()


def packet(fr: bytes, big_from: int = 999) -> bytes:
    """What the stand-in encodes a frame to: the sizes differ from frame to frame."""
    k = fr[0]
    return b"\xff\xd8" + digest(fr) + bytes([k]) * (BIG if k >= big_from else 3 + k * 37 % 101) + b"\xff\xd9"


class Boom(Exception):
    pass


class Buf:
    """encoder.PinnedBuffer's stand-in; every one made is in Buf.made."""
    made: list = []

    def __init__(self, nbytes):
        self.nbytes, self.array, self.freed = int(nbytes), np.zeros(int(nbytes), np.uint8), 0
        Buf.made.append(self)

    def free(self):
        self.freed += 1


class Enc:
    """encoder.MjpegEncoder's stand-in (see the module's docstring)."""
    host_depth = 2
    opened: list = []
    fail_submit = fail_sync = 0   # the call that raises Boom (1-based)
    big_from = 999

    def __init__(self, device, src_w, src_h, dst_w=None, dst_h=None, deint=None, **kw):
        self.frame_bytes, self.deint, self.kw = src_w * src_h * 3 // 2, deint, kw
        self.pending, self.submits, self.max_pending = deque(), [], 0
        self.closed = self.syncs = self.last_total = 0
        self.packets, self.pipe = [], None
        Enc.opened.append(self)

    def close(self):
        self.closed += 1

    def submit(self, arr, n, halo=0):
        if len(self.submits) + 1 == self.fail_submit:
            raise Boom("submit")
        assert len(self.pending) < self.host_depth, "a submit beyond host_depth"
        assert not halo or self.deint, "a halo submit to a context without a deinterlacer"
        fb, front = self.frame_bytes, halo & 1
        fr = [bytes(arr[i * fb:(i + 1) * fb]) for i in range(len(arr) // fb)]
        self.pending.append((arr, digest(arr), fr[front:front + n]))
        self.max_pending = max(self.max_pending, len(self.pending))
        self.submits.append(dict(n=n, halo=halo, nbytes=len(arr), first=fr[front][0],
                                 front=fr[0] if front else None, back=fr[front + n] if halo >> 1 else None))

    def sync(self):
        self.syncs += 1
        if self.syncs == self.fail_sync:
            raise Boom("sync")
        arr, d, frames = self.pending.popleft()
        assert digest(arr) == d, "a batch buffer changed before its submit was synced"
        self.packets = [packet(f, self.big_from) for f in frames]
        self.last_total = sum(len(p) for p in self.packets)

    def fetch_into(self, buf):
        assert buf.nbytes >= self.last_total, "an output buffer smaller than last_total"
        pipe = self.pipe
        with pipe.ofree.mutex:  # written by the muxer and handed back: anybody's
            for k in pipe.ofree.queue:
                if pipe.obufs[k] is not None:
                    pipe.obufs[k].array[:] = 0xAA
        out, o, mv = [], 0, memoryview(buf.array)
        for p in self.packets:
            buf.array[o:o + len(p)] = np.frombuffer(p, np.uint8)
            out.append(mv[o:o + len(p)])
            o += len(p)
        return out

    def holds(self, buf) -> bool:
        return any(np.shares_memory(buf.array, arr) for arr, _, _ in self.pending)


class Watched(queue.Queue):
    """A free list that checks every buffer index put back on it."""

    def __init__(self, check, n):
        super().__init__()
        self.check = check
        for i in range(n):
            super().put(i)

    def put(self, item, *a, **kw):
        self.check(item)
        super().put(item, *a, **kw)


class Mkv(container.MkvWriter):
    """The writer, remembering the packets it has taken and not yet written."""
    held: tuple = ()

    def write_frame(self, p):
        self.held += (p,)
        super().write_frame(p)

    def flush_pending(self):
        super().flush_pending()
        self.held = ()


class Out(io.BytesIO):
    """stdout: the `fail`-th cluster raises OSError, the `block`-th waits for `gate`."""

    def __init__(self, fail=0, block=0):
        super().__init__()
        self.fail, self.block, self.n, self.gate = fail, block, 0, threading.Event()

    def writelines(self, pieces):
        self.n += 1
        if self.n == self.fail:
            raise OSError("stdout is gone")
        if self.n == self.block:
            self.gate.wait(10)
        super().writelines(pieces)


class Src:
    """A worker.Source that records skip() and close(), and whose `block`-th read waits for `gate`."""

    def __init__(self, raw, block=0):
        self.real = worker.Source(raw, 2)
        self.info, self.duration = self.real.info, None
        self.skips, self.closes, self.reads, self.block, self.gate = [], [], 0, block, threading.Event()

    def read_into(self, buf, n):
        self.reads += 1
        if self.reads == self.block:
            self.gate.wait(10)
        return self.real.read_into(buf, n)

    def skip(self, n):
        self.skips.append(n)
        return self.real.skip(n)

    def close(self, kill=False):
        self.closes.append(kill)
        return self.real.close(kill)


@pytest.fixture(autouse=True)
def stand_ins(monkeypatch):
    """Context's lazy `from .encoder import ...` finds the stand-ins; nothing of the GPU is imported."""
    monkeypatch.setitem(sys.modules, "ffmpeg_distributed_amd.encoder",
                        types.SimpleNamespace(MjpegEncoder=Enc, PinnedBuffer=Buf))
    for name, v in (("opened", []), ("fail_submit", 0), ("fail_sync", 0), ("big_from", 999)):
        monkeypatch.setattr(Enc, name, v)
    monkeypatch.setattr(Buf, "made", [])
    monkeypatch.setattr(worker, "JOIN_TIMEOUT", 0.05)
    before = {k for k in sys.modules if k == "torch" or k.endswith("._lib")}
    yield
    assert {k for k in sys.modules if k == "torch" or k.endswith("._lib")} == before


def plan_of(deint=0, cls=worker.SegmentPlan, **kw):
    return cls(src_chroma="420", dst_chroma="420", deint=deint, orient=0, rect=None, in_size=(W, H), dst_w=W,
               dst_h=H, pad=None, enc_w=W, enc_h=H, unsharp=None, lut_in=None, lut_out=None, cmat=None,
               sar=(1, 1), **kw)


class Seg:
    """One segment through Context.acquire, Pipeline and Context.settle, as worker.run() takes it."""

    def __init__(self, data, cache=None, plan=None, args=ARGS, out=None, block_read=0):
        self.src = Src(io.BytesIO(data) if isinstance(data, bytes) else data, block_read)
        self.plan, self.out, self.err = plan or plan_of(), out or Out(), io.StringIO()
        prof, info = profile.try_parse(args)[0], self.src.info
        self.ctx = worker.Context.acquire(cache, 0, prof, info, self.plan, self.plan.batch(BATCH), False)
        self.enc, self.cache = self.ctx.enc, cache
        fps = self.plan.rate(info)
        self.pipe = pipe = worker.Pipeline(self.enc, self.ctx.bufs, self.ctx.obufs, self.ctx.new_obuf, self.src,
                                           Mkv(self.out, W, H, fps, (1, 1)), worker.Progress(self.err, fps, 5),
                                           self.plan.batch(BATCH), self.plan.framestep, bool(self.plan.deint))
        self.enc.pipe, self.enc.submits, self.enc.max_pending, self.enc.syncs = pipe, [], 0, 0  # per segment

        def batch_buffer_back(j):  # only after its submit was synced
            assert j < 0 or not self.enc.holds(pipe.bufs[j]), "a batch buffer handed back before its sync"

        def output_buffer_back(k):  # only after the muxer wrote its packets (a failed muxer writes no more)
            assert pipe.mux_err or not any(np.shares_memory(np.asarray(p), pipe.obufs[k].array) for p in pipe.mkv.held), \
                "an output buffer handed back before its packets were written"
        pipe.free, pipe.ofree = Watched(batch_buffer_back, len(pipe.bufs)), Watched(output_buffer_back, len(pipe.obufs))

    def run(self):
        try:
            self.pipe.run()
        finally:
            self.rc = self.pipe.stop()
            self.ctx.settle(self.cache, self.pipe)
        return self

    def packets(self):
        return [d for _, d in container.MkvReader(io.BytesIO(self.out.getvalue())).frames(1)]

    def threads_alive(self):
        return self.pipe.th.is_alive() or self.pipe.mt.is_alive()


def check_whole(s: Seg, kept):
    """A segment that went through: the packets of frames `kept` in order, the final progress line, every
    batch buffer back on the free list, no thread left, the source closed without a kill."""
    assert s.packets() == [packet(frame(k), s.enc.big_from) for k in kept]
    lines = s.err.getvalue().splitlines()
    assert re.match(rf"frame=\s*{len(kept)} ", lines[-1]), lines
    assert sorted(s.pipe.free.queue) == [-1] + list(range(len(s.pipe.bufs)))
    assert not s.threads_alive() and s.rc == 0 and s.src.closes == [False] and not s.pipe.failed
    nsub = -(-len(kept) // s.pipe.batch)
    assert len(s.enc.submits) == nsub and s.enc.max_pending == min(nsub, s.enc.host_depth) and not s.enc.pending


# ---------------------------------------------------------------------------------- order and completeness
@pytest.mark.parametrize("nbuf", [3, 4])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7])
def test_frames_come_out_in_order(monkeypatch, n, nbuf):
    monkeypatch.setattr(worker, "NBUF", nbuf)
    s = Seg(y4m(n)).run()
    assert len(s.pipe.bufs) == nbuf and all(b.nbytes == BATCH * FB for b in s.pipe.bufs)
    check_whole(s, range(n))
    assert [(u["n"], u["halo"], u["nbytes"]) for u in s.enc.submits] == \
        [(min(BATCH, n - f), 0, min(BATCH, n - f) * FB) for f in range(0, n, BATCH)]
    # one segment, no cache: everything is closed and freed once
    assert s.enc.closed == 1 and [b.freed for b in Buf.made] == [1] * len(Buf.made)


# ---------------------------------------------------------------------------------- deinterlaced segments
@pytest.mark.parametrize("nbuf", [3, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6])
def test_deinterlaced_submits_follow_the_schedule(monkeypatch, n, nbuf):
    monkeypatch.setattr(worker, "NBUF", nbuf)
    s = Seg(y4m(n), plan=plan_of(deint=1)).run()
    assert all(b.nbytes == (BATCH + 2) * FB for b in s.pipe.bufs)
    check_whole(s, range(n))
    sched = worker.deint_schedule(n, BATCH)
    assert [(u["first"], u["n"], bool(u["halo"] & 1), bool(u["halo"] >> 1)) for u in s.enc.submits] == sched
    for u, (first, m, hp, hn) in zip(s.enc.submits, sched):
        assert u["front"] == (frame(first - 1) if hp else None)
        assert u["back"] == (frame(first + m) if hn else None)
        assert u["nbytes"] == (m + hp + hn) * FB


# ---------------------------------------------------------------------------------- framestep
@pytest.mark.parametrize("n", [7, 9])
def test_framestep_keeps_every_third_frame(n):
    s = Seg(y4m(n), plan=plan_of(cls=worker.SheetPlan, framestep=3, out_fps=Fraction(25, 3))).run()
    check_whole(s, range(0, n, 3))
    assert s.src.skips == [2] * len(range(0, n, 3))  # after every frame kept; the last finds what is left


# ---------------------------------------------------------------------------------- output buffers
def test_a_larger_submit_regrows_its_output_buffer(monkeypatch):
    monkeypatch.setattr(worker, "NOUT", 1)
    monkeypatch.setattr(Enc, "big_from", 4)
    s = Seg(y4m(6)).run()
    check_whole(s, range(6))
    obufs = Buf.made[worker.NBUF:]
    assert [b.nbytes for b in obufs] == [1 << 20, (2 * len(packet(frame(4), 4))) * 3 // 2]
    assert [b.freed for b in obufs] == [1, 1] and s.pipe.obufs == [obufs[1]]


@pytest.mark.parametrize("nout", [1, 2, 6])
def test_output_buffers_are_reused(monkeypatch, nout):
    monkeypatch.setattr(worker, "NOUT", nout)
    s = Seg(y4m(23)).run()
    check_whole(s, range(23))
    assert len(Buf.made) - worker.NBUF == min(nout, 12)


# ---------------------------------------------------------------------------------- failures
def raw_mkv_cut_short(tmp_path):
    p = tmp_path / "cut.mkv"
    with open(p, "wb") as f:
        wr = container.MkvWriter(f, W, H, Fraction(25), codec="V_UNCOMPRESSED", colour_space=b"I420")
        for k in range(9):
            wr.write_frame(frame(k))
        wr.close()
    p.write_bytes(p.read_bytes()[:-5])  # the file ends inside the last frame
    return open(p, "rb")


@pytest.mark.parametrize("what", ["submit", "sync", "source", "stdout"])
def test_a_failing_segment_is_torn_down(monkeypatch, tmp_path, what):
    data, out, exc = y4m(9), Out(), Boom
    if what == "submit":
        monkeypatch.setattr(Enc, "fail_submit", 2)
    elif what == "sync":
        monkeypatch.setattr(Enc, "fail_sync", 2)
    elif what == "source":
        data, exc = raw_mkv_cut_short(tmp_path), ValueError
    else:
        out, exc = Out(fail=2), OSError
    cache = {}
    s = Seg(data, cache=cache, out=out)
    assert cache["ctx"] is s.ctx
    with pytest.raises(exc):
        s.run()
    assert s.pipe.failed and s.src.closes[-1] is True
    assert cache == {} and s.enc.closed == 1
    assert len(Buf.made) >= worker.NBUF and [b.freed for b in Buf.made] == [1] * len(Buf.made)
    assert not s.threads_alive()
    if not isinstance(data, bytes):
        data.close()


# ---------------------------------------------------------------------------------- stuck threads
def test_a_stuck_reader_keeps_the_batch_buffers(monkeypatch):
    cache = {}
    s = Seg(y4m(9), cache=cache, block_read=3)
    t0 = time.monotonic()
    try:
        with pytest.raises(Boom):   # the second submit fails while the reader sits in its third read
            monkeypatch.setattr(Enc, "fail_submit", 2)
            s.run()
        assert time.monotonic() - t0 < 1.0
        assert s.pipe.reader_stuck and not s.pipe.muxer_stuck and s.src.closes == [True, True]
        assert cache == {} and s.enc.closed == 1
        assert [b.freed for b in s.pipe.bufs] == [0] * worker.NBUF
        assert [b.freed for b in Buf.made[worker.NBUF:]] == [1] * (len(Buf.made) - worker.NBUF)
    finally:
        s.src.gate.set()
        s.pipe.th.join(5)
    assert not s.threads_alive()


def test_a_stuck_muxer_keeps_the_output_buffers(monkeypatch):
    cache = {}
    s = Seg(y4m(9), cache=cache, out=Out(block=1))
    t0 = time.monotonic()
    try:
        with pytest.raises(Boom):   # the fourth submit fails while the muxer sits in its first write
            monkeypatch.setattr(Enc, "fail_submit", 4)
            s.run()
        assert time.monotonic() - t0 < 1.0
        assert s.pipe.muxer_stuck and not s.pipe.reader_stuck
        assert cache == {} and s.enc.closed == 1
        assert [b.freed for b in s.pipe.bufs] == [1] * worker.NBUF
        obufs = Buf.made[worker.NBUF:]
        assert obufs and [b.freed for b in obufs] == [0] * len(obufs)
    finally:
        s.out.gate.set()
        s.pipe.mt.join(5)
    assert not s.threads_alive()


# ---------------------------------------------------------------------------------- context reuse
def test_a_context_serves_segments_of_one_key(monkeypatch):
    cache = {}
    a = Seg(y4m(5), cache=cache).run()
    b = Seg(y4m(3), cache=cache).run()
    check_whole(b, range(3))
    assert b.ctx is a.ctx and len(Enc.opened) == 1 and a.enc.closed == 0 and cache["ctx"] is a.ctx
    assert not any(x.freed for x in Buf.made)
    # another key (a deinterlacer): the first context is closed and freed before the second is opened
    first = list(Buf.made)
    seen = []
    monkeypatch.setattr(Enc, "__init__", lambda self, *a_, _init=Enc.__init__, **kw: (
        seen.append((a.enc.closed, [x.freed for x in first])), _init(self, *a_, **kw))[1])
    c = Seg(y4m(5), cache=cache, plan=plan_of(deint=1)).run()
    check_whole(c, range(5))
    assert seen == [(1, [1] * len(first))] and c.ctx is not a.ctx and cache["ctx"] is c.ctx
    # a failed segment in between: the next one of the same key opens a context of its own
    monkeypatch.setattr(Enc, "fail_sync", 1)
    with pytest.raises(Boom):
        Seg(y4m(5), cache=cache, plan=plan_of(deint=1)).run()
    assert cache == {} and c.enc.closed == 1
    monkeypatch.setattr(Enc, "fail_sync", 0)
    d = Seg(y4m(5), cache=cache, plan=plan_of(deint=1)).run()
    check_whole(d, range(5))
    assert d.ctx is not c.ctx and len(Enc.opened) == 3 and d.enc.closed == 0
    worker.release(cache)
    assert cache == {} and d.enc.closed == 1 and [x.freed for x in Buf.made] == [1] * len(Buf.made)


def test_the_plan_answers_for_batch_and_rate():
    info = container.StreamInfo(W, H, Fraction(30))
    assert (plan_of().framestep, plan_of().sheet, plan_of().rate(info), plan_of().batch(10)) == (1, None, 30, 10)
    sheet = plan_of(cls=worker.SheetPlan, sheet=(2, 2, 4, 0, 0), framestep=2, out_fps=Fraction(15, 4))
    assert (sheet.rate(info), sheet.batch(10), sheet.batch(3)) == (Fraction(15, 4), 8, 4)
    assert plan_of(cls=worker.SheetPlan, framestep=2).batch(10) == 10


# ---------------------------------------------------------------------------------- the trace line
TRACE = re.compile(r"mjg-trace: frames=(\d+) total=[\d.]+ setup=[\d.]+ (handoff=[\d.]+ (client=[\d.]+ )?)?"
                   + " ".join(rf"{k}=[\d.]+" for k in ("read", "submit", "sync", "fetch", "mux", "wait"))
                   + r" .*cpu_now=-?\d+ gpu_node=-?\d+ bound=\S+\n")


def test_the_trace_line():
    s = Seg(y4m(5)).run()
    t = time.monotonic()
    m = TRACE.fullmatch(worker.trace_line(worker.Options(trace=True), s.pipe, t - 2.0, t - 1.0))
    assert m and m.group(1) == "5" and m.group(2) is None
    line = worker.trace_line(worker.Options(trace=True, t_accept=t - 3.0, client_t0=t - 4.0), s.pipe, t - 2.0, t - 1.0)
    assert TRACE.fullmatch(line) and " setup=1.0000 handoff=1.0000 client=1.0000 read=" in line
    line = worker.trace_line(worker.Options(trace=True, t_accept=t - 3.0), s.pipe, t - 2.0, t - 1.0)
    assert TRACE.fullmatch(line) and " handoff=1.0000 read=" in line
