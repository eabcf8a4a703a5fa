"""`-vf hqdn3d` without a GPU: the parser both ways, the tables, the worked example of DESIGN §4.19, the plan
and its cache key, a segment through worker.Pipeline with stand-ins (the first submit plain, every later one
continued, with yadif's halos), and the library's refusals, which come before any HIP call.

The worked example holds frames 1 and 2, the final state row and frame 2 under a second pair of tables as
recorded figures.  A sequence's first frame is not its input: out_0 = c(M, L(s_0), V_0) >> 8 differs from s_0
in 5 of the example's 15 samples, by 1, and frame 1 and everything behind it depend on that very A_0, so frame 0
is asserted as the formulas give it."""
import ctypes as C
import io
import threading

import numpy as np
import pytest

import hqdn3d_ref as R
from ffmpeg_distributed_amd import _lib, container, profile, worker

TAIL = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact"


def parse(vf):
    return profile.try_parse(["-vf", vf] + TAIL.split())


# ------------------------------------------------------------------------- the parser
@pytest.mark.parametrize("vf,want", [
    ("hqdn3d", (4.0, 3.0, 6.0, 4.5)),
    ("hqdn3d=4:3:6:4.5", (4.0, 3.0, 6.0, 4.5)),
    ("hqdn3d=0", (4.0, 3.0, 6.0, 4.5)),                       # 0 is taken as the default
    ("hqdn3d=0:0:0:0", (4.0, 3.0, 6.0, 4.5)),
    ("hqdn3d=8", (8.0, 6.0, 12.0, 9.0)),
    ("hqdn3d=2:0:3", (2.0, 1.5, 3.0, 2.25)),
    ("hqdn3d=1.5:1.5:6:6", (1.5, 1.5, 6.0, 6.0)),
    ("hqdn3d=luma_tmp=3", (4.0, 3.0, 3.0, 2.25)),
    ("hqdn3d=luma_spatial=2:chroma_spatial=1:luma_tmp=5:chroma_tmp=7", (2.0, 1.0, 5.0, 7.0)),
    ("hqdn3d=2:chroma_tmp=1", (2.0, 1.5, 3.0, 1.0)),
    ("hqdn3d=.5", (0.5, 0.375, 0.75, 0.5625)),
])
def test_parse_strengths(vf, want):
    p, why = parse(vf)
    assert why is None and type(p) is profile.DenoiseProfile
    assert tuple(p.hqdn3d[k] for k in profile.HQDN3D_NAMES) == want
    assert want == R.strengths(*[0.0 if "=" not in vf else v for v in _given(vf)])


def _given(vf):
    """The four values as the graph gives them (0: absent), for the reference's own resolution."""
    vals, pos = dict.fromkeys(profile.HQDN3D_NAMES, 0.0), 0
    for p in (vf.split("=", 1)[1].split(":") if "=" in vf else []):
        if "=" in p:
            k, v = p.split("=")
            vals[profile.HQDN3D_KEYS[k]] = float(v)
        else:
            vals[profile.HQDN3D_NAMES[pos]] = float(p)
            pos += 1
    return [vals[k] for k in profile.HQDN3D_NAMES]


def test_graphs_with_it_parse():
    p, why = parse("hqdn3d,scale=64:32")
    assert why is None and type(p) is profile.DenoiseProfile and p.scale == (64, 32) and p.deint is None
    p, why = parse("yadif,hqdn3d=4:3:6:4.5")
    assert why is None and type(p) is profile.DenoiseProfile and p.deint == {"mode": 0, "parity": -1}
    assert p.hqdn3d == {"ls": 4.0, "cs": 3.0, "lt": 6.0, "ct": 4.5}
    p, why = parse("yadif,hqdn3d,vflip,crop=32:16,scale=16:8,unsharp,pad=20:10")
    assert why is None and p.orient == 4 and p.crop and p.pad and p.unsharp


@pytest.mark.parametrize("vf", [None, "scale=8:8", "yadif,scale=8:8", "crop=64:32,scale=32:16,unsharp,pad=40:24"])
def test_a_graph_without_it_is_the_profile_it_was(vf):
    p = profile.parse((["-vf", vf] if vf else []) + TAIL.split())
    assert type(p) is profile.Profile and not hasattr(p, "hqdn3d")
    assert "hqdn3d" not in profile.parse_graph(vf or "scale=8:8")


@pytest.mark.parametrize("vf,reason", [
    ("scale=64:32,hqdn3d", "hqdn3d after scale"),
    ("yadif,vflip,hqdn3d", "hqdn3d after vflip"),
    ("vflip,hqdn3d", "hqdn3d after vflip"),
    ("hqdn3d,yadif", "yadif after hqdn3d"),
    ("hqdn3d,hqdn3d", "a second hqdn3d"),
    ("yadif,hqdn3d,scale=8:8,hqdn3d", "a second hqdn3d"),
    ("hqdn3d=2*3", "hqdn3d ls='2*3'"),
    ("hqdn3d=4:min(3\\,2)", "hqdn3d"),
    ("hqdn3d=-1", "hqdn3d ls=-1: a negative strength"),
    ("hqdn3d=4:3:-0.5", "hqdn3d lt=-0.5: a negative strength"),
    ("hqdn3d=abc", "hqdn3d ls='abc'"),
    ("hqdn3d=luma_tmp=x", "hqdn3d lt='x'"),
    ("hqdn3d=strength=3", "hqdn3d option 'strength'"),
    ("hqdn3d=1:2:3:4:5", "more than four positional values"),
    ("hqdn3d=", "hqdn3d= without options"),
    ("framestep=2,hqdn3d", "hqdn3d together with framestep"),
    ("hqdn3d,scale=8:8,tile=2x2", "hqdn3d together with tile"),
    ("thumbnail=2,hqdn3d,scale=8:8,tile=2x2", "hqdn3d together with thumbnail"),
])
def test_rejects_name_their_reason(vf, reason):
    p, why = parse(vf)
    assert p is None and reason in why, why


# ------------------------------------------------------------------------- the tables
CHECK = {4.0: ([-38, -24, -8, 7, 23, 37, 52], -272, 273), 3.0: ([-38, -23, -8, 7, 23, 37, 50], -204, 204),
         6.0: ([-39, -24, -8, 7, 23, 38, 53], -409, 409), 4.5: ([-39, -24, -8, 7, 23, 38, 52], -307, 307)}


def test_table_check_values():
    tabs = profile.hqdn3d_tables({"ls": 4.0, "cs": 3.0, "lt": 6.0, "ct": 4.5})
    assert tabs.shape == (4, 8192) and tabs.dtype == np.int16
    for t, s in zip(tabs, (4.0, 3.0, 6.0, 4.5)):
        mid, lo, hi = CHECK[s]
        assert t[4093:4100].tolist() == mid and t[0] == 1
        assert (int(t[1:].min()), int(t.max())) == (lo, hi)


@pytest.mark.parametrize("spec", [(4.0, 3.0, 6.0, 4.5), R.STRENGTHS, (0.5, 300.0, 252.0, 1.0)])
def test_tables_equal_the_reference_builders(spec):
    got = profile.hqdn3d_tables(dict(zip(profile.HQDN3D_NAMES, spec)))
    for g, s in zip(got, spec):
        assert (g == R.table(s)).all()


# ------------------------------------------------------------------------- the worked example
def _example():
    return [[[100 + (7 * x + 5 * y + 3 * t + x * y * t) % 11 for x in range(5)] for y in range(3)] for t in range(3)]


def test_worked_example():
    fr = _example()
    outs, A = R.scalar_plane_sequence(fr, R.table(4.0), R.table(6.0))
    assert outs[1] == [[102, 108, 105, 104, 107], [106, 106, 106, 107, 107], [104, 103, 106, 108, 106]]
    assert outs[2] == [[104, 105, 107, 105, 103], [102, 106, 107, 107, 105], [104, 105, 106, 107, 105]]
    assert A[0] == [26861, 26899, 27466, 26974, 26611]
    # frame 0 is not the input (the module's docstring): five samples are off by 1
    assert outs[0] == [[100, 107, 103, 110, 106], [105, 102, 107, 105, 100], [110, 106, 103, 108, 105]]
    assert sum(a != b for ra, rb in zip(outs[0], fr[0]) for a, b in zip(ra, rb)) == 5
    outs2, _ = R.scalar_plane_sequence(fr, R.table(3.0), R.table(4.5))
    assert outs2[2] == [[105, 104, 107, 105, 102], [101, 107, 107, 107, 104], [104, 105, 107, 107, 105]]


def test_the_vector_reference_equals_the_scalar_loops():
    """5 x 3 4:4:4 frames whose three planes are the example's: luma with tables 4 / 6, chroma with 3 / 4.5;
    as one sequence, and as 1 + 2 frames continued through the state."""
    fr = np.array(_example(), np.uint8)
    frames = np.stack([np.concatenate([f.reshape(-1)] * 3) for f in fr])
    tabs = R.tables()
    out, st = R.denoise(frames, 5, 3, "444", tabs)
    yo, A = R.scalar_plane_sequence(fr.tolist(), tabs[0], tabs[2])
    co, Ac = R.scalar_plane_sequence(fr.tolist(), tabs[1], tabs[3])
    for t in range(3):
        assert out[t][:15].reshape(3, 5).tolist() == yo[t]
        assert out[t][15:30].reshape(3, 5).tolist() == co[t] == out[t][30:].reshape(3, 5).tolist()
    assert st[:15].reshape(3, 5).tolist() == A and st[15:30].reshape(3, 5).tolist() == Ac
    a, s1 = R.denoise(frames[:1], 5, 3, "444", tabs)
    b, s2 = R.denoise(frames[1:], 5, 3, "444", tabs, s1)
    assert (np.concatenate([a, b]) == out).all() and (s2 == st).all()
    c, _ = R.denoise(frames[1:], 5, 3, "444", tabs)
    assert not (c == out[1:]).all()      # a sequence of its own differs


@pytest.mark.parametrize("w,h,c", [(8, 8, "420"), (5, 3, "444")], ids=["8x8_420", "5x3_444"])
def test_denoise_indexed_equals_denoise_on_200_frames(w, h, c):
    """tests/test_gpu_long_stages.py's reference (the spatial scans once per distinct frame, the time scan over the
    index) byte for byte against denoise() on 200 frames that cycle through 7 base frames: as one sequence, and as
    two segments (77 + 123), which denoise() runs as two calls."""
    tabs = np.stack(R.tables(*R.STRENGTHS))
    base = R.make_frames("noise", w, h, c, 7, seed=3)
    idx = (np.arange(200) * 3 + np.arange(200) // 50) % 7
    frames = base[idx]
    want, wst = R.denoise(frames, w, h, c, tabs)
    got, gst = R.denoise_indexed(base, idx, w, h, c, tabs)
    assert got.dtype == np.uint8 and gst.dtype == np.uint16 and (got == want).all() and (gst == wst).all()
    assert not (want == frames).all() and len({f.tobytes() for f in want}) > 7      # the tables act, history matters
    a, _ = R.denoise(frames[:77], w, h, c, tabs)
    b, bst = R.denoise(frames[77:], w, h, c, tabs)
    got, gst = R.denoise_indexed(base, idx, w, h, c, tabs, segs=[(0, 77), (77, 123)])
    assert (got == np.concatenate([a, b])).all() and (gst == bst).all()
    assert not (b[0] == want[77]).all()      # the second segment starts over
    _, s77 = R.denoise_indexed(base, idx[:77], w, h, c, tabs)
    got, gst = R.denoise_indexed(base, idx[77:], w, h, c, tabs, state=s77)      # continued, as denoise(state=) is
    assert (got == want[77:]).all() and (gst == wst).all()
    with pytest.raises(AssertionError):
        R.denoise_indexed(base, idx, w, h, c, tabs, segs=[(0, 77), (78, 122)])


def test_the_reference_asserts_its_bounds():
    bad = R.table(4.0).copy()
    bad[4096 - 40:4096 + 40] = 30000
    with pytest.raises(AssertionError):
        R.denoise(R.make_frames("full", 8, 4, "444", 3), 8, 4, "444", (bad, bad, bad, bad))


# ------------------------------------------------------------------------- the plan and the cache key
class Info:
    width, height, chroma, full_range, field, sar, fps, bits = 64, 32, "420", False, "p", (1, 1), 25, 8
    frame_bytes = 64 * 32 * 3 // 2


def test_plan_carries_the_tables_and_the_key_the_strengths():
    p, _ = parse("yadif,hqdn3d=2:1:5:7,scale=32:16")
    plan = worker.plan_segment(p, Info())
    assert type(plan) is worker.DenoisePlan and plan.deint == 1
    assert (plan.denoise == profile.hqdn3d_tables(p.hqdn3d)).all()
    assert (plan.encoder_kwargs()["denoise"] == plan.denoise).all()
    key = plan.key(p, Info(), False, 4)
    assert key[-1] == ("hqdn3d", 2.0, 1.0, 5.0, 7.0)
    q, _ = parse("yadif,hqdn3d=2:1:5:6,scale=32:16")
    assert worker.plan_segment(q, Info()).key(q, Info(), False, 4) != key
    plain, _ = parse("yadif,scale=32:16")
    pp = worker.plan_segment(plain, Info())
    assert type(pp) is worker.SegmentPlan and pp.denoise is None and "denoise" not in pp.encoder_kwargs()
    assert pp.key(plain, Info(), False, 4) == key[:-1]


def test_more_than_eight_bits_fall_through():
    p, _ = parse("hqdn3d")

    class Deep(Info):
        bits = 10
    with pytest.raises(worker.Fallthrough) as e:
        worker.plan_segment(p, Deep())
    assert "hqdn3d on a 10-bit input" in str(e.value)

    class Wide(Info):
        frame_bytes = 2 * Info.frame_bytes
    with pytest.raises(worker.Fallthrough) as e:
        worker.plan_segment(p, Wide())
    assert "hqdn3d" in str(e.value) and "more than 8 bits" in str(e.value)
    assert worker.denoise_fallthrough_reason(parse("scale=8:8")[0], Deep()) is None


# ------------------------------------------------------------------------- the pipeline, with stand-ins
W, H, FB, BATCH = 4, 2, 12, 2


def _y4m(n):
    return b"YUV4MPEG2 W4 H2 F25:1 Ip A1:1 C420jpeg\n" + b"".join(b"FRAME\n" + bytes([k] * FB) for k in range(n))


class Buf:
    def __init__(self, nbytes):
        self.nbytes, self.array = int(nbytes), np.zeros(int(nbytes), np.uint8)

    def free(self):
        pass


class Enc:
    """encoder.MjpegEncoder's stand-in: it records every submit and encodes a frame to its first byte."""
    host_depth, frame_bytes = 2, FB

    def __init__(self):
        self.calls, self.pending, self.packets, self.last_total = [], [], [], 0

    def submit(self, arr, n, halo=0, cont=False):
        assert len(self.pending) < self.host_depth
        front = halo & 1
        fr = [int(arr[i * FB]) for i in range(len(arr) // FB)]
        self.calls.append((fr[front], n, halo & 1, halo >> 1, bool(cont)))
        assert len(fr) == n + front + (halo >> 1)
        self.pending.append(fr[front:front + n])

    def sync(self):
        self.packets = [b"\xff\xd8" + bytes([k]) * 5 + b"\xff\xd9" for k in self.pending.pop(0)]
        self.last_total = sum(len(p) for p in self.packets)

    def fetch_into(self, buf):
        out, o = [], 0
        for p in self.packets:
            buf.array[o:o + len(p)] = np.frombuffer(p, np.uint8)
            out.append(bytes(buf.array[o:o + len(p)]))
            o += len(p)
        return out


def _segment(n, deint, denoise=True, enc=None):
    src = worker.Source(io.BytesIO(_y4m(n)), 2)
    enc, out, err = enc or Enc(), io.BytesIO(), io.StringIO()
    bufs = [Buf((BATCH + (2 if deint else 0)) * FB) for _ in range(3)]
    pipe = worker.Pipeline(enc, bufs, [None] * 3, Buf, src, container.MkvWriter(out, W, H, 25, (1, 1)),
                           worker.Progress(err, 25, 5), BATCH, 1, deint, None, denoise)
    try:
        pipe.run()
    finally:
        assert pipe.stop() == 0
    assert not pipe.failed and threading.active_count() >= 1
    packets = [d for _, d in container.MkvReader(io.BytesIO(out.getvalue())).frames(1)]
    assert [p[2] for p in packets] == list(range(n))
    return enc


def test_pipeline_first_submit_plain_and_the_rest_continued():
    n = 3 * BATCH + 1
    enc = _segment(n, False)
    assert enc.calls == [(0, 2, 0, 0, False), (2, 2, 0, 0, True), (4, 2, 0, 0, True), (6, 1, 0, 0, True)]
    # a context from the serve cache starts its next segment with a plain submit
    _segment(n, False, enc=enc)
    assert enc.calls[4:] == enc.calls[:4]


def test_pipeline_with_yadif_follows_deint_schedule():
    n = 3 * BATCH + 1
    enc = _segment(n, True)
    sched = worker.deint_schedule(n, BATCH)
    assert len(sched) == 4
    assert enc.calls == [(first, k, int(hp), int(hn), i > 0) for i, (first, k, hp, hn) in enumerate(sched)]


def test_pipeline_without_a_denoiser_submits_as_before():
    """No `cont` keyword reaches an encoder of a graph without the filter (stand-ins of other tests have none)."""
    class Old(Enc):
        def submit(self, arr, n, halo=0):
            super().submit(arr, n, halo)
    enc = _segment(5, False, denoise=False, enc=Old())
    assert [c[4] for c in enc.calls] == [False] * 3


# ------------------------------------------------------------------------- the library, before any HIP call
def _cfg(w=16, h=16, cf=0):
    return _lib.MjgConfig(w, h, w, h, 1, 5, 1, 1, 4, 0, cf)


def _open(cfg, chain, sheet, dn):
    L = _lib.load()
    h = C.c_void_p()
    rc = L.mjg_open_denoise(0, None if cfg is None else C.byref(cfg), C.byref(chain),
                            None if sheet is None else C.byref(sheet), None if dn is None else C.byref(dn), C.byref(h))
    assert not h.value
    return rc, L.mjg_last_error().decode()


def test_library_refusals_come_before_any_hip_call():
    dn = _lib.MjgDenoise.from_buffer_copy(np.stack(R.tables()).astype(np.int16).tobytes())
    assert C.sizeof(_lib.MjgDenoise) == 4 * 8192 * 2
    rc, msg = _open(None, _lib.MjgChain(), None, dn)
    assert rc == _lib.MJG_E_INVALID and msg == "null argument"
    rc, msg = _open(_cfg(), _lib.MjgChain(), _lib.MjgSheet(2, 2, 0, 0, 0), dn)
    assert rc == _lib.MJG_E_INVALID and msg.startswith("denoise"), msg
    rc, msg = _open(_cfg(), _lib.MjgChain(orient=9), None, dn)          # the chain's own refusals come first
    assert rc == _lib.MJG_E_INVALID and msg.startswith("orient 9"), msg
    rc, msg = _open(_cfg(), _lib.MjgChain(), _lib.MjgSheet(0, 2, 0, 0, 0), dn)   # ... and the sheet's
    assert rc == _lib.MJG_E_INVALID and msg.startswith("sheet"), msg
    L = _lib.load()
    buf = (C.c_uint8 * 16)()
    assert L.mjg_submit_cont(None, buf, 1, 0, 0, 1) == _lib.MJG_E_INVALID
    assert L.mjg_last_error().decode() == "null argument"
    assert L.mjg_debug_denoise(None, 0, buf, 16) == _lib.MJG_E_INVALID
    assert L.mjg_debug_denoise_state(None, C.cast(buf, C.POINTER(C.c_uint16)), 8) == _lib.MJG_E_INVALID
    assert L.mjg_version() == 105


def test_encoder_refuses_tables_of_another_shape():
    from ffmpeg_distributed_amd.encoder import MjpegEncoder
    with pytest.raises(ValueError) as e:
        MjpegEncoder(0, 16, 16, denoise=np.zeros((3, 8192), np.int16))
    assert "(4, 8192) int16" in str(e.value)
