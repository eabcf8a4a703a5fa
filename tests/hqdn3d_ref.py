"""`-vf hqdn3d` restated for the tests: the 8-bit C path of vf_hqdn3d.c as DESIGN §4.19 gives it (unpinned
against FFmpeg), as index loops.  Every scan walks its own axis one index at a time; what is independent
of the scan (the other axis) is a numpy vector, and `scalar_*` below are the same loops on Python ints,
which tests/test_hqdn3d.py holds the vectors to.  Its own table builder.  Every value and every table
index a call meets is asserted to lie in 0..65535 and 1..8191.

    L(v) = (v << 8) + 127          c(tab, a, b) = b + tab[4096 + ((a - b) >> 4)]
    row 0:     P[0][0] = c(S, L(s[0][0]), L(s[0][0]));  P[0][x] = c(S, P[0][x-1], L(s[0][x]));  V[0][x] = P[0][x]
    rows y>=1: P[y][0] = L(s[y][0]);                    P[y][x] = c(S, P[y][x-1], L(s[y][x]))
               V[y][x] = c(S, V[y-1][x], P[y][x])
    time:      A_t = c(M, A_{t-1}, V_t),  A_{-1} = L(s_0);   out_t = A_t >> 8
"""
import math

import numpy as np

SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
DEFAULTS = (4.0, 3.0, 6.0, 4.5)

# (w, h, chroma) of tests/test_gpu_hqdn3d.py, and what tools/hqdn3d_host_check.py walks
GPU_SHAPES = [(3, 3, "444"), (16, 16, "420"), (33, 17, "444"), (130, 66, "422"), (4100, 5, "420"), (5, 1100, "444"),
              (640, 360, "420")]
CONTENTS = ("noise", "full", "flat")
STRENGTHS = (4.0, 2.5, 7.0, 1.5)   # four distinct ones: a swapped table shows
NFRAMES = 5


def strengths(ls=0.0, cs=0.0, lt=0.0, ct=0.0):
    """The filter's four strengths: a value that is missing or 0 is replaced, in this order."""
    ls = ls or 4.0
    cs = cs or 3.0 * ls / 4.0
    lt = lt or 6.0 * ls / 4.0
    ct = ct or lt * cs / ls
    return ls, cs, lt, ct


def table(s: float) -> np.ndarray:
    """int16 tab[8192] of one strength, in Python floats (C doubles)."""
    gamma = math.log(0.25) / math.log(1.0 - min(s, 252.0) / 255.0 - 0.00001)
    tab = np.zeros(8192, np.int16)
    for i in range(-4096, 4096):
        f = ((i << 5) + 15) / 512.0
        c = math.pow(max(0.0, 1.0 - abs(f) / 255.0), gamma) * 256.0 * f
        tab[4096 + i] = round(c)   # ties to even, as lrint
    tab[0] = 1
    return tab


def tables(ls=0.0, cs=0.0, lt=0.0, ct=0.0):
    """(ls, cs, lt, ct) tables of the resolved strengths."""
    return tuple(table(s) for s in strengths(ls, cs, lt, ct))


def _c(tab, a, b):
    """One step on int64 vectors (or ints), with the bound assertions."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    i = 4096 + ((a - b) >> 4)
    assert i.min() >= 1 and i.max() <= 8191, (int(i.min()), int(i.max()))
    r = b + tab[i].astype(np.int64)
    assert r.min() >= 0 and r.max() <= 65535, (int(r.min()), int(r.max()))
    return r


def _L(v):
    return (np.asarray(v, np.int64) << 8) + 127


def spatial(s: np.ndarray, S: np.ndarray) -> np.ndarray:
    """V of one plane s (h x w uint8) with the spatial table S: int64 h x w."""
    h, w = s.shape
    Ls = _L(s)
    P = np.zeros((h, w), np.int64)
    P[:, 0] = Ls[:, 0]
    P[0, 0] = _c(S, Ls[0, 0], Ls[0, 0])
    for x in range(1, w):            # the scan along each row; the rows are independent
        P[:, x] = _c(S, P[:, x - 1], Ls[:, x])
    V = P.copy()
    for y in range(1, h):            # the scan down each column; the columns are independent
        V[y] = _c(S, V[y - 1], P[y])
    return V


def planes(frame: np.ndarray, w: int, h: int, chroma: str):
    hs, vs = SHIFTS[chroma]
    cw, ch = (w + hs) >> hs, (h + vs) >> vs
    f = np.asarray(frame, np.uint8).reshape(-1)
    assert f.size == w * h + 2 * cw * ch, (f.size, w, h, chroma)
    return [f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:].reshape(ch, cw)]


def denoise(frames: np.ndarray, w: int, h: int, chroma: str, tabs, state=None):
    """frames (n, frame_bytes) uint8 through the filter with tabs = (ls, cs, lt, ct) tables: (out, state), out
    like frames and state the packed planar uint16 A of the last frame.  state None: a sequence of its own
    (A_{-1} is the first frame's own samples); else the state an earlier call returned, continued."""
    frames = np.asarray(frames, np.uint8)
    out = np.zeros_like(frames)
    A = None if state is None else [p.astype(np.int64) for p in _split16(state, w, h, chroma)]
    for t in range(len(frames)):
        pl = planes(frames[t], w, h, chroma)
        if A is None:
            A = [_L(p) for p in pl]
        o = []
        for k, p in enumerate(pl):
            V = spatial(p, tabs[1 if k else 0])
            A[k] = _c(tabs[3 if k else 2], A[k], V)   # the scan through time; the samples are independent
            o.append((A[k] >> 8).astype(np.uint8).reshape(-1))
        out[t] = np.concatenate(o)
    return out, np.concatenate([a.reshape(-1) for a in A]).astype(np.uint16)


def denoise_indexed(base, idx, w, h, chroma, tabs, segs=None, state=None):
    """denoise() of the frames base[idx] for long sequences that repeat few distinct frames: spatial() depends on
    the frame alone, so it is computed once per distinct base frame, and only the time scan walks idx, with the
    same _c (luma in one vector, U and V, which share a table, in another).  segs: (first, count) of each
    sequence in idx, in order and covering it (None: one sequence); the scan restarts from a sequence's own first
    frame; state (as denoise takes it): the first sequence continues the one that left it instead.  Returns
    (out, state) like denoise: state is the last sequence's."""
    base, idx = np.asarray(base, np.uint8), np.asarray(idx, np.int64)
    n, wh = len(idx), w * h
    segs = [(0, n)] if segs is None else [(int(a), int(k)) for a, k in segs]
    at = 0
    for first, count in segs:
        assert first == at and count >= 1, segs
        at += count
    assert at == n and base.shape[1] == frame_bytes(w, h, chroma)
    starts = {first for first, _ in segs}
    out = np.zeros((n, base.shape[1]), np.uint8)
    made = {}
    Ay = Ac = None
    if state is not None:
        st = np.asarray(state, np.uint16).reshape(-1).astype(np.int64)
        assert st.size == base.shape[1]
        Ay, Ac = st[:wh], st[wh:]
        starts.discard(0)
    for t in range(n):
        b = int(idx[t])
        if b not in made:
            pl = planes(base[b], w, h, chroma)
            made[b] = (_L(base[b]), spatial(pl[0], tabs[0]).reshape(-1),
                       np.concatenate([spatial(pl[1], tabs[1]).reshape(-1), spatial(pl[2], tabs[1]).reshape(-1)]))
        L, Vy, Vc = made[b]
        if t in starts:
            Ay, Ac = L[:wh], L[wh:]
        Ay, Ac = _c(tabs[2], Ay, Vy), _c(tabs[3], Ac, Vc)
        out[t, :wh], out[t, wh:] = Ay >> 8, Ac >> 8
    return out, np.concatenate([Ay, Ac]).astype(np.uint16)


def _split16(state, w, h, chroma):
    hs, vs = SHIFTS[chroma]
    cw, ch = (w + hs) >> hs, (h + vs) >> vs
    st = np.asarray(state, np.uint16).reshape(-1)
    return [st[:w * h].reshape(h, w), st[w * h:w * h + cw * ch].reshape(ch, cw), st[w * h + cw * ch:].reshape(ch, cw)]


def scalar_plane_sequence(frames, S, M):
    """The same loops on Python ints for one plane through time: frames a list of h x w lists of ints.
    Returns (outs, final A)."""
    def c(tab, a, b):
        i = 4096 + ((a - b) >> 4)
        assert 1 <= i <= 8191, i
        r = b + int(tab[i])
        assert 0 <= r <= 65535, r
        return r

    def L(v):
        return (v << 8) + 127

    h, w = len(frames[0]), len(frames[0][0])
    A = [[L(frames[0][y][x]) for x in range(w)] for y in range(h)]
    outs = []
    for s in frames:
        P = [[0] * w for _ in range(h)]
        V = [[0] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                if x == 0:
                    P[y][0] = c(S, L(s[0][0]), L(s[0][0])) if y == 0 else L(s[y][0])
                else:
                    P[y][x] = c(S, P[y][x - 1], L(s[y][x]))
        for y in range(h):
            for x in range(w):
                V[y][x] = P[y][x] if y == 0 else c(S, V[y - 1][x], P[y][x])
        for y in range(h):
            for x in range(w):
                A[y][x] = c(M, A[y][x], V[y][x])
        outs.append([[A[y][x] >> 8 for x in range(w)] for y in range(h)])
    return outs, A


def frame_bytes(w, h, chroma):
    hs, vs = SHIFTS[chroma]
    return w * h + 2 * ((w + hs) >> hs) * ((h + vs) >> vs)


def make_frames(kind: str, w: int, h: int, chroma: str, n: int = NFRAMES, seed: int = 1) -> np.ndarray:
    """n frames: "noise" seeded low-contrast noise 100 +- 12 (so that the tables act), "full" full-range
    noise, "flat" one value a plane and frame."""
    fb = frame_bytes(w, h, chroma)
    rng = np.random.default_rng(seed * 1000003 + w * 131 + h * 7 + len(kind))
    if kind == "noise":
        return rng.integers(88, 113, (n, fb), dtype=np.uint8)
    if kind == "full":
        return rng.integers(0, 256, (n, fb), dtype=np.uint8)
    if kind == "flat":
        return np.repeat(rng.integers(0, 256, (n, 1), dtype=np.uint8), fb, axis=1)
    raise ValueError(kind)
