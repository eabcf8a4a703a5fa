"""Reference for `-vf eq` on 8-bit planar frames: the three byte tables, written
twice (an index loop in Python ints and floats, and a numpy form), and the composed reference of a
frame that went through them.  Independent of ffmpeg_distributed_amd.profile.eq_tables, which the
tests compare with it.  The formula restates vf_eq.c's 8-bit path; no FFmpeg build has been compared
with it.

Every option value is rounded to IEEE single first (the filter clips its options with a float
function).  Per plane (C, B, G, W): Y (contrast, brightness, gamma * gamma_g, gamma_weight), U
(saturation, 0, sqrt(gamma_b / gamma_g), gamma_weight), V (saturation, 0, sqrt(gamma_r / gamma_g),
gamma_weight), in double."""
import math
import zlib

import numpy as np

NAMES = ("contrast", "brightness", "saturation", "gamma", "gamma_r", "gamma_g", "gamma_b", "gamma_weight")
DEFAULT = dict(contrast=1.0, brightness=0.0, saturation=1.0, gamma=1.0, gamma_r=1.0, gamma_g=1.0, gamma_b=1.0,
               gamma_weight=1.0)
ANCHOR_AT = (0, 16, 128, 235, 255)


def plane_params(spec, single=True):
    """[(C, B, G, W)] for Y, U, V.  single=False leaves the float step out (the double-only formula)."""
    o = {k: float(spec.get(k, DEFAULT[k])) for k in NAMES}
    if single:
        o = {k: float(np.float32(v)) for k, v in o.items()}
    w = o["gamma_weight"]
    return [(o["contrast"], o["brightness"], o["gamma"] * o["gamma_g"], w),
            (o["saturation"], 0.0, math.sqrt(o["gamma_b"] / o["gamma_g"]), w),
            (o["saturation"], 0.0, math.sqrt(o["gamma_r"] / o["gamma_g"]), w)]


def form(C, B, G):
    if C == 1.0 and B == 0.0 and G == 1.0:
        return "id"
    return "linear" if G == 1.0 and math.fabs(C) < 7.9 else "table"


def cdiv(a, b):
    """C integer division (truncates toward zero; Python's // floors)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def linear_ints(C, B):
    ci = int(C * 256 * 16)                          # (int): truncation toward zero, as Python's int()
    bi = cdiv(int(100.0 * B + 100.0) * 511, 200) - 128 - cdiv(ci, 32)
    return ci, bi


def table_loop(C, B, G, W):
    """One plane's table, an index loop in Python ints and floats."""
    f = form(C, B, G)
    out = []
    for v in range(256):
        if f == "id":
            out.append(v)
        elif f == "linear":
            ci, bi = linear_ints(C, B)
            pel = ((v * ci) >> 12) + bi             # Python's >> on a negative int is arithmetic
            out.append(0 if pel < 0 else 255 if pel > 255 else pel)
        else:
            x = v / 255.0
            x = C * (x - 0.5) + 0.5 + B
            if x <= 0.0:
                out.append(0)
            else:
                x = x * (1.0 - W) + math.pow(x, 1.0 / G) * W
                out.append(255 if x >= 1.0 else int(256.0 * x))
    return out


def table_numpy(C, B, G, W):
    """The same table in numpy (float64 / int64; pow through math.pow, libm's, element by element)."""
    v = np.arange(256, dtype=np.int64)
    f = form(C, B, G)
    if f == "id":
        return v.astype(np.uint8)
    if f == "linear":
        ci, bi = linear_ints(C, B)
        return np.clip(((v * ci) >> 12) + bi, 0, 255).astype(np.uint8)
    x = C * (v.astype(np.float64) / 255.0 - 0.5) + 0.5 + B
    pos = x > 0.0
    p = np.array([math.pow(t, 1.0 / G) if t > 0.0 else 0.0 for t in x.tolist()], np.float64)
    y = x * (1.0 - W) + p * W
    out = np.where(y >= 1.0, 255, np.trunc(256.0 * np.where(y >= 1.0, 0.0, y))).astype(np.int64)
    return np.where(pos, out, 0).astype(np.uint8)


def tables(spec, how="loop", single=True):
    """(3, 256) uint8, rows Y, U, V."""
    fn = table_loop if how == "loop" else table_numpy
    return np.array([np.asarray(fn(*p), np.uint8) for p in plane_params(spec, single)], np.uint8)


def crc(table) -> int:
    return zlib.crc32(bytes(bytearray(int(b) for b in table)))


def plane_sizes(w, h, chroma):
    hs, vs = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[str(chroma)]
    cw, ch = (w + hs) >> hs, (h + vs) >> vs
    return w * h, cw * ch


def map_frames(frames, w, h, chroma, tabs):
    """Packed planar frames (n, bytes) of w x h in `chroma` through the three tables."""
    frames = np.asarray(frames, np.uint8)
    tabs = np.asarray(tabs, np.uint8)
    ny, nc = plane_sizes(w, h, chroma)
    assert frames.shape[-1] == ny + 2 * nc
    out = np.empty_like(frames)
    out[..., :ny] = tabs[0][frames[..., :ny]]
    out[..., ny:ny + nc] = tabs[1][frames[..., ny:ny + nc]]
    out[..., ny + nc:] = tabs[2][frames[..., ny + nc:]]
    return out


def map_picture(frames, cw, ch, chroma, px, py, w, h, tabs):
    """The w x h picture at (px, py) of packed planar cw x ch canvases through the tables; every other
    byte (a pad's border) stays."""
    frames = np.asarray(frames, np.uint8)
    tabs = np.asarray(tabs, np.uint8)
    hs, vs = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[str(chroma)]
    out = frames.copy().reshape(-1, frames.shape[-1])
    at = 0
    for p in range(3):
        W, H = (cw, ch) if p == 0 else ((cw + hs) >> hs, (ch + vs) >> vs)
        x, y = (px, py) if p == 0 else (px >> hs, py >> vs)
        pw, ph = (w, h) if p == 0 else ((w + hs) >> hs, (h + vs) >> vs)
        pl = out[:, at:at + W * H].reshape(-1, H, W)
        pl[:, y:y + ph, x:x + pw] = tabs[p][pl[:, y:y + ph, x:x + pw]]
        at += W * H
    return out.reshape(frames.shape)


def perm_tables(seed):
    """Three seeded random permutation tables, different for Y, U and V, with t[0] != 0 and
    t[128] != 128: any mis-indexed byte, a U table used for V and a map that spills all change bytes."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < 3:
        t = rng.permutation(256).astype(np.uint8)
        if t[0] != 0 and t[128] != 128 and not any((t == u).all() for u in out):
            out.append(t)
    return np.array(out, np.uint8)


IDENTITY = np.arange(256, dtype=np.uint8)
