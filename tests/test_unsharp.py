"""`-vf unsharp` without a GPU: the two forms of the reference (tests/unsharp_ref.py) agree, the test
inputs can tell the likely mistakes apart, the profile's grammar, the worker's routing and the
library's argument checks."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from unsharp_ref import DEFAULT, amount_i, unsharp_plane_loop, unsharp_plane_vec
from ffmpeg_distributed_amd import _lib, profile, worker
from ffmpeg_distributed_amd.container import StreamInfo

TAIL = " -c:v mjpeg -q:v 5 -dct int -huffman default -bitexact"

SHAPES = [(3, 3), (5, 4), (17, 9), (33, 17), (70, 37)]
SIZES = [(3, 3), (5, 5), (3, 7), (13, 13), (23, 3), (5, 21)]
AMOUNTS = [1.0, -0.5, 0.3, 5.0, -2.0]


def noise(w, h, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def ramp(w, h, seed=2):
    """A ramp with noise of 0..40 on it: sample minus blur then reaches +-10 and its multiples, the
    differences at which amounts 19660 and 19661 part (10 * 19660 = 3 * 65536 - 8)."""
    rng = np.random.default_rng(seed)
    return ((np.add.outer(3 * np.arange(h), 5 * np.arange(w)) + rng.integers(0, 41, (h, w))) % 256).astype(np.uint8)


# ------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("w,h", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("mx,my", SIZES, ids=lambda v: str(v))
def test_loop_form_equals_closed_form(w, h, mx, my):
    """The filter's running pair sums against the binomial closed form, planes narrower than the
    window included (3 x 3 with 23 taps)."""
    for k, a in enumerate(AMOUNTS):
        p = noise(w, h, 10 + k) if k % 2 == 0 else ramp(w, h, 10 + k)
        if k == 0:
            p[: (h + 1) // 2, : (w + 1) // 2] = 255     # the largest sums
        assert (unsharp_plane_loop(p, mx, my, amount_i(a)) == unsharp_plane_vec(p, mx, my, amount_i(a))).all(), a


def test_amount_zero_is_a_copy():
    p = noise(17, 9)
    assert (unsharp_plane_loop(p, 5, 5, 0) == p).all() and (unsharp_plane_vec(p, 23, 23, 0) == p).all()


def test_amount_is_truncated_not_rounded():
    assert amount_i(0.3) == 19660 and amount_i(-0.5) == -32768 and amount_i(1.0) == 65536
    assert amount_i(-0.3) == -19660        # towards zero, as a C cast
    assert round(0.3 * 65536.0) == 19661


@pytest.mark.parametrize("make", [noise, ramp], ids=["noise", "ramp"])
def test_the_inputs_tell_the_mistakes_apart(make):
    """On each test input the reference changes in at least one sample for every likely mistake."""
    for (w, h) in ((33, 17), (70, 37)):
        p = make(w, h)
        ref = unsharp_plane_vec(p, 5, 5, 65536)
        n_clip = (int((ref == 0).sum()), int((ref == 255).sum()))
        asym = unsharp_plane_vec(p, 3, 7, 65536)
        diffs = {
            "mx, my swapped": int((asym != unsharp_plane_vec(p, 7, 3, 65536)).sum()),
            "sign of the amount": int((ref != unsharp_plane_vec(p, 5, 5, -65536)).sum()),
            "edge reflected": int((ref != unsharp_plane_vec(p, 5, 5, 65536, reflect=True)).sum()),
            "half dropped": int((ref != unsharp_plane_vec(p, 5, 5, 65536, half_on=False)).sum()),
            "0.3 rounded": int((unsharp_plane_vec(p, 5, 5, 19660) != unsharp_plane_vec(p, 5, 5, 19661)).sum()),
        }
        print(f"{make.__name__} {w}x{h}: clipped at 0 / 255: {n_clip}, of {p.size}; differing samples: {diffs}")
        assert all(v > 0 for v in diffs.values()), diffs
        assert (unsharp_plane_loop(p, 5, 5, 65536, half_on=False) == unsharp_plane_vec(p, 5, 5, 65536, half_on=False)).all()


# ------------------------------------------------------------------------- the profile
ACCEPT = [
    ("unsharp", dict(unsharp=DEFAULT)),
    ("scale=1280:720,unsharp", dict(scale=(1280, 720), unsharp=DEFAULT)),
    ("scale=160:90,unsharp=3:3:0.8", dict(scale=(160, 90), unsharp=(3, 3, 0.8, 5, 5, 0.0))),
    ("unsharp=3:7:1.5:7:3:-0.5", dict(unsharp=(3, 7, 1.5, 7, 3, -0.5))),
    ("unsharp=lx=7:la=2", dict(unsharp=(7, 5, 2.0, 5, 5, 0.0))),
    ("unsharp=luma_msize_x=3:luma_msize_y=9:luma_amount=-1:chroma_msize_x=7:chroma_msize_y=11:chroma_amount=.5",
     dict(unsharp=(3, 9, -1.0, 7, 11, 0.5))),
    ("unsharp=5:5:1.0:cx=3:cy=3:ca=1e-1", dict(unsharp=(5, 5, 1.0, 3, 3, 0.1))),
    ("unsharp=13:13:5:13:13:-2", dict(unsharp=(13, 13, 5.0, 13, 13, -2.0))),
    ("unsharp=23:23:0:3:23:1", dict(unsharp=(23, 23, 0.0, 3, 23, 1.0))),        # an unfiltered plane may have any size
    ("unsharp=23:23:0.00001", dict(unsharp=(23, 23, 0.00001, 5, 5, 0.0))),     # (int)(a * 65536) is 0
    ("crop=64:32:2:2,unsharp", dict(crop={"w": 64, "h": 32, "x": 2, "y": 2}, unsharp=DEFAULT)),
    ("crop=64:32:2:2,scale=32:16,unsharp=7:7", dict(scale=(32, 16), unsharp=(7, 7, 1.0, 5, 5, 0.0))),
    ("scale=64:32,unsharp,pad=80:48:8:8", dict(scale=(64, 32), pad={"w": 80, "h": 48, "x": 8, "y": 8}, unsharp=DEFAULT)),
    ("unsharp,pad=80:48:8:8", dict(pad={"w": 80, "h": 48, "x": 8, "y": 8}, unsharp=DEFAULT)),
    ("crop=64:32,scale=32:16,unsharp,pad=40:20", dict(scale=(32, 16), unsharp=DEFAULT)),
    ("vflip,unsharp", dict(orient=4, unsharp=DEFAULT)),
    ("yadif,transpose=1,crop=62:126:2:2,scale=32:64,unsharp,pad=48:80:8:8",
     dict(orient=3, scale=(32, 64), deint={"mode": 0, "parity": -1}, unsharp=DEFAULT)),
    ("yadif,unsharp", dict(deint={"mode": 0, "parity": -1}, unsharp=DEFAULT)),
]


@pytest.mark.parametrize("vf,want", ACCEPT, ids=[a[0] for a in ACCEPT])
def test_parser_accepts(vf, want):
    prof, why = profile.try_parse("-vf " + vf + TAIL)
    assert prof is not None, why
    for k, v in want.items():
        assert getattr(prof, k) == v, (k, getattr(prof, k))
    assert isinstance(prof.unsharp[0], int) and isinstance(prof.unsharp[2], float)


REJECT = [
    ("unsharp=4:5", ["lx=4", "even"]),
    ("unsharp=5:6", ["ly=6", "even"]),
    ("unsharp=5:5:1:8:5", ["cx=8", "even"]),
    ("unsharp=25:5", ["lx=25", "3..23"]),
    ("unsharp=1:5", ["lx=1", "3..23"]),
    ("unsharp=5:5:1:5:-3", ["cy=-3", "3..23"]),
    ("unsharp=13:15", ["sx + sy = 13", "32-bit"]),
    ("unsharp=23:23", ["sx + sy = 22", "32-bit"]),
    ("unsharp=5:5:1:23:5:0.5", ["chroma 23x5", "sx + sy = 13", "32-bit"]),
    ("unsharp=5:5:5.5", ["la=5.5", "-2..5"]),
    ("unsharp=5:5:1:5:5:-2.5", ["ca=-2.5", "-2..5"]),
    ("unsharp=5:5:la=iw/100", ["la=iw/100", "expression"]),
    ("unsharp=lx=2+1", ["lx=2+1", "expression"]),
    ("unsharp=5.0:5", ["lx=5.0", "plain number"]),
    ("unsharp=ax=3", ["'ax'"]),
    ("unsharp=aa=1", ["'aa'"]),
    ("unsharp=alpha_msize_y=3", ["'alpha_msize_y'"]),
    ("unsharp=5:5:1:5:5:0:3", ["'3'", "alpha"]),
    ("unsharp=opencl=1", ["'opencl'"]),
    ("unsharp=", ["unsharp=", "without options"]),
    ("unsharp,unsharp", ["second unsharp"]),
    ("scale=64:32,unsharp,unsharp=3:3,pad=80:48", ["second unsharp"]),
    ("unsharp,scale=64:32", ["unsharp before scale"]),
    ("crop=64:32,unsharp,scale=32:16", ["unsharp before scale"]),
    ("unsharp,crop=64:32", ["unsharp before crop"]),
    ("scale=64:32,pad=80:48,unsharp", ["pad is not the last filter"]),
    ("unsharp,vflip", ["vflip after unsharp"]),
    ("unsharp,yadif", ["yadif after unsharp"]),
    ("unsharp,hue=s=0", ["unsharp before hue"]),
    ("scale=64:32,hue=s=0,unsharp", ["'scale=64:32,hue=s=0'", "only crop, scale or crop,scale"]),   # what is in front of it
    ("crop=8:8,scale=64:32,hue=s=0,unsharp", ["3 filters"]),
]


@pytest.mark.parametrize("vf,words", REJECT, ids=[r[0] for r in REJECT])
def test_parser_rejects_with_a_reason_that_names_the_cause(vf, words):
    prof, why = profile.try_parse("-vf " + vf + TAIL)
    assert prof is None
    for w in words:
        assert w in why, (w, why)


TODAY = [
    ("scale=1280:720", dict(scale=(1280, 720))),
    ("crop=64:32:2:2", dict(crop={"w": 64, "h": 32, "x": 2, "y": 2})),
    ("crop=64:32:2:2,scale=32:16:flags=bicubic", dict(scale=(32, 16))),
    ("scale=64:32,pad=80:48:8:8", dict(scale=(64, 32), pad={"w": 80, "h": 48, "x": 8, "y": 8})),
    ("pad=80:48", dict(pad={"w": 80, "h": 48, "x": None, "y": None})),
    ("vflip,transpose=1,crop=10:10,scale=8:8,pad=16:16", dict(orient=profile.compose_orient(["vflip", "transpose=1"]))),
    ("yadif=2:bff,scale=64:32", dict(deint={"mode": 2, "parity": 1}, scale=(64, 32))),
]
TODAY_REASONS = [
    ("a,b,c", "filter graph 'a,b,c': 3 filters (only crop, scale or crop,scale is GPU-accelerated)"),
    ("a,b,c,d", "filter graph 'a,b,c,d': 4 filters (only crop, scale or crop,scale is GPU-accelerated)"),
    ("crop=2:2,scale=4:4,hue,pad=8:8",
     "filter graph 'crop=2:2,scale=4:4,hue,pad=8:8': 4 filters (only crop, scale or crop,scale is GPU-accelerated)"),
    ("pad=8:8,scale=4:4", "filter graph 'pad=8:8,scale=4:4': pad is not the last filter (only [crop,][scale,]pad in this "
                          "order is GPU-accelerated)"),
    ("scale=4:4,crop=2:2", "filter graph 'scale=4:4,crop=2:2': scale before crop (only crop,scale in this order is "
                           "GPU-accelerated)"),
    ("hue=s=0", "filter graph 'hue=s=0' (only crop, scale or crop,scale is GPU-accelerated)"),
]


@pytest.mark.parametrize("vf,want", TODAY, ids=[a[0] for a in TODAY])
def test_graphs_without_unsharp_parse_as_before(vf, want):
    prof, why = profile.try_parse("-vf " + vf + TAIL)
    assert prof is not None, why
    assert prof.unsharp is None
    for k, v in want.items():
        assert getattr(prof, k) == v, (k, getattr(prof, k))


@pytest.mark.parametrize("vf,reason", TODAY_REASONS, ids=[a[0] for a in TODAY_REASONS])
def test_reasons_for_graphs_without_unsharp_stay_letter_for_letter(vf, reason):
    prof, why = profile.try_parse("-vf " + vf + TAIL)
    assert prof is None and why == reason


def test_no_vf_has_no_unsharp():
    prof, why = profile.try_parse(TAIL)
    assert prof is not None and prof.unsharp is None
    assert "unsharp" in {f.name for f in dataclasses.fields(profile.Profile)}


# ------------------------------------------------------------------------- the worker
def _prof(vf):
    prof, why = profile.try_parse("-vf " + vf + TAIL)
    assert prof is not None, why
    return prof


def test_unsharp_fallthrough_reason():
    f = worker.unsharp_fallthrough_reason
    msg = "unsharp without a scale on a tv-range / converted input: FFmpeg sharpens before its converter"
    with_scale, alone, none = _prof("scale=64:32,unsharp"), _prof("unsharp"), _prof("scale=64:32")
    cropped = _prof("crop=64:32,unsharp,pad=80:48")
    # behind a scale the scaler delivers the encoder's format: any source
    for full in (False, True):
        for src, dst in (("420", "420"), ("444", "420")):
            assert f(with_scale, full, src, dst) is None
            assert f(none, full, src, dst) is None
    # without one: only a full-range source in the encoded format
    assert f(alone, True, "420", "420") is None and f(cropped, True, "444", "444") is None
    assert f(alone, False, "420", "420") == msg
    assert f(alone, True, "444", "420") == msg
    assert f(cropped, False, "444", "444") == msg


def test_encoder_key_holds_the_six_values():
    info = StreamInfo(width=130, height=66, fps=25, sar=(1, 1), full_range=False, chroma="420")
    a, b, c = _prof("scale=70:38,unsharp"), _prof("scale=70:38,unsharp=5:5:0.3"), _prof("scale=70:38")

    def key(p):
        return worker.encoder_key(p, info, 70, 38, (1, 1), False, 8, unsharp=p.unsharp)

    assert key(a) != key(b) and key(a) != key(c) and key(b) != key(c)
    assert key(a) == key(_prof("scale=70:38,unsharp=5:5:1.0:5:5:0.0"))
    assert key(a)[-1] == (5, 5, 1.0, 5, 5, 0.0) and key(c)[-1] is None
    assert worker.encoder_key(c, info, 70, 38, (1, 1), False, 8) == key(c)       # the default


# ------------------------------------------------------------------------- the library
def _open_sharp(us, w=64, h=32):
    L = _lib.load()
    cfg = _lib.MjgConfig(w, h, w, h, 0, 5, 1, 1, 4, 0, _lib.CHROMA_FORMATS["420"])
    hnd = C.c_void_p()
    u = _lib.MjgUnsharp(*us)
    rc = L.mjg_open_sharp(0, C.byref(cfg), _lib.CHROMA_FORMATS["420"], 0, 0, 0, 0, w, h, C.byref(u), 0, 0, w, h,
                          C.byref(hnd))
    return rc, L.mjg_last_error().decode()


@pytest.mark.parametrize("us,words", [
    ((4, 5, 65536, 5, 5, 0), ["lx 4", "even"]),
    ((5, 5, 65536, 5, 6, 0), ["cy 6", "even"]),
    ((25, 5, 65536, 5, 5, 0), ["lx 25", "3..23"]),
    ((5, 1, 65536, 5, 5, 0), ["ly 1", "3..23"]),
    ((5, 5, 0, 24, 5, 0), ["cx 24", "3..23"]),
    ((13, 15, 65536, 5, 5, 0), ["luma 13x15", "sx + sy = 13", "32-bit sum"]),
    ((5, 5, 65536, 23, 5, 1), ["chroma 23x5", "sx + sy = 13", "32-bit sum"]),
    ((5, 5, 5 * 65536 + 1, 5, 5, 0), ["la 327681", "amount"]),
    ((5, 5, 65536, 5, 5, -2 * 65536 - 1), ["ca -131073", "amount"]),
], ids=lambda v: str(v))
def test_open_sharp_refuses_bad_arguments_before_any_hip_call(us, words):
    rc, msg = _open_sharp(us)
    assert rc == _lib.MJG_E_INVALID
    assert msg.startswith("unsharp"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_open_sharp_is_declared_and_bound():
    assert {"mjg_open_sharp", "mjg_debug_presharp", "mjg_debug_unsharp"} <= set(_lib.EXPORTS)
    L = _lib.load()
    assert L.mjg_version() == 105
    assert L.mjg_debug_unsharp(None, None) == _lib.MJG_E_INVALID
    assert L.mjg_debug_presharp(None, 0, None, 0) == _lib.MJG_E_INVALID
