"""mjg_open_chain on the GPU against the entry points from before it, and the six frame readbacks'
refusals.  Three frames of 70x38; the base chain (open_chain_calls.BASE, here with two different
permutation tables as lut_in and lut_out) has every stage.  A context opened through an older entry
point and one opened through mjg_open_chain with the equal fields must hold the same state, give the same
header and encode one host submit to the same bytes: both run the same code behind check_config, so a
difference is a field that went astray on its way into the chain."""
import ctypes as C

import numpy as np
import pytest

import eq_ref
import open_chain_calls as oc
from open_chain_calls import BASE, UNSHARP
from ffmpeg_distributed_amd import _lib
from ffmpeg_distributed_amd.encoder import i420_frame_bytes

pytestmark = pytest.mark.gpu

NF = 3
T_IN, T_OUT = eq_ref.perm_tables(101), eq_ref.perm_tables(202)
FULL = dict(BASE, lut_in=T_IN, lut_out=T_OUT)
SRC_BYTES = i420_frame_bytes(oc.SRC_W, oc.SRC_H, "420")   # 3990
ENC_BYTES = i420_frame_bytes(32, 48, "420")                # the canvas of BASE's pad: 2304
_SRC = {}


def _frames(chroma="420"):
    """NF frames of seeded noise per format, made once and left unchanged."""
    if chroma not in _SRC:
        rng = np.random.default_rng(int(chroma))
        f = rng.integers(0, 256, (NF, i420_frame_bytes(oc.SRC_W, oc.SRC_H, chroma)), dtype=np.uint8)
        f.setflags(write=False)
        _SRC[chroma] = f
    return _SRC[chroma]


def _opened(rc, msg, hnd):
    assert rc == _lib.MJG_OK and hnd, (rc, msg)
    return hnd


def _header(hnd):
    L, n = _lib.load(), C.c_size_t()
    _lib.check(L.mjg_header(hnd, None, 0, C.byref(n)))
    buf = (C.c_uint8 * n.value)()
    _lib.check(L.mjg_header(hnd, buf, n.value, C.byref(n)))
    return bytes(buf)


def _encode(hnd, frames):
    """One host submit of all the frames: (the frame sizes, the packed bytes)."""
    L = _lib.load()
    assert frames.shape[1] == L.mjg_frame_bytes(hnd)
    _lib.check(L.mjg_submit(hnd, frames.ctypes.data, len(frames), 0))
    sizes, total = (C.c_uint64 * len(frames))(), C.c_uint64()
    _lib.check(L.mjg_sync(hnd, sizes, C.byref(total)))
    out = np.zeros(total.value, np.uint8)
    _lib.check(L.mjg_fetch(hnd, out.ctypes.data, out.size))
    assert sum(sizes) == total.value and min(sizes) > 0
    return list(sizes), out.tobytes()


def _state(hnd):
    """What the host-state hooks tell of the context."""
    L = _lib.load()
    us, cm, luts = _lib.MjgUnsharp(), _lib.MjgCmatrix(), [_lib.MjgLut(), _lib.MjgLut()]
    return dict(orient=L.mjg_debug_orient(hnd), deint=L.mjg_debug_deint_flags(hnd),
                unsharp=(L.mjg_debug_unsharp(hnd, C.byref(us)), bytes(us)),
                lut_in=(L.mjg_debug_lut(hnd, 0, C.byref(luts[0])), bytes(luts[0])),
                lut_out=(L.mjg_debug_lut(hnd, 1, C.byref(luts[1])), bytes(luts[1])),
                cmat=(L.mjg_debug_cmat(hnd, C.byref(cm)), bytes(cm)), frame_bytes=L.mjg_frame_bytes(hnd))


def test_the_widest_entry_point_and_the_chain_open_the_same_context():
    a = b = None
    try:
        a = _opened(*oc.open_wrapper("mjg_open_cmat", 0, **FULL))
        b = _opened(*oc.open_chain(0, **FULL))
        sa, sb = _state(a), _state(b)
        assert sa == sb
        assert sb["orient"] == 3 and sb["deint"] == 1 and sb["frame_bytes"] == SRC_BYTES
        assert sb["unsharp"] == (1, bytes(_lib.MjgUnsharp(*UNSHARP))) and sb["cmat"] == (1, bytes(_lib.MjgCmatrix(*oc.CMAT)))
        assert sb["lut_in"] == (1, T_IN.tobytes()) and sb["lut_out"] == (1, T_OUT.tobytes())
        assert _header(a) == _header(b)
        assert _encode(a, _frames()) == _encode(b, _frames())
    finally:
        oc.close(a)
        oc.close(b)


ORIENTED = dict(src_chroma_format=0, orient=3, crop=(2, 4, 32, 60), pad=(6, 10, 36, 52))
NARROWER = {
    "mjg_open_src": dict(src_chroma_format=_lib.CHROMA_FORMATS["444"]),
    "mjg_open_crop": dict(src_chroma_format=0, crop=(2, 4, 32, 30)),
    "mjg_open_pad": dict(src_chroma_format=0, crop=(2, 4, 32, 30), pad=(6, 10, 36, 52)),
    "mjg_open_orient": ORIENTED,
    "mjg_open_deint": dict(ORIENTED, deint=5),
    "mjg_open_sharp": dict(ORIENTED, deint=1, unsharp=UNSHARP),
    "mjg_open_lut": dict(ORIENTED, deint=1, unsharp=UNSHARP, lut_in=T_IN, lut_out=T_OUT),
}


@pytest.mark.parametrize("name", list(NARROWER))
def test_a_narrower_entry_point_and_the_chain_with_its_fields_encode_the_same_bytes(name):
    fields = NARROWER[name]
    frames = _frames("444" if fields["src_chroma_format"] == 2 else "420")
    a = b = None
    try:
        a = _opened(*oc.open_wrapper(name, 0, **fields))
        b = _opened(*oc.open_chain(0, **fields))
        assert _state(a) == _state(b)
        assert _header(a) == _header(b)
        assert _encode(a, frames) == _encode(b, frames)
    finally:
        oc.close(a)
        oc.close(b)


# (the hook, its refusal on a context without the stage, the bytes of a frame of it)
READBACKS = [
    ("mjg_debug_planes", "context has no sws stage (same size, same chroma format)", ENC_BYTES),
    ("mjg_debug_presharp", "context has no sharpen (no unsharp, or both amounts 0)", ENC_BYTES),
    ("mjg_debug_lut_in", "context has no table in front of the sws stage (none, or identity tables)", SRC_BYTES),
    ("mjg_debug_cmat_out", "context has no colour matrix (none, or the identity)", SRC_BYTES),
    ("mjg_debug_oriented", "context has no orientation (orient 0)", SRC_BYTES),
    ("mjg_debug_deint", "context has no deinterlacer (deint 0)", SRC_BYTES),
]


@pytest.mark.parametrize("hook,no_stage,nbytes", READBACKS, ids=[r[0] for r in READBACKS])
def test_a_frame_readback_refuses_as_before_and_reads_a_whole_frame(hook, no_stage, nbytes):
    L = _lib.load()
    read = getattr(L, hook)
    out = np.zeros(nbytes, np.uint8)
    ptr = out.ctypes.data_as(C.POINTER(C.c_uint8))

    def call(hnd, frame, cap):
        return read(hnd, frame, ptr, cap), L.mjg_last_error().decode()

    plain = full = None
    try:
        cfg, h = oc.config(dst=(oc.SRC_W, oc.SRC_H)), C.c_void_p()
        _lib.check(L.mjg_open(0, C.byref(cfg), C.byref(h)))
        plain = h.value
        assert call(plain, 0, nbytes) == (_lib.MJG_E_STATE, no_stage)
        assert read(None, 0, ptr, nbytes) == _lib.MJG_E_INVALID and read(plain, 0, None, nbytes) == _lib.MJG_E_INVALID
        full = _opened(*oc.open_chain(0, **FULL))
        assert call(full, 0, nbytes) == (_lib.MJG_E_STATE, "sync every queued submit first")
        _encode(full, _frames())
        assert call(full, -1, nbytes) == (_lib.MJG_E_INVALID, "frame -1")
        assert call(full, NF, nbytes) == (_lib.MJG_E_INVALID, f"frame {NF}")
        assert call(full, 0, nbytes - 1) == (_lib.MJG_E_CAPACITY, f"need {nbytes} bytes")
        assert not out.any()
        assert call(full, NF - 1, nbytes)[0] == _lib.MJG_OK
        assert out.any()
    finally:
        oc.close(plain)
        oc.close(full)
