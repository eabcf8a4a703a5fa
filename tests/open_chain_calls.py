"""One chain, given as keywords, handed to mjg_open_chain or to one of the entry points from before it
(tests/test_open_chain.py, tests/test_gpu_open_chain.py).  The keywords are mjg_chain's: src_chroma_format,
deint, orient, cmat (six ints), lut_in / lut_out ((3, 256) uint8), crop and pad (x, y, w, h; absent: has_crop /
has_pad 0), unsharp (six ints)."""
import ctypes as C

from ffmpeg_distributed_amd import _lib

CMAT = (6657, 12850, 64871, -7252, -4748, 64448)   # profile.colormatrix_coefs("bt709", "bt601")
UNSHARP = (5, 5, 65536, 5, 5, 32768)
# 70x38 4:2:0 tv -> yadif -> transpose=1 (38x70) -> colormatrix -> crop -> 24x40 -> unsharp -> pad
BASE = dict(src_chroma_format=0, deint=1, orient=3, cmat=CMAT, crop=(2, 4, 32, 60), unsharp=UNSHARP, pad=(4, 2, 32, 48))
SRC_W, SRC_H = 70, 38


def config(dst=(24, 40)):
    return _lib.MjgConfig(SRC_W, SRC_H, dst[0], dst[1], 0, 5, 1, 1, 3, 0, _lib.CHROMA_FORMATS["420"])


def _lut(t):
    return None if t is None else _lib.MjgLut.from_buffer_copy(t.tobytes())


def make_chain(src_chroma_format=0, deint=0, orient=0, cmat=None, lut_in=None, crop=None, lut_out=None, unsharp=None,
               pad=None):
    """A MjgChain; the structs behind its pointers live as long as it does."""
    ch = _lib.MjgChain(src_chroma_format=src_chroma_format, deint=deint, orient=orient)
    if cmat is not None:
        ch.cmat = C.pointer(_lib.MjgCmatrix(*cmat))
    if lut_in is not None:
        ch.lut_in = C.pointer(_lut(lut_in))
    if crop is not None:
        ch.has_crop, ch.crop_x, ch.crop_y, ch.crop_w, ch.crop_h = (1,) + tuple(crop)
    if lut_out is not None:
        ch.lut_out = C.pointer(_lut(lut_out))
    if unsharp is not None:
        ch.unsharp = C.pointer(_lib.MjgUnsharp(*unsharp))
    if pad is not None:
        ch.has_pad, ch.pad_x, ch.pad_y, ch.pad_w, ch.pad_h = (1,) + tuple(pad)
    return ch


def open_chain(device, cfg=None, **fields):
    """(rc, message, handle) of mjg_open_chain; the caller closes a handle that is not None."""
    L = _lib.load()
    cfg, ch, hnd = cfg or config(), make_chain(**fields), C.c_void_p()
    rc = L.mjg_open_chain(device, C.byref(cfg), C.byref(ch), C.byref(hnd))
    return rc, L.mjg_last_error().decode(), hnd.value


# the arguments of each entry point between cfg and out, in its own order
WRAPPER_ARGS = {
    "mjg_open_src": ("src_chroma_format",),
    "mjg_open_crop": ("src_chroma_format", "crop"),
    "mjg_open_pad": ("src_chroma_format", "crop", "pad"),
    "mjg_open_orient": ("src_chroma_format", "orient", "crop", "pad"),
    "mjg_open_deint": ("src_chroma_format", "deint", "orient", "crop", "pad"),
    "mjg_open_sharp": ("src_chroma_format", "deint", "orient", "crop", "unsharp", "pad"),
    "mjg_open_lut": ("src_chroma_format", "deint", "orient", "crop", "lut_in", "lut_out", "unsharp", "pad"),
    "mjg_open_cmat": ("src_chroma_format", "deint", "orient", "crop", "cmat", "lut_in", "lut_out", "unsharp", "pad"),
}


def open_wrapper(name, device, cfg=None, **fields):
    """(rc, message, handle) of the entry point `name` for the same keywords, which must be ones it has; a
    rectangle it has is always given."""
    L = _lib.load()
    assert set(fields) <= set(WRAPPER_ARGS[name]), (name, fields)
    cfg, hnd, args, keep = cfg or config(), C.c_void_p(), [], []
    for key in WRAPPER_ARGS[name]:
        v = fields.get(key)
        if key in ("crop", "pad"):
            args += list(v)
        elif key in ("cmat", "unsharp", "lut_in", "lut_out"):
            if v is not None:
                keep.append({"cmat": _lib.MjgCmatrix, "unsharp": _lib.MjgUnsharp}[key](*v) if key in ("cmat", "unsharp")
                            else _lut(v))
            args.append(None if v is None else C.byref(keep[-1]))
        else:
            args.append(v or 0)
    rc = getattr(L, name)(device, C.byref(cfg), *args, C.byref(hnd))
    return rc, L.mjg_last_error().decode(), hnd.value


def close(hnd):
    if hnd:
        _lib.load().mjg_close(C.c_void_p(hnd))
