"""mjg_open_chain and the entry points from before it, without a GPU: check_config runs before the
first HIP call, so a refusal is MJG_E_INVALID with its message here as on a GPU machine, and a valid
chain gets past it (MJG_E_HIP here, a context there, which is closed).

The base chain (open_chain_calls.BASE) is 70x38 4:2:0 tv -> yadif -> transpose=1 (38x70) -> colormatrix ->
crop 32x60 at (2,4) -> 24x40 -> unsharp -> pad 32x48 with the picture at (4,2).  Every refusal is asked for
through mjg_open_chain, and again through each older entry point with the argument groups that one
carries, where the message must be the one mjg_open_chain gives for the equal chain.  In those calls the
scalar arguments differ pairwise (the device among them: no refusal gets as far as the device), and every
one of them shows in an asserted message, so two arguments swapped on their way into the chain fail."""
import ctypes as C
import os
import re

import pytest

import open_chain_calls as oc
from open_chain_calls import BASE, CMAT, UNSHARP
from ffmpeg_distributed_amd import _lib
from ffmpeg_distributed_amd.encoder import MjpegEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = 11   # the refusals come before any HIP call; a valid chain is opened on device 0


def _passes_validation(rc, msg, hnd):
    oc.close(hnd)
    assert rc in (_lib.MJG_OK, _lib.MJG_E_HIP), (rc, msg)


def _refused(rc, msg, hnd, message):
    oc.close(hnd)
    assert rc == _lib.MJG_E_INVALID and msg.startswith(message) and not hnd, (rc, msg)
    return msg


# ---------------------------------------------------------------------- mjg_open_chain
def test_the_base_chain_passes_validation():
    _passes_validation(*oc.open_chain(0, **BASE))


REFUSALS = [
    (dict(crop=(3, 4, 32, 60)), "crop 32x60 at (3,4): the position is not a multiple"),
    (dict(crop=(2, 4, 32, 68)), "crop 32x68 at (2,4) is outside the 38x70 frame (the oriented one)"),
    (dict(pad=(3, 2, 32, 48)), "pad 32x48 with the picture at (3,2): not multiples"),
    (dict(deint=8), "deint 8:"),
    (dict(orient=9), "orient 9 not in 0..7"),
    (dict(unsharp=(4, 5, 65536, 5, 5, 32768)), "unsharp lx 4: size is even"),
    (dict(cmat=(300000,) + CMAT[1:]), "cmatrix yu 300000:"),
    (dict(src_chroma_format=7), "src_chroma_format 7"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=["crop_x", "crop_h", "pad_x", "deint", "orient", "unsharp_lx",
                                                          "cmat_yu", "src_chroma_format"])
def test_open_chain_refuses_one_changed_field_with_the_message_of_its_check(change, message):
    _refused(*oc.open_chain(DEVICE, **dict(BASE, **change)), message)


def test_rectangles_that_are_switched_off_are_not_read():
    """has_crop 0 / has_pad 0 with garbage in the four values: the whole oriented frame, no pad."""
    L = _lib.load()
    for off in ("crop", "pad"):
        cfg, hnd = oc.config(), C.c_void_p()
        ch = oc.make_chain(**BASE)
        if off == "crop":
            ch.has_crop, ch.crop_x, ch.crop_y, ch.crop_w, ch.crop_h = 0, -7, 1 << 30, 0, -1
        else:
            ch.has_pad, ch.pad_x, ch.pad_y, ch.pad_w, ch.pad_h = 0, -7, 1 << 30, 0, -1
        rc = L.mjg_open_chain(0, C.byref(cfg), C.byref(ch), C.byref(hnd))
        _passes_validation(rc, (off, L.mjg_last_error().decode()), hnd.value)
    # the same garbage switched on is refused, so the cases above did get as far as those checks
    _refused(*oc.open_chain(DEVICE, **dict(BASE, crop=(-7, 1 << 30, 0, -1))),
             "crop 0x-1 at (-7,1073741824): the size is not positive")
    _refused(*oc.open_chain(DEVICE, **dict(BASE, pad=(-7, 1 << 30, 0, -1))),
             "pad 0x-1 with the picture at (-7,1073741824): the size is not positive")


def test_a_null_chain_is_a_null_argument():
    L = _lib.load()
    cfg, hnd = oc.config(), C.c_void_p()
    assert L.mjg_open_chain(0, C.byref(cfg), None, C.byref(hnd)) == _lib.MJG_E_INVALID
    assert L.mjg_last_error() == b"null argument" and not hnd.value


# ---------------------------------------------------------------------- the older entry points
# Pairwise different scalars: device 11, format 0, deint 1, orient 3, crop 2 4 32 60, pad 6 10 36 52; each case
# brings one more value in (5, 7, 8 or 9).  Without an orientation the frame is 70x38 and the crop 32x30.
ORIENTED = dict(src_chroma_format=0, orient=3, crop=(2, 4, 32, 60), pad=(6, 10, 36, 52))
FLAT = dict(src_chroma_format=0, crop=(2, 4, 32, 30))
BAD_FORMAT = (dict(src_chroma_format=7), "src_chroma_format 7")
BAD_ORIENT = (dict(orient=9), "orient 9 not in 0..7")
BAD_DEINT = (dict(deint=8), "deint 8:")
BAD_CROP_O = (dict(crop=(5, 4, 32, 60)), "crop 32x60 at (5,4): the position is not a multiple")
BAD_CROP_F = (dict(crop=(3, 4, 32, 30)), "crop 32x30 at (3,4): the position is not a multiple")
BAD_PAD = (dict(pad=(7, 10, 36, 52)), "pad 36x52 with the picture at (7,10): not multiples")
BAD_SHARP = (dict(unsharp=(4, 5, 65536, 5, 5, 32768)), "unsharp lx 4: size is even")
BAD_CMAT = (dict(cmat=(300000,) + CMAT[1:]), "cmatrix yu 300000:")
WRAPPERS = {
    "mjg_open_src": (dict(src_chroma_format=0), [BAD_FORMAT]),
    "mjg_open_crop": (FLAT, [BAD_FORMAT, BAD_CROP_F]),
    "mjg_open_pad": (dict(FLAT, pad=(6, 10, 36, 52)), [BAD_FORMAT, BAD_CROP_F, BAD_PAD]),
    "mjg_open_orient": (ORIENTED, [BAD_FORMAT, BAD_ORIENT, BAD_CROP_O, BAD_PAD]),
    "mjg_open_deint": (dict(ORIENTED, deint=1), [BAD_FORMAT, BAD_DEINT, BAD_ORIENT, BAD_CROP_O, BAD_PAD]),
    "mjg_open_sharp": (dict(ORIENTED, deint=1, unsharp=UNSHARP),
                       [BAD_FORMAT, BAD_DEINT, BAD_ORIENT, BAD_CROP_O, BAD_SHARP, BAD_PAD]),
    "mjg_open_lut": (dict(ORIENTED, deint=1, unsharp=UNSHARP),
                     [BAD_FORMAT, BAD_DEINT, BAD_ORIENT, BAD_CROP_O, BAD_SHARP, BAD_PAD]),
    "mjg_open_cmat": (dict(ORIENTED, deint=1, unsharp=UNSHARP, cmat=CMAT),
                      [BAD_FORMAT, BAD_DEINT, BAD_ORIENT, BAD_CMAT, BAD_CROP_O, BAD_SHARP, BAD_PAD]),
}


def test_the_scalars_of_a_wrapper_call_differ_pairwise_and_each_is_in_a_message():
    for name, (good, cases) in WRAPPERS.items():
        shown = set()
        for change, _ in cases:
            f = dict(good, **change)
            vals = [DEVICE] + [f[k] for k in oc.WRAPPER_ARGS[name] if isinstance(f.get(k), int)]
            vals += list(f.get("crop", ())) + list(f.get("pad", ()))
            assert len(set(vals)) == len(vals), (name, change, vals)
            shown |= set(change)
        scalars = {k for k in oc.WRAPPER_ARGS[name] if k not in ("lut_in", "lut_out")}
        assert shown == scalars, (name, scalars - shown)


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_a_wrapper_refuses_what_the_equal_chain_refuses_with_the_same_message(name):
    good, cases = WRAPPERS[name]
    _passes_validation(*oc.open_wrapper(name, 0, **good))     # the arguments the cases start from are valid
    for change, message in cases:
        fields = dict(good, **change)
        msg = _refused(*oc.open_wrapper(name, DEVICE, **fields), message)
        assert msg == _refused(*oc.open_chain(DEVICE, **fields), message), change


# ---------------------------------------------------------------------- the interface
def test_header_declares_the_struct_and_the_function_and_the_binding_mirrors_them():
    with open(os.path.join(ROOT, "include", "mjgpu.h")) as f:
        hdr = f.read()
    m = re.search(r"typedef\s+struct\s+mjg_chain\s*\{(.*?)\}\s*mjg_chain\s*;", hdr, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names, ctypes_of = [], {"int32_t": C.c_int32, "const mjg_cmatrix": C.POINTER(_lib.MjgCmatrix),
                            "const mjg_lut": C.POINTER(_lib.MjgLut), "const mjg_unsharp": C.POINTER(_lib.MjgUnsharp)}
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        typ, rest = re.match(r"((?:const\s+)?\w+)\s+(.*)", decl, re.S).groups()
        names += [(n.strip().lstrip("*").strip(), ctypes_of[typ]) for n in rest.split(",")]
    assert names == [(n, t) for n, t in _lib.MjgChain._fields_]
    assert [n for n, _ in names] == ["src_chroma_format", "deint", "orient", "cmat", "lut_in", "has_crop", "crop_x",
                                     "crop_y", "crop_w", "crop_h", "lut_out", "unsharp", "has_pad", "pad_x", "pad_y",
                                     "pad_w", "pad_h"]
    assert re.search(r"\bint\s+mjg_open_chain\s*\(\s*int\s+device\s*,\s*const\s+mjg_config\s*\*\s*cfg\s*,\s*"
                     r"const\s+mjg_chain\s*\*\s*chain\s*,\s*mjg_ctx\s*\*\*\s*out\s*\)\s*;", hdr)
    L = _lib.load()
    assert "mjg_open_chain" in _lib.EXPORTS and hasattr(L, "mjg_open_chain")
    assert L.mjg_version() == 105


# ---------------------------------------------------------------------- MjpegEncoder on a library without the symbol
class _OldLibrary:
    """What MjpegEncoder.__init__ touches of a library from before mjg_open_chain."""

    def __init__(self):
        self.calls = []

    def mjg_open(self, device, cfg, hnd):
        self.calls.append(("mjg_open", device))
        return 0

    def mjg_open_src(self, device, cfg, src_chroma_format, hnd):
        self.calls.append(("mjg_open_src", device, src_chroma_format))
        return 0

    def mjg_open_crop(self, *args):
        self.calls.append(("mjg_open_crop",))
        return 0

    def mjg_frame_bytes(self, hnd):
        return 70 * 38 * 3 // 2

    def mjg_close(self, hnd):
        pass


def test_an_encoder_with_nothing_in_its_chain_opens_without_mjg_open_chain(monkeypatch):
    old = _OldLibrary()
    monkeypatch.setattr(_lib, "load", lambda: old)
    MjpegEncoder(0, 70, 38)
    assert old.calls == [("mjg_open", 0)]
    MjpegEncoder(0, 70, 38, chroma="420", src_chroma="444")
    assert old.calls[1:] == [("mjg_open_src", 0, _lib.CHROMA_FORMATS["444"])]
    with pytest.raises(_lib.MjgError, match="library lacks mjg_open_chain") as e:
        MjpegEncoder(0, 70, 38, crop=(2, 4, 32, 30))
    assert e.value.code == _lib.MJG_E_STATE and len(old.calls) == 2
