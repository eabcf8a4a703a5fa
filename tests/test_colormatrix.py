"""`-vf colormatrix` without a GPU: the six coefficients (profile.colormatrix_coefs against
tests/colormatrix_ref.py and the anchors of DESIGN §4.16), both forms of the reference against the pixel
and CRC anchors, the parser (Profile.colormatrix and why every other form stays on the CPU), what the
worker makes of it, and the library's refusal of a coefficient that would overflow."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import colormatrix_ref as ref
from ffmpeg_distributed_amd import _lib, profile, worker
from ffmpeg_distributed_amd.container import StreamInfo

TAIL = " -c:v mjpeg -q:v 5 -dct int -huffman default -bitexact"

COEFS = [
    ("bt709", "bt601", (6657, 12850, 64871, -7252, -4748, 64448)),
    ("bt601", "bt709", (-7746, -13939, 66758, 7512, 4918, 67196)),
    ("bt2020", "bt709", (1189, -6235, 65806, 3360, -755, 65325)),
    ("fcc", "bt601", (532, 48, 65532, -27, -379, 65408)),
]
C_79 = COEFS[0][2]
C_67 = COEFS[1][2]


@pytest.mark.parametrize("src,dst,want", COEFS, ids=[f"{a}->{b}" for a, b, _ in COEFS])
def test_coefficients_from_the_reference_and_the_profile(src, dst, want):
    assert ref.coefs(src, dst) == want
    assert profile.colormatrix_coefs(src, dst) == want


def test_first_column_is_the_identity_for_all_25_pairs_and_the_profile_agrees():
    names = list(ref.LUMA)
    assert len(names) == 5 and set(names) == set(profile.COLORMATRIX_LUMA)
    for s in names:
        for d in names:
            m = ref.matrix(s, d)
            assert [r[0] for r in m] == [65536, 0, 0], (s, d, m)
            assert profile.colormatrix_coefs(s, d) == ref.coefs(s, d), (s, d)
            if s == d:
                assert ref.coefs(s, d) == ref.IDENTITY
            assert max(abs(v) for v in ref.coefs(s, d)) <= 262144
    for alias in ("bt470", "bt470bg", "smpte170m"):
        assert profile.colormatrix_coefs("bt709", alias) == C_79 and profile.colormatrix_coefs(alias, "bt709") == C_67


def test_no_entry_is_near_a_rounding_tie():
    """|frac(65536 n) - 0.5| >= 0.007 for every entry of the 20 pairs: the order of the double operations
    cannot change a coefficient."""
    for s in ref.LUMA:
        for d in ref.LUMA:
            if s != d:
                c = ref.yuv_matrix(d) @ np.linalg.inv(ref.yuv_matrix(s))
                fr = np.abs(c * 65536.0) % 1.0
                assert (np.abs(fr - 0.5) >= 0.007).all(), (s, d)


ANCHORS_79 = [((16, 128, 128), (16, 128, 128)), ((63, 102, 240), (82, 90, 240)), ((173, 42, 26), (144, 54, 34)),
              ((0, 0, 0), (0, 15, 11)), ((255, 255, 255), (255, 240, 244)), ((250, 16, 16), (217, 30, 26)),
              ((5, 240, 240), (38, 226, 230))]
ANCHORS_67 = [((0, 0, 0), (42, 0, 0)), ((250, 16, 16), (255, 1, 5)), ((5, 240, 240), (0, 255, 251)),
              ((173, 42, 26), (205, 29, 17))]


@pytest.mark.parametrize("c,anchors", [(C_79, ANCHORS_79), (C_67, ANCHORS_67)], ids=["bt709->bt601", "bt601->bt709"])
def test_pixel_anchors_from_both_forms(c, anchors):
    for src, want in anchors:
        assert ref.pixel(*src, c) == want, src
        one = np.array(src, np.uint8)                      # a 1 x 1 4:4:4 frame
        assert tuple(int(v) for v in ref.convert_frames(one, 1, 1, "444", c)) == want, src
        assert tuple(int(v) for v in ref.convert_frame_loop(one, 1, 1, "444", c)) == want, src


@pytest.mark.parametrize("c,crcs", [(C_79, (0x3b20c9e3, 0x5f59a7fd, 0x302886d8)), (C_67, (0x700fd411, 0x7cd2c754, 0x3735c7e3))],
                         ids=["bt709->bt601", "bt601->bt709"])
def test_crc_anchors_from_both_forms(c, crcs):
    assert tuple(ref.crc(t) for t in ref.uv_tables(c)) == crcs
    assert tuple(ref.crc(t) for t in ref.uv_tables_loop(c)) == crcs


def test_the_luma_identity():
    """(65536 a + b) >> 16 == a + (b >> 16): the loop form uses the left side, the numpy form and the kernel the right."""
    rng = np.random.default_rng(3)
    for a, b in zip(rng.integers(-300, 300, 2000).tolist(), rng.integers(-2 ** 27, 2 ** 27, 2000).tolist()):
        assert (65536 * a + b) >> 16 == a + (b >> 16)


@pytest.mark.parametrize("w,h,c", [(5, 3, "420"), (33, 17, "420"), (7, 4, "422"), (3, 3, "444"), (1, 1, "420"), (2, 1, "422")],
                         ids=lambda v: str(v))
def test_odd_cells_both_forms_agree(w, h, c):
    """With odd sizes the last chroma column or row covers one luma column or row."""
    for plane in range(3):
        f = ref.noise_frames(w, h, c, 2, plane)
        for coefs in (C_79, C_67, ref.MADE_UP):
            got = ref.convert_frames(f, w, h, c, coefs)
            for i in range(2):
                assert (got[i] == ref.convert_frame_loop(f[i], w, h, c, coefs)).all()
    # 5x3 4:2:0: luma (4, 2), the last column and row, reads chroma (2, 1), the last sample of a 3 x 2 plane
    f = np.full(15 + 2 * 6, 128, np.uint8)
    f[:15] = 100
    f[15 + 5] = 240
    out = ref.convert_frames(f, 5, 3, "420", C_79)
    changed = np.flatnonzero(out[:15] != ref.pixel(100, 128, 128, C_79)[0]).tolist()
    assert changed == [14] and out[14] == ref.pixel(100, 240, 128, C_79)[0]


def test_the_identity_changes_nothing_and_the_made_up_matrix_is_asymmetric():
    f = ref.noise_frames(33, 17, "420", 2, 1)
    assert (ref.convert_frames(f, 33, 17, "420", ref.IDENTITY) == f).all()
    assert len(set(ref.MADE_UP)) == 6 and max(abs(v) for v in ref.MADE_UP) <= 262144


# ------------------------------------------------------------------------- the parser
def _try(vf):
    return profile.try_parse("-vf " + vf + TAIL)


def _prof(vf):
    prof, why = _try(vf)
    assert prof is not None, why
    return prof


ACCEPTED = [
    ("colormatrix=bt709:bt601", ("bt709", "bt601")),
    ("colormatrix=src=bt709:dst=bt601", ("bt709", "bt601")),
    ("colormatrix=dst=bt601:src=bt709", ("bt709", "bt601")),
    ("colormatrix=bt709:dst=bt601", ("bt709", "bt601")),
    ("colormatrix=bt601:bt709", ("bt601", "bt709")),
    ("colormatrix=bt2020:smpte170m", ("bt2020", "bt601")),
    ("colormatrix=bt470bg:fcc", ("bt601", "fcc")),
    ("colormatrix=bt470:smpte240m", ("bt601", "smpte240m")),
    ("colormatrix=bt709:bt601,scale=1280:720", ("bt709", "bt601")),
    ("yadif,colormatrix=bt709:bt601", ("bt709", "bt601")),
    ("vflip,transpose=1,colormatrix=bt709:bt601,scale=64:32", ("bt709", "bt601")),
    ("colormatrix=bt709:bt601,crop=32:16:2:2,scale=64:32", ("bt709", "bt601")),
    ("crop=32:16:2:2,colormatrix=bt709:bt601,scale=64:32", ("bt709", "bt601")),
    ("colormatrix=bt709:bt601,eq=1.1,scale=64:32", ("bt709", "bt601")),
    ("colormatrix=bt709:bt601,scale=64:32,eq=1.1", ("bt709", "bt601")),
    ("colormatrix=bt709:bt601,unsharp,pad=80:48", ("bt709", "bt601")),
    ("crop=32:16,colormatrix=bt709:bt601,pad=80:48", ("bt709", "bt601")),
    ("yadif,colormatrix=bt709:bt601,eq=1.1,scale=70:38,pad=80:48", ("bt709", "bt601")),
]


@pytest.mark.parametrize("vf,pair", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_accepted(vf, pair):
    p = _prof(vf)
    assert p.colormatrix == pair
    rest = ",".join(f for f in vf.split(",") if not f.startswith("colormatrix"))
    if rest:                                               # everything else is what the graph without it gives
        assert dataclasses.replace(p, colormatrix=None) == _prof(rest)
    else:
        assert dataclasses.replace(p, colormatrix=None) == profile.try_parse(TAIL)[0]


def test_the_chain_graph_keeps_its_other_stages():
    p = _prof("yadif,colormatrix=bt709:bt601,eq=1.1,scale=70:38,pad=80:48")
    assert p.deint == {"mode": 0, "parity": -1} and p.eq["slot"] == "in" and p.eq["contrast"] == 1.1
    assert p.scale == (70, 38) and p.pad == {"w": 80, "h": 48, "x": None, "y": None}


REJECTED = [
    ("colormatrix=bt709:bt601,colormatrix=bt601:bt709", ["a second colormatrix"]),
    ("colormatrix=bt709:bt601,scale=64:32,colormatrix=bt601:bt709", ["a second colormatrix"]),
    ("colormatrix=bt709", ["colormatrix without a dst"]),
    ("colormatrix=src=bt709", ["colormatrix without a dst"]),
    ("colormatrix", ["colormatrix without a dst"]),
    ("colormatrix=dst=bt601", ["colormatrix without a src", "metadata"]),
    ("colormatrix=bt709:bt709", ["colormatrix src and dst are both bt709"]),
    ("colormatrix=bt601:smpte170m", ["colormatrix src and dst are both bt601"]),
    ("colormatrix=bt709:rec601", ["colormatrix dst=rec601"]),
    ("colormatrix=BT709:bt601", ["colormatrix src=BT709"]),
    ("colormatrix=src=bt709:dst=bt601:range=tv", ["colormatrix option 'range'"]),
    ("colormatrix=bt709:bt601:fcc", ["colormatrix option 'fcc'", "positional"]),
    ("eq=1.1,colormatrix=bt709:bt601", ["colormatrix behind the eq"]),
    ("eq=1.1,colormatrix=bt709:bt601,scale=64:32", ["colormatrix behind the eq"]),
    ("scale=64:32,colormatrix=bt709:bt601", ["colormatrix behind the scale"]),
    ("crop=32:16,scale=64:32,colormatrix=bt709:bt601", ["colormatrix behind the scale"]),
    ("unsharp,colormatrix=bt709:bt601", ["colormatrix behind the unsharp"]),
    ("pad=80:48,colormatrix=bt709:bt601", ["colormatrix behind the pad"]),
    ("colormatrix=bt709:bt601,yadif", ["colormatrix in front of yadif"]),
    ("colormatrix=bt709:bt601,vflip", ["colormatrix in front of vflip"]),
    ("vflip,colormatrix=bt709:bt601,transpose=1", ["colormatrix in front of transpose"]),
    ("colormatrix=bt709:bt601,crop=32:16,transpose=1", ["colormatrix in front of transpose"]),
]


@pytest.mark.parametrize("vf,parts", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_with_the_cause_in_the_reason(vf, parts):
    prof, why = _try(vf)
    assert prof is None
    for p in parts:
        assert p in why, why


# the reasons of graphs that do not name colormatrix, copied from tests/test_eq.py
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


@pytest.mark.parametrize("vf,reason", TODAY_REASONS, ids=[a[0] for a in TODAY_REASONS])
def test_reasons_for_graphs_without_colormatrix_stay_letter_for_letter(vf, reason):
    prof, why = _try(vf)
    assert prof is None and why == reason


def test_todays_reasons_are_the_copy_in_test_eq():
    import test_eq
    assert TODAY_REASONS == test_eq.TODAY_REASONS


def test_eq_reasons_stay_with_a_colormatrix_in_front():
    """The eq's own refusals are the ones it has without the colormatrix, letter for letter."""
    for vf in ("eq=1.2,eq=1.1", "scale=64:32,unsharp,eq=1.2", "eq=eval=frame"):
        assert _try("colormatrix=bt709:bt601," + vf)[1] == _try(vf)[1]


def test_graphs_without_colormatrix_have_none():
    for vf in ("scale=64:32", "crop=32:16,scale=64:32,unsharp,pad=80:48", "yadif,vflip", "eq=1.2,scale=64:32"):
        assert _prof(vf).colormatrix is None
    prof, why = profile.try_parse(TAIL)
    assert prof is not None and prof.colormatrix is None
    assert "colormatrix" in {f.name for f in dataclasses.fields(profile.Profile)}


# ------------------------------------------------------------------------- the worker
INFO = StreamInfo(width=130, height=66, fps=25, sar=(1, 1), full_range=False, chroma="420")


def test_cmat_fallthrough_reason():
    f = worker.cmat_fallthrough_reason
    p = _prof("colormatrix=bt709:bt601,scale=70:38")
    assert f(_prof("scale=70:38"), INFO) is None and f(p, INFO) is None
    full = dataclasses.replace(INFO, full_range=True)
    assert f(_prof("scale=70:38"), full) is None
    why = f(p, full)
    assert why.startswith("colormatrix on a full-range") and "yuv420p" in why
    deep = dataclasses.replace(INFO)
    deep.bits = 10
    assert f(p, deep) == "colormatrix on a 10-bit input: only the filter's 8-bit planar path is GPU-accelerated"


def test_encoder_key_differs_by_pair_and_is_unchanged_without_the_filter():
    a, b, none = (_prof(v + "scale=70:38") for v in ("colormatrix=bt709:bt601,", "colormatrix=bt601:bt709,", ""))

    def key(p):
        cm = None if p.colormatrix is None else profile.colormatrix_coefs(*p.colormatrix)
        return worker.encoder_key(p, INFO, 70, 38, (1, 1), False, 8, cmat=cm)

    assert len({key(a), key(b), key(none)}) == 3
    assert key(a) == key(_prof("colormatrix=src=bt709:dst=smpte170m,scale=70:38"))
    assert key(none) == worker.encoder_key(none, INFO, 70, 38, (1, 1), False, 8)
    assert key(a)[:len(key(none))] == key(none) and key(a)[-1] == ("cmat",) + C_79
    # the parent's key, element for element: nothing was inserted
    assert key(none)[-1] is None and key(none)[-2] == (None, None) and len(key(none)) == 19


# ------------------------------------------------------------------------- the library
def _open_cmat(cm, w=64, h=32):
    L = _lib.load()
    cfg = _lib.MjgConfig(w, h, w, h, 0, 5, 1, 1, 4, 0, _lib.CHROMA_FORMATS["420"])
    hnd = C.c_void_p()
    m = _lib.MjgCmatrix(*cm)
    rc = L.mjg_open_cmat(0, C.byref(cfg), _lib.CHROMA_FORMATS["420"], 0, 0, 0, 0, w, h, C.byref(m), None, None, None,
                         0, 0, w, h, C.byref(hnd))
    return rc, L.mjg_last_error().decode()


@pytest.mark.parametrize("at,value", [(0, 262145), (1, -262145), (2, 2 ** 31 - 1), (3, -2 ** 31), (4, 300000), (5, -262145)],
                         ids=lambda v: str(v))
def test_open_cmat_refuses_a_coefficient_past_four_times_unity_before_any_hip_call(at, value):
    cm = list(C_79)
    cm[at] = value
    rc, msg = _open_cmat(cm)
    assert rc == _lib.MJG_E_INVALID
    assert msg.startswith("cmatrix"), msg
    assert ("yu", "yv", "uu", "uv", "vu", "vv")[at] in msg and str(value) in msg, msg


def test_the_bound_keeps_every_sum_inside_int32():
    worst = 2 * 262144 * 128 + 8421376
    assert worst < 2 ** 27 < 2 ** 31 and ((2 * 262144 * 128 + 1081344) >> 16) + 255 < 2 ** 15


def test_open_cmat_is_declared_and_bound():
    assert {"mjg_open_cmat", "mjg_debug_cmat", "mjg_debug_cmat_out"} <= set(_lib.EXPORTS)
    L = _lib.load()
    assert L.mjg_version() == 105
    assert L.mjg_debug_cmat(None, None) == _lib.MJG_E_INVALID
    assert L.mjg_debug_cmat_out(None, 0, None, 0) == _lib.MJG_E_INVALID
    assert C.sizeof(_lib.MjgCmatrix) == 24
