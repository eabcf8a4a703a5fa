"""`-vf eq` without a GPU: the three byte tables (profile.eq_tables against both forms of
tests/eq_ref.py and the anchors of DESIGN §4.15), the parser (Profile.eq, its slot, and why every
other form stays on the CPU), and what the worker makes of it."""
import dataclasses

import numpy as np
import pytest

import eq_ref
from ffmpeg_distributed_amd import profile, worker
from ffmpeg_distributed_amd.container import StreamInfo

TAIL = " -c:v mjpeg -q:v 5 -dct int -huffman default -bitexact"
ID_CRC = 688229491
BIG = dict(gamma=2.2, saturation=1.5, contrast=0.9, brightness=0.05)

# (options, plane, form, the table at 0 16 128 235 255, zlib.crc32 of the table)
ANCHORS = [
    (dict(brightness=0.1), 0, "linear", (25, 41, 153, 255, 255), 1232863594),
    (dict(contrast=1.2), 0, "linear", (0, 0, 127, 255, 255), 4166937608),
    (dict(contrast=1.2, brightness=-0.07), 0, "linear", (0, 0, 107, 235, 255), 3800653831),
    (dict(brightness=-0.93), 0, "linear", (0, 0, 0, 0, 14), 2049565153),
    (dict(contrast=-1), 0, "linear", (255, 239, 127, 20, 0), 3661340938),
    (dict(contrast=-2.5, brightness=0.3), 0, "linear", (255, 255, 204, 0, 0), 4270798267),
    (dict(contrast=7.89), 0, "linear", (0, 0, 127, 255, 255), 1192363889),
    (dict(contrast=7.9), 0, "table", (0, 0, 131, 255, 255), 3205417094),      # float 7.9 is not < 7.9
    (dict(contrast=8), 0, "table", (0, 0, 132, 255, 255), 3225532473),
    (dict(saturation=1.3), 1, "linear", (0, 0, 127, 255, 255), 519133773),
    (dict(saturation=1.3), 2, "linear", (0, 0, 127, 255, 255), 519133773),
    (dict(saturation=0), 1, "linear", (127, 127, 127, 127, 127), 2950893963),
    (dict(saturation=0), 2, "linear", (127, 127, 127, 127, 127), 2950893963),
    (dict(saturation=3), 1, "linear", (0, 0, 127, 255, 255), 2538486373),
    (dict(saturation=3), 2, "linear", (0, 0, 127, 255, 255), 2538486373),
    (dict(gamma=1.1), 0, "table", (0, 20, 136, 237, 255), 2932472636),
    (dict(gamma=0.1), 0, "table", (0, 0, 0, 113, 255), 4151166569),
    (dict(gamma=10), 0, "table", (0, 194, 238, 253, 255), 3126540911),
    (dict(gamma=0.5, gamma_weight=0.5), 0, "table", (0, 8, 96, 226, 255), 1620225745),
    (BIG, 0, "table", (89, 110, 195, 247, 255), 4135632183),
    (BIG, 1, "linear", (0, 0, 127, 255, 255), 12809410),
    (BIG, 2, "linear", (0, 0, 127, 255, 255), 12809410),
    (dict(gamma_r=1.2, gamma_b=0.8), 1, "table", (0, 11, 118, 233, 255), 2242250836),
    (dict(gamma_r=1.2, gamma_b=0.8), 2, "table", (0, 20, 136, 237, 255), 1075568808),
    # identity planes: chroma of a luma-only request, luma of a chroma-only one, everything of the defaults
    (dict(brightness=0.1), 1, "id", (0, 16, 128, 235, 255), ID_CRC),
    (dict(saturation=1.3), 0, "id", (0, 16, 128, 235, 255), ID_CRC),
    (dict(gamma_r=1.2, gamma_b=0.8), 0, "id", (0, 16, 128, 235, 255), ID_CRC),
    (dict(), 0, "id", (0, 16, 128, 235, 255), ID_CRC),
    (dict(), 2, "id", (0, 16, 128, 235, 255), ID_CRC),
]


def _id(a):
    return ":".join(f"{k}={v}" for k, v in a[0].items()) + "/" + "YUV"[a[1]]


@pytest.mark.parametrize("spec,plane,form,values,crc", ANCHORS, ids=[_id(a) for a in ANCHORS])
def test_anchor_from_both_forms_of_the_reference_and_the_profile(spec, plane, form, values, crc):
    assert eq_ref.form(*eq_ref.plane_params(spec)[plane][:3]) == form
    for name, t in (("loop", eq_ref.tables(spec, "loop")[plane]), ("numpy", eq_ref.tables(spec, "numpy")[plane]),
                    ("profile.eq_tables", profile.eq_tables(spec)[plane])):
        assert tuple(int(t[v]) for v in eq_ref.ANCHOR_AT) == values, name
        assert eq_ref.crc(t) == crc, name


def test_eq_tables_shape_and_both_forms_on_a_sweep():
    t = profile.eq_tables(dict(contrast=1.2))
    assert t.shape == (3, 256) and t.dtype == np.uint8
    rng = np.random.default_rng(7)
    lo = dict(contrast=-3.0, brightness=-1.0, saturation=0.0, gamma=0.1, gamma_r=0.1, gamma_g=0.1, gamma_b=0.1, gamma_weight=0.0)
    hi = dict(contrast=9.0, brightness=1.0, saturation=3.0, gamma=10.0, gamma_r=10.0, gamma_g=10.0, gamma_b=10.0, gamma_weight=1.0)
    for i in range(60):
        spec = {k: round(float(rng.uniform(lo[k], hi[k])), 3) for k in eq_ref.NAMES if rng.random() < 0.5}
        a, b, c = eq_ref.tables(spec, "loop"), eq_ref.tables(spec, "numpy"), profile.eq_tables(spec)
        assert (a == b).all() and (a == c).all(), spec


def test_the_float_step_changes_brightness_minus_093():
    """(int)(100 * B + 100) is 6 through IEEE single and 7 in plain double: the table ends 12 13 14, not 14 15 16."""
    single = eq_ref.tables(dict(brightness=-0.93))[0]
    double = eq_ref.tables(dict(brightness=-0.93), single=False)[0]
    assert int(100.0 * float(np.float32(-0.93)) + 100.0) == 6 and int(100.0 * -0.93 + 100.0) == 7
    assert [int(v) for v in single[-3:]] == [12, 13, 14]
    assert [int(v) for v in double[-3:]] == [14, 15, 16]
    assert (profile.eq_tables(dict(brightness=-0.93))[0] == single).all()


def test_division_truncates_toward_zero_for_a_negative_ci():
    C = float(np.float32(-1.0))
    ci = int(C * 256 * 16)
    assert ci == -4096 and eq_ref.cdiv(ci, 32) == -128
    # a ci that 32 does not divide: C truncates (-80), Python's // floors (-81)
    ci2, _ = eq_ref.linear_ints(float(np.float32(-0.63)), 0.0)
    assert ci2 % 32 != 0 and eq_ref.cdiv(ci2, 32) == -(-ci2 // 32) == ci2 // 32 + 1
    floored = [min(255, max(0, ((v * ci2) >> 12) + (100 * 511) // 200 - 128 - ci2 // 32)) for v in range(256)]
    assert floored != [int(v) for v in profile.eq_tables(dict(contrast=-0.63))[0]]
    assert (profile.eq_tables(dict(contrast=-0.63))[0] == eq_ref.tables(dict(contrast=-0.63))[0]).all()
    assert profile._c_div(-7, 2) == -3 and profile._c_div(7, -2) == -3 and profile._c_div(-7, -2) == 3


# ------------------------------------------------------------------------- the parser
def _try(vf):
    return profile.try_parse("-vf " + vf + TAIL)


def _prof(vf):
    prof, why = _try(vf)
    assert prof is not None, why
    return prof


def _numbers(prof):
    return {k: prof.eq[k] for k in profile.EQ_NAMES}


def test_eq_alone_positional():
    p = _prof("eq=1.2")
    assert p.eq["slot"] == "in" and _numbers(p) == dict(profile.EQ_DEFAULT, contrast=1.2)
    assert p.scale is None and p.crop is None and p.pad is None and p.unsharp is None and p.orient == 0 and p.deint is None
    p = _prof("eq=1.1:0.05:1.3:0.9:1.1:1.2:0.8:0.5")
    assert _numbers(p) == dict(contrast=1.1, brightness=0.05, saturation=1.3, gamma=0.9, gamma_r=1.1, gamma_g=1.2,
                               gamma_b=0.8, gamma_weight=0.5)


def test_eq_in_front_of_the_scale():
    p = _prof("eq=brightness=0.06:saturation=1.3,scale=64:32")
    assert p.eq["slot"] == "in" and p.scale == (64, 32)
    assert _numbers(p) == dict(profile.EQ_DEFAULT, brightness=0.06, saturation=1.3)


def test_eq_between_the_crop_and_the_scale_and_in_front_of_the_crop():
    for vf in ("crop=32:16:2:2,eq=gamma=1.1,scale=64:32", "eq=gamma=1.1,crop=32:16:2:2,scale=64:32"):
        p = _prof(vf)
        assert p.eq["slot"] == "in" and p.scale == (64, 32) and p.crop == {"w": 32, "h": 16, "x": 2, "y": 2}
        assert p.eq["gamma"] == 1.1


def test_eq_directly_behind_the_scale():
    p = _prof("scale=64:32,eq=gamma=1.1,unsharp,pad=80:48")
    assert p.eq["slot"] == "out" and p.scale == (64, 32) and p.unsharp == (5, 5, 1.0, 5, 5, 0.0)
    assert p.pad == {"w": 80, "h": 48, "x": None, "y": None}
    assert _prof("scale=64:32,eq=1.2").eq["slot"] == "out"


def test_eq_behind_the_yadif_and_the_orientation():
    p = _prof("yadif,transpose=1,eq=contrast=1.2")
    assert p.eq["slot"] == "in" and p.deint == {"mode": 0, "parity": -1} and p.orient == 3 and p.eq["contrast"] == 1.2


def test_eq_without_a_scale_in_front_of_the_unsharp_and_the_pad():
    p = _prof("eq=1.2,unsharp,pad=80:48")
    assert p.eq["slot"] == "in" and p.scale is None and p.unsharp is not None and p.pad is not None
    assert _prof("crop=32:16,eq=1.2,pad=80:48").eq["slot"] == "in"


REJECTED = [
    ("eq=1.2,scale=64:32,eq=1.1", ["a second eq"]),
    ("eq=1.2,eq=1.1", ["a second eq"]),
    ("scale=64:32,unsharp,eq=1.2", ["eq behind the unsharp"]),
    ("unsharp,eq=1.2", ["eq behind the unsharp"]),
    ("scale=64:32,pad=80:48,eq=1.2", ["eq behind the pad"]),
    ("pad=80:48,eq=1.2", ["eq behind the pad"]),
    ("eq=1.2,yadif", ["yadif after eq"]),
    ("eq=1.2,vflip", ["vflip after eq"]),
    ("vflip,eq=1.2,transpose=1", ["transpose after eq"]),
    ("eq=eval=frame", ["eq eval=frame"]),
    ("eq=contrast=1.2:eval=init", ["eq eval=init"]),
    ("eq=contrast=1+t/10", ["eq contrast=1+t/10", "expression"]),
    ("eq=brightness=sin(t)", ["eq brightness=sin(t)", "expression"]),
    ("eq=contrast=1000.5", ["eq contrast=1000.5", "-1000..1000"]),
    ("eq=brightness=1.01", ["eq brightness=1.01", "-1..1"]),
    ("eq=brightness=-1.5", ["eq brightness=-1.5", "-1..1"]),
    ("eq=saturation=3.5", ["eq saturation=3.5", "0..3"]),
    ("eq=saturation=-0.1", ["eq saturation=-0.1", "0..3"]),
    ("eq=gamma=0.05", ["eq gamma=0.05", "0.1..10"]),
    ("eq=gamma_r=11", ["eq gamma_r=11", "0.1..10"]),
    ("eq=gamma_g=0", ["eq gamma_g=0", "0.1..10"]),
    ("eq=gamma_b=10.5", ["eq gamma_b=10.5", "0.1..10"]),
    ("eq=gamma_weight=1.5", ["eq gamma_weight=1.5", "0..1"]),
    ("eq=1:0:1:1:1:1:1:1:1", ["eq option '1'", "positional"]),
    ("eq=hue=3", ["eq option 'hue'"]),
    ("eq=", ["eq= without options"]),
    ("scale=64:32,eq=", ["eq= without options"]),
]


@pytest.mark.parametrize("vf,parts", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_with_the_cause_in_the_reason(vf, parts):
    prof, why = _try(vf)
    assert prof is None
    for p in parts:
        assert p in why, why


# the reasons of graphs that do not name eq, copied from tests/test_unsharp.py and tests/test_yadif.py
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
def test_reasons_for_graphs_without_eq_stay_letter_for_letter(vf, reason):
    prof, why = _try(vf)
    assert prof is None and why == reason


def test_graphs_without_eq_have_no_eq():
    for vf in ("scale=64:32", "crop=32:16,scale=64:32,unsharp,pad=80:48", "yadif,vflip"):
        assert _prof(vf).eq is None
    prof, why = profile.try_parse(TAIL)
    assert prof is not None and prof.eq is None
    assert "eq" in {f.name for f in dataclasses.fields(profile.Profile)}


# ------------------------------------------------------------------------- the worker
INFO = StreamInfo(width=130, height=66, fps=25, sar=(1, 1), full_range=False, chroma="420")


def test_encoder_key_differs_when_only_the_tables_differ():
    a, b, none = _prof("eq=1.2,scale=70:38"), _prof("eq=1.3,scale=70:38"), _prof("scale=70:38")
    out = _prof("scale=70:38,eq=1.2")

    def key(p):
        return worker.encoder_key(p, INFO, 70, 38, (1, 1), False, 8, luts=worker.eq_luts(p))

    assert len({key(a), key(b), key(none), key(out)}) == 4
    assert key(a) == key(_prof("eq=contrast=1.2,scale=70:38"))
    assert key(none) == worker.encoder_key(none, INFO, 70, 38, (1, 1), False, 8)


def test_eq_luts_puts_the_tables_in_the_slot():
    lin, lout = worker.eq_luts(_prof("eq=1.2:0.1,scale=70:38"))
    assert lout is None and (lin == eq_ref.tables(dict(contrast=1.2, brightness=0.1))).all()
    lin, lout = worker.eq_luts(_prof("scale=70:38,eq=gamma=1.1"))
    assert lin is None and (lout == eq_ref.tables(dict(gamma=1.1))).all()
    assert worker.eq_luts(_prof("scale=70:38")) == (None, None)


def test_eq_fallthrough_reason():
    f = worker.eq_fallthrough_reason
    assert f(_prof("scale=70:38"), INFO) is None
    assert f(_prof("eq=1.2"), INFO) is None and f(_prof("scale=70:38,eq=1.2"), INFO) is None
    deep = dataclasses.replace(INFO)
    deep.bits = 16
    assert f(_prof("eq=1.2"), deep) == "eq on a 16-bit input: only the filter's 8-bit path is GPU-accelerated"
    bad = dataclasses.replace(_prof("eq=1.2"), eq=dict(_prof("eq=1.2").eq, slot="out"))      # the parser never makes this
    with pytest.raises(AssertionError):
        f(bad, INFO)
