"""worker.plan_segment: a profile resolved against one segment's input, without a device, a stream or
stderr.  The expectations are literals worked out by hand from the FFmpeg rules the helpers restate
(vf_crop's rounding and clamping, vf_pad's placement, vf_transpose's 1 / SAR, vf_scale's SAR, yadif's
parity), not computed with the helpers; the reasons are the worker's, letter for letter."""
import dataclasses

import numpy as np
import pytest

from ffmpeg_distributed_amd import profile, worker
from ffmpeg_distributed_amd.container import StreamInfo
from test_scale_stream import _run

TAIL = "-c:v mjpeg -q:v 5 -dct int -huffman default -bitexact"
INFO = StreamInfo(130, 66, sar=(4, 3), chroma="420")
FULL = "yadif,transpose=1,colormatrix=bt709:bt601,crop=62:126:2:2,eq=1.2,scale=32:64,unsharp,pad=48:80:8:8"
C_709_601 = (6657, 12850, 64871, -7252, -4748, 64448)     # tests/test_colormatrix.py pins these against the filter
IDENTITY = list(range(256))


def _prof(vf=None, *extra):
    return profile.parse((["-vf", vf] if vf else []) + TAIL.split() + list(extra))


def _info(w=130, h=66, bits=None, **kw):
    info = StreamInfo(w, h, **kw)
    if bits is not None:
        info.bits = bits          # as tests/test_eq.py makes a deeper input
    return info


def _plan(vf=None, info=INFO, *extra):
    return worker.plan_segment(_prof(vf, *extra), info)


def _fields(plan, **want):
    """Every field of the plan but the tables, against `want` (defaults: a plan that resolves nothing)."""
    base = dict(deint=0, orient=0, rect=None, pad=None, unsharp=None, cmat=None)
    base.update(want)
    got = {f.name: getattr(plan, f.name) for f in dataclasses.fields(plan) if f.name not in ("lut_in", "lut_out")}
    assert got == base
    assert all(isinstance(v, (int, str, tuple, type(None))) for v in got.values())


def _contrast_1_2(tab):
    # vf_eq's linear form for contrast 1.2 (as a float: 1.2000000477): ci = (int)(c * 4096) = 4915,
    # bi = 255 - 128 - 4915 / 32 = -26, pel = clip((v * 4915 >> 12) - 26); chroma: saturation 1, copied
    assert tab.shape == (3, 256) and tab.dtype == np.uint8
    assert [int(tab[0][v]) for v in (0, 21, 22, 128, 234, 235, 255)] == [0, 0, 0, 127, 254, 255, 255]
    assert tab[1].tolist() == IDENTITY and tab[2].tolist() == IDENTITY


# ------------------------------------------------------------------------------------ accepted
def test_the_whole_chain_every_field():
    plan = _plan(FULL)
    _fields(plan,
            src_chroma="420", dst_chroma="420",
            deint=1,                          # yadif on: mode 0, parity auto -> tff of a progressive stream
            orient=3,                         # transpose=1 (clock): T | FX
            rect=(2, 2, 62, 126),             # of the 66 x 130 oriented frame: 126 rows do not fit the 130 x 66 one
            in_size=(62, 126), dst_w=32, dst_h=64,
            pad=(8, 8, 48, 80), enc_w=48, enc_h=80,
            unsharp=(5, 5, 1.0, 5, 5, 0.0),
            cmat=C_709_601,
            # 1 / (4:3) = 3:4 under the transpose, then the scale's: 3/4 * (64 * 62) / (32 * 126) = 31:42
            # (from the 48 x 80 canvas it would be 155:252, without the inversion 248:189)
            sar=(31, 42))
    _contrast_1_2(plan.lut_in)                # the eq stands in front of the scale
    assert plan.lut_out is None
    with pytest.raises(dataclasses.FrozenInstanceError):
        plan.orient = 0


def test_without_a_crop():
    plan = _plan("transpose=1,scale=32:64,pad=48:80:8:8")
    # 3:4 * (64 * 66) / (32 * 130) = 99:130
    _fields(plan, src_chroma="420", dst_chroma="420", orient=3, in_size=(66, 130), dst_w=32, dst_h=64,
            pad=(8, 8, 48, 80), enc_w=48, enc_h=80, sar=(99, 130))
    assert plan.lut_in is None and plan.lut_out is None


def test_without_a_scale():
    plan = _plan("crop=62:30:2:2,pad=80:48:-1:-1")
    # the picture is the rectangle; centred at (80 - 62) / 2 = 9 and (48 - 30) / 2 = 9, rounded down to 4:2:0's 2
    _fields(plan, src_chroma="420", dst_chroma="420", rect=(2, 2, 62, 30), in_size=(62, 30), dst_w=62, dst_h=30,
            pad=(8, 8, 80, 48), enc_w=80, enc_h=48, sar=(4, 3))


def test_without_a_pad_and_the_eq_behind_the_scale():
    plan = _plan("yadif=2:bff,crop=64:32,scale=32:16,eq=1.2")
    # centred: (130 - 64) / 2 = 33 -> 32, (66 - 32) / 2 = 17 -> 16; the encoded size is the picture's
    _fields(plan, src_chroma="420", dst_chroma="420", deint=1 | 2 | 4, rect=(32, 16, 64, 32), in_size=(64, 32),
            dst_w=32, dst_h=16, enc_w=32, enc_h=16, sar=(4, 3))
    assert plan.lut_in is None
    _contrast_1_2(plan.lut_out)


def test_pix_fmt_420_from_a_444_input():
    plan = _plan("crop=31:15:3:1", _info(chroma="444", sar=(1, 1)), "-pix_fmt", "yuvj420p")
    # the crop sees the decoded 4:4:4: nothing is rounded
    _fields(plan, src_chroma="444", dst_chroma="420", rect=(3, 1, 31, 15), in_size=(31, 15), dst_w=31, dst_h=15,
            enc_w=31, enc_h=15, sar=(1, 1))


def test_a_full_range_input_without_filters():
    plan = _plan(None, _info(full_range=True))
    _fields(plan, src_chroma="420", dst_chroma="420", in_size=(130, 66), dst_w=130, dst_h=66, enc_w=130, enc_h=66,
            sar=(0, 0))
    assert plan.lut_in is None and plan.lut_out is None


def test_an_unknown_sar_stays_unknown_under_a_transpose():
    assert _plan("transpose=2,scale=32:64", _info()).sar == (0, 0)


# ------------------------------------------------------------------------------------ the ten ways out
CPU, FAIL = "cpu", "fail"
RESAMPLE = "-pix_fmt needs 420 -> 444 chroma resampling"
PARITY = ("yadif parity=auto on a stream of mixed or unknown field order (Im): per-frame field flags are not "
          "GPU-accelerated")
TRANSPOSE = "transpose of a 4:2:2 input: FFmpeg converts the format first"
CROP = "Invalid too big or non positive size for width '200' or height '16' (crop of a {}x{} input)"
PAD_FMT = "pad before the 444 -> 420 -pix_fmt conversion (no scale in the graph: the converter runs after the pad)"
PAD = "Input area {}:{}:{}:{} not within the padded area 0:0:64:32 or zero-sized (pad of a 130x66 input)"
UNSHARP = "unsharp without a scale on a tv-range / converted input: FFmpeg sharpens before its converter"
EQ = "eq on a 10-bit input: only the filter's 8-bit path is GPU-accelerated"
CMAT = ("colormatrix on a full-range (yuvj) input: the filter takes yuv420p / yuv422p / yuv444p, and FFmpeg "
        "converts the range first, which is not GPU-accelerated")
CASCADE = "scale 1024x64 -> 16x8 needs swscale's cascade"
TO_444, TO_420 = ("-pix_fmt", "yuvj444p"), ("-pix_fmt", "yuvj420p")


def _way_out(vf, info, extra=()):
    """(kind, text) of the way plan_segment leaves."""
    prof = _prof(vf, *extra)
    try:
        worker.plan_segment(prof, info)
    except worker.Fallthrough as e:
        return CPU, str(e)
    except profile.CropError as e:
        return FAIL, f"crop: {e}"
    except profile.PadError as e:
        return FAIL, f"pad: {e}"
    return None, None


@pytest.mark.parametrize("vf,info,extra,kind,text", [
    (None, _info(), TO_444, CPU, RESAMPLE),
    ("yadif", _info(field="m"), (), CPU, PARITY),
    ("transpose=1", _info(chroma="422"), (), CPU, TRANSPOSE),
    ("crop=200:16", _info(), (), FAIL, "crop: " + CROP.format(130, 66)),
    ("pad=160:80", _info(chroma="444"), TO_420, CPU, PAD_FMT),
    # a 64 x 32 canvas: x = (64 - 130) / 2 = -33 -> -34 in 4:2:0, y = (32 - 66) / 2 = -17 -> -18
    ("pad=64:32", _info(), (), FAIL, "pad: " + PAD.format(-34, -18, 96, 48)),
    ("unsharp", _info(), (), CPU, UNSHARP),
    ("eq=1.2", _info(bits=10), (), CPU, EQ),
    ("colormatrix=bt709:bt601", _info(full_range=True), (), CPU, CMAT),
    ("scale=16:8", _info(1024, 64), (), CPU, CASCADE),
])
def test_each_way_out_alone(vf, info, extra, kind, text):
    assert _way_out(vf, info, extra) == (kind, text)


# one input that trips two neighbouring checks (the earlier one is reported), and the same input with
# the earlier cause taken away (the later one is)
@pytest.mark.parametrize("both,later", [
    ((("yadif", _info(field="m"), TO_444), (CPU, RESAMPLE)),
     (("yadif", _info(field="m")), (CPU, PARITY))),
    ((("yadif,transpose=1", _info(chroma="422", field="m")), (CPU, PARITY)),
     (("yadif,transpose=1", _info(chroma="422")), (CPU, TRANSPOSE))),
    ((("transpose=1,crop=200:16", _info(chroma="422")), (CPU, TRANSPOSE)),
     (("transpose=1,crop=200:16", _info()), (FAIL, "crop: " + CROP.format(66, 130)))),
    ((("crop=200:16,pad=240:80", _info(chroma="444"), TO_420), (FAIL, "crop: " + CROP.format(130, 66))),
     (("crop=64:16,pad=240:80", _info(chroma="444"), TO_420), (CPU, PAD_FMT))),
    ((("pad=64:32", _info(chroma="444"), TO_420), (CPU, PAD_FMT)),
     (("pad=64:32", _info(chroma="444")), (FAIL, "pad: " + PAD.format(-33, -17, 97, 49)))),    # 4:4:4: nothing rounded
    ((("unsharp,pad=64:32", _info()), (FAIL, "pad: " + PAD.format(-34, -18, 96, 48))),
     (("unsharp,pad=160:80", _info()), (CPU, UNSHARP))),
    ((("eq=1.2,unsharp", _info(bits=10)), (CPU, UNSHARP)),
     (("eq=1.2,unsharp", _info(bits=10, full_range=True)), (CPU, EQ))),
    ((("colormatrix=bt709:bt601,eq=1.2", _info(bits=10, full_range=True)), (CPU, EQ)),
     (("colormatrix=bt709:bt601,eq=1.2", _info(full_range=True)), (CPU, CMAT))),
    ((("colormatrix=bt709:bt601,scale=16:8", _info(1024, 64, full_range=True)), (CPU, CMAT)),
     (("colormatrix=bt709:bt601,scale=16:8", _info(1024, 64)), (CPU, CASCADE))),
], ids=["resample<deint", "deint<transpose", "transpose<crop", "crop<pad-format", "pad-format<pad", "pad<unsharp",
        "unsharp<eq", "eq<colormatrix", "colormatrix<cascade"])
def test_of_two_neighbouring_ways_out_the_earlier_is_reported(both, later):
    for args, want in (both, later):
        assert _way_out(*args) == want


# ------------------------------------------------------------------------------------ the cache key
def _key(vf, batch=8):
    prof = _prof(vf)
    return worker.plan_segment(prof, INFO).key(prof, INFO, False, batch)


def test_the_key_is_encoder_key_of_the_plans_own_fields():
    prof = _prof(FULL)
    p = worker.plan_segment(prof, INFO)
    assert p.key(prof, INFO, False, 8) == _key(FULL)                      # built twice
    assert p.key(prof, INFO, False, 8) == worker.encoder_key(
        prof, INFO, 32, 64, (31, 42), False, 8, (2, 2, 62, 126), (8, 8, 48, 80), 3, 1, (5, 5, 1.0, 5, 5, 0.0),
        (p.lut_in, None), C_709_601)
    assert p.key(prof, INFO, False, 8)[-1] == ("cmat",) + C_709_601
    assert p.key(prof, INFO, True, 8) != _key(FULL) != _key(FULL, 4)


@pytest.mark.parametrize("what,old,new", [
    ("rect", "crop=62:126:2:2", "crop=62:126:4:2"),
    ("pad", "pad=48:80:8:8", "pad=48:80:8:10"),
    ("orient", "transpose=1", "transpose=2"),
    ("deint", "yadif", "yadif=2"),
    ("unsharp", "unsharp", "unsharp=3:3:0.5"),
    ("the eq's numbers", "eq=1.2", "eq=1.3"),
    ("the eq's slot", "eq=1.2,scale=32:64", "scale=32:64,eq=1.2"),
    ("the colormatrix pair", "colormatrix=bt709:bt601", "colormatrix=bt601:bt709"),
])
def test_the_key_changes_with(what, old, new):
    assert old in FULL
    a, b = _key(FULL), _key(FULL.replace(old, new))
    assert a != b and len(a) == len(b)
    assert sum(x != y for x, y in zip(a, b)) == 1, what       # nothing else of the key moved


def test_the_encoder_gets_the_plan():
    kw = _plan(FULL).encoder_kwargs()
    tab = kw.pop("lut_in")
    _contrast_1_2(tab)
    assert kw == dict(sar=(31, 42), chroma="420", src_chroma="420", crop=(2, 2, 62, 126), pad=(8, 8, 48, 80), orient=3,
                      deint=1, unsharp=(5, 5, 1.0, 5, 5, 0.0), lut_out=None, cmat=C_709_601)
    assert _plan("scale=32:16").encoder_kwargs()["deint"] is None        # the encoder's "no deinterlacer"


# ------------------------------------------------------------------------------------ run() itself
def test_run_writes_one_line_for_a_fallthrough_and_hands_the_args_on(monkeypatch):
    rc, calls, err, args = _run(monkeypatch, 130, 66, "unsharp")
    assert rc == 0 and calls == [args]
    assert err.splitlines() == [f"gpu:3: {UNSHARP}; running ffmpeg on the CPU"]


@pytest.mark.parametrize("vf,line", [
    ("crop=200:16", "gpu:3: crop: " + CROP.format(130, 66)),
    ("pad=64:32", "gpu:3: pad: " + PAD.format(-34, -18, 96, 48)),
])
def test_run_fails_as_ffmpeg_does_when_the_filter_cannot_be_configured(monkeypatch, vf, line):
    rc, calls, err, _ = _run(monkeypatch, 130, 66, vf)
    assert rc == 1                  # not None: bind_numa was not reached
    assert calls == [] and err.splitlines() == [line]
