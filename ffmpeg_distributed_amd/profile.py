"""Parse the reference's `remote_args` (ffmpeg_distributed.py:190 shlex-splits them and
:134 passes them to the worker ffmpeg) into the GPU encode profile, or report why the
arguments fall outside it (the worker then runs the real ffmpeg unchanged).

Supported profile (BASELINE north star, plus FFmpeg's default -huffman optimal):
    [-vf FILTERS] -c:v mjpeg -q:v N -dct int [-huffman default|optimal] -bitexact
with FILTERS one of
    scale=W:H[:flags=bicubic...]
    crop=w:h[:x:y]                          (also w= / out_w=, h= / out_h=, x=, y=; keep_aspect=0, exact=0)
    crop=...,scale=W:H[:flags=bicubic...]   (in this order)
    any of these, or nothing, followed by
    unsharp[=lx:ly:la:cx:cy:ca]             (also luma_msize_x= / lx=, luma_msize_y= / ly=, luma_amount= / la=,
                                            chroma_msize_x= / cx=, chroma_msize_y= / cy=, chroma_amount= / ca=)
    any of these, or nothing, followed by
    pad=W:H[:x:y[:black]]                   (also width= / w=, height= / h=, x=, y=, color= / c=; last)
    and in front of any of these, or alone, a run of any length and order of
    vflip | transpose=N | transpose=dir=N | transpose=<name>   (N 0..3; cclock_flip, clock, cclock,
                                            clock_flip; optionally :passthrough=none)
which is composed here into one of eight plane maps, `Profile.orient` = T | FX << 1 | FY << 2
(`vflip,vflip` is 0 and costs nothing).  `hflip` is not parsed: the library and the
encoder take its map (orient 2) and compose_orient composes it, but a graph that names it stays
outside the profile, as it was (DESIGN §4.12 says why).  In front of all of that, as the very
first filter of the graph or alone,
    yadif[=mode[:parity[:deint]]]           (also mode=, parity=, deint=; send_frame / 0, send_frame_nospatial / 2;
                                            tff / 0, bff / 1, auto / -1; all / 0)
is `Profile.deint` = {"mode": 0 | 2, "parity": -1 | 0 | 1} (parity auto is resolved by
the worker from the container's field order).  The field-rate modes 1 and 3, deint=interlaced, a
yadif anywhere else in the graph, and bwdif, w3fdif, estdif and the other deinterlacers are outside
the profile, each with a reason that names it.  `unsharp` is `Profile.unsharp` = (lx, ly, la, cx, cy,
ca), the filter's defaults 5:5:1.0:5:5:0.0 filled in: plain numbers only, odd sizes
3..23, amounts -2..5, and lx // 2 + ly // 2 <= 12 for a plane whose amount is not 0 (past that the
filter's 32-bit sum wraps).  Its alpha and opencl options, an expression, a second unsharp and an
unsharp anywhere but directly in front of the pad or the end are outside the profile.  One
    eq[=contrast:brightness:saturation:gamma:gamma_r:gamma_g:gamma_b:gamma_weight]   (or by these names)
behind the yadif and the orientation run is `Profile.eq`: anywhere in front of the
scale (slot "in"; without a scale, in front of the unsharp and the pad) or directly behind it (slot
"out").  Plain numbers inside the filter's ranges only; `eval=`, an expression, a second eq and an eq
behind the unsharp or the pad are outside the profile.  `eq_tables` makes the three byte tables, a
restatement of vf_eq.c's 8-bit path that is unpinned against FFmpeg.  One
    colormatrix=SRC:DST                     (also src=, dst=; bt709, fcc, bt601, smpte240m, bt2020, and bt470,
                                            bt470bg, smpte170m for bt601)
behind the yadif and the orientation run, in front of any eq and of the scale (without a scale: in
front of the unsharp and the pad), before or after the crop, is `Profile.colormatrix` = the canonical
(src, dst).  A second colormatrix, a missing dst, a missing src (FFmpeg takes it from
frame metadata), src equal to dst (FFmpeg refuses it itself), an unknown name or key and any other
position are outside the profile, each with a reason that names it.  `colormatrix_coefs` makes the six
16.16 coefficients, a restatement of vf_colormatrix.c's 8-bit planar path that is unpinned against
FFmpeg.  Around all of that,
    framestep=N | framestep=step=N          (the very first filter; not with yadif)
    tile[=COLSxROWS[:nb_frames[:margin[:padding[:black[:0[:0]]]]]]]   (also layout=, nb_frames=, margin=, padding=,
                                            color=, overlap=, init_padding=; the very last filter; not with pad)
make the profile a `SheetProfile`: `framestep` = N, which the worker's reader applies,
and `tile` = the request as given, which the worker resolves against the cell.  Decimal integers only; a
colour other than black, an overlap or init_padding other than 0, an expression, a second one of either,
any other position and what FFmpeg itself rejects (nb_frames above cols x rows, a step below 1) are
outside the profile, each with a reason that names it.  `framestep=1` is no filter, and a graph that
names neither filter parses to the plain `Profile` it always did.  Both are restatements (vf_tile.c,
vf_framestep.c) that are unpinned against FFmpeg.  In front of such a graph,
    thumbnail | thumbnail=N | thumbnail=n=N (the very first filter, or the second directly behind a leading
                                            framestep; only in a graph that ends in tile; not with yadif)
makes it a `ThumbProfile`: `thumbnail` = N (2 or more; the default is 100), the group of
consecutive frames of which the worker's reader keeps one, the frame whose histogram is closest to the
group's mean histogram (`thumbnail_pick`, on histograms the GPU counts).  A second thumbnail, any other
position, a graph that also names yadif, a graph whose last filter is no tile (the filter keeps its link's
frame rate and emits sparse timestamps, which MkvWriter does not write), N below 2, a non-integer and an
unknown key are outside the profile, each with a reason that names it.  A restatement of vf_thumbnail.c's
8-bit planar path (FFmpeg 5.1 and later) that is unpinned against FFmpeg.  One
    hqdn3d[=luma_spatial[:chroma_spatial[:luma_tmp[:chroma_tmp]]]]   (or by these names)
as the very first filter, or directly behind a leading yadif, makes the profile a `DenoiseProfile` (DESIGN
§4.19): `hqdn3d` = the four strengths, a missing or zero one replaced as the filter replaces it (4, 3 ls / 4,
6 ls / 4, lt cs / ls).  A second hqdn3d, any other position, an expression, a negative or non-numeric value,
an unknown key, more than four positional values and a graph that also names framestep, thumbnail or tile
are outside the profile, each with a reason that names it.  `hqdn3d_tables` makes the four tables, a
restatement of vf_hqdn3d.c's 8-bit path that is unpinned against FFmpeg.  An orientation filter after a crop, scale
or pad, transpose values 4..7, a passthrough other than none and any other option are outside the
profile.  The crop values are decimal integers (no expressions); `Profile.crop` is the request as
given and `resolve_crop` turns it into a rectangle of a given input (vf_crop.c's rounding,
defaults and clamping: DESIGN §4.8).  The pad values are decimal integers too (W / H 0 or absent:
the input's; a negative x / y centres), plus the two centring expressions x=(ow-iw)/2 and
y=(oh-ih)/2; the colour is black; `Profile.pad` is the request as given and `resolve_pad` turns it
into the picture's place and the canvas size for a given input (vf_pad.c's centring and rounding:
DESIGN §4.10).  Any other pad expression or colour, `eval=`, `aspect=`, and a pad that is not
the last filter are outside the profile.  The scale may be any size pair whose bicubic filters stay
below 256 taps in each direction, on the luma and the chroma planes: down to about 64:1
(3840x2160 -> 64x36 runs), and any upscale.  At 256 taps or more swscale cascades two scalers,
which the GPU path does not: the worker finds that out before it touches the GPU
(worker.scale_cascade_reason) and sends the segment to ffmpeg on the CPU.  Plus
  - the slice-threaded (RST) layout: -slices N (N > 1), or -thread_type slice with -threads
    other than 1 (mpegvideo's slice_context_count > 1: DRI + one restart interval per MCU
    row; mjpegenc.c then forces -huffman default);
  - -pix_fmt yuvj420p / yuvj422p / yuvj444p (the output sampling; when the input's has more
    chroma samples the GPU path down-samples, worker.resample_plan);
  - options that do not change the video bitstream: -an -sn -dn -y -threads N
    -thread_type frame -f matroska -map 0:v[:0].
Of several -vf / -filter:v options the last one wins, as in FFmpeg: each replaces every chain field
of the one before it (an earlier graph outside the profile still refuses the arguments).  The graph
is split once into filters, and the stages of GRAPH_STAGES take theirs off that list in turn.
"""
from __future__ import annotations

import re
import math
import shlex
from math import gcd
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union


@dataclass
class Profile:
    qscale: int                      # effective mpegvideo qscale (update_qscale mapping)
    q_arg: float                     # the -q:v value as given
    scale: Optional[Tuple[int, int]] = None   # -vf scale=W:H
    sws_flags: Tuple[str, ...] = ("bicubic",)
    huffman: str = "optimal"         # mjpegenc.c "huffman" option, default optimal
    rst: bool = False                # slice threading: DRI + RST per MCU row
    chroma: Optional[str] = None     # "420"/"422"/"444" from -pix_fmt (None: the input's)
    # -vf crop=...: the request as given, {"w", "h", "x", "y"} -> int or None (absent), unresolved
    # (resolve_crop needs the input's size and format); None: no crop
    crop: Optional[dict] = None
    # -vf ...,pad=...: the request as given, {"w", "h", "x", "y"} -> int, None (absent) or, for x / y,
    # the centring expression; unresolved (resolve_pad needs the pad's input size and format); None: no pad
    pad: Optional[dict] = None
    # a leading run of vflip / transpose filters, composed: T | FX << 1 | FY << 2 (compose_orient);
    # the crop, the scale and the pad then see the oriented frame.  0: none
    orient: int = 0
    # -vf yadif as the very first filter: {"mode": 0 | 2, "parity": -1 (auto: the container's field
    # order, worker.resolve_parity) | 0 (tff) | 1 (bff)}; None: no deinterlacer
    deint: Optional[dict] = None
    # -vf ...,unsharp[,pad]: (lx, ly, la, cx, cy, ca), sizes as ints and amounts as floats, the
    # filter's defaults filled in; None: no unsharp
    unsharp: Optional[tuple] = None
    # -vf ...,eq=...: {"slot": "in" (in front of the scale, on the decoded samples) | "out" (directly
    # behind the scale, on its full-range output), and the filter's eight numbers (EQ_NAMES), the
    # defaults filled in}; eq_tables turns them into the three tables.  None: no eq
    eq: Optional[dict] = None
    # -vf ...,colormatrix=SRC:DST: the canonical (src, dst) names (COLORMATRIX_LUMA's keys), in front of
    # any eq and the scale; colormatrix_coefs turns them into the six coefficients.  None: no colormatrix
    colormatrix: Optional[Tuple[str, str]] = None


@dataclass
class SheetProfile(Profile):
    """The Profile of a graph that names `tile` or a `framestep` above 1 (parse returns one exactly then;
    every other graph gives a plain Profile, field for field what it was)."""
    # -vf ...,tile=...: the request as given, {"cols", "rows", "nb_frames" (0: cols * rows), "margin", "padding"};
    # None: no tile
    tile: Optional[dict] = None
    # -vf framestep=N,...: the reader keeps every N-th frame of the segment; 1: every frame
    framestep: int = 1


THUMBNAIL_DEFAULT = 100  # vf_thumbnail.c's n


@dataclass
class ThumbProfile(SheetProfile):
    """The SheetProfile of a graph that names `thumbnail` (parse returns one exactly then)."""
    # -vf [framestep=S,]thumbnail=N,...,tile: of every N consecutive frames (behind the framestep) the reader keeps
    # the one that thumbnail_pick selects
    thumbnail: int = THUMBNAIL_DEFAULT


@dataclass
class DenoiseProfile(Profile):
    """The Profile of a graph that names `hqdn3d` (parse returns one exactly then; every other graph gives the
    Profile it always did)."""
    # -vf [yadif,]hqdn3d[=ls:cs:lt:ct]: the four strengths, resolved ({"ls", "cs", "lt", "ct"} -> float, every one
    # positive); hqdn3d_tables turns them into the four tables
    hqdn3d: Optional[dict] = None


class Unsupported(ValueError):
    pass


def effective_qscale(q: float) -> int:
    """mpegvideo_enc.c update_qscale for a fixed -q:v: lambda = q*FF_QP2LAMBDA(118),
    qscale = (lambda*139 + 128*64) >> 14, clipped to [qmin=2, qmax=31]."""
    lam = int(q * 118)
    return max(2, min(31, (lam * 139 + 128 * 64) >> 14))


_FLAGS_OK = {"bicubic", "accurate_rnd", "bitexact", "full_chroma_int", "full_chroma_inp"}


class CropError(ValueError):
    """A crop request that does not fit the input (ffmpeg fails to configure the filter)."""
    filter = "crop"


_CROP_KEYS = {"w": "w", "out_w": "w", "h": "h", "out_h": "h", "x": "x", "y": "y"}


def _parse_crop(f: str) -> dict:
    """`crop=...` -> {"w", "h", "x", "y"}: int, or None where the option is absent."""
    out = {"w": None, "h": None, "x": None, "y": None}
    pos = 0
    for p in f[len("crop="):].split(":"):
        if "=" in p:
            k, v = p.split("=", 1)
        else:
            if pos >= 4:
                raise Unsupported(f"crop option {p!r} (positional options are w:h:x:y)")
            k, v = "whxy"[pos], p
            pos += 1
        if k in ("keep_aspect", "exact"):
            if v != "0":
                raise Unsupported(f"crop {k}={v} (only {k}=0 is GPU-accelerated)")
            continue
        if k not in _CROP_KEYS:
            raise Unsupported(f"crop option {k!r}")
        if not (v.isascii() and v.isdigit()):
            raise Unsupported(f"crop {k}={v} (an expression; only decimal integer literals are GPU-accelerated)")
        out[_CROP_KEYS[k]] = int(v)
    return out


class PadError(ValueError):
    """A pad request that does not fit its input (ffmpeg fails to configure the filter)."""
    filter = "pad"


PAD_CENTRE = {"x": "(ow-iw)/2", "y": "(oh-ih)/2"}   # the two expressions taken, each for its own option
_PAD_KEYS = {"width": "w", "w": "w", "height": "h", "h": "h", "x": "x", "y": "y", "color": "color", "c": "color"}


def _parse_pad(f: str) -> dict:
    """`pad=...` -> {"w", "h", "x", "y"}: w / h int or None (absent); x / y int (a negative one
    centres), the centring expression as given (PAD_CENTRE), or None (absent).  Only black."""
    out = {"w": None, "h": None, "x": None, "y": None}
    pos = 0
    order = ("w", "h", "x", "y", "color")
    for p in f[len("pad="):].split(":"):
        if "=" in p:
            k, v = p.split("=", 1)
        else:
            if pos >= len(order):
                raise Unsupported(f"pad option {p!r} (positional options are width:height:x:y:color)")
            k, v = order[pos], p
            pos += 1
        if k in ("eval", "aspect"):
            raise Unsupported(f"pad {k}={v} (not GPU-accelerated)")
        if k not in _PAD_KEYS:
            raise Unsupported(f"pad option {k!r}")
        k = _PAD_KEYS[k]
        if k == "color":
            if v != "black":
                raise Unsupported(f"pad color={v} (only black is GPU-accelerated)")
        elif v.isascii() and v.isdigit():
            out[k] = int(v)
        elif k in "xy" and v.startswith("-") and v[1:].isascii() and v[1:].isdigit():
            out[k] = -int(v[1:])
        elif k in "xy" and v == PAD_CENTRE[k]:
            out[k] = v
        else:
            raise Unsupported(f"pad {k}={v} (an expression; only decimal integers and the centring forms "
                              f"x={PAD_CENTRE['x']}, y={PAD_CENTRE['y']} are GPU-accelerated)")
    return out


def resolve_pad(spec: dict, in_w: int, in_h: int, chroma: str) -> Tuple[int, int, int, int]:
    """(x, y, W, H): where a pad request puts an in_w x in_h input and the canvas size, in
    `chroma` ("420"/"422"/"444": the format the filter sees), as vf_pad.c config_input does: an
    absent or zero W / H is the input's; an x / y that is negative, asked to centre, or leaves
    the input past the canvas edge becomes (W - in_w) / 2 (C truncation); then W, x are rounded
    down to the horizontal and H, y to the vertical sub-sampling.  A canvas the input does not
    fit in raises PadError (ffmpeg fails; nothing is passed through)."""
    hs, vs = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[str(chroma)]
    W = int(spec.get("w") or 0) or in_w
    H = int(spec.get("h") or 0) or in_h

    def place(v, size, canvas):
        v = 0 if v is None else v
        if isinstance(v, str) or v < 0 or v + size > canvas:
            d = canvas - size
            v = d // 2 if d >= 0 else -((-d) // 2)
        return int(v)

    x, y = place(spec.get("x"), in_w, W), place(spec.get("y"), in_h, H)
    W &= ~((1 << hs) - 1)
    x &= ~((1 << hs) - 1)
    H &= ~((1 << vs) - 1)
    y &= ~((1 << vs) - 1)
    if x < 0 or y < 0 or W <= 0 or H <= 0 or x + in_w > W or y + in_h > H:
        raise PadError(f"Input area {x}:{y}:{x + in_w}:{y + in_h} not within the padded area 0:0:{W}:{H} "
                       f"or zero-sized (pad of a {in_w}x{in_h} input)")
    return x, y, W, H


ORIENT_FILTERS = ("vflip", "transpose")     # what _take_orient takes as a leading run (hflip: see the module docstring)
TRANSPOSE_DIRS = {"cclock_flip": 0, "clock": 1, "cclock": 2, "clock_flip": 3}


def orient_after(orient: int, flt: int) -> int:
    """The orientation (T | FX << 1 | FY << 2: every plane becomes flip_FX,FY(T ? P' : P)) of
    `orient` followed by the filter with orientation `flt`.  A flip after a flip toggles its bit;
    transposing a flipped plane transposes it and swaps the two flips (a mirrored column order
    becomes a mirrored row order), and the filter's own flips follow."""
    t, fx, fy = orient & 1, (orient >> 1) & 1, (orient >> 2) & 1
    if flt & 1:
        t, fx, fy = t ^ 1, fy, fx
    return t | ((fx ^ ((flt >> 1) & 1)) << 1) | ((fy ^ ((flt >> 2) & 1)) << 2)


def _parse_orient(f: str) -> int:
    """One hflip / vflip / transpose filter -> its orientation.  vf_transpose.c: dir 0 cclock_flip
    out[y][x] = in[x][y], 1 clock in[h-1-x][y], 2 cclock in[x][w-1-y], 3 clock_flip
    in[h-1-x][w-1-y]: the transpose, then a flip of the columns (1), the rows (2) or both (3)."""
    name, _, opts = f.partition("=")
    if name in ("hflip", "vflip"):
        if opts or "=" in f:
            raise Unsupported(f"{name} option {opts!r} (the filter takes none on the GPU path)")
        return 2 if name == "hflip" else 4
    d, pos = None, 0
    for p in opts.split(":") if opts else []:
        if "=" in p:
            k, v = p.split("=", 1)
        else:
            if pos >= 2:
                raise Unsupported(f"transpose option {p!r} (positional options are dir:passthrough)")
            k, v = ("dir", "passthrough")[pos], p
            pos += 1
        if k == "passthrough":
            if v != "none":
                raise Unsupported(f"transpose passthrough={v} (only passthrough=none is GPU-accelerated)")
        elif k == "dir":
            if v in TRANSPOSE_DIRS:
                d = TRANSPOSE_DIRS[v]
            elif v.isascii() and v.isdigit() and int(v) <= 3:
                d = int(v)
            else:
                raise Unsupported(f"transpose dir={v} (only 0..3 or cclock_flip, clock, cclock, clock_flip are "
                                  f"GPU-accelerated; 4..7 are the deprecated passthrough forms)")
        else:
            raise Unsupported(f"transpose option {k!r}")
    d = 0 if d is None else d          # vf_transpose's default dir is cclock_flip
    return 1 | ((d & 1) << 1) | ((d >> 1) << 2)


def compose_orient(filters: Sequence[str]) -> int:
    """The orientation a run of hflip / vflip / transpose filters composes to (0..7)."""
    o = 0
    for f in filters:
        o = orient_after(o, _parse_orient(f))
    return o


YADIF_MODES = {"send_frame": 0, "send_field": 1, "send_frame_nospatial": 2, "send_field_nospatial": 3}
YADIF_PARITIES = {"tff": 0, "bff": 1, "auto": -1}
YADIF_DEINTS = {"all": 0, "interlaced": 1}
# the deinterlacers that are named only to say that they run on the CPU
OTHER_DEINTERLACERS = ("bwdif", "w3fdif", "estdif", "kerndeint", "nnedi", "mcdeint", "fieldmatch", "pullup",
                       "yadif_cuda", "bwdif_cuda", "bwdif_vulkan", "deinterlace_vaapi", "deinterlace_qsv")


def _parse_yadif(f: str) -> dict:
    """`yadif[=mode[:parity[:deint]]]` -> {"mode": 0 | 2, "parity": -1 | 0 | 1}.  The field-rate
    modes and deint=interlaced are outside the profile."""
    name, _, opts = f.partition("=")
    vals = {"mode": 0, "parity": -1, "deint": 0}
    tables = {"mode": YADIF_MODES, "parity": YADIF_PARITIES, "deint": YADIF_DEINTS}
    order, pos = ("mode", "parity", "deint"), 0
    if "=" in f and not opts:
        raise Unsupported("yadif= without options")
    for p in opts.split(":") if opts else []:
        if "=" in p:
            k, v = p.split("=", 1)
        else:
            if pos >= len(order):
                raise Unsupported(f"yadif option {p!r} (positional options are mode:parity:deint)")
            k, v = order[pos], p
            pos += 1
        if k not in tables:
            raise Unsupported(f"yadif option {k!r}")
        if v in tables[k]:
            vals[k] = tables[k][v]
        elif v.lstrip("-").isascii() and v.lstrip("-").isdigit() and int(v) in tables[k].values():
            vals[k] = int(v)
        else:
            raise Unsupported(f"yadif {k}={v}")
    if vals["mode"] in (1, 3):
        raise Unsupported(f"yadif mode={vals['mode']} (field rate: one frame per field doubles the frame count and "
                          f"the rate; only modes 0 and 2 are GPU-accelerated)")
    if vals["deint"] != 0:
        raise Unsupported("yadif deint=interlaced (per-frame field flags; only deint=all is GPU-accelerated)")
    return {"mode": vals["mode"], "parity": vals["parity"]}


UNSHARP_KEYS = {"luma_msize_x": 0, "lx": 0, "luma_msize_y": 1, "ly": 1, "luma_amount": 2, "la": 2,
                "chroma_msize_x": 3, "cx": 3, "chroma_msize_y": 4, "cy": 4, "chroma_amount": 5, "ca": 5}
UNSHARP_NAMES = ("lx", "ly", "la", "cx", "cy", "ca")
UNSHARP_DEFAULT = (5, 5, 1.0, 5, 5, 0.0)
UNSHARP_MAX_HALF_SUM = 12   # 8 + 2 (sx + sy) <= 32: the filter's uint32_t sum
_INT_RE = re.compile(r"[+-]?\d+\Z")
_NUM_RE = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?\Z")


def unsharp_amount_i(amount: float) -> int:
    """The filter's integer amount: (int)(amount * 65536.0), C truncation."""
    return int(float(amount) * 65536.0)


def _parse_unsharp(f: str) -> tuple:
    """`unsharp[=lx:ly:la:cx:cy:ca]` -> (lx, ly, la, cx, cy, ca) with the defaults filled in."""
    name, _, opts = f.partition("=")
    vals = list(UNSHARP_DEFAULT)
    pos = 0
    if "=" in f and not opts:
        raise Unsupported("unsharp= without options")
    for p in opts.split(":") if opts else []:
        if "=" in p:
            k, v = p.split("=", 1)
            if k not in UNSHARP_KEYS:
                raise Unsupported(f"unsharp option {k!r} (only the luma and chroma sizes and amounts are "
                                  f"GPU-accelerated)")
            at = UNSHARP_KEYS[k]
        else:
            if pos >= len(UNSHARP_NAMES):
                raise Unsupported(f"unsharp option {p!r} (positional options are lx:ly:la:cx:cy:ca; the alpha "
                                  f"plane's are not GPU-accelerated)")
            at, v = pos, p
            pos += 1
        nm = UNSHARP_NAMES[at]
        if not (_NUM_RE if at in (2, 5) else _INT_RE).match(v):
            raise Unsupported(f"unsharp {nm}={v}: an expression or not a plain number (plain numbers only)")
        vals[at] = float(v) if at in (2, 5) else int(v)
    for at in (0, 1, 3, 4):
        if not 3 <= vals[at] <= 23:
            raise Unsupported(f"unsharp {UNSHARP_NAMES[at]}={vals[at]}: size outside 3..23")
        if not vals[at] & 1:
            raise Unsupported(f"unsharp {UNSHARP_NAMES[at]}={vals[at]}: even size (the filter takes odd sizes)")
    for at in (2, 5):
        if not -2.0 <= vals[at] <= 5.0:
            raise Unsupported(f"unsharp {UNSHARP_NAMES[at]}={vals[at]}: amount outside -2..5")
        hs = vals[at - 2] // 2 + vals[at - 1] // 2
        if unsharp_amount_i(vals[at]) and hs > UNSHARP_MAX_HALF_SUM:
            raise Unsupported(f"unsharp {'luma' if at == 2 else 'chroma'} {vals[at - 2]}x{vals[at - 1]}: sx + sy = {hs} > "
                              f"{UNSHARP_MAX_HALF_SUM}, the filter's 32-bit sum wraps (not GPU-accelerated)")
    return tuple(vals)


EQ_NAMES = ("contrast", "brightness", "saturation", "gamma", "gamma_r", "gamma_g", "gamma_b", "gamma_weight")
EQ_DEFAULT = {"contrast": 1.0, "brightness": 0.0, "saturation": 1.0, "gamma": 1.0, "gamma_r": 1.0, "gamma_g": 1.0,
              "gamma_b": 1.0, "gamma_weight": 1.0}
EQ_RANGES = {"contrast": (-1000.0, 1000.0), "brightness": (-1.0, 1.0), "saturation": (0.0, 3.0), "gamma": (0.1, 10.0),
             "gamma_r": (0.1, 10.0), "gamma_g": (0.1, 10.0), "gamma_b": (0.1, 10.0), "gamma_weight": (0.0, 1.0)}


def _parse_eq(f: str) -> dict:
    """`eq=contrast:brightness:saturation:gamma:gamma_r:gamma_g:gamma_b:gamma_weight` -> the eight
    numbers with the defaults filled in.  Plain numbers inside the filter's ranges only: FFmpeg clips a
    value outside its range, which is not restated here."""
    name, _, opts = f.partition("=")
    vals = dict(EQ_DEFAULT)
    pos = 0
    if "=" in f and not opts:
        raise Unsupported("eq= without options")
    for p in opts.split(":") if opts else []:
        if "=" in p:
            k, v = p.split("=", 1)
            if k == "eval":
                raise Unsupported(f"eq eval={v} (per-frame evaluation is not GPU-accelerated)")
            if k not in EQ_DEFAULT:
                raise Unsupported(f"eq option {k!r} (only contrast, brightness, saturation and the gammas are "
                                  f"GPU-accelerated)")
        else:
            if pos >= len(EQ_NAMES):
                raise Unsupported(f"eq option {p!r} (positional options are {':'.join(EQ_NAMES)})")
            k, v = EQ_NAMES[pos], p
            pos += 1
        if not _NUM_RE.match(v):
            raise Unsupported(f"eq {k}={v}: an expression or not a plain number (plain numbers only)")
        vals[k] = float(v)
        lo, hi = EQ_RANGES[k]
        if not lo <= vals[k] <= hi:
            raise Unsupported(f"eq {k}={v}: outside {lo:g}..{hi:g} (FFmpeg clips it; the clip is not GPU-accelerated)")
    return vals


def _c_div(a: int, b: int) -> int:
    """C integer division: truncates toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def eq_plane_table(C: float, B: float, G: float, W: float) -> list:
    """One plane's 256 bytes for contrast C, brightness B, gamma G and gamma weight W (doubles):
    vf_eq.c's 8-bit path as DESIGN §4.15 restates it."""
    import math
    if C == 1.0 and B == 0.0 and G == 1.0:
        return list(range(256))                    # the filter copies the plane
    out = []
    if G == 1.0 and abs(C) < 7.9:                  # the linear form: C ints, truncating conversions and division
        ci = int(C * 256 * 16)
        bi = _c_div(int(100.0 * B + 100.0) * 511, 200) - 128 - _c_div(ci, 32)
        for v in range(256):
            pel = ((v * ci) >> 12) + bi
            out.append(0 if pel < 0 else 255 if pel > 255 else pel)
        return out
    for v in range(256):                           # the table form
        x = C * (v / 255.0 - 0.5) + 0.5 + B
        if x <= 0.0:
            out.append(0)
            continue
        x = x * (1.0 - W) + math.pow(x, 1.0 / G) * W
        out.append(255 if x >= 1.0 else int(256.0 * x))
    return out


def eq_tables(spec: dict):
    """(3, 256) uint8, rows Y, U, V: the tables `-vf eq` with the options `spec` (EQ_NAMES; absent:
    the default) applies to 8-bit planar frames.  Every option goes through IEEE single first, as the
    filter's float clip does; the rest is double arithmetic."""
    import math
    import numpy as np
    o = {k: float(np.float32(spec.get(k, EQ_DEFAULT[k]))) for k in EQ_NAMES}
    W = o["gamma_weight"]
    planes = ((o["contrast"], o["brightness"], o["gamma"] * o["gamma_g"], W),
              (o["saturation"], 0.0, math.sqrt(o["gamma_b"] / o["gamma_g"]), W),
              (o["saturation"], 0.0, math.sqrt(o["gamma_r"] / o["gamma_g"]), W))
    return np.array([eq_plane_table(*p) for p in planes], np.uint8)


# luma weights (G, B, R) per colour space, and the other names of bt601
COLORMATRIX_LUMA = {"bt709": (0.7152, 0.0722, 0.2126), "fcc": (0.59, 0.11, 0.30), "bt601": (0.587, 0.114, 0.299),
                    "smpte240m": (0.701, 0.087, 0.212), "bt2020": (0.678, 0.0593, 0.2627)}
COLORMATRIX_ALIASES = {"bt470": "bt601", "bt470bg": "bt601", "smpte170m": "bt601"}


def _colormatrix_name(v: str) -> Optional[str]:
    v = COLORMATRIX_ALIASES.get(v, v)
    return v if v in COLORMATRIX_LUMA else None


def _yuv_matrix(name: str):
    g, b, r = COLORMATRIX_LUMA[name]
    bs, rs = 0.5 / (b - 1.0), 0.5 / (r - 1.0)
    return [[g, b, r], [bs * g, 0.5, bs * r], [rs * g, rs * b, 0.5]]


def _inverse3(m):
    (a, b, c), (d, e, f), (g, h, i) = m
    co = [[e * i - f * h, c * h - b * i, b * f - c * e],
          [f * g - d * i, a * i - c * g, c * d - a * f],
          [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * co[0][0] + b * co[1][0] + c * co[2][0]
    return [[v / det for v in row] for row in co]


def colormatrix_coefs(src: str, dst: str) -> Tuple[int, int, int, int, int, int]:
    """(c2, c3, c4, c5, c6, c7): the six 16.16 coefficients `-vf colormatrix=src:dst` applies to 8-bit
    planar frames, as DESIGN §4.16 restates vf_colormatrix.c: C = M_dst inverse(M_src) in double, each
    entry rounded half away from zero by the filter's NS(); the first column is always (65536, 0, 0)
    and is left out.  The names are COLORMATRIX_LUMA's and the other names of bt601."""
    import sys
    names = (_colormatrix_name(src), _colormatrix_name(dst))
    if None in names:
        raise ValueError(f"colormatrix {src}:{dst}: not two of {', '.join(COLORMATRIX_LUMA)}")
    md, inv = _yuv_matrix(names[1]), _inverse3(_yuv_matrix(names[0]))
    c = [[sum(md[i][k] * inv[k][j] for k in range(3)) for j in range(3)] for i in range(3)]

    def ns(n: float) -> int:
        return int(n * 65536.0 - 0.5 + sys.float_info.epsilon) if n < 0 else int(n * 65536.0 + 0.5)
    return (ns(c[0][1]), ns(c[0][2]), ns(c[1][1]), ns(c[1][2]), ns(c[2][1]), ns(c[2][2]))


def _parse_colormatrix(f: str) -> Tuple[str, str]:
    """`colormatrix=SRC:DST` (also src=, dst=, and mixed) -> the canonical (src, dst)."""
    _, _, opts = f.partition("=")
    vals = {}
    pos = 0
    for p in opts.split(":") if opts else []:
        if "=" in p:
            k, v = p.split("=", 1)
            if k not in ("src", "dst"):
                raise Unsupported(f"colormatrix option {k!r} (only src and dst are GPU-accelerated)")
        else:
            if pos >= 2:
                raise Unsupported(f"colormatrix option {p!r} (positional options are src:dst)")
            k, v = ("src", "dst")[pos], p
            pos += 1
        name = _colormatrix_name(v)
        if name is None:
            raise Unsupported(f"colormatrix {k}={v}: not one of {', '.join(list(COLORMATRIX_LUMA) + list(COLORMATRIX_ALIASES))}")
        vals[k] = name
    if "dst" not in vals:
        raise Unsupported(f"colormatrix without a dst ({f!r}: the filter needs one)")
    if "src" not in vals:
        raise Unsupported(f"colormatrix without a src ({f!r}: FFmpeg takes it from the frame's metadata, which is not "
                          f"GPU-accelerated)")
    if vals["src"] == vals["dst"]:
        raise Unsupported(f"colormatrix src and dst are both {vals['src']} ({f!r}: FFmpeg refuses it)")
    return vals["src"], vals["dst"]


# The graph layer.  parse_graph splits a -vf value once into (name, text) filters; every stage below
# takes its filter or filters off that list (`fs`, never empty when a stage gets it) and writes its
# own field of `out`.  A reason that quotes "the graph" quotes what is on the list at that stage.

def _names(fs) -> List[str]:
    return [name for name, _ in fs]


def _graph(fs) -> str:
    return ",".join(text for _, text in fs)


def _in_front(name: str) -> bool:
    """A filter whose place is in front of the colormatrix and the eq (or that refuses the graph)."""
    return name == "yadif" or name in ORIENT_FILTERS or name in OTHER_DEINTERLACERS or name == "hflip"


TILE_OPTIONS = ("layout", "nb_frames", "margin", "padding", "color", "overlap", "init_padding")
_DEC_RE = re.compile(r"\d+\Z")


def _parse_tile(f: str) -> dict:
    """`tile[=layout:nb_frames:margin:padding:color:overlap:init_padding]`, positional in that order or by
    name -> {"cols", "rows", "nb_frames", "margin", "padding"} (vf_tile.c's defaults: 6x5, 0 = cols * rows,
    0, 0).  Unsupported for what the GPU path does not do (a colour other than black, overlap, init_padding,
    expressions) and for what FFmpeg itself rejects."""
    vals = {"layout": "6x5", "nb_frames": "0", "margin": "0", "padding": "0", "color": "black", "overlap": "0",
            "init_padding": "0"}
    pos = 0
    for part in (f.split("=", 1)[1].split(":") if "=" in f else []):
        if "=" in part:
            k, v = part.split("=", 1)
            if k not in vals:
                raise Unsupported(f"tile option {k!r}")
            pos = len(TILE_OPTIONS)      # (a positional value behind a named one: FFmpeg refuses it)
        else:
            if pos >= len(TILE_OPTIONS):
                raise Unsupported(f"tile {f!r}: a positional value behind a named one, or too many")
            k, v = TILE_OPTIONS[pos], part
            pos += 1
        vals[k] = v
    m = re.match(r"(\d+)x(\d+)\Z", vals["layout"])
    if not m:
        raise Unsupported(f"tile layout {vals['layout']!r}: not COLSxROWS in decimal integers (expressions are not "
                          f"GPU-accelerated)")
    cols, rows = int(m.group(1)), int(m.group(2))
    num = {}
    for k in ("nb_frames", "margin", "padding", "overlap", "init_padding"):
        if not _DEC_RE.match(vals[k]):
            raise Unsupported(f"tile {k} {vals[k]!r}: not a decimal integer of 0 or more (expressions are not "
                              f"GPU-accelerated; FFmpeg rejects a negative value)")
        num[k] = int(vals[k])
    if vals["color"].lower() != "black":
        raise Unsupported(f"tile color {vals['color']!r} (only black is GPU-accelerated)")
    if num["overlap"]:
        raise Unsupported(f"tile overlap {num['overlap']} (only overlap 0 is GPU-accelerated)")
    if num["init_padding"]:
        raise Unsupported(f"tile init_padding {num['init_padding']} (only init_padding 0 is GPU-accelerated)")
    if cols < 1 or rows < 1:
        raise Unsupported(f"tile layout {cols}x{rows}: FFmpeg rejects a layout below 1x1")
    if num["nb_frames"] > cols * rows:
        raise Unsupported(f"tile nb_frames {num['nb_frames']}: FFmpeg rejects more frames than the {cols}x{rows} "
                          f"layout has cells")
    return {"cols": cols, "rows": rows, "nb_frames": num["nb_frames"], "margin": num["margin"], "padding": num["padding"]}


def _parse_framestep(f: str) -> int:
    """`framestep=N` / `framestep=step=N` -> N (vf_framestep.c: step, 1 or more; the default is 1)."""
    v = f.split("=", 1)[1] if "=" in f else "1"
    if v.startswith("step="):
        v = v[len("step="):]
    if not _DEC_RE.match(v):
        raise Unsupported(f"framestep {v!r}: not a decimal integer (expressions are not GPU-accelerated)")
    if int(v) < 1:
        raise Unsupported(f"framestep {v}: FFmpeg rejects a step below 1")
    return int(v)


def _parse_thumbnail(f: str) -> int:
    """`thumbnail` / `thumbnail=N` / `thumbnail=n=N` -> N (vf_thumbnail.c: n, 2 or more; the default is 100)."""
    n = str(THUMBNAIL_DEFAULT)
    for at, part in enumerate(f.split("=", 1)[1].split(":") if "=" in f else []):
        if "=" in part:
            k, v = part.split("=", 1)
            if k != "n":
                raise Unsupported(f"thumbnail option {k!r} (only n is GPU-accelerated)")
        elif at:
            raise Unsupported(f"thumbnail {f!r}: more than one positional value")
        else:
            v = part
        n = v
    if not _DEC_RE.match(n):
        raise Unsupported(f"thumbnail {n!r}: not a decimal integer (expressions are not GPU-accelerated)")
    if int(n) < 2:
        raise Unsupported(f"thumbnail {n}: FFmpeg rejects a group below 2 frames")
    return int(n)


def thumbnail_pick(hists) -> int:
    """vf_thumbnail.c's selection among the n frames of a group: `hists` is n rows of 768
    counters, and the pick is the first frame whose sum of squared differences from the mean row is smallest.
    Python floats are C doubles, and the order is the filter's: the mean column by column, each a sum over
    the frames in order divided by n; then per frame a sequential sum over j = 0..767 of d * d with d = avg[j] -
    hist[i][j]; a strict `<`, so ties go to the earliest frame (n = 2: both errors are equal, frame 0)."""
    rows = [[float(v) for v in h] for h in hists]
    n = len(rows)
    if not n:
        raise ValueError("thumbnail_pick: no frame")
    avg = []
    for j in range(len(rows[0])):
        a = 0.0
        for i in range(n):
            a += rows[i][j]
        avg.append(a / n)
    best, best_e = 0, 0.0
    for i in range(n):
        e = 0.0
        row = rows[i]
        for j in range(len(avg)):
            d = avg[j] - row[j]
            e += d * d
        if i == 0 or e < best_e:
            best, best_e = i, e
    return best


def _take_sheet(fs, out):
    """A framestep as the very first filter, a thumbnail as the first or directly behind that framestep, and
    a tile as the very last one, taken off before the other stages see the list.  A graph that names none of
    them is left exactly as it is."""
    names = _names(fs)
    if "tile" not in names and "framestep" not in names and "thumbnail" not in names:
        return
    vf = _graph(fs)
    if "thumbnail" in names:
        at = names.index("thumbnail")
        if names.count("thumbnail") > 1:
            raise Unsupported(f"filter graph {vf!r}: a second thumbnail (one thumbnail, in front, is GPU-accelerated)")
        if at and not (at == 1 and names[0] == "framestep"):
            raise Unsupported(f"filter graph {vf!r}: thumbnail after {names[at - 1]} (thumbnail is GPU-accelerated only as "
                              f"the first filter, or directly behind a leading framestep)")
        if "yadif" in names:
            raise Unsupported(f"filter graph {vf!r}: thumbnail together with yadif (the deinterlacer would need the "
                              f"dropped frames' neighbours)")
        if names[-1] != "tile":
            raise Unsupported(f"filter graph {vf!r}: thumbnail without a tile as the last filter (thumbnail keeps its "
                              f"link's frame rate and emits sparse timestamps, which MkvWriter does not write)")
    if "framestep" in names:
        if names.count("framestep") > 1:
            raise Unsupported(f"filter graph {vf!r}: a second framestep (one framestep, as the first filter, is "
                              f"GPU-accelerated)")
        if names[0] != "framestep":
            at = names.index("framestep")
            raise Unsupported(f"filter graph {vf!r}: framestep after {names[at - 1]} (framestep is GPU-accelerated only "
                              f"as the first filter)")
        if "yadif" in names:
            raise Unsupported(f"filter graph {vf!r}: framestep together with yadif (the deinterlacer would need the "
                              f"dropped frames' neighbours)")
    if "tile" in names:
        if names.count("tile") > 1:
            raise Unsupported(f"filter graph {vf!r}: a second tile (one tile, as the last filter, is GPU-accelerated)")
        if names[-1] != "tile":
            raise Unsupported(f"filter graph {vf!r}: tile is not the last filter (tile is GPU-accelerated only as the "
                              f"last filter)")
        if "pad" in names:
            raise Unsupported(f"filter graph {vf!r}: tile in a graph with pad (tile behind a pad is not GPU-accelerated)")
    if names[0] == "framestep":
        step = _parse_framestep(fs.pop(0)[1])
        if step > 1:
            out["framestep"] = step
    if fs and fs[0][0] == "thumbnail":
        out["thumbnail"] = _parse_thumbnail(fs.pop(0)[1])
    if fs and fs[-1][0] == "tile":
        out["tile"] = _parse_tile(fs.pop()[1])


HQDN3D_KEYS = {"luma_spatial": "ls", "chroma_spatial": "cs", "luma_tmp": "lt", "chroma_tmp": "ct"}
HQDN3D_NAMES = ("ls", "cs", "lt", "ct")


def _parse_hqdn3d(f: str) -> dict:
    """`hqdn3d[=luma_spatial[:chroma_spatial[:luma_tmp[:chroma_tmp]]]]`, positional in that order or by those
    names -> {"ls", "cs", "lt", "ct"}, resolved as vf_hqdn3d.c's init does: a value that is missing or 0 is
    replaced, in this order, by 4.0, 3 ls / 4, 6 ls / 4 and lt cs / ls.  Plain non-negative numbers only."""
    vals = dict.fromkeys(HQDN3D_NAMES, 0.0)
    if "=" in f:
        body = f.split("=", 1)[1]
        if not body:
            raise Unsupported("hqdn3d= without options")
        pos = 0
        for p in body.split(":"):
            if "=" in p:
                k, v = p.split("=", 1)
                if k not in HQDN3D_KEYS:
                    raise Unsupported(f"hqdn3d option {k!r} (luma_spatial, chroma_spatial, luma_tmp and chroma_tmp are "
                                      f"GPU-accelerated)")
                k = HQDN3D_KEYS[k]
            else:
                if pos >= 4:
                    raise Unsupported(f"hqdn3d option {p!r}: more than four positional values "
                                      f"(luma_spatial:chroma_spatial:luma_tmp:chroma_tmp)")
                k, v = HQDN3D_NAMES[pos], p
                pos += 1
            if not _NUM_RE.match(v):
                raise Unsupported(f"hqdn3d {k}={v!r} (plain numbers only: expressions are not GPU-accelerated)")
            if float(v) < 0:
                raise Unsupported(f"hqdn3d {k}={v}: a negative strength")
            vals[k] = float(v)
    ls = vals["ls"] or 4.0
    cs = vals["cs"] or 3.0 * ls / 4.0
    lt = vals["lt"] or 6.0 * ls / 4.0
    ct = vals["ct"] or lt * cs / ls
    return {"ls": ls, "cs": cs, "lt": lt, "ct": ct}


def hqdn3d_table(s: float) -> list:
    """One strength's table, 8192 ints (int16), in Python floats as vf_hqdn3d.c's precalc_coefs computes it in C
    doubles: tab[4096 + i] = lrint(pow(max(0, 1 - |f| / 255), gamma) * 256 f) with f = ((i << 5) + 15) / 512 and
    gamma = log(0.25) / log(1 - min(s, 252) / 255 - 0.00001); tab[0] = 1, the filter's own flag, which no
    input reaches."""
    gamma = math.log(0.25) / math.log(1.0 - min(s, 252.0) / 255.0 - 0.00001)
    tab = [0] * 8192
    for i in range(-4096, 4096):
        f = ((i << 5) + 15) / 512.0
        tab[4096 + i] = round(math.pow(max(0.0, 1.0 - abs(f) / 255.0), gamma) * 256.0 * f)   # ties to even, as lrint
    tab[0] = 1
    return tab


def hqdn3d_tables(spec: dict):
    """The four tables of a resolved request ({"ls", "cs", "lt", "ct"}): a (4, 8192) int16 array, rows luma
    spatial, chroma spatial, luma temporal, chroma temporal (mjg_denoise's order).  A restatement that is
    unpinned against FFmpeg."""
    import numpy as np
    return np.array([hqdn3d_table(float(spec[k])) for k in HQDN3D_NAMES], np.int16)


def _take_denoise(fs, out):
    """One hqdn3d as the very first filter, or directly behind a leading yadif, taken off behind _take_sheet
    (whose framestep, thumbnail and tile refuse the graph here) and before the other stages see the list.  A
    graph that does not name it is left exactly as it is."""
    names = _names(fs)
    if "hqdn3d" not in names:
        return
    vf = _graph(fs)
    for nm in ("framestep", "thumbnail", "tile"):
        if nm in out:
            raise Unsupported(f"filter graph with {vf!r}: hqdn3d together with {nm} (the time scan needs every frame, and "
                              f"a denoiser context has no contact sheet)")
    if names.count("hqdn3d") > 1:
        raise Unsupported(f"filter graph {vf!r}: a second hqdn3d (one hqdn3d, in front, is GPU-accelerated)")
    at = names.index("hqdn3d")
    if at and not (at == 1 and names[0] == "yadif"):
        raise Unsupported(f"filter graph {vf!r}: hqdn3d after {names[at - 1]} (hqdn3d is GPU-accelerated only as the "
                          f"first filter, or directly behind a leading yadif)")
    if at == 0 and "yadif" in names:
        raise Unsupported(f"filter graph {vf!r}: yadif after hqdn3d (the deinterlacer runs in front of the denoiser: only "
                          f"yadif,hqdn3d in this order is GPU-accelerated)")
    out["hqdn3d"] = _parse_hqdn3d(fs.pop(at)[1])


def _take_colormatrix(fs, out):
    """One colormatrix, behind the yadif and the orientation run, in front of any eq and of the scale
    (without a scale: in front of the unsharp and the pad); before or after the crop, with which it
    commutes (crop offsets are multiples of the sub-sampling)."""
    names = _names(fs)
    if "colormatrix" not in names:
        return
    if names.count("colormatrix") > 1:
        raise Unsupported(f"filter graph {_graph(fs)!r}: a second colormatrix (one colormatrix, in front of the eq and "
                          f"the scale, is GPU-accelerated)")
    at = names.index("colormatrix")
    for nm in names[at + 1:]:
        if _in_front(nm):
            raise Unsupported(f"filter graph {_graph(fs)!r}: colormatrix in front of {nm} (colormatrix is GPU-accelerated "
                              f"only behind the yadif and the orientation run)")
    for nm in ("eq", "scale", "unsharp", "pad"):
        if nm in names[:at]:
            raise Unsupported(f"filter graph {_graph(fs)!r}: colormatrix behind the {nm} (colormatrix is GPU-accelerated "
                              f"only in front of the eq, the scale, the unsharp and the pad)")
    out["colormatrix"] = _parse_colormatrix(fs.pop(at)[1])


def _take_eq(fs, out):
    """One eq, behind the yadif and the orientation run: slot "in" anywhere in front of the scale
    (without a scale: in front of the unsharp and the pad), slot "out" directly behind the scale."""
    names = _names(fs)
    if "eq" not in names:
        return
    if names.count("eq") > 1:
        raise Unsupported(f"filter graph {_graph(fs)!r}: a second eq (one eq, in front of the scale or directly behind "
                          f"it, is GPU-accelerated)")
    at = names.index("eq")
    if any(_in_front(nm) for nm in names[at + 1:]):
        # "yadif after eq", "vflip after eq", ...: the eq stays on the list, and the stage that owns the
        # filter behind it refuses the graph (at the latest _take_crop_scale, which knows no eq)
        return
    for nm in ("unsharp", "pad"):
        if nm in names[:at]:
            raise Unsupported(f"filter graph {_graph(fs)!r}: eq behind the {nm} (eq is GPU-accelerated only in front of "
                              f"the scale or directly behind it, in front of the unsharp and the pad)")
    slot = "in"
    if "scale" in names:
        si = names.index("scale")
        if at > si + 1:
            raise Unsupported(f"filter graph {_graph(fs)!r}: eq behind {names[at - 1]} (behind the scale, eq is "
                              f"GPU-accelerated only directly behind it)")
        slot = "in" if at < si else "out"
    out["eq"] = dict(_parse_eq(fs.pop(at)[1]), slot=slot)


def _take_deint(fs, out):
    """A yadif as the very first filter; any other deinterlacer refuses the graph."""
    names = _names(fs)
    other = [nm for nm in names if nm in OTHER_DEINTERLACERS]
    if other:
        raise Unsupported(f"filter graph {_graph(fs)!r}: {other[0]} is not GPU-accelerated (of the deinterlacers only "
                          f"yadif is)")
    if "yadif" in names[1:]:
        at = 1 + names[1:].index("yadif")
        raise Unsupported(f"filter graph {_graph(fs)!r}: yadif after {names[at - 1]} (yadif is GPU-accelerated only as "
                          f"the first filter)")
    if names[0] == "yadif":
        out["deint"] = _parse_yadif(fs.pop(0)[1])


def _take_orient(fs, out):
    """A leading run of vflip / transpose filters, composed; the limits on the number and order of
    filters apply to what follows."""
    names = _names(fs)
    n = 0
    while n < len(fs) and names[n] in ORIENT_FILTERS:
        n += 1
    late = [nm for nm in names[n:] if nm in ORIENT_FILTERS]
    if late:
        raise Unsupported(f"filter graph {_graph(fs)!r}: {len(fs)} filters, {late[0]} after {names[n]} (vflip and "
                          f"transpose are GPU-accelerated only in front of [crop,][scale,][pad])")
    if n and "hflip" in names:
        raise Unsupported(f"filter graph {_graph(fs)!r}: hflip is not GPU-accelerated (of the orientation filters only "
                          f"vflip and transpose are)")
    if n:
        out["orient"] = compose_orient(text for _, text in fs[:n])
        del fs[:n]


def _take_pad_unsharp(fs, out):
    """The end of the graph, [unsharp][,pad]: the pad is taken off, then the unsharp, which must be
    the last of what is left.  One stage for the two, because a graph that names unsharp is checked
    for a second one before its pad is looked at, and quotes the graph with the pad still on it.  A
    pad that is not taken (without options, or behind more than two filters of a graph without
    unsharp) stays on the list for _take_crop_scale to refuse."""
    names, vf = _names(fs), _graph(fs)
    sharp = "unsharp" in names
    if names.count("unsharp") > 1:
        raise Unsupported(f"filter graph {vf!r}: a second unsharp (one unsharp, directly in front of the pad or the "
                          f"end, is GPU-accelerated)")
    if "pad" in names[:-1]:
        raise Unsupported(f"filter graph {vf!r}: pad is not the last filter (only [crop,][scale,]"
                          f"{'[unsharp,]' if sharp else ''}pad in this order is GPU-accelerated)")
    if names[-1] == "pad":
        if "=" in fs[-1][1]:
            if sharp or len(fs) <= 3:
                out["pad"] = _parse_pad(fs.pop()[1])
        elif sharp:
            raise Unsupported(f"filter graph {vf!r}: pad without options")
    if sharp:
        names = _names(fs)
        if names[-1] != "unsharp":
            at = names.index("unsharp")
            raise Unsupported(f"filter graph {vf!r}: unsharp before {names[at + 1]} (unsharp is GPU-accelerated only "
                              f"behind [crop,][scale] and directly in front of the pad or the end)")
        out["unsharp"] = _parse_unsharp(fs.pop()[1])


def _take_crop_scale(fs, out):
    """[crop][,scale]: all that may be left, so this stage takes the whole list or refuses it."""
    names, vf = _names(fs), _graph(fs)
    if len(fs) > 2:
        raise Unsupported(f"filter graph {vf!r}: {len(fs)} filters (only crop, scale or crop,scale is "
                          f"GPU-accelerated)")
    if names == ["scale", "crop"]:
        raise Unsupported(f"filter graph {vf!r}: scale before crop (only crop,scale in this order is "
                          f"GPU-accelerated)")
    if names in (["crop"], ["crop", "scale"]) and "=" in fs[0][1]:
        if len(fs) == 2:
            out["scale"], out["sws_flags"] = _parse_scale(fs[1][1])
        out["crop"] = _parse_crop(fs[0][1])
    elif len(fs) == 1:
        out["scale"], out["sws_flags"] = _parse_scale(vf)
    else:
        raise Unsupported(f"filter graph {vf!r} (only crop, scale or crop,scale is GPU-accelerated)")
    del fs[:]


# in this order, which decides the reason a graph outside the profile is refused with
GRAPH_STAGES = (_take_sheet, _take_denoise, _take_colormatrix, _take_eq, _take_deint, _take_orient, _take_pad_unsharp, _take_crop_scale)


def parse_graph(vf: str) -> dict:
    """A -vf value -> the chain fields of Profile that the graph sets, by name (crop, scale,
    sws_flags, pad, orient, deint, unsharp, eq, colormatrix, SheetProfile's tile and framestep, ThumbProfile's
    thumbnail and DenoiseProfile's hqdn3d; a field
    the graph does not set is left out, so Profile's own defaults are the only ones), or Unsupported."""
    if ";" in vf:
        raise Unsupported(f"filter graph {vf!r} (only crop, scale or crop,scale is GPU-accelerated)")
    fs = [(f.split("=", 1)[0], f) for f in vf.split(",")]
    out: dict = {}
    for take in GRAPH_STAGES:
        if not fs:
            break
        take(fs, out)
    return out


def resolve_crop(spec: dict, in_w: int, in_h: int, src_chroma: str) -> Tuple[int, int, int, int]:
    """The rectangle (x, y, w, h) a crop request selects from an in_w x in_h input in
    `src_chroma` ("420"/"422"/"444": the decoded format, which the filter sees before any
    -pix_fmt conversion), as vf_crop.c config_input / filter_frame do with exact=0: absent w / h
    are the input's, both rounded down to the chroma sub-sampling; absent x / y centre the
    rectangle, given ones are clamped into the frame, both then rounded down alike.  A size
    below 1 or beyond the input raises CropError (ffmpeg fails; nothing is passed through)."""
    hs, vs = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[str(src_chroma)]
    w = in_w if spec.get("w") is None else int(spec["w"])
    h = in_h if spec.get("h") is None else int(spec["h"])
    w &= ~((1 << hs) - 1)
    h &= ~((1 << vs) - 1)
    if w < 1 or h < 1 or w > in_w or h > in_h:
        raise CropError(f"Invalid too big or non positive size for width '{w}' or height '{h}' "
                        f"(crop of a {in_w}x{in_h} input)")
    x = (in_w - w) // 2 if spec.get("x") is None else max(0, min(int(spec["x"]), in_w - w))
    y = (in_h - h) // 2 if spec.get("y") is None else max(0, min(int(spec["y"]), in_h - h))
    x &= ~((1 << hs) - 1)
    y &= ~((1 << vs) - 1)
    return x, y, w, h


def _parse_scale(vf: str) -> Tuple[Tuple[int, int], Tuple[str, ...]]:
    if "," in vf or ";" in vf or not vf.startswith("scale="):
        raise Unsupported(f"filter graph {vf!r} (only crop, scale or crop,scale is GPU-accelerated)")
    parts = vf[len("scale="):].split(":")
    kv, pos = {}, []
    for p in parts:
        if "=" in p:
            k, v = p.split("=", 1)
            kv[k] = v
        else:
            pos.append(p)
    w = kv.pop("w", kv.pop("width", pos[0] if len(pos) > 0 else None))
    h = kv.pop("h", kv.pop("height", pos[1] if len(pos) > 1 else None))
    flags = tuple(f for f in kv.pop("flags", "bicubic").replace("+", " ").split() if f)
    if kv:
        raise Unsupported(f"scale options {sorted(kv)}")
    try:
        W, H = int(w), int(h)
    except (TypeError, ValueError):
        raise Unsupported(f"scale size {w}:{h} (explicit positive W:H required)")
    if W <= 0 or H <= 0:
        raise Unsupported(f"scale size {W}:{H}")
    if not flags or flags[0] != "bicubic" or any(f not in _FLAGS_OK for f in flags):
        raise Unsupported(f"scale flags {flags}")
    return (W, H), flags


def _flag_ops(v: str) -> List[Tuple[str, str]]:
    """An AVOption flags string (`+a-b`, `a+b`, `a`) as (op, name) pairs; op '' replaces the
    whole set (libavutil opt.c set_string_flags: a leading name without +/- starts from 0)."""
    out, op, name = [], "", ""
    for ch in v:
        if ch in "+-":
            if name:
                out.append((op, name))
            op, name = ch, ""
        else:
            name += ch
    if name:
        out.append((op, name))
    if not out:
        raise Unsupported(f"flags {v!r}")
    return out


def _apply_flag(cur: bool, ops: List[Tuple[str, str]]) -> bool:
    for op, _ in ops:
        cur = op != "-"
    return cur


def parse(args: Union[str, Sequence[str]]) -> Profile:
    """Profile for `remote_args`, or raise Unsupported(reason)."""
    a: List[str] = shlex.split(args) if isinstance(args, str) else list(args)
    codec = q = dct = huff = None
    bitexact = False
    slices = 0
    threads: Optional[int] = None     # None: auto (0)
    thread_type = "slice+frame"       # AVCodecContext default: FF_THREAD_FRAME | FF_THREAD_SLICE
    chroma = None
    chain: dict = {}                  # the chain fields the last -vf sets (parse_graph)
    i = 0

    def val():
        nonlocal i
        if i + 1 >= len(a):
            raise Unsupported(f"{a[i]} without a value")
        i += 1
        return a[i]

    while i < len(a):
        o = a[i]
        if o in ("-c:v", "-codec:v", "-vcodec", "-c", "-codec"):
            codec = val()
        elif o in ("-q:v", "-qscale:v", "-q", "-qscale"):
            try:
                q = float(val())
            except ValueError:
                raise Unsupported(f"{o} {a[i]}")
        elif o == "-dct":
            dct = val()
        elif o == "-huffman":
            huff = val()
        elif o == "-bitexact":
            bitexact = True
        elif o in ("-flags", "-flags:v"):
            # AVCodecContext.flags: the only codec flag on the GPU path is bitexact; any other
            # (+gray, +qscale, ...) changes the bitstream, so it is not accepted silently
            v = val()
            ops = _flag_ops(v)
            if any(name != "bitexact" for _, name in ops):
                raise Unsupported(f"{o} {v} (only bitexact is GPU-accelerated)")
            bitexact = _apply_flag(bitexact, ops)
        elif o == "-fflags":
            # AVFormatContext.fflags: a muxer flag (format-level bitexact, no Lavf version
            # strings); it never reaches the encoder, so it does not count as codec bitexact
            v = val()
            if any(name != "bitexact" for _, name in _flag_ops(v)):
                raise Unsupported(f"-fflags {v}")
        elif o in ("-vf", "-filter:v"):
            chain = parse_graph(val())   # FFmpeg applies only the last -vf of a stream: all of an earlier one goes
        elif o in ("-an", "-sn", "-dn", "-y"):
            pass
        elif o in ("-threads", "-threads:v"):
            v = val()
            try:
                threads = None if v == "auto" else int(v)
            except ValueError:
                raise Unsupported(f"{o} {v}")
            if threads == 0:
                threads = None
        elif o in ("-thread_type", "-thread_type:v"):
            thread_type = val()
            if any(t not in ("slice", "frame") for t in thread_type.split("+")):
                raise Unsupported(f"-thread_type {thread_type}")
        elif o in ("-slices", "-slices:v"):
            try:
                slices = int(val())
            except ValueError:
                raise Unsupported(f"-slices {a[i]}")
        elif o in ("-pix_fmt", "-pix_fmt:v"):
            pf = val()
            if pf not in PIX_FMT_CHROMA:
                raise Unsupported(f"-pix_fmt {pf} (GPU path writes yuvj420p/422p/444p)")
            chroma = PIX_FMT_CHROMA[pf]
        elif o == "-f":
            if val() != "matroska":
                raise Unsupported(f"-f {a[i]}")
        elif o == "-map":
            if val() not in ("0:v", "0:v:0", "0"):
                raise Unsupported(f"-map {a[i]}")
        else:
            raise Unsupported(f"option {o}")
        i += 1
    if codec != "mjpeg":
        raise Unsupported(f"codec {codec!r}")
    if q is None:
        raise Unsupported("no -q:v (rate control modes are not GPU-accelerated)")
    if dct != "int":
        raise Unsupported(f"-dct {dct!r} (only the integer jfdctint is bit-exact reproducible)")
    if huff is None:
        huff = "optimal"  # mjpegenc.c: the "huffman" AVOption defaults to HUFFMAN_TABLE_OPTIMAL
    if huff not in ("default", "optimal"):
        raise Unsupported(f"-huffman {huff!r}")
    if not bitexact:
        raise Unsupported("no -bitexact (the Lavc COM segment is build-specific)")
    rst = uses_slices(slices, threads, thread_type)
    if rst:
        huff = "default"  # mjpegenc.c: slice_context_count > 1 forces HUFFMAN_TABLE_DEFAULT
    # (a SheetProfile exactly when the winning graph names a tile or a framestep above 1)
    # (and a ThumbProfile exactly when it names a thumbnail)
    # (and a DenoiseProfile exactly when it names a hqdn3d, which goes with none of the three)
    cls = (DenoiseProfile if "hqdn3d" in chain else ThumbProfile if "thumbnail" in chain
           else SheetProfile if "tile" in chain or "framestep" in chain else Profile)
    return cls(qscale=effective_qscale(q), q_arg=q, huffman=huff, rst=rst, chroma=chroma, **chain)


PIX_FMT_CHROMA = {"yuvj420p": "420", "yuvj422p": "422", "yuvj444p": "444"}


def uses_slices(slices: int, threads: Optional[int], thread_type: str) -> bool:
    """Whether the mjpeg encoder runs with slice_context_count > 1 (mpegvideo.c
    ff_mpv_init_context: nb_slices = -slices if set, else the thread count when slice
    threading is active; the frame-threading encoder, preferred whenever "frame" is in
    -thread_type, gives each frame a single-threaded context).  The layout then does not
    depend on the slice count (a restart interval per MCU row either way); -threads auto
    counts as more than one thread.  A one-MCU-row picture still gets no RST (the slice
    count is clipped to mb_height), which the encoder handles."""
    if slices:
        return slices > 1
    if threads == 1:
        return False
    return "frame" not in thread_type.split("+")


def av_reduce(num: int, den: int, max_v: int) -> Tuple[int, int]:
    """libavutil av_reduce: the best rational approximation of num/den with both terms
    <= max_v (continued-fraction convergents, then the best semiconvergent)."""
    a0n, a0d, a1n, a1d = 0, 1, 1, 0
    sign = (num < 0) != (den < 0)
    num, den = abs(num), abs(den)
    g = gcd(num, den)
    if g:
        num, den = num // g, den // g
    if num <= max_v and den <= max_v:
        a1n, a1d, den = num, den, 0
    while den:
        x = num // den
        next_den = num - den * x
        a2n, a2d = x * a1n + a0n, x * a1d + a0d
        if a2n > max_v or a2d > max_v:
            if a1n:
                x = (max_v - a0n) // a1n
            if a1d:
                x = min(x, (max_v - a0d) // a1d)
            if den * (2 * x * a1d + a0d) > num * a1d:
                a1n, a1d = x * a1n + a0n, x * a1d + a0d
            break
        a0n, a0d, a1n, a1d = a1n, a1d, a2n, a2d
        num, den = den, next_den
    return (-a1n if sign else a1n), a1d


def scaled_sar(sar: Tuple[int, int], src: Tuple[int, int], dst: Tuple[int, int]) -> Tuple[int, int]:
    """Sample aspect ratio after the scale filter (vf_scale config_props: an unknown SAR
    stays unknown, otherwise SAR * (out_h*in_w)/(out_w*in_h), reduced), then the 16-bit
    reduction the JFIF APP0 writer applies (mjpegenc_common.c jpeg_put_comments)."""
    if sar[0] <= 0 or sar[1] <= 0:
        return (0, 0)
    n, d = av_reduce(dst[1] * src[0] * sar[0], dst[0] * src[1] * sar[1], 2**31 - 1)
    if n > 65535 or d > 65535:
        n, d = av_reduce(n, d, 65535)
    return n, d


def try_parse(args) -> Tuple[Optional[Profile], Optional[str]]:
    try:
        return parse(args), None
    except Unsupported as e:
        return None, str(e)
