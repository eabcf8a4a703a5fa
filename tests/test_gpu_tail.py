"""The stuffing tail alone on the GPU (k_scan_bits / k_scan_bits_seg, k_count_ff, k_scan_ff, k_write
through mjg_debug_tail: the submit's launches on chunks the test chooses) against the plain
reference tests/tail_ref.py, on the layouts of tests/tail_layouts.py: every start bit and last-word
bit count of a chunk, chunks ending in lane 63 and at a window's last word, slots filled to the
last bit and lengths past them, scans that carry (groups, segments, frames, chunks), 0xFF bytes
wherever a word, a round, a window or the padding can put them.  A picture reaches these by chance;
here each is built.  Everything is compared exactly: the frame offsets, every byte of every frame,
and every byte behind the last frame (the buffer is 0xA5 before k_write and has a guard past its
capacity).  Every layout runs with the scratch buffer's other words 0 and all ones: a load of a
word k_encode would not have written must never reach the output."""
import ctypes as C

import numpy as np
import pytest

import tail_layouts
import tail_ref
from ffmpeg_distributed_amd import _lib
from tail_layouts import G

pytestmark = pytest.mark.gpu

GUARD = _lib.MJG_TAIL_GUARD
_ref_cache = {}


def reference(lay):
    """The reference frames of a layout (computed once; read only)."""
    if lay.name not in _ref_cache:
        _ref_cache[lay.name] = [tail_ref.frame(header(lay, f), [lay.segment(f * lay.nseg + si) for si in range(lay.nseg)])
                                for f in range(lay.nframes)]
    return _ref_cache[lay.name]


def header(lay, f):
    if not lay.optimal:
        return lay.hdr
    pos, end, dht, nval = lay.optimal
    return tail_ref.optimal_header(lay.hdr, pos, end, dht[f], nval[f])


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def run_tail(lay, fill, out_cap):
    """mjg_debug_tail on the layout: (out bytes with the guard, frame_offsets, group_ff, status)."""
    L = _lib.load()
    bits = np.ascontiguousarray(lay.lengths, np.uint32)
    words = lay.words()
    hdr = np.frombuffer(lay.hdr, np.uint8)
    job = _lib.MjgTailJob(nframes=lay.nframes, nseg=lay.nseg, nchunks=lay.nchunks, chunk_bits=_ptr(bits, C.c_uint32),
                          words=_ptr(words, C.c_uint32), fill=fill, hdr=_ptr(hdr, C.c_uint8), hdr_len=len(hdr),
                          out_cap=out_cap)
    if lay.optimal:
        pos, end, dht, nval = lay.optimal
        dht, nval = np.ascontiguousarray(dht, np.uint8), np.ascontiguousarray(nval, np.uint32)
        job.dht, job.nval, job.dht_pos, job.dht_end = _ptr(dht, C.c_uint8), _ptr(nval, C.c_uint32), pos, end
    gps = -(-lay.nchunks // G)
    out = np.zeros(out_cap + GUARD, np.uint8)
    offs = np.zeros(lay.nframes + 1, np.uint64)
    gff = np.zeros(lay.nframes * lay.nseg * gps, np.uint32)
    status = C.c_uint32(0xDEAD)
    rc = L.mjg_debug_tail(0, C.byref(job), _ptr(out, C.c_uint8), _ptr(offs, C.c_uint64), _ptr(gff, C.c_uint32),
                          C.byref(status))
    assert rc == 0, f"{lay.name}: mjg_debug_tail: {rc} {L.mjg_last_error()}"
    return out, offs, gff, status.value


def locate(lay, f, pos, gff):
    """Where byte `pos` of frame f lies: its segment and group, and the group's 0xFF count (the
    kernel's against the reference's: a miscount, or a misplaced byte)."""
    hl = len(header(lay, f))
    if pos < hl:
        return f"in the header ({hl} bytes)"
    at = hl
    gps = -(-lay.nchunks // G)
    for si in range(lay.nseg):
        s = f * lay.nseg + si
        pay = tail_ref.payload(lay.segment(s))
        size = len(tail_ref.escape(pay)) + 2
        if pos < at + size:
            ends = np.cumsum(lay.clamped()[s * lay.nchunks:(s + 1) * lay.nchunks])
            padded = pay + bytes(4)
            where = "the trailer"
            counts = []
            for g in range(gps):
                o0 = 0 if g == 0 else int(ends[g * G - 1])
                o1 = int(ends[min(g * G + G, lay.nchunks) - 1])
                k0, k1 = (o0 + 31) // 32, (o1 + 31) // 32  # the group's words: those whose first bit it holds
                b0 = at + len(tail_ref.escape(pay[:4 * k0]))
                b1 = at + len(tail_ref.escape(pay[:4 * k1]))
                counts.append(padded[4 * k0:4 * k1].count(0xFF))
                if b0 <= pos < b1:
                    where = (f"group {g} (words {k0}..{k1 - 1} of the segment, frame bytes {b0}..{b1 - 1}), group_ff "
                             f"{int(gff[s * gps + g])} against the reference's {counts[-1]}")
            return f"in segment {si} (frame bytes {at}..{at + size - 1}), {where}"
        at += size
    return "behind the frame"


def check(lay, out, offs, gff, status, out_cap, fitting=None):
    """frame_offsets, every frame that fits byte for byte, 0xA5 from the end of the last written
    frame on.  fitting: how many frames fit (None: all)."""
    ref = reference(lay)
    want = np.concatenate([[0], np.cumsum([len(r) for r in ref])]).astype(np.uint64)
    bad = np.nonzero(offs != want)[0]
    assert not len(bad), (f"{lay.name}: frame_offsets differ first at frame {bad[0]}: {int(offs[bad[0]])} against "
                          f"{int(want[bad[0]])} (frame {max(bad[0] - 1, 0)} has {len(ref[max(bad[0] - 1, 0)])} bytes)")
    n = lay.nframes if fitting is None else fitting
    total = int(want[n])
    exp = np.frombuffer(b"".join(ref[:n]), np.uint8)
    got = out[:total]
    if not np.array_equal(got, exp):
        p = int(np.nonzero(got != exp)[0][0])
        f = int(np.searchsorted(want, p, side="right")) - 1
        rel = p - int(want[f])
        assert False, (f"{lay.name}: frame {f} of {lay.nframes} differs first at its byte {rel} (output byte {p}): "
                       f"got {got[p]:02x}, want {exp[p]:02x}, {int((got != exp).sum())} bytes differ in all; "
                       f"{locate(lay, f, rel, gff)}")
    rest = out[total:]
    assert len(rest) == out_cap + GUARD - total
    stray = np.nonzero(rest != 0xA5)[0]
    assert not len(stray), (f"{lay.name}: byte {total + int(stray[0])} is {rest[stray[0]]:02x}, written behind the "
                            f"last frame that fits (its end {total}, out_cap {out_cap}, {len(stray)} such bytes)")
    assert status == (0 if n == lay.nframes else 1), f"{lay.name}: status {status}"


@pytest.mark.parametrize("fill", [0, 0xFFFFFFFF], ids=["fill0", "fill1"])
@pytest.mark.parametrize("name", tail_layouts.names())
def test_tail_matches_reference(name, fill):
    lay = tail_layouts.layouts()[name]
    total = sum(len(r) for r in reference(lay))
    out_cap = total + 37  # some room behind the last frame, all of it to stay 0xA5
    out, offs, gff, status = run_tail(lay, fill, out_cap)
    check(lay, out, offs, gff, status, out_cap)


def test_light_and_heavy_first_segment_give_the_same_bytes():
    """tail_priority raises the waves' priority by the first segment's bits per chunk; the frames
    behind it hold the same chunks in both layouts and come out as the same bytes."""
    outs = []
    for heavy in (False, True):
        lay = tail_layouts.layouts()[f"{'heavy' if heavy else 'light'} first segment"]
        first = lay.clamped()[:lay.nchunks].sum()
        assert (first >= tail_layouts.LIGHT_BITS * lay.nchunks) == heavy
        total = sum(len(r) for r in reference(lay))
        out, offs, gff, status = run_tail(lay, 0, total)
        check(lay, out, offs, gff, status, total)
        outs.append(out[int(offs[1]):int(offs[-1])].tobytes())
    assert outs[0] == outs[1]


@pytest.mark.parametrize("name", ["65 frames of 2 chunks", "67 segments a frame"])
def test_capacity(name):
    """out_cap the total exactly: everything written, the guard untouched.  The last frame's size
    less, and one byte less: k_write refuses the last frame alone, flags it, and writes nothing from
    its offset on; the sizes are the full ones."""
    lay = tail_layouts.layouts()[name]
    ref = reference(lay)
    total = sum(len(r) for r in ref)
    out, offs, gff, status = run_tail(lay, 0, total)
    check(lay, out, offs, gff, status, total)
    for cap in (total - len(ref[-1]), total - 1):
        out, offs, gff, status = run_tail(lay, 0, cap)
        check(lay, out, offs, gff, status, cap, fitting=lay.nframes - 1)
