"""CPU side of the stuffing tail's GPU tests (tests/test_gpu_tail.py): the reference tests/tail_ref.py
against the oracle's bytes, the layouts' constants against kernels.hip, the layouts' own promises,
and mjg_debug_tail's argument checks, which answer before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import tail_layouts
import tail_ref
from ffmpeg_distributed_amd import _lib
from tail_layouts import G, R, SLOT, SLOT_BITS
from test_oracle import segments, smooth_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = open(os.path.join(ROOT, "ffmpeg_distributed_amd", "csrc", "kernels.hip")).read()


def _const(name):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", KERNELS)
    assert m, name
    return int(m.group(1))


def test_constants_match_the_kernels():
    assert SLOT == (64 * _const("kMaxBlockBits") + 31) // 32
    assert re.search(r"kSlotWords = \(64 \* kMaxBlockBits \+ 31\) / 32;", KERNELS)
    assert G == _const("kChunksPerWave")
    assert R == _const("kTailRounds")
    assert tail_layouts.LIGHT_BITS == _const("kTailLightBits")
    assert tail_ref.SLOT_BITS == SLOT_BITS == 32 * SLOT
    m = re.search(r"#define\s+MJG_TAIL_GUARD\s+(\d+)", open(os.path.join(ROOT, "include", "mjgpu.h")).read())
    assert m and int(m.group(1)) == _lib.MJG_TAIL_GUARD
    m = re.search(r"#define\s+MJG_TAIL_MAX_SLOTS\s+(\d+)", open(os.path.join(ROOT, "include", "mjgpu.h")).read())
    assert m and int(m.group(1)) == _lib.MJG_TAIL_MAX_SLOTS


@pytest.mark.parametrize("rst", [False, True])
def test_reference_restuffs_an_oracle_frame(rst):
    """An oracle-encoded frame, its scan un-stuffed and cut into chunks at arbitrary bit lengths
    (the payload is byte-aligned: the padding is in it), comes back byte for byte from the
    reference; under RST segment by segment, with the RSTn markers."""
    w, h = 72, 40
    y, u, v = smooth_frame(w, h, seed=5)
    y[8:16, 8:24] = np.random.default_rng(5).integers(0, 256, (8, 16))  # enough entropy for 0xFF bytes
    jpg = oracle.encode_frame(y, u, v, qscale=2, full_range=True, rst=rst)
    scan = segments(jpg)[-1][1]
    hdr = jpg[:len(jpg) - 2 - len(scan)]
    parts = re.split(rb"\xff[\xd0-\xd7]", scan) if rst else [scan]
    assert len(parts) == (3 if rst else 1) and b"\xff\x00" in scan
    rng = np.random.default_rng(6)
    segs = []
    for part in parts:
        bits = np.unpackbits(np.frombuffer(tail_ref.unescape(part), np.uint8))
        cuts = np.sort(rng.choice(np.arange(1, len(bits)), 6, replace=False))
        segs.append([(len(b), b) for b in np.split(bits, cuts)])
    assert tail_ref.frame(hdr, segs) == jpg


def test_reference_pads_before_it_escapes():
    """Data bits 1111 and the four padding bits make a 0xFF, which is escaped (or_flush_segment)."""
    ones = np.ones(12, np.uint8)
    assert tail_ref.frame(b"H", [[(12, ones)]]) == b"H\xff\x00\xff\x00\xff\xd9"
    assert tail_ref.frame(b"H", [[(4, ones)], [(9, np.zeros(9, np.uint8))]]) == b"H\xff\x00\xff\xd0\x00\x7f\xff\xd9"
    # a length past the slot: the slot's bits only
    big = np.zeros(SLOT_BITS + 8, np.uint8)
    assert len(tail_ref.frame(b"", [[(SLOT_BITS + 8, big), (0xFFFFFFFF, big)]])) == 2 * SLOT_BITS // 8 + 2


def test_layouts_are_deterministic_and_in_the_domain():
    lays = tail_layouts.layouts()
    again = [b() for b in tail_layouts._BUILDERS[:4]]
    for b in again:
        a = lays[b.name]
        assert np.array_equal(a.lengths, b.lengths) and all(np.array_equal(x, y) for x, y in zip(a.bits, b.bits))
    for lay in lays.values():
        n = lay.nframes * lay.nseg * lay.nchunks
        assert 1 <= n <= _lib.MJG_TAIL_MAX_SLOTS, lay.name
        L = lay.lengths.reshape(-1, lay.nchunks)
        assert (L >= 1).all() and (L[:, :-1] >= 32).all(), lay.name
        assert all(len(b) == c for b, c in zip(lay.bits, lay.clamped())), lay.name
        assert len(lay.words()) == int(((lay.clamped() + 31) // 32).sum())


def test_sweep_reaches_every_start_bit_and_last_word_count():
    """Chunks 1 and 2 of the sweep's segments: every off x rem pair of chunk 1, both sides of the
    second-slot-word load with every off, and a last chunk inside its predecessor's last word."""
    seen, xload, inside = set(), set(), 0
    for L0, L1, L2 in tail_layouts.sweep_segments():
        assert 32 <= (L0 if L0 <= 95 else L0 - 32 * 7) <= 95 and 32 <= (L1 if L1 <= 95 else L1 - 32 * 5) <= 95
        off = -L0 % 32
        end = L0 + L1
        rem = end - 32 * ((end + 31) // 32 - 1)
        seen.add((off, rem))
        if off:
            xload.add((off, rem > 32 - off))
        inside += (end % 32 != 0) and (end % 32 + L2 <= 32)
    assert seen == {(o, r) for o in range(32) for r in range(1, 33)}
    assert xload == {(o, x) for o in range(1, 32) for x in (False, True)}
    assert inside > 50


def _job(nframes, nseg, nchunks, lengths):
    bits = np.asarray(lengths, np.uint32)
    words = np.zeros(int(((np.minimum(bits, SLOT_BITS).astype(np.int64) + 31) // 32).sum()) + 1, np.uint32)
    hdr = np.zeros(4, np.uint8)
    job = _lib.MjgTailJob(nframes=nframes, nseg=nseg, nchunks=nchunks,
                          chunk_bits=bits.ctypes.data_as(C.POINTER(C.c_uint32)),
                          words=words.ctypes.data_as(C.POINTER(C.c_uint32)), fill=0,
                          hdr=hdr.ctypes.data_as(C.POINTER(C.c_uint8)), hdr_len=4, out_cap=1024)
    return job, (bits, words, hdr)


@pytest.mark.parametrize("case,needle", [
    ("null job", b"null"), ("null out", b"null"), ("null words", b"null"), ("zero frames", b"below 1"),
    ("zero header", b"below 1"), ("zero-bit chunk", b"0 bits"), ("short chunk", b"not its segment's last"),
    ("short chunk ending a frame's first segment", b"not its segment's last"), ("too many slots", b"more than 8192 slots"),
    ("too many slots, 32-bit wrap", b"more than 8192 slots"), ("nval without dht", b"dht"),
])
def test_debug_tail_refuses_bad_arguments_without_a_device(case, needle):
    """Every refusal is MJG_E_INVALID with a message and comes before the first HIP call (device
    1000 is never reached)."""
    L = _lib.load()
    job, keep = _job(2, 1, 3, [40, 50, 7, 32, 32, 1])
    out = (C.c_uint8 * (1024 + _lib.MJG_TAIL_GUARD))()
    offs = (C.c_uint64 * 3)()
    status = C.c_uint32(7)
    if case == "null out":
        out = None
    elif case == "null words":
        job.words = None
    elif case == "zero frames":
        job.nframes = 0
    elif case == "zero header":
        job.hdr_len = 0
    elif case == "zero-bit chunk":
        job, keep = _job(2, 1, 3, [40, 50, 7, 32, 32, 0])
    elif case == "short chunk":
        job, keep = _job(2, 1, 3, [40, 31, 7, 32, 32, 1])
    elif case == "short chunk ending a frame's first segment":
        job, keep = _job(1, 1, 6, [40, 50, 7, 32, 32, 1])  # in the domain as 2 segments of 3
    elif case == "too many slots":
        job.nframes, job.nchunks = 91, 91
    elif case == "too many slots, 32-bit wrap":
        job.nframes, job.nseg, job.nchunks = 65536, 65536, 1
    elif case == "nval without dht":
        nv = np.zeros(8, np.uint32)
        keep += (nv,)
        job.nval = nv.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = L.mjg_debug_tail(1000, None if case == "null job" else C.byref(job), out, offs, None, C.byref(status))
    assert rc == _lib.MJG_E_INVALID, (rc, L.mjg_last_error())
    assert needle in L.mjg_last_error(), L.mjg_last_error()
    assert status.value == 7


def test_debug_tail_accepts_the_domain_then_needs_a_device():
    """A last chunk of one bit and lengths past the slot are in the domain: the same call passes
    the checks and fails at the device (1000: none such), not with MJG_E_INVALID."""
    L = _lib.load()
    job, keep = _job(1, 2, 2, [SLOT_BITS + 777, 1, 0xFFFFFFFF, 31])
    out = (C.c_uint8 * (1024 + _lib.MJG_TAIL_GUARD))()
    offs = (C.c_uint64 * 2)()
    status = C.c_uint32(7)
    rc = L.mjg_debug_tail(1000, C.byref(job), out, offs, None, C.byref(status))
    assert rc == _lib.MJG_E_HIP, (rc, L.mjg_last_error())
