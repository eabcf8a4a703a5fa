"""Plain reference of the stuffing tail for tests/test_gpu_tail.py: what
k_scan_bits / k_count_ff / k_scan_ff / k_write make of chunks of bits, restated from the JPEG
side with numpy and bytes, no lanes, words or groups:

  segment  the chunks' first min(L, slot bits) bits one after another, padded with 1-bits to a
           byte (ff_mjpeg_encode_stuffing), then a 0x00 after every 0xFF (ff_mjpeg_escape_FF:
           the padding comes first, so a byte the padding completes to 0xFF is escaped too; as
           or_flush_segment in oracle/mjpeg_oracle.c), then FF D0+(si & 7), or FF D9 after the
           frame's last segment
  frame    the header, then the segments
  header   the given bytes; with -huffman optimal's per-frame tables the bytes before dht_pos, one
           DHT (FF C4, length, then DC0, DC1, AC0, AC1: class byte, 16 BITS, the table's values),
           the bytes from dht_end on (kernels.hip write_header)

It shares nothing with tests/tail_model.py, which restates the kernel's indexing."""
from __future__ import annotations

import numpy as np

SLOT_BITS = 64 * 1664  # a chunk's slot: 64 blocks of kMaxBlockBits (a multiple of 32)


def payload(chunks, slot_bits=SLOT_BITS) -> bytes:
    """A segment's bytes before escaping: `chunks` is a list of (L, bits), bits a uint8 array of
    0 / 1 holding at least min(L, slot_bits) entries."""
    parts = [np.asarray(b, np.uint8)[:min(int(L), slot_bits)] for L, b in chunks]
    for (L, _), p in zip(chunks, parts):
        assert len(p) == min(int(L), slot_bits), "chunk holds fewer bits than its length"
    bits = np.concatenate(parts)
    pad = -len(bits) % 8
    return np.packbits(np.concatenate([bits, np.ones(pad, np.uint8)])).tobytes()


def escape(data: bytes) -> bytes:
    return data.replace(b"\xff", b"\xff\x00")


def unescape(scan: bytes) -> bytes:
    return scan.replace(b"\xff\x00", b"\xff")


def trailer(si: int, nseg: int) -> bytes:
    return b"\xff\xd9" if si == nseg - 1 else bytes([0xFF, 0xD0 + (si & 7)])


def optimal_header(hdr: bytes, dht_pos: int, dht_end: int, dht, nval) -> bytes:
    """dht: [4][272] uint8 (16 BITS then values), nval: [4], tables DC luma, DC chroma, AC luma,
    AC chroma."""
    dht = np.asarray(dht, np.uint8).reshape(4, 272)
    body = b""
    for t, cls in enumerate((0x00, 0x01, 0x10, 0x11)):
        body += bytes([cls]) + dht[t, :16 + int(nval[t])].tobytes()
    n = 2 + len(body)
    return hdr[:dht_pos] + b"\xff\xc4" + bytes([n >> 8, n & 255]) + body + hdr[dht_end:]


def frame(header: bytes, segs, slot_bits=SLOT_BITS) -> bytes:
    """segs: the frame's segments, each a list of (L, bits) chunks."""
    out = header
    for si, chunks in enumerate(segs):
        out += escape(payload(chunks, slot_bits)) + trailer(si, len(segs))
    return out
