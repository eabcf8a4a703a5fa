"""Chunk layouts for the stuffing tail, named and deterministic, for two consumers: the GPU tests
(tests/test_gpu_tail.py: mjg_debug_tail against tests/tail_ref.py) and the lane model
(tests/test_tail_model.py: the same segments, where a load outside the words k_encode wrote can
be seen).  A layout is nframes x nseg x nchunks chunks: per chunk a bit length as k_encode would
leave it (it may exceed the slot: the scan clamps) and the min(L, slot) bits it holds.  Contents
are laid out on the segment's bit stream (the chunks' bits one after another), where a byte
position means what it means in the JPEG, and then cut into the chunks.

Every layout is the smallest that reaches its branch; the docstring of each builder says which.
The domain is k_encode's: no empty chunk, and every chunk but a segment's last holds 32 bits or
more (include/mjgpu.h, mjg_debug_tail)."""
from __future__ import annotations

import numpy as np

from tail_model import G, R, SLOT

SLOT_BITS = 32 * SLOT
WINDOW = 64 * R  # words a wave takes in one pass of its loop
LIGHT_BITS = 1800  # kTailLightBits: tail_priority's test on the first segment's bits per chunk


class Layout:
    def __init__(self, name, nframes, nseg, nchunks, lengths, bits, hdr_len, model=True, optimal=None):
        self.name, self.nframes, self.nseg, self.nchunks = name, nframes, nseg, nchunks
        self.lengths = np.asarray(lengths, np.uint32).reshape(-1)  # as given to the scan (unclamped)
        self.bits = bits  # per chunk: uint8 0 / 1, min(L, SLOT_BITS) of them
        self.model = model  # False: its segments reach the model through another layout
        assert len(self.lengths) == nframes * nseg * nchunks == len(bits)
        rng = np.random.default_rng(hdr_len)
        self.hdr = rng.integers(0, 256, hdr_len, dtype=np.uint8).tobytes()
        self.optimal = optimal  # None, or (dht_pos, dht_end, dht [nframes][4][272], nval [nframes][4])

    def clamped(self):
        return np.minimum(self.lengths, SLOT_BITS).astype(np.int64)

    def segment(self, s):
        """Segment s (frame-major) as [(L, bits)], L unclamped."""
        i0 = s * self.nchunks
        return [(int(self.lengths[i]), self.bits[i]) for i in range(i0, i0 + self.nchunks)]

    def words(self):
        """The chunks' slot words one after another, as mjg_tail_job.words wants them."""
        out = []
        for b in self.bits:
            p = np.zeros(-(-len(b) // 32) * 32, np.uint8)
            p[:len(b)] = b
            out.append(np.packbits(p).view(">u4").astype(np.uint32))
        return np.ascontiguousarray(np.concatenate(out))


# ------------------------------------------------------------------ contents
def _random_bits(rng, n, density=0.5):
    return (rng.random(n) < density).astype(np.uint8)


def _quiet_bits(rng, n):
    """n bits whose bytes (from bit 0) are never 0xFF, whatever follows them."""
    # bit 4 of every byte is 0, so the 1-bit padding cannot complete a 0xFF either
    by = rng.integers(0, 256, -(-n // 8), dtype=np.uint8) & 0xEF
    return np.unpackbits(by)[:n]


def _set_ff(stream, byte_positions):
    for p in byte_positions:
        assert 8 * p + 8 <= len(stream), "0xFF past the segment's whole bytes"
        stream[8 * p:8 * p + 8] = 1


def _cut(stream, lengths):
    """The segment's stream cut into chunks of the clamped lengths."""
    L = np.minimum(np.asarray(lengths, np.int64), SLOT_BITS)
    assert int(L.sum()) == len(stream)
    ends = np.cumsum(L)
    return [stream[e - l:e].copy() for e, l in zip(ends, L)]


def _build(name, nframes, nseg, nchunks, seg_lengths, content, hdr_len, seed, model=True, optimal=None):
    """seg_lengths: per segment a list of nchunks lengths.  content(rng, s, T) -> the segment's T bits."""
    rng = np.random.default_rng(seed)
    lengths, bits = [], []
    assert len(seg_lengths) == nframes * nseg
    for s, L in enumerate(seg_lengths):
        assert len(L) == nchunks
        T = int(np.minimum(np.asarray(L, np.int64), SLOT_BITS).sum())
        stream = np.asarray(content(rng, s, T), np.uint8)
        lengths += list(L)
        bits += _cut(stream, L)
    return Layout(name, nframes, nseg, nchunks, lengths, bits, hdr_len, model, optimal)


def _rand(density=0.5):
    return lambda rng, s, T: _random_bits(rng, T, density)


# ------------------------------------------------------------------ the layouts
SWEEP_LAST = (1, 7, 8, 12, 31, 32, 33)


def sweep_segments():
    """1,024 segments [L0, L1, Llast]: L0 % 32 and L1 % 32 each over 0..31, so chunk 1 and chunk 2
    start at every slot bit (off) and end with every count of bits in their last word (rem), on
    both sides of the second-slot-word load (rem > 32 - off), with rem == 32 and off == 0; Llast
    from SWEEP_LAST, among them last chunks that lie wholly inside their predecessor's last
    word.  L0, L1 in 32..95; every fifth / seventh segment has a chunk of several words more."""
    segs = []
    for a in range(32):
        for b in range(32):
            i = 32 * a + b
            L0 = 32 * (1 + (b & 1)) + a + (32 * 7 if i % 5 == 0 else 0)
            L1 = 32 * (1 + (a & 1)) + b + (32 * 5 if i % 7 == 0 else 0)
            segs.append([L0, L1, SWEEP_LAST[i % 7]])
    return segs


def sweep(rst):
    """The sweep as 1,024 frames of one segment, or as 16 frames of 64 segments (RST: the
    per-segment scan, segment sizes and offsets, RSTn)."""
    segs = sweep_segments()
    if rst:
        return _build("sweep off x rem, 16 frames x 64 segments", 16, 64, 3, segs, _rand(), 7, 11, model=False)
    return _build("sweep off x rem, 1024 frames", 1024, 1, 3, segs, _rand(), 2, 11)


EDGE_WORDS = (62, 63, 64, 65, 254, 255, 256, 257, 511, 512)


def edges(nchunks):
    """A chunk whose last owned word is word r of its group, r around lane 63 of a round, around
    the last word of a 256-word window and of the second window, with 1, 31 and 32 bits in that
    word (rem), the chunk starting at slot bit 0, 1 and 31 (off).  With 3 chunks a further chunk
    follows (its start is marked in the second, third and fourth round and in the next window);
    with 2 the segment, and so the group, ends in that word."""
    segs = []
    for r in EDGE_WORDS:
        for rem in (1, 31, 32):
            for off in (0, 1, 31):
                L0 = 64 - off
                L1 = 32 * r + rem - L0
                segs.append([L0, L1] + ([100] if nchunks == 3 else []))
    return _build(f"lane and window edges, {nchunks} chunks", len(segs), 1, nchunks, segs, _rand(0.7), 3, 12 + nchunks)


def max_slot(lead):
    """Chunks that fill their slot: 13 windows a chunk.  Frame 1 has one length 777 above the slot,
    frame 2 one of 0xFFFFFFFF: the scan clamps both to the slot, as the reference does.  The slot
    is a whole number of words, so these chunks all start at slot bit 0; with `lead`, a chunk of
    45 bits in front of them moves every one to slot bit 19, and each of its 3,328 words is made
    of two slot words, the last of them of the chunk's last word and the next chunk's first."""
    head = [45] if lead else []
    segs = [head + [SLOT_BITS, SLOT_BITS, SLOT_BITS, 4], head + [SLOT_BITS, SLOT_BITS + 777, SLOT_BITS, 4],
            head + [SLOT_BITS, SLOT_BITS, 0xFFFFFFFF, 4]]
    name = "maximum-slot chunks and the clamp" + (", behind 45 bits" if lead else "")
    return _build(name, 3, 1, len(segs[0]), segs, _rand(), 64, 14 + lead)


def many_groups():
    """2,100 chunks of 32 to 40 bits in one segment: 66 groups, so k_scan_ff's loop over the groups
    carries, and k_scan_bits' block scan carries twice.  Bits at density 0.95: every group has
    0xFF counts for the carry to lose."""
    rng = np.random.default_rng(15)
    segs = [rng.integers(32, 41, 2100).tolist()]
    return _build("66 groups in a segment", 1, 1, 2100, segs, _rand(0.95), 65, 15)


def many_segments():
    """67 segments a frame, 3 chunks each: seg_off's loop carries; 134 segments leave
    k_scan_bits_seg's last workgroup half empty."""
    rng = np.random.default_rng(16)
    segs = [rng.integers(32, 300, 3).tolist() for _ in range(2 * 67)]
    return _build("67 segments a frame", 2, 67, 3, segs, _rand(0.9), 17, 16)


def long_rst_segments():
    """RST segments of 70 and 130 chunks: the per-segment scan of the bit lengths carries."""
    rng = np.random.default_rng(17)
    segs = [rng.integers(32, 120, 130).tolist() for _ in range(2 * 3)]
    return _build("130 chunks a segment under RST", 2, 3, 130, segs, _rand(0.9), 600, 17)


def many_frames(nframes, nchunks=2):
    """nframes frames: 63 / 64 / 65 around a round of the frame_offsets loop, 130 for two carries
    (64-bit).  With 33 chunks a frame has two groups, the second of one chunk."""
    rng = np.random.default_rng(100 + nframes)
    segs = [rng.integers(32, 200, nchunks).tolist() for _ in range(nframes)]
    return _build(f"{nframes} frames of {nchunks} chunks", nframes, 1, nchunks, segs, _rand(0.8), 5 + (nframes & 1), nframes)


def group_boundary(nchunks):
    """nchunks around the group size.  The chunk that ends the first group (the segment's last
    when there is one group only) ends word-aligned, one bit short of a word and one bit
    over, in frames 0 to 2; frame 3's last chunk is 5 bits behind a chunk that ends one bit into
    a word, so with 33 or 65 chunks the last group owns no word at all."""
    rng = np.random.default_rng(200 + nchunks)
    segs = []
    for end in (0, 31, 1, 1):
        L = rng.integers(32, 200, nchunks)
        e = min(G, nchunks) - 1 if len(segs) < 3 else nchunks - 2
        if e >= 0:
            before = int(L[:e].sum())
            L[e] = 64 + (end - before - 64) % 32
            assert (before + int(L[e])) % 32 == end
        if len(segs) == 3:
            L[-1] = 5 if nchunks > 1 else 37
        segs.append(L.tolist())
    return _build(f"group boundary, {nchunks} chunks", 4, 1, nchunks, segs, _rand(0.8), 19, 200 + nchunks)


def all_ones():
    """Every byte 0xFF: every byte stuffed, the frame twice its bits."""
    segs = [[100, 333, 6000, 17], [96, 32, 64, 32]]
    return _build("all ones", 2, 1, 4, segs, lambda rng, s, T: np.ones(T, np.uint8), 1, 20)


def ff_byte_positions():
    """One 0xFF at each of a word's four bytes (frame p: byte p of words 3, 10 and 70), between
    bytes that are not 0xFF."""
    segs = [[1000, 1500, 333]] * 4

    def content(rng, s, T):
        st = _quiet_bits(rng, T)
        _set_ff(st, [4 * w + s for w in (3, 10, 70)])
        return st
    return _build("0xFF at each byte of a word", 4, 1, 3, segs, content, 4, 21)


def ff_lane63():
    """0xFF bytes in lane 63's word of rounds 0 to 3 and around the window change (words 63, 127,
    191, 255, 256), one a frame and all together, and a frame with 0xFF in every word before
    them: k_write's carry of the 0xFF prefix across rounds and windows."""
    segs = [[5000, 6000, 7000, 3000]] * 7
    spots = [[63], [127], [191], [255], [256], [63, 127, 191, 255, 256]]

    def content(rng, s, T):
        st = _quiet_bits(rng, T)
        if s < 6:
            _set_ff(st, [4 * w + (w + s) % 4 for w in spots[s]])
        else:
            _set_ff(st, [4 * w + w % 4 for w in range(300)])
        return st
    return _build("0xFF in lane 63 and at the window change", 7, 1, 4, segs, content, 3, 22)


def short_last_word():
    """The segment's last word with 1, 2, 3 and 4 bytes; without 0xFF, with its last byte 0xFF
    (0xFF straight before the trailer) and with all its bytes 0xFF."""
    segs, kinds = [], []
    for nb in (1, 2, 3, 4):
        for kind in range(3):
            segs.append([70, 32 * 9 + 8 * nb - 70])
            kinds.append((nb, kind))

    def content(rng, s, T):
        st = _quiet_bits(rng, T)
        nb, kind = kinds[s]
        last = T // 8 - 1
        if kind:
            _set_ff(st, [last] if kind == 1 else range(last - nb + 1, last + 1))
        return st
    return _build("short last word", len(segs), 1, 2, segs, content, 6, 23)


def ff_by_padding():
    """A last byte that is 0xFF only through the padding: the data ends 1111 and 4 pad bits
    follow; the segment's last word then has 1, 2, 3 and 4 bytes.  Frames 4 to 7: the data ends
    in a single 1 and 7 pad bits follow."""
    segs, tails = [], []
    for k in (4, 1):
        for nb in (1, 2, 3, 4):
            segs.append([45, 32 * 5 + 8 * (nb - 1) + k - 45])
            tails.append(k)

    def content(rng, s, T):
        st = _quiet_bits(rng, T)
        st[T - 8:] = 0
        st[T - tails[s]:] = 1
        return st
    return _build("0xFF through the padding", len(segs), 1, 2, segs, content, 9, 24)


def dense(density):
    rng = np.random.default_rng(int(density * 100))
    segs = [rng.integers(32, 3000, 40).tolist() for _ in range(4)]
    return _build(f"random bits, density {density}", 4, 1, 40, segs, _rand(density), 623, 25)


def priority(heavy):
    """tail_priority's two arms: the first segment averages 100 or 3,000 bits a chunk (below and
    above LIGHT_BITS); the other frames are the same bits in both."""
    rng = np.random.default_rng(26)
    first = [3000 if heavy else 100] * 8
    assert (sum(first) < LIGHT_BITS * 8) == (not heavy)
    segs = [first] + [rng.integers(32, 2500, 8).tolist() for _ in range(3)]

    def content(_, s, T):
        return _random_bits(np.random.default_rng(1000 + s), T, 0.8)
    return _build(f"{'heavy' if heavy else 'light'} first segment", 4, 1, 8, segs, content, 33, 26)


def header_length(hdr_len):
    rng = np.random.default_rng(27)
    segs = [rng.integers(32, 500, 5).tolist() for _ in range(5)]
    return _build(f"header of {hdr_len} bytes", 5, 1, 5, segs, _rand(0.8), hdr_len, 27, model=hdr_len == 1)


def optimal_headers():
    """-huffman optimal: a DHT of its own per frame, the value counts differing (0 and 256 among
    them), so every frame starts at another byte alignment."""
    rng = np.random.default_rng(28)
    nframes, dht_pos = 6, 141
    dht_end = dht_pos + 420
    nval = np.array([[12, 12, 162, 162], [0, 1, 2, 3], [12, 11, 256, 255], [5, 12, 97, 30], [12, 12, 161, 162],
                     [1, 0, 0, 256]], np.uint32)
    dht = rng.integers(0, 256, (nframes, 4, 272), dtype=np.uint8)
    segs = [rng.integers(32, 500, 5).tolist() for _ in range(nframes)]
    return _build("per-frame optimal headers", nframes, 1, 5, segs, _rand(0.8), dht_end + 14, 28,
                  optimal=(dht_pos, dht_end, dht, nval))


_BUILDERS = [
    lambda: sweep(False), lambda: sweep(True), lambda: edges(3), lambda: edges(2), lambda: max_slot(0), lambda: max_slot(1), many_groups,
    many_segments, long_rst_segments, lambda: many_frames(1), lambda: many_frames(63), lambda: many_frames(64),
    lambda: many_frames(65), lambda: many_frames(130, 33),
    *[(lambda n: lambda: group_boundary(n))(n) for n in (1, 31, 32, 33, 64, 65)],
    all_ones, ff_byte_positions, ff_lane63, short_last_word, ff_by_padding, lambda: dense(0.5), lambda: dense(0.9),
    lambda: priority(False), lambda: priority(True),
    *[(lambda n: lambda: header_length(n))(n) for n in (1, 2, 64, 65)], optimal_headers,
]
_cache = {}


def layouts():
    """Every layout, built once a process (they are read only)."""
    if not _cache:
        for b in _BUILDERS:
            lay = b()
            assert lay.name not in _cache
            _cache[lay.name] = lay
    return _cache


def names():
    return list(layouts())
