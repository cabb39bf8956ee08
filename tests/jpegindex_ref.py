"""Plain restatement of the sync index of libx3djpeg.so (include/x3djpeg.h, "Sync index"): the authority the C indexer
x3djpeg_index_build is held to byte for byte.  Built on the Huffman code tables of tests/jpeg_ref.py and the unstuffing of
tests/jpeg_entropy_cases.py, bit by bit; nothing shared with the library.  No test in here.

The rule.  A prepared scan is cut into segments (one per restart interval) and every segment into subsequences of
index_bits bits: max(1, ceil(bits / index_bits)) of them.  There is one entry per subsequence.  Entry 0 of a segment is
(p, b, k, block) = (0, 0, 0, 0).  Entry i + 1 is the state in which the serial decoder stands at the first symbol
boundary at or after bit (i + 1) * index_bits -- a symbol is one Huffman code with its extra bits; p is the bit position
within the segment, b the block within the MCU, k the zigzag index (0: a DC code is next), block the index within the
segment of the block the state is in -- or, if the segment's last block ends before that bit, the state at that end: (its
bit position, 0, 0, the segment's block count).  An entry is two uint32 words: p, then b | k << 3 | block << 10."""
import numpy as np

from tests import jpeg_entropy_cases as jc
from tests import jpeg_ref as jr

MAX_BLOCKS = 1 << 22


def nsub(segs, index_bits):
    """Entries of a frame: segs as jc.unstuff gives them."""
    return sum(max(1, -(-8 * ln // index_bits)) for _, ln, _, _ in segs)


class _SegBits:
    """Bits of one segment of unstuffed bytes, one at a time; zero past its end."""

    def __init__(self, scan, off, ln):
        self.d, self.off, self.ln, self.p = scan, off, ln, 0

    def bit(self):
        byte = self.p >> 3
        v = (self.d[self.off + byte] >> (7 - (self.p & 7))) & 1 if byte < self.ln else 0
        self.p += 1
        return v

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v


def states(data, index_bits):
    """[(p, b, k, block)] of every entry of the file's index, in order; the frame's segment list beside it."""
    assert index_bits >= 32 and index_bits % 32 == 0
    info = jr.parse(data)
    comps = info["comps"]
    tabs = {key: jr._codes(*v) for key, v in info["huff"].items()}
    scan, segs = jc.unstuff(data, info["scan_off"], info["mcus_x"] * info["mcus_y"], info["restart_interval"])
    comp_of = [ci for ci, c in enumerate(comps) for _ in range(c["h"] * c["v"])]      # block of an MCU -> component
    bpm = len(comp_of)
    out = []
    for off, ln, _, mcu_count in segs:
        n = max(1, -(-8 * ln // index_bits))
        total = mcu_count * bpm
        assert total < MAX_BLOCKS
        br = _SegBits(scan, off, ln)
        ent = [(0, 0, 0, 0)]
        b = k = block = 0
        while block < total:
            while len(ent) < n and br.p >= len(ent) * index_bits:     # a symbol boundary at or after the cut
                ent.append((br.p, b, k, block))
            c = comps[comp_of[b]]
            if k == 0:
                s = jr._sym(br, tabs[(0, c["td"])])
                br.bits(s)
                k = 1
            else:
                rs = jr._sym(br, tabs[(1, c["ta"])])
                r, s = rs >> 4, rs & 15
                if s == 0:
                    k = k + 16 if r == 15 else 64
                else:
                    k += r
                    assert k <= 63
                    br.bits(s)
                    k += 1
            if k >= 64:
                k, b, block = 0, (b + 1) % bpm, block + 1
        assert b == 0 and br.p <= 8 * ln
        while len(ent) < n:                                           # the segment's blocks ended before these cuts
            ent.append((br.p, 0, 0, total))
        out += ent
    return out, segs


def pack(st):
    """uint32 [n, 2] of a list of states: the two words of every entry."""
    e = np.zeros((len(st), 2), np.uint32)
    for i, (p, b, k, block) in enumerate(st):
        e[i] = (p, b | (k << 3) | (block << 10))
    return e


def entries(data, index_bits):
    """uint32 [n, 2]: the index as x3djpeg_index_build writes it."""
    return pack(states(data, index_bits)[0])
