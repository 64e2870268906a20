"""An independent baseline JPEG encoder for coefficient-level tests of szg_jpeg_open (include/szg/jpeg.h rules 1 and 2). It
shares no code with the decoder: it takes QUANTISED blocks and writes them, it never transforms a picture.

Huffman codes are (nearly) fixed-length: T.81 allows any prefix code described by 16 length counts, and n symbols at one length
L (n < 2^L, so the all-ones code stays unused) are the codes 0 .. n - 1 in L bits.
"""
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, length):
        assert 0 <= value < (1 << length) or length == 0
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0x00)  # stuffing
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)  # pad with ones


def _category(v):
    return 0 if v == 0 else int(abs(v)).bit_length()


def _put_value(bits, v, s):
    if s:
        bits.put(v if v >= 0 else v + (1 << s) - 1, s)


def _segment(marker, body, fill):
    return b"\xFF" * fill + bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def encode(width, height, components, tables, scans=None, restart_interval=0, dc_bits=5, ac_bits=9, fill=0, ids=None):
    """components: [(h, v, tq, blocks)] with blocks an int array [blocks_h, blocks_w, 8, 8] (natural order) over the MCU-padded
    grid; tables: {tq: int array [8, 8] (natural order); an entry above 255 makes the table a 16-bit one}; scans: lists of component
    indices (default: one interleaved scan of all); fill: 0xFF fill bytes in front of every marker. DC differences and AC values
    may have up to 15 magnitude bits. Returns the file's bytes."""
    n = len(components)
    ids = list(ids) if ids is not None else list(range(1, n + 1))
    scans = scans if scans is not None else [list(range(n))]
    h_max = max(c[0] for c in components)
    v_max = max(c[1] for c in components)
    mcus_x, mcus_y = -(-width // (8 * h_max)), -(-height // (8 * v_max))
    out = bytearray(b"\xFF\xD8")
    for tq, table in sorted(tables.items()):
        table = np.asarray(table).reshape(64)
        wide = int(table.max()) > 255
        body = bytes([(16 if wide else 0) | tq])
        for k in ZIGZAG:
            body += struct.pack(">H", int(table[k])) if wide else bytes([int(table[k])])
        out += _segment(0xDB, body, fill)
    body = bytes([8]) + struct.pack(">HH", height, width) + bytes([n])
    for (h, v, tq, _), cid in zip(components, ids):
        body += bytes([cid, (h << 4) | v, tq])
    out += _segment(0xC0, body, fill)
    # DC: 16 symbols at dc_bits. AC: a length count is one byte, so the 256 symbols are 128 codes of ac_bits (0 .. 127) and
    # 128 of ac_bits + 1 (256 .. 383, the canonical continuation)
    dc_code = {s: (s, dc_bits) for s in range(16)}
    ac_code = {s: (s, ac_bits) if s < 128 else (256 + s - 128, ac_bits + 1) for s in range(256)}
    assert 5 <= dc_bits <= 16 and 8 <= ac_bits <= 15
    counts = [0] * 16
    counts[dc_bits - 1] = 16
    out += _segment(0xC4, bytes([0x00]) + bytes(counts) + bytes(range(16)), fill)
    counts = [0] * 16
    counts[ac_bits - 1] = counts[ac_bits] = 128
    out += _segment(0xC4, bytes([0x10]) + bytes(counts) + bytes(range(256)), fill)
    if restart_interval:
        out += _segment(0xDD, struct.pack(">H", restart_interval), fill)

    def put_block(bits, block, pred):
        zz = [int(block.reshape(64)[k]) for k in ZIGZAG]
        diff = zz[0] - pred
        s = _category(diff)
        assert s <= 15
        bits.put(*dc_code[s])
        _put_value(bits, diff, s)
        run = 0
        last = max([k for k in range(1, 64) if zz[k] != 0], default=0)
        for k in range(1, last + 1):
            if zz[k] == 0:
                run += 1
                continue
            while run > 15:
                bits.put(*ac_code[0xF0])
                run -= 16
            s = _category(zz[k])
            assert s <= 15
            bits.put(*ac_code[(run << 4) | s])
            _put_value(bits, zz[k], s)
            run = 0
        if last < 63:
            bits.put(*ac_code[0x00])
        return zz[0]

    for scan in scans:
        body = bytes([len(scan)])
        for c in scan:
            body += bytes([ids[c], 0x00])
        out += _segment(0xDA, body + bytes([0, 63, 0]), fill)
        bits = _Bits()
        pred = {c: 0 for c in scan}
        if len(scan) == 1:
            c = scan[0]
            h, v, _, blocks = components[c]
            units = [[(c, by, bx)] for by in range(-(-(-(-height * v // v_max)) // 8)) for bx in range(-(-(-(-width * h // h_max)) // 8))]
        else:
            units = [[(c, my * components[c][1] + y, mx * components[c][0] + x) for c in scan for y in range(components[c][1])
                      for x in range(components[c][0])] for my in range(mcus_y) for mx in range(mcus_x)]
        rst = 0
        for k, unit in enumerate(units):
            if restart_interval and k and k % restart_interval == 0:
                bits.flush()
                bits.out += b"\xFF" * fill + bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) % 8
                pred = {c: 0 for c in scan}
            for c, by, bx in unit:
                pred[c] = put_block(bits, np.asarray(components[c][3])[by, bx], pred[c])
        bits.flush()
        out += bits.out
    out += b"\xFF" * fill + b"\xFF\xD9"
    return bytes(out)


def coded_mask(width, height, components, scans=None):
    """For each component a bool [blocks_h, blocks_w]: the blocks some scan writes (a non-interleaved scan covers only the blocks
    that hold samples of the picture, an interleaved one the whole MCU-padded grid)."""
    n = len(components)
    scans = scans if scans is not None else [list(range(n))]
    h_max = max(c[0] for c in components)
    v_max = max(c[1] for c in components)
    masks = [np.zeros(np.asarray(c[3]).shape[:2], bool) for c in components]
    for scan in scans:
        for c in scan:
            if len(scan) > 1:
                masks[c][:] = True
            else:
                h, v = components[c][:2]
                masks[c][:-(-(-(-height * v // v_max)) // 8), :-(-(-(-width * h // h_max)) // 8)] = True
    return masks
