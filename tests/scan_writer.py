"""A baseline JPEG written from coefficients, and what its writer knows without any decoder.

`write_baseline` extends the idea of test_huffman_shapes_gpu._recode: where that one re-codes an encoder's file, this one starts from
the coefficients alone (own DQT of ones, SOF0, DHT, DRI, SOS), so a test decides every symbol of the scan -- tables of one symbol,
magnitudes of all ones, blocks longer than a subsequence -- and gets the symbol counts, the magnitude bits and the position of every
symbol back for checks that go through no decoder.  `parse_baseline` reads a single-scan baseline file back into its DHT lengths and
scan bytes (the optimizer's OUTPUT is checked with it); `expected_scan_length` is the arithmetic between the two.
Plain Python: nothing here imports the library under test."""
import numpy as np

from golden_util import BitWriter, block_symbols, canonical_codes


def _lengths(freq, shape, is_dc):
    syms = sorted(freq, key=lambda s: (-freq[s], s))
    if shape == "flat":  # every symbol the same length: the first lookup level decides everything
        return {s: (4 if is_dc else 8) for s in syms}
    if shape == "deep":  # 2 .. 11 bits for the ten most frequent symbols, 16 bits for all the others
        return {s: (i + 2 if i < 10 else 16) for i, s in enumerate(syms)}
    raise ValueError(shape)


def write_baseline(coefs, width, height, ncomp=1, dri=0, table_shape="flat"):
    """coefs[nblocks, 64]: zig-zag blocks in scan order (4:4:4: the components of an MCU side by side), one MCU per 8 x 8 pixels.
    Gray files use tables DC 0 / AC 0, three-component files DC 0 / AC 0 for the first component and DC 1 / AC 1 for the others.
    Returns (file bytes, info):
      tables          {(class, identifier): {symbol: count}}, class 0 = DC, 1 = AC
      magnitude_bits  all bits behind the code words
      intervals       per restart interval (one for dri = 0): ({(class, identifier, symbol): count}, magnitude bits)
      entropy_bytes   bytes between the SOS header and EOI, stuffing and RSTn included
      stuffed         zero bytes stuffed behind an FF;  rst_markers  RSTn markers written
      block_bits      unstuffed bit position of every block's first bit, counted inside its own interval
      symbols         dri = 0 only: (bit position of the code, code length, magnitude length, block) per symbol
      block_symbols   per block: (table identifier, [(class, symbol)]) in the order written (`priced_block_bits` prices them)
      header_bytes    length of everything in front of the entropy data"""
    coefs = np.asarray(coefs)
    mcus = ((width + 7) // 8) * ((height + 7) // 8)
    assert ncomp in (1, 3) and coefs.shape == (mcus * ncomp, 64), (coefs.shape, mcus, ncomp)
    per_interval = ncomp * dri if dri else len(coefs) + 1
    freq, parsed, pred = {}, [], [0] * ncomp
    for i, blk in enumerate(coefs):
        c = i % ncomp
        if i % per_interval == 0:
            pred = [0] * ncomp
        (dcat, dbits), ac = block_symbols(blk, pred[c])
        assert dcat <= 11 and all((s & 15) <= 10 for s, _, _ in ac), "outside baseline's categories"
        pred[c] = int(blk[0])
        t = 0 if c == 0 else 1
        freq.setdefault((0, t), {})
        freq.setdefault((1, t), {})
        freq[(0, t)][dcat] = freq[(0, t)].get(dcat, 0) + 1
        for sym, _, _ in ac:
            freq[(1, t)][sym] = freq[(1, t)].get(sym, 0) + 1
        parsed.append((t, dcat, dbits, ac))
    codes = {key: canonical_codes(_lengths(f, table_shape, key[0] == 0)) for key, f in freq.items()}

    out = bytearray(b"\xff\xd8\xff\xdb\x00\x43\x00" + b"\x01" * 64)
    out += b"\xff\xc0" + (8 + 3 * ncomp).to_bytes(2, "big") + b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        out += bytes([c + 1, 0x11, 0])
    for (cls, t) in sorted(codes, key=lambda k: (k[1], k[0])):
        _, bits, vals = codes[(cls, t)]
        payload = bytes([(cls << 4) | t]) + bytes(bits) + bytes(vals)
        out += b"\xff\xc4" + (len(payload) + 2).to_bytes(2, "big") + payload
    if dri:
        out += b"\xff\xdd\x00\x04" + dri.to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * ncomp).to_bytes(2, "big") + bytes([ncomp])
    for c in range(ncomp):
        out += bytes([c + 1, 0x00 if c == 0 else 0x11])
    out += b"\x00\x3f\x00"

    w, pos, magnitude_bits, rst = BitWriter(), 0, 0, 0
    intervals, cur, cur_mag, block_bits, symbols = [], {}, 0, [], []
    for i, (t, dcat, dbits, ac) in enumerate(parsed):
        if i and i % per_interval == 0:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + (rst & 7)])
            rst += 1
            intervals.append((cur, cur_mag))
            cur, cur_mag, pos = {}, 0, 0
        block_bits.append(pos)
        for cls, sym, m, s in [(0, dcat, dbits, dcat)] + [(1, sym, m, s) for sym, m, s in ac]:
            code, ln = codes[(cls, t)][0][sym]
            w.put(code, ln)
            if s:
                w.put(m, s)
            if not dri:
                symbols.append((pos, ln, s, i))
            pos += ln + s
            cur_mag += s
            magnitude_bits += s
            cur[(cls, t, sym)] = cur.get((cls, t, sym), 0) + 1
    w.flush()
    intervals.append((cur, cur_mag))
    entropy = bytes(w.out)
    info = {"tables": freq, "magnitude_bits": magnitude_bits, "intervals": intervals, "entropy_bytes": len(entropy),
            "stuffed": entropy.count(b"\xff\x00"), "rst_markers": rst, "block_bits": block_bits, "symbols": symbols,
            "header_bytes": len(out), "block_symbols": [(t, [(0, dcat)] + [(1, sym) for sym, _, _ in ac]) for t, dcat, _, ac in parsed]}
    return bytes(out) + entropy + b"\xff\xd9", info


def priced_block_bits(info, lengths):
    """bits of every block -- code words and the magnitude bits behind them -- when info's symbols are coded with `lengths`
    ({(class, identifier): {symbol: code length}}, as parse_baseline reads them from a file's DHT)"""
    return [sum(lengths[(cls, t)][sym] + (sym & 15) for cls, sym in syms) for t, syms in info["block_symbols"]]


def unstuffed_length(info):
    """bytes of entropy-coded data as a decoder sees them: neither stuffing nor markers"""
    return info["entropy_bytes"] - info["stuffed"] - 2 * info["rst_markers"]


def stuffed_offset(entropy, unstuffed_bytes):
    """offset in stuffed entropy data (no RSTn inside) of the byte that follows `unstuffed_bytes` data bytes"""
    p = 0
    for _ in range(unstuffed_bytes):
        p += 2 if entropy[p] == 0xFF else 1
    return p


def parse_baseline(data):
    """A single-scan baseline file -> (lengths {(class, identifier): {symbol: code length}}, scan bytes between the SOS header and the
    marker that ends the scan, RSTn included)"""
    d, p, lengths = bytes(data), 2, {}
    assert d[:2] == b"\xff\xd8"
    while True:
        assert d[p] == 0xFF, p
        marker, n = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        if marker == 0xC4:
            q, end = p + 4, p + 2 + n
            while q < end:
                key, bits = (d[q] >> 4, d[q] & 15), d[q + 1:q + 17]
                q += 17
                tab = {}
                for ln, count in enumerate(bits, 1):
                    for _ in range(count):
                        tab[d[q]] = ln
                        q += 1
                lengths[key] = tab
        if marker == 0xDA:
            break
        p += 2 + n
    p += 2 + n
    q = p
    while not (d[q] == 0xFF and d[q + 1] != 0 and not 0xD0 <= d[q + 1] <= 0xD7):
        q += 1
    return lengths, d[p:q]


def unstuff(scan):
    """the scan's data bytes with the stuffed zeros taken out (scans without RSTn)"""
    return bytes(scan).replace(b"\xff\x00", b"\xff")


def expected_scan_length(info, lengths, scan):
    """What the scan of a file that re-codes info's symbols with `lengths` must measure: per restart interval the code and magnitude bits
    rounded up to a byte, two bytes per RSTn, and one byte for every FF the scan itself stuffs (the one input taken from `scan`)."""
    total = 0
    for counts, mag in info["intervals"]:
        bits = mag + sum(n * lengths[(cls, t)][sym] for (cls, t, sym), n in counts.items())
        total += (bits + 7) // 8
    return total + 2 * (len(info["intervals"]) - 1) + bytes(scan).count(b"\xff\x00")
