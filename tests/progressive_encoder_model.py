"""A serial model of libjpeg's optimal Huffman tables and its progressive entropy coder (include/jpgpu.h, 4e), on top of
libjpeg_encoder_model.quantised_blocks: what coding="optimized" and coding="progressive" of the libjpeg arithmetic write, byte for byte.

    optimal_table(freq)          jpeg_gen_optimal_table: (bits[16], values)
    scan_script(components)      jpeg_simple_progression: [(component indices, Ss, Se, Ah, Al)]
    scan_blocks(...)             the blocks of a scan in the order the scan visits them
    encode_progressive(pixels)   the whole SOF2 file
    encode_optimized(pixels)     the whole SOF0 file with tables built from the image
    COUNTERS                     how often each flush reason fired in the last encode_progressive call
"""
import numpy as np

import libjpeg_encoder_model as M

COUNTERS = {}


def _reset_counters():
    COUNTERS.clear()
    COUNTERS.update(block_flush=0, eobrun_limit=0, be_limit=0, scan_end=0, zrl_flush=0, cross_256=0, max_run=0)


# ---------------------------------------------------------------------------------------------- optimal tables
def optimal_table(freq):
    """jpeg_gen_optimal_table: freq[256] -> (bits[16], values).  Symbol 256 is the pseudo-symbol that keeps the all-ones code free.
    A histogram without any symbol gives the empty table."""
    if not any(int(x) for x in freq):
        return [0] * 16, []
    f = [int(x) for x in freq] + [1]
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, 1 << 62
        for i in range(257):  # least non-zero frequency, the largest index among equals
            if f[i] and f[i] <= v:
                v, c1 = f[i], i
        c2, v = -1, 1 << 62
        for i in range(257):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            assert codesize[i] <= 32
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
                assert j > 0
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    values = [s for size in range(1, 33) for s in range(256) if codesize[s] == size]
    return bits[1:17], values


def longest_unlimited_code(freq):
    """The longest code length before the limit to 16 is applied (what a test asserts to be above 16)."""
    f = [int(x) for x in freq] + [1]
    import heapq

    heap = [(w, 0) for w in f if w]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


# ---------------------------------------------------------------------------------------------- scans
def scan_script(components):
    """jpeg_simple_progression as Pillow's files show it: (component indices, Ss, Se, Ah, Al)"""
    if components == 3:
        return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
    return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


def scan_blocks(width, height, components, luma, comps):
    """[(component, block index in quantised_blocks' order)] as the scan visits them: an interleaved scan in MCU order with its
    dummy blocks, a one-component scan over the component's real blocks in raster order."""
    max_h, max_v, mpl, mpc, bpm = M.geometry(width, height, components, luma)
    if len(comps) > 1:
        ny = max_h * max_v
        return [(0 if b < ny else b - ny + 1, mcu * bpm + b) for mcu in range(mpl * mpc) for b in range(bpm)]
    c = comps[0]
    h, v = (max_h, max_v) if c == 0 else (1, 1)
    wc, hc = -(-width * h // max_h), -(-height * v // max_v)
    wb, hb = -(-wc // 8), -(-hc // 8)
    first = 0 if c == 0 else max_h * max_v + c - 1
    return [(c, ((by // v) * mpl + bx // h) * bpm + first + (by % v) * h + bx % h) for by in range(hb) for bx in range(wb)]


class _Sink:
    """Counts symbols (codes None) or writes them."""

    def __init__(self, codes=None):
        self.codes, self.freq, self.w = codes, {}, M._Bits()

    def symbol(self, table, s):
        if self.codes is None:
            self.freq.setdefault(table, [0] * 256)[s] += 1
        else:
            self.w.put(*self.codes[table][s])

    def bits(self, value, n):
        if self.codes is not None and n:
            self.w.put(value, n)


def _code_scan(blocks, order, spec, sink):
    """One scan of jcphuff.c over `order` = scan_blocks(...)"""
    comps, ss, se, ah, al = spec
    if ss == 0:
        pred = [0, 0, 0]
        for c, b in order:
            v = int(blocks[b][0]) >> al
            if ah:
                sink.bits(v & 1, 1)
                continue
            n, extra = M._magnitude(v - pred[c])
            pred[c] = v
            sink.symbol(("dc", 0 if c == 0 else 1), n)
            sink.bits(extra, n)
        return
    table = ("ac", 0 if comps[0] == 0 else 1)
    state = {"run": 0, "be": []}

    def flush(reason):
        if state["run"]:
            COUNTERS[reason] += 1
            COUNTERS["max_run"] = max(COUNTERS["max_run"], state["run"])
            n = state["run"].bit_length() - 1
            sink.symbol(table, n << 4)
            sink.bits(state["run"], n)
            state["run"] = 0
            for bit in state["be"]:
                sink.bits(bit, 1)
            state["be"] = []

    for at, (c, b) in enumerate(order):
        coef = [int(x) for x in blocks[b]]
        if ah == 0:
            r = 0
            for k in range(ss, se + 1):
                t = abs(coef[k]) >> al
                if t == 0:
                    r += 1
                    continue
                flush("block_flush")
                while r > 15:
                    sink.symbol(table, 0xF0)
                    r -= 16
                n = t.bit_length()
                sink.symbol(table, (r << 4) + n)
                sink.bits(t if coef[k] >= 0 else ~t, n)
                r = 0
            if r > 0:
                state["run"] += 1
                if state["run"] == 0x7FFF:
                    flush("eobrun_limit")
        else:
            absv = {k: abs(coef[k]) >> al for k in range(ss, se + 1)}
            eob = max([k for k in absv if absv[k] == 1] or [0])
            r, br = 0, []
            for k in range(ss, se + 1):
                t = absv[k]
                if t == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    flush("zrl_flush")
                    sink.symbol(table, 0xF0)
                    r -= 16
                    for bit in br:
                        sink.bits(bit, 1)
                    br = []
                if t > 1:
                    br.append(t & 1)
                    continue
                flush("block_flush")
                sink.symbol(table, (r << 4) + 1)
                sink.bits(0 if coef[k] < 0 else 1, 1)
                for bit in br:
                    sink.bits(bit, 1)
                br, r = [], 0
            if r > 0 or br:
                state["run"] += 1
                state["be"] += br
                if state["run"] == 0x7FFF:
                    flush("eobrun_limit")
                elif len(state["be"]) > 937:
                    flush("be_limit")
        if state["run"]:  # a run that goes on into the next block: does it cross a multiple of 256 blocks of the scan?
            if (at + 1) % 256 == 0 and at + 1 < len(order):
                COUNTERS["cross_256"] += 1
    flush("scan_end")


def _dht(table, bits, values):
    kind, ident = table
    return M._segment(0xC4, bytes([((1 if kind == "ac" else 0) << 4) | ident]) + bytes(bits) + bytes(values))


def _frame_header(width, height, components, luma, qt, sof):
    max_h, max_v = luma if components == 3 else (1, 1)
    h = b"\xff\xd8" + M._segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if components == 3 else 1):
        h += M._segment(0xDB, bytes([t]) + bytes(int(x) for x in qt[t]))
    body = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([components])
    for c in range(components):
        body += bytes([c + 1, (max_h << 4 | max_v) if c == 0 else 0x11, 0 if c == 0 else 1])
    return h + M._segment(sof, body)


def _prepare(pixels, luma, quality, rgb, tables):
    a = np.asarray(pixels, np.uint8)
    height, width = a.shape[:2]
    components = 1 if a.ndim == 2 or a.shape[2] == 1 else 3
    qt = M.quant_tables(quality) if tables is None else [np.asarray(t, np.uint16).reshape(64) for t in tables]
    return a, width, height, components, qt, M.quantised_blocks(a, luma, quality, rgb, qt)


def encode_progressive(pixels, luma=(2, 2), quality=75, rgb=True, tables=None, blocks=None):
    """The whole file of Image.save(..., progressive=True)."""
    _reset_counters()
    a, width, height, components, qt, model_blocks = _prepare(pixels, luma, quality, rgb, tables)
    blocks = model_blocks if blocks is None else blocks
    out = bytearray(_frame_header(width, height, components, luma, qt, 0xC2))
    for spec in scan_script(components):
        comps, ss, se, ah, al = spec
        order = scan_blocks(width, height, components, luma, comps)
        keep = dict(COUNTERS)
        stats = _Sink()
        _code_scan(blocks, order, spec, stats)
        COUNTERS.update(keep)  # (the statistics pass takes the same road: count it once)
        codes = {}
        for table in sorted(stats.freq, key=lambda t: t[1]):  # DC0 then DC1; an AC scan has one table
            bits, values = optimal_table(stats.freq[table])
            codes[table] = M.huffman_codes(bits, values)
            out += _dht(table, bits, values)
        sos = bytes([len(comps)])
        for c in comps:
            t = 0 if c == 0 else 1
            sos += bytes([c + 1, t if ss else (0 if ah else t << 4)])  # (a DC refinement scan names no table)
        out += M._segment(0xDA, sos + bytes([ss, se, (ah << 4) | al]))
        sink = _Sink(codes)
        _code_scan(blocks, order, spec, sink)
        sink.w.flush()
        out += sink.w.out
    return bytes(out + b"\xff\xd9")


def _sequential(blocks, width, height, components, luma, restart_interval, sink, out):
    max_h, max_v, mpl, mpc, bpm = M.geometry(width, height, components, luma)
    ny = bpm - (2 if components == 3 else 0)
    pred = [0, 0, 0]
    for mcu in range(mpl * mpc):
        if restart_interval and mcu and mcu % restart_interval == 0:
            if out is not None:
                sink.w.flush()
                out += sink.w.out + bytes((0xFF, 0xD0 + (mcu // restart_interval - 1) % 8))
                sink.w = M._Bits()
            pred = [0, 0, 0]
        for b in range(bpm):
            comp = 0 if b < ny else b - ny + 1
            t = 0 if comp == 0 else 1
            blk = [int(x) for x in blocks[mcu * bpm + b]]
            n, extra = M._magnitude(blk[0] - pred[comp])
            pred[comp] = blk[0]
            sink.symbol(("dc", t), n)
            sink.bits(extra, n)
            run = 0
            for k in range(1, 64):
                if blk[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    sink.symbol(("ac", t), 0xF0)
                    run -= 16
                n, extra = M._magnitude(blk[k])
                sink.symbol(("ac", t), (run << 4) | n)
                sink.bits(extra, n)
                run = 0
            if run:
                sink.symbol(("ac", t), 0)


def encode_optimized(pixels, luma=(2, 2), quality=75, rgb=True, restart_interval=0, tables=None):
    """The whole file of Image.save(..., optimize=True)."""
    a, width, height, components, qt, blocks = _prepare(pixels, luma, quality, rgb, tables)
    stats = _Sink()
    _sequential(blocks, width, height, components, luma, restart_interval, stats, None)
    out = bytearray(_frame_header(width, height, components, luma, qt, 0xC0))
    codes = {}
    for t in range(2 if components == 3 else 1):  # DC0, AC0, DC1, AC1
        for kind in ("dc", "ac"):
            bits, values = optimal_table(stats.freq[(kind, t)])
            codes[(kind, t)] = M.huffman_codes(bits, values)
            out += _dht((kind, t), bits, values)
    if restart_interval:
        out += M._segment(0xDD, restart_interval.to_bytes(2, "big"))
    sos = bytes([components])
    for c in range(components):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    out += M._segment(0xDA, sos + b"\x00\x3f\x00")
    sink = _Sink(codes)
    _sequential(blocks, width, height, components, luma, restart_interval, sink, out)
    sink.w.flush()
    return bytes(out + sink.w.out + b"\xff\xd9")


def split_markers(data):
    """[(marker, offset, length)] of a JPEG file's segments, the entropy-coded data counted to the SOS in front of it: what a byte
    mismatch is named by."""
    out, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        m = data[i + 1]
        if m == 0xD9:
            break
        n = int.from_bytes(data[i + 2:i + 4], "big") + 2
        if m == 0xDA:
            j = i + n
            while j + 1 < len(data) and not (data[j] == 0xFF and data[j + 1] != 0 and not 0xD0 <= data[j + 1] <= 0xD7):
                j += 1
            n = j - i
        out.append((m, i, n))
        i += n
    return out


def describe_mismatch(got, want):
    """A sentence naming the first segment in which two files differ."""
    if got == want:
        return "equal"
    a, b = split_markers(got), split_markers(want)
    scan = 0
    for k, ((ma, ia, na), (mb, ib, nb)) in enumerate(zip(a, b)):
        scan += ma == 0xDA
        if ma != mb or got[ia:ia + na] != want[ib:ib + nb]:
            return "segment %d (FF%02X / FF%02X, scan %d): %d bytes at %d against %d bytes at %d" % (k, ma, mb, scan, na, ia, nb, ib)
    return "%d segments against %d, lengths %d against %d" % (len(a), len(b), len(got), len(want))
