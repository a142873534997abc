"""TEST INFRASTRUCTURE ONLY: a literal, serial restatement of the reference's JpegEncoder.Encode() (src/JpegLibrary/JpegEncoder.cs:255-291)
for ANY arrangement AddComponent accepts -- the slow obvious version, block after block, written from the reference's behaviour:

  * WriteScanData (:662-741): ONE block buffer for the whole scan; ReadBlockWithSubsample (:756-799) adds into it, a plain ReadBlock
    overwrites it, ZigZagAndQuantizeBlock writes the coefficients back into it.  Block (x, y) of a component is read at pixel
    ((colMcu * maxH + x) * 8, (rowMcu * maxV + y) * 8).  The buffer starts as zeros (the reference: whatever the stack held).
  * TransformBlocks / BuildHuffmanTables / WritePreparedScanData (:414-656): a JpegBlockAllocator (JpegBlockAllocator.cs:35-114) with its
    dummy block 0 for every block outside a component's own grid; block (x, y) is read at pixel ((colMcu * h + x) * 8 * hs, ...).
    Statistics go to builders only, shared tables add up, a builder without symbols throws "No symbol is recorded.".
  * JpegHuffmanEncodingTable(codes) (JpegHuffmanEncodingTable.cs:21-100): TryWrite writes the last `codeCount` entries, GetCode
    answers a symbol the table does not hold with entry 0.
  * headers from the lists: DQT = SetQuantizationTable order, DHT = SetHuffmanTable order, SOF0 / SOS = AddComponent order.
  * restart intervals: the extension as oracle/jpegenc.c (jref_encode_8bit_dri) defines it.

The arithmetic that is pinned elsewhere comes from the oracle: pyoracle.fdct_quantize_block, pyoracle.build_optimal_table.
"""
import numpy as np

from oracle import pyoracle


class ModelError(Exception):
    def __init__(self, kind, message):
        super().__init__(message)
        self.kind = kind


class Component:
    def __init__(self, component_index, quant_id, dc_id, ac_id, h, v, quant):
        self.component_index, self.quant_id, self.dc_id, self.ac_id, self.h, self.v = component_index, quant_id, dc_id, ac_id, h, v
        self.quant = np.asarray(quant, np.uint16).reshape(64)  # what AddComponent captured


class Arrangement:
    """components: [Component] in AddComponent order; quant_tables: [(identifier, elements)] in SetQuantizationTable order;
    huffman_tables: [(table_class, identifier, codes | None)] in SetHuffmanTable order, codes = [(symbol, code, length)]."""

    def __init__(self, components, quant_tables, huffman_tables, restart_interval=0, most_optimal=False):
        self.components, self.quant_tables, self.huffman_tables = components, quant_tables, huffman_tables
        self.restart_interval, self.most_optimal = restart_interval, most_optimal

    def optimize_coding(self):  # ContainsTableBuilder
        return any(codes is None for _, _, codes in self.huffman_tables)


# ---------------------------------------------------------------------------------------------- tables
class EncodingTable:
    """JpegHuffmanEncodingTable(JpegHuffmanCanonicalCode[] codes)."""

    def __init__(self, codes):
        self.codes = [(int(s), int(c), int(n)) for s, c, n in codes]
        self.symbol_map = [0] * 256
        self.code_count = 0
        for i, (symbol, _, length) in enumerate(self.codes):
            if length != 0:
                self.symbol_map[symbol] = i & 0xFF
                self.code_count += 1

    def dht(self):  # TryWrite
        tail = self.codes[len(self.codes) - self.code_count:]
        return bytes(sum(1 for _, _, n in tail if n == length) & 0xFF for length in range(1, 17)) + bytes(s for s, _, _ in tail)

    def get_code(self, symbol):  # GetCode
        _, code, length = self.codes[self.symbol_map[symbol]]
        return code, length


class BuiltTable:
    """What JpegHuffmanEncodingTableBuilder.Build leaves: the oracle's restatement gives the DHT lists and GetCode for all symbols."""

    def __init__(self, freq, most_optimal):
        try:
            self.bits, self.values, self.code, self.length = pyoracle.build_optimal_table(freq, most_optimal)
        except pyoracle.OracleError as e:
            raise ModelError("InvalidOperationException", str(e))

    def dht(self):
        return bytes(self.bits.tolist()) + bytes(self.values.tolist())

    def get_code(self, symbol):
        return int(self.code[symbol]), int(self.length[symbol])


def canonical_codes(bits, values):
    """JpegStandardHuffmanEncodingTable.BuildCanonicalCode (:85-131): (symbol, code, length) in the order of `values`."""
    lengths = []
    for n, count in enumerate(bits):
        lengths += [n + 1] * count
    out = []
    code, cur = 0, lengths[0]
    for i, (symbol, length) in enumerate(zip(values, lengths)):
        if i > 0:
            code += 1
            if length > cur:
                code <<= length - cur
                cur = length
        out.append((symbol, code, length))
    return out


_STANDARD = None


def standard_tables():
    """The four JpegStandardHuffmanEncodingTable tables as code lists [DC lum, AC lum, DC chr, AC chr]: read out of the DHT the
    (pinned) EncodeAction restatement writes."""
    global _STANDARD
    if _STANDARD is None:
        data = pyoracle.encode_8bit(np.zeros((8, 8, 3), np.uint8), 1, 1, 75)
        at = data.index(b"\xff\xc4") + 4
        tabs = {}
        for _ in range(4):
            tc_th = data[at]
            bits = list(data[at + 1:at + 17])
            n = sum(bits)
            tabs[tc_th] = canonical_codes(bits, list(data[at + 17:at + 17 + n]))
            at += 17 + n
        _STANDARD = [tabs[0x00], tabs[0x10], tabs[0x01], tabs[0x11]]
    return _STANDARD


# ---------------------------------------------------------------------------------------------- writer
class Writer:
    def __init__(self):
        self.out = bytearray()
        self.reg, self.nbits = 0, 0

    def marker(self, m):
        self.out += bytes((0xFF, m))

    def length(self, n):
        self.out += bytes((((n + 2) >> 8) & 0xFF, (n + 2) & 0xFF))

    def bits(self, value, length):  # WriteBits + FlushRegister: FF is followed by 00
        if length == 0:
            return
        self.reg = (self.reg << length) | (value & ((1 << length) - 1))
        self.nbits += length
        while self.nbits >= 8:
            b = (self.reg >> (self.nbits - 8)) & 0xFF
            self.nbits -= 8
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.reg &= (1 << self.nbits) - 1

    def exit_bit_mode(self):  # pad the last byte with one-bits
        if self.nbits:
            self.bits((1 << (8 - self.nbits)) - 1, 8 - self.nbits)


def write_headers(w, arr, width, height, tables):
    w.marker(0xD8)
    w.marker(0xDB)
    w.length(65 * len(arr.quant_tables))
    for identifier, elements in arr.quant_tables:
        w.out.append(identifier & 0xFF)
        w.out += bytes(int(e) & 0xFF for e in elements)
    if arr.restart_interval:
        w.marker(0xDD)
        w.length(2)
        w.out += bytes((arr.restart_interval >> 8, arr.restart_interval & 0xFF))
    nc = len(arr.components)
    w.marker(0xC0)
    w.length(6 + 3 * nc)
    w.out += bytes((8, height >> 8, height & 0xFF, width >> 8, width & 0xFF, nc))
    for c in arr.components:
        w.out += bytes((c.component_index, (c.h << 4) | c.v, c.quant_id))
    w.marker(0xC4)
    body = bytearray()
    for (table_class, identifier, _), t in zip(arr.huffman_tables, tables):
        body.append((table_class << 4) | (identifier & 0xF))
        body += t.dht()
    w.length(len(body))
    w.out += body
    w.marker(0xDA)
    w.length(1 + 2 * nc + 3)
    w.out.append(nc)
    for c in arr.components:
        w.out += bytes((c.component_index, ((c.dc_id << 4) | (c.ac_id & 0xF)) & 0xFF))
    w.out += bytes((0, 63, 0))


# ---------------------------------------------------------------------------------------------- blocks
def reader_read_block(pixels, block, component, x, y):
    """JpegBufferInputReader.ReadBlock (apps/JpegEncode/JpegBufferInputReader.cs:26-50)."""
    height, width = pixels.shape[:2]
    bw, bh = min(width - x, 8), min(height - y, 8)
    if bw != 8 or bh != 8:
        block[:] = 0
    if bw > 0 and bh > 0:
        block.reshape(8, 8)[:bh, :bw] = pixels[y:y + bh, x:x + bw, component]


def read_block(pixels, block, component, x, y, hs, vs):
    """ReadBlock / ReadBlockWithSubsample / CopySubsampleBlock (:743-799): `block` (int16[64]) is NOT cleared."""
    if hs == 1 and vs == 1:
        reader_read_block(pixels, block, component, x, y)
        return
    h_shift, v_shift = hs.bit_length() - 1, vs.bit_length() - 1
    temp = np.zeros(64, np.int16)
    b2 = block.reshape(8, 8)
    for v in range(vs):
        for h in range(hs):
            reader_read_block(pixels, temp, component, x + 8 * h, y + 8 * v)
            box, boy = h << (3 - h_shift), v << (3 - v_shift)
            # block[boy + (yy >> vShift)][box + (xx >> hShift)] += temp[yy][xx] for all 64: short += short wraps, and wrapping sums
            # do not depend on their order, so the pixels of a box are added up first
            box_sums = temp.reshape(8 // vs, vs, 8 // hs, hs).astype(np.int32).sum(axis=(1, 3))
            region = b2[boy:boy + 8 // vs, box:box + 8 // hs]
            region[:] = (region.astype(np.int32) + box_sums).astype(np.int16)
    total = h_shift + v_shift
    if total > 0:
        block[:] = ((block.astype(np.int32) + (1 << (total - 1))) >> total).astype(np.int16)


def bit_count(a):
    return a.bit_length() if a < 0x100 else 8 + (a >> 8).bit_length()


def block_symbols(block, predictor):
    """EncodeBlock / GatherBlockStatistics: [(is_dc, symbol, value bits, bit count)]."""
    out = []

    def run_length(is_dc, run, value):
        a, b = (-value, value - 1) if value < 0 else (value, value)
        n = bit_count(a)
        out.append((is_dc, ((run << 4) | n) & 0xFF, b & ((1 << n) - 1), n))

    run_length(True, 0, int(block[0]) - predictor)
    run = 0
    for i in range(1, 64):
        t = int(block[i])
        if t == 0:
            run += 1
        else:
            while run > 15:
                out.append((False, 0xF0, 0, 0))
                run -= 16
            run_length(False, run, t)
            run = 0
    if run > 0:
        out.append((False, 0x00, 0, 0))
    return out


def _mcu_blocks(arr):
    """(component position, x, y) of every block of an MCU in encode order."""
    return [(ci, x, y) for ci, c in enumerate(arr.components) for y in range(c.v) for x in range(c.h)]


def encode(pixels, arr):
    """pixels: uint8 (H, W, samples per pixel).  Returns (stream, coefficients int16 (blocks, 64) in encode order, in_grid bool (blocks,)):
    on the TransformBlocks path the coefficients are what WritePreparedScanData reads (dummy block included) and in_grid tells
    the blocks that lie inside their component's own grid."""
    pixels = np.ascontiguousarray(pixels, np.uint8)
    if pixels.ndim == 2:
        pixels = pixels.reshape(pixels.shape[0], pixels.shape[1], 1)
    height, width = pixels.shape[:2]
    comps = arr.components
    max_h, max_v = max(c.h for c in comps), max(c.v for c in comps)
    for c in comps:
        c.hs, c.vs = max_h // c.h, max_v // c.v
    mcus_per_line, mcus_per_column = -(-width // (8 * max_h)), -(-height // (8 * max_v))
    n_mcus = mcus_per_line * mcus_per_column
    order = _mcu_blocks(arr)
    n_blocks = n_mcus * len(order)
    coefs = np.zeros((n_blocks, 64), np.int16)
    in_grid = np.ones(n_blocks, bool)

    def slot_of(table_class, identifier):
        for k, (tc, ident, _) in enumerate(arr.huffman_tables):
            if tc == table_class and ident == identifier:
                return k
        raise ModelError("ArgumentException", "Huffman table is not defined.")

    dc_slot = [slot_of(0, c.dc_id) for c in comps]
    ac_slot = [slot_of(1, c.ac_id) for c in comps]
    tables = [None if codes is None else EncodingTable(codes) for _, _, codes in arr.huffman_tables]
    ri = arr.restart_interval

    if arr.optimize_coding():
        # ---- JpegBlockAllocator + TransformBlocks
        hb, vb = (width + 7) // 8, (height + 7) // 8
        grid_w = [-(-hb // c.hs) for c in comps]
        grid_h = [-(-vb // c.vs) for c in comps]
        grid_off, index = [], 1
        for ci in range(len(comps)):
            grid_off.append(index)
            index += grid_w[ci] * grid_h[ci]
        store = np.zeros((index, 64), np.int16)

        def block_ref(ci, bx, by):
            return 0 if bx >= grid_w[ci] or by >= grid_h[ci] else grid_off[ci] + by * grid_w[ci] + bx

        for m in range(n_mcus):
            row_mcu, col_mcu = divmod(m, mcus_per_line)
            for ci, x, y in order:
                c = comps[ci]
                bx, by = col_mcu * c.h + x, row_mcu * c.v + y
                blk = store[block_ref(ci, bx, by)]
                read_block(pixels, blk, ci, bx * 8 * c.hs, by * 8 * c.vs, c.hs, c.vs)
                blk[:] = pyoracle.fdct_quantize_block(blk, c.quant)[0]
        # ---- BuildHuffmanTables: statistics to builders only
        freq = [np.zeros(256, np.uint32) for _ in tables]
        pred = [0] * len(comps)
        for m in range(n_mcus):
            row_mcu, col_mcu = divmod(m, mcus_per_line)
            if ri and m > 0 and m % ri == 0:
                pred = [0] * len(comps)
            for ci, x, y in order:
                c = comps[ci]
                blk = store[block_ref(ci, col_mcu * c.h + x, row_mcu * c.v + y)]
                for is_dc, symbol, _, _ in block_symbols(blk, pred[ci]):
                    k = dc_slot[ci] if is_dc else ac_slot[ci]
                    if tables[k] is None:
                        freq[k][symbol] += 1
                pred[ci] = int(blk[0])
        tables = [BuiltTable(freq[k], arr.most_optimal) if t is None else t for k, t in enumerate(tables)]  # BuildTables, in list order
        w = Writer()
        write_headers(w, arr, width, height, tables)
        # ---- WritePreparedScanData
        pred = [0] * len(comps)
        rst, n = 0, 0
        for m in range(n_mcus):
            row_mcu, col_mcu = divmod(m, mcus_per_line)
            if ri and m > 0 and m % ri == 0:
                w.exit_bit_mode()
                w.marker(0xD0 + (rst & 7))
                rst += 1
                pred = [0] * len(comps)
            for ci, x, y in order:
                c = comps[ci]
                ref = block_ref(ci, col_mcu * c.h + x, row_mcu * c.v + y)
                blk = store[ref]
                coefs[n] = blk
                in_grid[n] = ref != 0
                n += 1
                for is_dc, symbol, value, nbits in block_symbols(blk, pred[ci]):
                    code, length = tables[dc_slot[ci] if is_dc else ac_slot[ci]].get_code(symbol)
                    w.bits(code, length)
                    w.bits(value, nbits)
                pred[ci] = int(blk[0])
        w.exit_bit_mode()
    else:
        w = Writer()
        write_headers(w, arr, width, height, tables)
        # ---- WriteScanData: one block buffer
        buffer = np.zeros(64, np.int16)
        pred = [0] * len(comps)
        rst, n = 0, 0
        for m in range(n_mcus):
            row_mcu, col_mcu = divmod(m, mcus_per_line)
            if ri and m > 0 and m % ri == 0:
                w.exit_bit_mode()
                w.marker(0xD0 + (rst & 7))
                rst += 1
                pred = [0] * len(comps)
            for ci, x, y in order:
                c = comps[ci]
                read_block(pixels, buffer, ci, (col_mcu * max_h + x) * 8, (row_mcu * max_v + y) * 8, c.hs, c.vs)
                buffer[:] = pyoracle.fdct_quantize_block(buffer, c.quant)[0]
                coefs[n] = buffer
                n += 1
                for is_dc, symbol, value, nbits in block_symbols(buffer, pred[ci]):
                    code, length = tables[dc_slot[ci] if is_dc else ac_slot[ci]].get_code(symbol)
                    w.bits(code, length)
                    w.bits(value, nbits)
                pred[ci] = int(buffer[0])
        w.exit_bit_mode()
    w.marker(0xD9)
    return bytes(w.out), coefs, in_grid


def header(arr, width, height):
    """SOI .. SOS of the WriteScanData path (every table given)."""
    w = Writer()
    write_headers(w, arr, width, height, [EncodingTable(codes) for _, _, codes in arr.huffman_tables])
    return bytes(w.out)


# ---------------------------------------------------------------------------------------------- the EncodeAction arrangement
STD_LUMINANCE = (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
                 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101,
                 103, 99)  # T.81 Table K.1, zig-zag
STD_CHROMINANCE = (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66) + (99,) * 50  # Table K.2


def scale_by_quality(table, quality):  # JpegStandardQuantizationTable.ScaleByQuality (:64-87)
    scale = 5000 // quality if quality < 50 else 200 - quality * 2
    return [min(max((x * scale + 50) // 100, 1), 255) for x in table]


def encode_action(h, v, components, quality, optimize_coding=False, restart_interval=0, most_optimal=False):
    """apps/JpegEncode/EncodeAction.cs:38-63 as an Arrangement."""
    lum, chrom = scale_by_quality(STD_LUMINANCE, quality), scale_by_quality(STD_CHROMINANCE, quality)
    std = [None] * 4 if optimize_coding else standard_tables()
    comps = [Component(1, 0, 0, 0, h, v, lum)]
    if components == 3:
        comps += [Component(2, 1, 1, 1, 1, 1, chrom), Component(3, 1, 1, 1, 1, 1, chrom)]
    return Arrangement(comps, [(0, lum), (1, chrom)], [(0, 0, std[0]), (1, 0, std[1]), (0, 1, std[2]), (1, 1, std[3])], restart_interval,
                       most_optimal)
