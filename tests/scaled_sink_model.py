"""What the INTERLEAVED_U8_SCALED tests share: a model of the reference's three buffer writers, and frames aimed at their edges.

The model restates apps/JpegDecode/JpegBufferOutputWriter8Bit.cs, JpegBufferOutputWriterLessThan8Bit.cs and
JpegBufferOutputWriterGreaterThan8Bit.cs loop by loop (ExpandBits with its `while`, not a closed form), chosen by the precision
the way DecodeAction.cs:41-54 chooses.  It is independent of the product: neither jpeglibrary_amd's writer classes nor its C
replay are used.  Expected images are the oracle's samples (po.block_dequant_idct_shift, po.decode_with_callbacks) through it."""
import functools

import numpy as np

from test_idct_float64_cpu import in_envelope
from test_idct_stage_gpu import _full, _planes, _tables

# ------------------------------------------------------------------------------------------------ the three writers, sample by sample


def clamp(v, lo, hi):  # Math.Clamp
    return lo if v < lo else (hi if v > hi else v)


def fast_expand_bits(bits, bit_count):  # JpegBufferOutputWriterLessThan8Bit.cs:67-73
    remaining_bits = 8 - bit_count
    return ((bits << remaining_bits) | (bits & ((1 << remaining_bits) - 1))) & 0xFFFFFFFF


def expand_bits(bits, bit_count):  # :75-93
    current_bit_count = bit_count
    while current_bit_count < 8:
        bits = ((bits << bit_count) | bits) & 0xFFFFFFFF
        current_bit_count += bit_count
    if current_bit_count > 8:
        bits = bits >> bit_count
        current_bit_count -= bit_count
        bits = fast_expand_bits(bits, current_bit_count)
    return bits


def less_than_8bit_byte(sample, precision):  # :41, :59-60
    value = clamp(sample, 0, (1 << precision) - 1)
    return expand_bits(value, precision) & 0xFF  # (byte)


def greater_than_8bit_byte(sample, precision):  # JpegBufferOutputWriterGreaterThan8Bit.cs:29, :57, :64-67
    return clamp(sample >> (precision - 8), 0, 255)  # (Python's >> of a negative int is the arithmetic shift of C#'s int)


def eight_bit_byte(sample):  # JpegBufferOutputWriter8Bit.cs ClampTo8Bit
    return clamp(sample, 0, 255)


def decode_action_byte(sample, precision):  # DecodeAction.cs:41-54
    if precision == 8:
        return eight_bit_byte(sample)
    if precision < 8:
        return less_than_8bit_byte(sample, precision)
    return greater_than_8bit_byte(sample, precision)


class ModelWriter:
    """One of the three writers (to_byte: sample, precision -> byte; default DecodeAction's choice); WriteBlock as the C# loops"""

    def __init__(self, width, height, precision, component_count, to_byte=None, output=None):
        self.width, self.height, self.precision, self.component_count = width, height, precision, component_count
        self.to_byte = to_byte or decode_action_byte
        self.output = np.zeros(width * height * component_count, np.uint8) if output is None else output

    def WriteBlock(self, block, component_index, x, y):  # noqa: N802
        component_count, width, height, precision = self.component_count, self.width, self.height, self.precision
        if x > width or y > height:
            return
        write_width, write_height = min(width - x, 8), min(height - y, 8)
        destination = y * width * component_count + x * component_count + component_index
        block_off = 0
        for dest_y in range(write_height):
            row = destination + dest_y * width * component_count
            for dest_x in range(write_width):
                self.output[row + dest_x * component_count] = self.to_byte(int(block[block_off + dest_x]), precision)
            block_off += 8

    def image(self):
        return self.output.reshape(self.height, self.width, self.component_count)


@functools.lru_cache(maxsize=None)
def byte_table(precision):
    """decode_action_byte for every int16 sample: table[sample + 32768]"""
    return np.array([decode_action_byte(s, precision) for s in range(-32768, 32768)], np.uint8)


def model_image(frame, planes):
    """[H, W, C] of a frame whose sampling factors are the maximum or 1 (test_idct_stage_gpu._full), through the model"""
    t = byte_table(frame["precision"])
    return np.stack([t[f.astype(np.int32) + 32768] for f in _full(frame, planes)], axis=-1)


# ------------------------------------------------------------------------------------------------ frames aimed at the writers' edges

def edge_targets(precision):
    """the samples either side of every place where the writer's output changes character"""
    if precision < 8:
        return [-1, 0, (1 << precision) - 1, 1 << precision]
    s = precision - 8
    return sorted({-1, 0, (1 << s) - 1, 1 << s, (256 << s) - 1, 256 << s})


def edge_block(rng, q, shift, precision):
    """one zig-zag block for table q: DC-only blocks whose samples land on an edge_target or next to it (exactly with the all-ones
    table, within q[0] / 16 otherwise) or clearly below 0 / above the maximum whatever the table, the int16 wrap, random dense
    blocks, zero blocks (every sample the level shift)"""
    z = np.zeros(64, np.int64)
    kind = rng.random()
    if kind < 0.40:
        target = int(rng.choice(edge_targets(precision))) + int(rng.integers(-1, 2))
        z[0] = int(np.clip(round(8 * (target - shift) / int(q[0])), -32768, 32767))
    elif kind < 0.55:
        margin = int(q[0]) // 8 + 3  # further from the edge than the table's step can miss it by
        top = (1 << precision) - 1 if precision < 8 else (256 << (precision - 8)) - 1
        target = -margin - int(rng.integers(0, 64)) if rng.random() < 0.5 else top + margin
        z[0] = int(np.clip(round(8 * (target - shift) / int(q[0])), -32768, 32767))
    elif kind < 0.67:
        z[0] = rng.choice([32767, -32768, 30000, -30000])  # past the int16 wrap of the (short) cast with q >= 8
    elif kind < 0.92:
        z[:] = rng.integers(-64, 65, 64)
        z[0] = rng.integers(-2048, 2048)
    if int(q.max()) > 255 and not in_envelope(z, q):  # 16-bit tables: inside the int32 envelope (test_idct_stage_gpu._block)
        z[1:] = 0
        z[0] = np.clip(z[0], -4000, 4000)
        if not in_envelope(z, q):
            z[0] = 0
    return z.astype(np.int16)


def edge_frame(rng, w, h, sampling, precision, covered_from=0):
    """(frame dict, tables [4][64], coefficient blocks in MCU scan order, the oracle's planes), like test_idct_stage_gpu._frame
    with edge_block.  A frame of at least `covered_from` pixels is drawn again (tables, selectors and blocks) until the ORACLE's
    visible samples reach every regime of the writer (coverage): which frames the GPU is given depends on the oracle alone."""
    n = len(sampling)
    max_h, max_v = max(s[0] for s in sampling), max(s[1] for s in sampling)
    mcus = (-(-w // (8 * max_h))) * (-(-h // (8 * max_v)))
    shift = 1 << (precision - 1)
    for _ in range(400):
        sel = [int(t) for t in rng.permutation(4)[:n]]
        comps = [(i + 1, hh, vv, sel[i]) for i, (hh, vv) in enumerate(sampling)]
        qt = _tables(rng)
        blocks = np.stack([edge_block(rng, qt[sel[c]], shift, precision) for _ in range(mcus) for c, (hh, vv) in enumerate(sampling) for _ in range(hh * vv)])
        frame = {"width": w, "height": h, "precision": precision, "components": comps}
        planes = _planes(frame, qt, blocks)
        if w * h < covered_from or all(coverage(frame, planes).values()):
            return frame, qt, blocks, planes
    raise AssertionError(("no frame with every regime", w, h, sampling, precision))


def edge_cases(seed, geometries, precision, covered_from=0):
    """([(frame, tables, blocks)], [planes])"""
    rng = np.random.default_rng(seed)
    drawn = [edge_frame(rng, w, h, s, precision, covered_from) for (w, h, s) in geometries]
    return [d[:3] for d in drawn], [d[3] for d in drawn]


def coverage(frame, planes):
    """which regimes of the writer the VISIBLE samples of a frame reach: {below, inside, above, inexact}.  `above` cannot exist
    at P = 15 and 16: an int16 sample shifted by 7 or 8 never exceeds 255 (the wrap makes it negative instead)."""
    p = frame["precision"]
    v = np.concatenate([f.astype(np.int32).reshape(-1) for f in _full(frame, planes)])
    if p < 8:
        mx = (1 << p) - 1
        return {"below": bool((v < 0).any()), "inside": bool(((v >= 0) & (v <= mx)).any()), "above": bool((v > mx).any()), "inexact": True}
    s = p - 8
    t = v >> s
    return {"below": bool((v < 0).any()), "inside": bool(((t >= 0) & (t <= 255)).any()), "above": bool((t > 255).any()) or (256 << s) > 32767,
            "inexact": p == 8 or bool(((v < 0) & ((v & ((1 << s) - 1)) != 0)).any())}


def assert_covered(cases, planes, per_case_from=0):
    """every case with at least `per_case_from` pixels reaches every regime by itself; all cases together do in any event"""
    total = {"below": False, "inside": False, "above": False, "inexact": False}
    for (frame, _, _), pl in zip(cases, planes):
        c = coverage(frame, pl)
        if frame["width"] * frame["height"] >= per_case_from:
            assert all(c.values()), (frame["precision"], frame["width"], frame["height"], frame["components"], c)
        total = {k: total[k] or c[k] for k in total}
    assert all(total.values()), total


# the frame hand-off cases of tests/test_scaled_sink_gpu.py (seeds fixed: the same frames in every session); the CPU test checks
# their coverage with the oracle alone
MATRIX_COVERED_FROM = 1024  # pixels: a 1 x 1 image shows one sample of each component
PRECISION_GEOMETRIES = [(64, 32, [(2, 2), (1, 1), (1, 1)]), (40, 24, [(1, 1)]), (24, 17, [(1, 1), (1, 1), (1, 1)])]


@functools.lru_cache(maxsize=None)
def precision_cases(p):
    return edge_cases(7000 + p, PRECISION_GEOMETRIES, p)


@functools.lru_cache(maxsize=None)
def matrix_cases(p):
    from test_idct_stage_gpu import BIG, GEOMETRIES, TILE_ROWS

    return edge_cases(7100 + p, GEOMETRIES + TILE_ROWS + BIG, p, covered_from=MATRIX_COVERED_FROM)
