"""tests/marker_index_model.py without a GPU: the restatement on known answers written out by hand, pinned to the reference's decoder
through the oracle, and the case writer's own promises (tests/test_marker_index_gpu.py trusts all three)."""
import numpy as np
import pytest

import jpeglibrary_amd as jl
import marker_index_model as mm
from oracle import pyoracle as po
from tools import jpegsynth

H = bytes.fromhex


def _answer(udata, ends, ends_u, terminator, decoded_mcus, end_pos):
    return dict(udata=H(udata), ends=ends, ends_u=ends_u, n_ends=len(ends), terminator=terminator, decoded_mcus=decoded_mcus, end_pos=end_pos, ulen=ends_u[-1])


# (data, dri, n_intervals, total_mcus) -> the index, worked out by hand from JpegBitReader.cs:95-138 and common.h's DevScanStatus
KNOWN = {
    "plain bytes, EOI": (("01 02 03 ff d9", 0, 1, 6), _answer("01 02 03 ff ff", [3], [3], 0xD9, 6, 3)),
    "stuffed byte": (("01 ff 00 02 ff d9", 0, 1, 6), _answer("01 ff 02 ff ff", [4], [3], 0xD9, 6, 4)),
    "fill in front of a stuffed byte": (("01 ff ff ff 00 02 ff d9", 0, 1, 6), _answer("01 ff 02 ff ff", [6], [3], 0xD9, 6, 6)),
    "fill in front of EOI": (("01 ff ff ff d9 05", 0, 1, 6), _answer("01 ff ff", [3], [1], 0xD9, 6, 3)),
    "entries, then EOI": (("01 ff d0 02 03 ff d1 ff d9", 2, 4, 7), _answer("01 ff ff 02 03 ff ff ff ff", [1, 5, 7], [1, 5, 7], 0xD9, 6, 7)),
    "fill in front of an entry": (("01 ff ff d0 02 ff d9", 1, 3, 3), _answer("01 ff ff 02 ff ff", [2, 5], [1, 4], 0xD9, 2, 5)),
    "empty intervals": (("ff d0 ff d1 ff d2 ff d9", 1, 9, 9), _answer("ff ff ff ff ff ff ff ff", [0, 2, 4, 6], [0, 2, 4, 6], 0xD9, 4, 6)),
    "the n-th RST closes": (("01 ff d0 02 ff d1 03 ff d2 ff d9", 1, 2, 2), _answer("01 ff ff 02 ff ff", [1, 4], [1, 4], 0xD1, 2, 4)),
    "an RST ends a DRI 0 scan": (("01 02 ff d3 04 ff d9", 0, 1, 5), _answer("01 02 ff ff", [2], [2], 0xD3, 5, 2)),
    "a COM ends the scan": (("01 ff fe 00 02 ff d9", 4, 3, 9), _answer("01 ff ff", [1], [1], 0xFE, 4, 1)),
    "behind the terminator nothing counts": (("01 ff d9 ff d0 ff 00 ff d1", 1, 5, 5), _answer("01 ff ff", [1], [1], 0xD9, 1, 1)),
    "the data runs out": (("01 02 03", 1, 3, 3), _answer("01 02 03 ff ff", [3], [3], 0, 1, 3)),
    "it runs out behind an FF": (("01 02 ff", 0, 1, 4), _answer("01 02 ff ff", [3], [2], 0, 4, 3)),
    "it runs out behind FF FF": (("01 ff ff", 0, 1, 4), _answer("01 ff ff", [3], [1], 0, 4, 3)),
    "it runs out behind FF 00": (("01 ff 00", 0, 1, 4), _answer("01 ff ff ff", [3], [2], 0, 4, 3)),
    "it runs out behind an entry": (("01 ff d0", 1, 3, 3), _answer("01 ff ff ff ff", [1, 3], [1, 3], 0, 2, 3)),
    "no data at all": (("", 1, 3, 3), _answer("ff ff", [0], [0], 0, 1, 0)),
    "covered MCUs stop at the frame's": (("01 ff d0 02 ff d9", 5, 2, 7), _answer("01 ff ff 02 ff ff", [1, 4], [1, 4], 0xD9, 7, 4)),
}


@pytest.mark.parametrize("name", list(KNOWN))
def test_model_on_known_answers(name):
    (data, dri, n_intervals, total_mcus), want = KNOWN[name]
    assert mm.model(H(data), dri, n_intervals, total_mcus) == want


def _scan_data_at(f):
    at = f.rindex(b"\xff\xda")
    return at + 2 + int.from_bytes(f[at + 2:at + 4], "big")


@pytest.mark.parametrize("shape", [(200, 120, "420", 97, 1), (136, 104, "444", 95, 0), (152, 96, "422", 96, 3)])
@pytest.mark.parametrize("fill", [False, True])
def test_model_is_what_the_reference_decodes(shape, fill):
    """independent of the kernel and of the hand-made answers: a segment rebuilt from the model's output alone (FF re-stuffed, the
    marker bytes back at the entries) decodes, in the reference's restatement, to the samples of the file it came from"""
    w, h, ss, q, dri = shape
    f = bytes(jpegsynth.encode(w, h, ss, q, dri, seed=w))
    if fill:
        f = mm.insert_fill(f, seed=h)
        assert f.count(b"\xff\xff") > 20
    at = _scan_data_at(f)
    mcu = {"420": (16, 16), "444": (8, 8), "422": (16, 8)}[ss]
    total = -(-w // mcu[0]) * -(-h // mcu[1])
    n = -(-total // dri) if dri else 1
    m = mm.model(f[at:], dri, n, total)
    assert m["terminator"] == 0xD9 and m["n_ends"] == n and m["decoded_mcus"] == total and m["end_pos"] == len(f) - at - 2
    rebuilt = f[:at] + mm.rebuild(m, f[at:])
    assert b"\xff\xff" not in rebuilt[at:] and len(rebuilt) <= len(f) and (fill or rebuilt == f)
    assert np.array_equal(po.decode_8bit(rebuilt)[0], po.decode_8bit(f)[0])
    assert mm.model(rebuilt[at:], dri, n, total)["udata"] == m["udata"]


def test_fill_insertion_changes_no_sample():
    f = bytes(jpegsynth.encode(120, 88, "420", 98, 1, seed=3))
    e = mm.insert_fill(f, seed=9)
    assert len(e) > len(f) and np.array_equal(po.decode_8bit(e)[0], po.decode_8bit(f)[0])


def test_case_writer_keeps_its_promises():
    cases = mm.corpus()
    assert len({c.name for c in cases}) == len(cases) and {c.family for c in cases} == set(mm.FAMILIES)
    for c in cases:
        c.check_instances()  # the instances are where they claim
        assert (c.data_pos - c.misalign) % 16 == 0 and 0 <= c.misalign < 16
        # outside the instances the segment holds no FF (the long segment is random bytes with every FF stuffed)
        seg = bytearray(c.file[c.data_pos:c.data_pos + c.seg_len])
        for _, at, pat in c.instances:
            seg[at - c.misalign:at - c.misalign + len(pat)] = bytes(len(pat))
        assert c.family == "long" or 0xFF not in seg, c.name
        ends = sorted((at, at + len(pat)) for _, at, pat in c.instances)
        assert all(b[0] - a[1] >= 64 for a, b in zip(ends, ends[1:])), c.name
    assert mm.segment_bytes() < 31 << 20
    assert mm.long_case().seg_len >= 66 * mm.GROUP + 65536


def test_cases_the_host_refuses_are_the_ones_the_writer_names():
    """a cut file passes Identify() only when its last bytes are a marker (JpegDecoder.cs:88-97): the cases say which"""
    for c in mm.corpus():
        d = jl.JpegDecoder(host_only=True)
        d.SetInput(c.file)
        try:
            d.Identify()
            ok = True
        except jl.InvalidDataException:
            ok = False
        assert ok == c.identify_ok, c.name
        if ok:
            assert (d.Width, d.Height, d.GetRestartInterval()) == (c.width, c.height, c.dri), c.name


def test_the_interesting_cases_are_what_they_are_named_for():
    """the model itself says that a case reaches the rule it is named for"""
    by_name = {c.name: c for c in mm.corpus()}
    m = mm.expected(by_name["cap/closing@group1|2-1"])
    assert m["n_ends"] == 6 and m["terminator"] == 0xD5 and m["end_pos"] + by_name["cap/closing@group1|2-1"].misalign == 2 * mm.GROUP - 1
    m = mm.expected(by_name["cut/ffd3@chunk+0/dri1"])
    assert m["terminator"] == 0 and m["n_ends"] == 3 and m["ends"][-1] == m["end_pos"] == len(by_name["cut/ffd3@chunk+0/dri1"].data)
    m = mm.expected(by_name["term/rst_dri0@wave-1/dri0"])
    assert m["terminator"] == 0xD4 and m["n_ends"] == 1
    c = by_name["term/sos2@chunk+0/dri1"]
    assert mm.expected(c, 1)["terminator"] == 0xD9 and mm.expected(c, 1)["ends"] == [40]
    long = mm.expected(mm.long_case())
    gaps = np.diff(long["ends"])
    assert long["terminator"] == 0xD9 and long["n_ends"] > 5000 and gaps.min() >= 40 and gaps.max() < 800
