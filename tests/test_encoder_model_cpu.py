"""The general encoder's test model (encoder_model.py) pinned against the oracle, and the library's host-only header entry
(jpgpu_encode_description_header) pinned against the model.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import encoder_arrangements as ea
import encoder_model as em
from oracle import pyoracle


@pytest.mark.parametrize("width,height", [(16, 16), (37, 29), (90, 41), (61, 35)])
def test_model_is_the_encode_action_restatement_on_its_family(width, height):
    """Byte for byte what pyoracle.encode_8bit (oracle/jpegenc.c) writes: luma 1x1 / 2x1 / 2x2 / 4x4, one and three components,
    standard and built tables, restart intervals 0, 1, 3."""
    px = ea.pixels(width, height, 3, 100 + width)
    for h, v in ((1, 1), (2, 1), (2, 2), (4, 4)):
        for components in (1, 3):
            img = px if components == 3 else px[:, :, :1]
            for optimize in (False, True):
                for ri in (0, 1, 3):
                    arr = em.encode_action(h, v, components, 75, optimize, ri)
                    what = (h, v, components, optimize, ri)
                    if optimize and components == 1:  # the chrominance builders stay empty
                        with pytest.raises(pyoracle.OracleError):
                            pyoracle.encode_8bit(img, h, v, 75, optimize_coding=True, restart_interval=ri)
                        with pytest.raises(em.ModelError, match="No symbol is recorded."):
                            em.encode(img, arr)
                        continue
                    ref, ref_coefs = pyoracle.encode_8bit(img, h, v, 75, want_coefficients=True, optimize_coding=optimize, restart_interval=ri)
                    got, coefs, _ = em.encode(img, arr)
                    assert np.array_equal(coefs, ref_coefs), what
                    assert got == ref, what


@pytest.mark.parametrize("name", ["A", "C", "E"])
@pytest.mark.parametrize("built", [False, True])
def test_general_streams_decode_to_the_models_coefficients(name, built):
    """At most ten blocks per MCU: the (golden-pinned) decoder restatement reads back what the model says it wrote."""
    for width, height in ea.SIZES[name]:
        if width * height > 100 * 100:
            width, height = 72, 40  # (the CPU decode of the large size adds nothing here)
        px = ea.pixels(width, height, len(ea.SAMPLING[name]), 7)
        stream, coefs, in_grid = em.encode(px, ea.arrangement(name, built))
        decoded, _ = pyoracle.decode_coefficients(stream)
        assert decoded.shape == coefs.shape
        assert np.array_equal(decoded[in_grid], coefs[in_grid]), (name, built, width, height)
        if not built:
            assert in_grid.all()


def _header(desc):
    from jpeglibrary_amd import encoder

    return encoder.description_header(desc)


def _header_cases():
    cases = []
    for name in "ABCDEJ":
        for width, height in ea.SIZES[name]:
            cases.append((name, ea.arrangement(name), width, height))
            cases.append((name + "-dri", ea.arrangement(name, restart_interval=3), width, height))
    for name in "BC":
        cases.append((name + "-identifiers", ea.identifiers(name), 90, 41))
    return cases


def test_header_entry_writes_the_models_bytes():
    """SOI, DQT, (DRI,) SOF0, DHT, SOS of the WriteScanData path for every arrangement of the GPU tests -- without a device."""
    for what, arr, width, height in _header_cases():
        rc, message, data = _header(ea.to_description(arr, width, height))
        assert rc == 0, (what, rc, message)
        assert data == em.header(arr, width, height), what
    # a given table that is no standard table: entries without a code in front, symbols missing
    codes = [(5, 0, 0), (0, 0b0, 1), (1, 0b10, 2), (0xF0, 0b110, 3), (0x11, 0b1110, 4)]
    arr = ea.arrangement("A")
    arr.huffman_tables[1] = (1, 0, codes)
    rc, message, data = _header(ea.to_description(arr, 37, 29))
    assert rc == 0 and data == em.header(arr, 37, 29)
    # the EncodeAction arrangement: what the oracle writes in front of its scan
    ref = pyoracle.encode_8bit(ea.pixels(90, 41, 3, 1), 2, 2, 75)
    rc, message, data = _header(ea.to_description(ea.arrangement("B"), 90, 41))
    assert rc == 0 and ref.startswith(data) and data.endswith(b"\x00\x3f\x00")


def test_header_entry_reports_what_an_encode_would():
    from jpeglibrary_amd import _capi

    # tables to be built: the DHT depends on the image
    rc, message, data = _header(ea.to_description(ea.arrangement("C", built=True), 90, 41))
    assert (rc, data) == (_capi.OK, b"")
    # no component at the maximum factors in both directions: the one fence, on both paths
    for built in (False, True):
        rc, message, data = _header(ea.to_description(ea.arrangement("F", built), 40, 24))
        assert rc == _capi.ERR_NOT_SUPPORTED and "maximum sampling" in message and data == b""
    # a builder no component feeds
    rc, message, data = _header(ea.to_description(ea.unused_builder("B"), 90, 41))
    assert (rc, message, data) == (_capi.ERR_INVALID_OPERATION, "No symbol is recorded.", b"")

    def status(change, arr=None):
        d = ea.to_description(arr or ea.arrangement("B"), 90, 41)
        change(d)
        rc, message, _ = _header(d)
        return rc, message

    def set_(path, value):
        def change(d):
            obj = d
            for p in path[:-1]:
                obj = getattr(obj, p) if isinstance(p, str) else obj[p]
            setattr(obj, path[-1], value)
        return change

    arg = _capi.ERR_ARGUMENT
    assert status(set_(("components", 1, "h"), 3)) == (arg, "Subsampling factor can only be 1, 2 or 4.")
    assert status(set_(("components", 2, "component_index"), 1)) == (arg, "The component index is already used by another component.")
    assert status(set_(("components", 0, "td"), 5)) == (arg, "Huffman table is not defined.")
    assert status(set_(("components", 0, "ta"), 5)) == (arg, "Huffman table is not defined.")
    assert status(set_(("width",), 0))[0] == arg
    assert status(set_(("height",), 65536))[0] == arg
    assert status(set_(("num_components",), 5))[0] == arg
    assert status(set_(("num_components",), 0)) == (_capi.ERR_INVALID_OPERATION, "No component is specified.")
    assert status(set_(("in_components",), 2))[0] == arg
    assert status(set_(("input_rgb",), 3))[0] == arg
    assert status(set_(("input_rgb",), 1), ea.arrangement("A"))[0] == arg  # RGB input needs exactly three components
    assert status(set_(("restart_interval",), 65536))[0] == arg
    assert status(set_(("num_quant_tables",), 9))[0] == arg
    assert status(set_(("num_huffman_tables",), 0))[0] == arg
    assert status(lambda d: d.components[0].quant.__setitem__(5, 0))[0] == arg
    assert status(lambda d: d.quant_tables[1].elements.__setitem__(63, 256))[0] == arg
    assert status(set_(("huffman_tables", 2, "identifier"), 0))[0] == _capi.ERR_INVALID_OPERATION  # AddTable of a pair that exists
    assert status(lambda d: d.huffman_tables[0].length.__setitem__(0, 17))[0] == arg
    # a destination that is too small: the size needed comes back
    d = ea.to_description(ea.arrangement("B"), 90, 41)
    n = C.c_size_t(0)
    assert _capi.lib.jpgpu_encode_description_header(C.byref(d), None, 0, C.byref(n), None, 0) == arg
    assert n.value == len(em.header(ea.arrangement("B"), 90, 41))
    assert _capi.lib.jpgpu_encode_description_header(None, None, 0, C.byref(n), None, 0) == arg


def test_description_structs_have_the_librarys_sizes():
    from jpeglibrary_amd import _capi

    for name, mirror in (("component", _capi.EncodeComponent), ("quant_table", _capi.EncodeQuantTable), ("huffman_table", _capi.EncodeHuffmanTable),
                         ("description", _capi.EncodeDescription)):
        assert getattr(_capi.lib, "jpgpu_sizeof_encode_" + name)() == C.sizeof(mirror)
