"""Orientation without a GPU: the model's table against Pillow, the Exif rule (jpgpu_identify_orientation) against Pillow and case by case, the
new symbols and the argument checks that need no device, and the stand-alone sanitizer harness of the rule (tools/fuzz/exif_orientation_asan.cpp)."""
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from jpeglibrary_amd.errors import InvalidOperationException
import color_model as cm
import orient_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["jpgpu_batch_set_orientation_policy", "jpgpu_batch_set_orientations", "jpgpu_batch_image_orientation", "jpgpu_identify_orientation"]


def _plain(w=16, h=8):
    return cm.pillow_jpeg(w, h, "RGB")


# ------------------------------------------------------------------------------------------------ the table

@pytest.mark.parametrize("shape", [(5, 7), (1, 3), (3, 1), (1, 1)])
@pytest.mark.parametrize("o", om.ORIENTATIONS)
def test_the_model_is_pillows_exif_transpose(o, shape):
    from PIL import Image, ImageOps

    h, w = shape
    a = np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3)
    im = Image.fromarray(a, "RGB")
    exif = Image.Exif()
    exif[0x0112] = o
    im.info["exif"] = exif.tobytes()
    im.getexif()[0x0112] = o
    want = np.asarray(ImageOps.exif_transpose(im))
    got = om.orient(o, a)
    assert got.shape == om.oriented_size(o, h, w) + (3,) and np.array_equal(got, want), o
    # planes: the same pixels with the axes elsewhere
    assert np.array_equal(om.orient(o, a.transpose(2, 0, 1), (1, 2)), got.transpose(2, 0, 1))


def test_pillows_method_names_are_the_tables():
    from PIL import Image

    a = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)
    names = {2: "FLIP_LEFT_RIGHT", 3: "ROTATE_180", 4: "FLIP_TOP_BOTTOM", 5: "TRANSPOSE", 6: "ROTATE_270", 7: "TRANSVERSE", 8: "ROTATE_90"}
    for o, name in names.items():
        assert np.array_equal(om.orient(o, a), np.asarray(Image.fromarray(a).transpose(getattr(Image.Transpose, name)))), name


# ------------------------------------------------------------------------------------------------ the rule

@pytest.mark.parametrize("o", om.ORIENTATIONS)
def test_identify_orientation_reads_what_pillow_writes_and_reads(o):
    from PIL import Image

    exif = Image.Exif()
    exif[0x010F] = "maker"
    exif[0x0112] = o
    buf = io.BytesIO()
    Image.fromarray(cm.picture(16, 8, 3), "RGB").save(buf, format="JPEG", exif=exif.tobytes())
    f = buf.getvalue()
    assert Image.open(io.BytesIO(f)).getexif().get(0x0112, 1) == o == jl.identify_orientation(f)
    assert jl.identify_orientation(np.frombuffer(f, np.uint8)) == o


def test_a_file_without_exif_and_pillow_agree():
    from PIL import Image

    f = _plain()
    assert Image.open(io.BytesIO(f)).getexif().get(0x0112, 1) == 1 == jl.identify_orientation(f)


@pytest.mark.parametrize("order", ["MM", "II"])
def test_the_rule_case_by_case(order):
    from PIL import Image

    f = _plain()
    ident = jl.identify_orientation
    for o in om.ORIENTATIONS:
        g = om.with_orientation(f, o, order)
        assert ident(g) == o == Image.open(io.BytesIO(g)).getexif().get(0x0112, 1)
    e = ">" if order == "MM" else "<"
    import struct

    tag = (0x0112, 3, 1, struct.pack(e + "HH", 6, 0))
    other = [(0x010F, 2, 4, b"abc\0"), (0x0131, 2, 4, b"xyz\0")]
    assert ident(om.with_orientation(f, None, order)) == 1  # tag absent
    assert ident(om.with_orientation(f, None, order, entries=other + [tag])) == 6  # the third entry
    assert ident(om.with_orientation(f, None, order, entries=[tag])) == 6
    assert ident(om.with_orientation(f, 6, order, typ=4)) == 1  # LONG
    assert ident(om.with_orientation(f, 6, order, n=2)) == 1  # count 2
    assert ident(om.with_orientation(f, 0, order)) == 1 and ident(om.with_orientation(f, 9, order)) == 1
    assert ident(om.with_orientation(f, 0x0600, order)) == 1  # (6 in the other byte order)
    assert ident(om.with_orientation(f, 6, order, magic=43)) == 1
    assert ident(om.with_orientation(f, 6, order, ifd_offset=5000, ifd_at=8)) == 1  # past the end
    assert ident(om.with_orientation(f, 6, order, ifd_offset=0xFFFFFFF0, ifd_at=8)) == 1
    assert ident(om.with_orientation(f, None, order, entries=other, count=300)) == 1  # the entry count reaches past the segment
    assert ident(om.with_orientation(f, 6, order, ifd_offset=24)) == 6  # IFD0 need not follow the header
    assert ident(cm.insert_after_soi(f, cm.segment(0xE1, b"Exif\0\0"))) == 1  # a 6-byte payload
    assert ident(cm.insert_after_soi(f, cm.segment(0xE1, b"Exif\0\0" + om.tiff(6, order)[:9]))) == 1  # cut inside the header
    whole = om.tiff(None, order, entries=[tag])
    assert ident(cm.insert_after_soi(f, cm.segment(0xE1, b"Exif\0\0" + whole[:8 + 2 + 12]))) == 6  # the entry is whole, nothing behind it
    assert ident(cm.insert_after_soi(f, cm.segment(0xE1, b"Exif\0\0" + whole[:8 + 2 + 11]))) == 1  # one byte short
    # where the segment lies
    sos = cm.segments(f)[-1][2]
    assert ident(f[:sos] + om.exif_segment(6, order) + f[sos:]) == 1  # behind the first SOS (the walk stops at its header)
    assert ident(cm.insert_after_soi(f, om.exif_segment(5, order), om.exif_segment(7, order))) == 5  # the first of two counts
    assert ident(cm.insert_after_soi(f, om.exif_segment(6, order, magic=43), om.exif_segment(7, order))) == 1  # ... even when it is broken
    assert ident(cm.insert_after_soi(f, om.XMP, om.exif_segment(8, order))) == 8  # an XMP APP1 in front
    assert ident(cm.insert_before_frame(f, om.exif_segment(3, order))) == 3  # behind the file's own APPn
    padded = cm.insert_after_soi(f, cm.segment(0xE2, b"\x11" * 40000), cm.segment(0xED, b"\x22" * 40000), om.exif_segment(4, order))
    assert padded.index(b"Exif") > 80000 and ident(padded) == 4
    assert ident(om.with_orientation(cm.with_app1_padding(f), 6, order)) == 6 and ident(cm.with_app1_padding(om.with_orientation(f, 6, order))) == 1


def test_a_bad_block_never_fails_and_a_bad_file_does():
    f = _plain()
    rng = np.random.default_rng(7)
    seg = om.exif_segment(6, "II")
    for _ in range(300):
        b = bytearray(seg)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(10, len(b)))] = int(rng.integers(0, 256))  # (behind the marker, the length and "Exif\0\0")
        assert 1 <= jl.identify_orientation(cm.insert_after_soi(f, bytes(b))) <= 8
    with pytest.raises(InvalidOperationException):
        jl.identify_orientation(b"\xff\xd8\xff\xd9")


# ------------------------------------------------------------------------------------------------ symbols, arguments

def test_the_symbols_the_header_and_the_refusals_without_a_device():
    header = open(os.path.join(ROOT, "include", "jpgpu.h")).read()
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert len(re.findall(r"^int %s\(" % name, header, re.M)) == 1, name
        assert name in bound and hasattr(_capi.lib, name), name
    assert re.search(r"JPGPU_ORIENT_STORED = 0,.*\n\s*JPGPU_ORIENT_FILE = 1", header)
    block = header[header.index("---- Orientation"):header.index("typedef enum jpgpu_orientation_policy")]
    for fenced in ("jpgpu_decoder_*", "jpgpu_decode_scan", "jpgpu_progressive_*", "jpgpu_multi_*"):
        assert fenced in block
    assert _capi.ORIENTATION_POLICIES == ("stored", "file")
    o = _capi.C.c_int(-7)
    assert _capi.lib.jpgpu_identify_orientation(None, 0, _capi.C.byref(o)) == _capi.ERR_ARGUMENT and o.value == -7
    assert _capi.lib.jpgpu_identify_orientation(b"\xff\xd8", 2, None) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_set_orientation_policy(None, 1) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_set_orientations(None, (_capi.C.c_uint8 * 1)(1), 1) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_image_orientation(None, 0, _capi.C.byref(o)) == _capi.ERR_ARGUMENT


@pytest.mark.parametrize("bad", ["FILE", "exif", "", None, 1, b"file", ("file",)])
def test_the_helpers_refuse_another_policy_before_any_library_call(bad):
    from jpeglibrary_amd import batch as jb

    with pytest.raises(ValueError, match="stored"):
        jb._orientation_policy(bad)
    for call in (lambda: jl.decode_batch([b"x"], jl.FMT_RGB_U8, orientation=bad), lambda: jl.decode_to_tensors([b"x"], orientation=bad)):
        with pytest.raises(ValueError, match="stored"):
            call()


@pytest.mark.parametrize("bad", [[9], [-1], [1.0], [True], ["6"], [None], [1, 2]])
def test_the_helpers_refuse_a_bad_list_before_any_library_call(bad):
    import torch

    from jpeglibrary_amd import batch as jb

    assert jb._orientation_list(None) is None and jb._orientation_list([0, 8, np.int64(3)]) == [0, 8, 3]
    for call in (lambda: jl.decode_batch([b"x"], jl.FMT_RGB_U8, orientations=bad), lambda: jl.decode_to_tensors([b"x"], orientations=bad),
                 lambda: jl.decode_resized([b"x"], (8, 8), torch.uint8, orientations=bad)):
        with pytest.raises(ValueError, match="orientation"):
            call()
    assert jl.identify_orientation is jb.identify_orientation and "identify_orientation" in jl.__all__


# ------------------------------------------------------------------------------------------------ the sanitizer harness

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_rule_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "exif_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=address,undefined",
                    "-I", os.path.join(ROOT, "jpeglibrary_amd", "csrc"), os.path.join(ROOT, "tools", "fuzz", "exif_orientation_asan.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "exif ok: 4000 edits" in r.stdout and " 0 failures" in r.stdout
