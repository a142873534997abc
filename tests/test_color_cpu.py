"""The colour policy without a GPU: the rule (jpgpu_identify_color) on every row of its table, the new symbols, the integer division by 255,
the model (tests/color_model.py) against Pillow's converter and Pillow's decode, and the Python argument checks.

Model against Pillow's decode, measured on these inputs (45 x 67 at Q75 / 90 / 100; the model over the oracle's samples, Pillow's
Image.open(...).convert("RGB"); the two decoders use different IDCTs): largest difference CMYK 2, YCCK 2, CMYK without APP14 2, Adobe-RGB 1,
Adobe-RGB by ids 1.  The tests assert those values plus 1, the margin for a Pillow built against another libjpeg."""
import io
import re

import numpy as np
import pytest

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from jpeglibrary_amd.errors import InvalidOperationException, NotSupportedException
import color_model as cm

MEASURED = {"cmyk": 2, "ycck": 2, "cmyk_bare": 2, "rgb_adobe": 1, "rgb_ids": 1}  # largest |model - Pillow| over Q75, Q90, Q100 (docstring)
NEW = ("jpgpu_batch_set_color_policy", "jpgpu_batch_image_color", "jpgpu_identify_color")


# ------------------------------------------------------------------------------------------------ the rule

def _cmyk():
    return cm.kind_file("cmyk")[0]


def _rgb():
    return cm.kind_file("rgb_adobe")[0]


def _ycc3():
    return cm.pillow_jpeg(45, 67, "RGB")  # JFIF, ids 1 2 3


RULE = [
    ("gray", lambda: cm.pillow_jpeg(45, 67, "L"), "gray"),
    ("gray_adobe_0", lambda: cm.insert_after_soi(cm.remove_segments(cm.pillow_jpeg(45, 67, "L"), 0xE0), cm.app14(0)), "gray"),
    ("3_jfif", _ycc3, "ycbcr"),
    ("3_jfif_and_adobe_0", lambda: cm.kind_file("jfif_wins")[0], "ycbcr"),
    ("3_adobe_0", _rgb, "rgb"),
    ("3_adobe_1", lambda: cm.patch_adobe_transform(_rgb(), 1), "ycbcr"),
    ("3_adobe_2", lambda: cm.patch_adobe_transform(_rgb(), 2), "ycbcr"),
    ("3_ids_rgb", lambda: cm.kind_file("rgb_ids")[0], "rgb"),
    ("3_ids_rgb_with_jfif", lambda: cm.insert_after_soi(cm.kind_file("rgb_ids")[0], cm.JFIF), "ycbcr"),
    ("3_ids_123_no_marker", lambda: cm.remove_segments(_ycc3(), 0xE0), "ycbcr"),
    ("3_ids_rgB_no_marker", lambda: cm.patch_component_ids(cm.kind_file("rgb_ids")[0], (0x52, 0x47, 0x62)), "ycbcr"),
    ("4_adobe_0", _cmyk, "cmyk"),
    ("4_adobe_1", lambda: cm.patch_adobe_transform(_cmyk(), 1), "ycck"),
    ("4_adobe_2", lambda: cm.kind_file("ycck")[0], "ycck"),
    ("4_no_adobe", lambda: cm.kind_file("cmyk_bare")[0], "cmyk"),
    ("4_jfif_ignored", lambda: cm.insert_after_soi(cm.kind_file("cmyk_bare")[0], cm.JFIF), "cmyk"),
    ("4_jfif_and_adobe_2", lambda: cm.insert_after_soi(cm.kind_file("ycck")[0], cm.JFIF), "ycck"),
    # a short APP14 (11 payload bytes: no transform byte) is no Adobe marker
    ("4_short_app14", lambda: cm.insert_after_soi(cm.kind_file("cmyk_bare")[0], cm.app14(2, 11)), "cmyk"),
    ("3_short_app14", lambda: cm.insert_after_soi(cm.remove_segments(_ycc3(), 0xE0), cm.app14(0, 11)), "ycbcr"),
    # a short APP0 (13 payload bytes) is no JFIF marker: the Adobe marker decides
    ("3_short_jfif", lambda: cm.insert_after_soi(_rgb(), cm.segment(0xE0, b"JFIF\0" + bytes(8))), "rgb"),
    # two APP14: the last wins
    ("4_two_app14_last_0", lambda: cm.insert_after_soi(_cmyk(), cm.app14(2)), "cmyk"),
    ("4_two_app14_last_2", lambda: cm.insert_before_frame(_cmyk(), cm.app14(2)), "ycck"),
    # 80 KB of APP1 in front of the Adobe marker
    ("4_behind_80k", lambda: cm.with_app1_padding(cm.kind_file("ycck")[0]), "ycck"),
    ("4_progressive", lambda: cm.pillow_jpeg(45, 67, "CMYK", progressive=True), "cmyk"),
    ("4_subsampled", cm.subsampled_ycck, "ycck"),
]


@pytest.mark.parametrize("name,make,kind", RULE, ids=[r[0] for r in RULE])
def test_the_rule(name, make, kind):
    assert jl.identify_color(make()) == kind


def test_what_pillow_writes_is_what_the_inputs_assume():
    f = _cmyk()
    segs = cm.segments(f)
    assert segs[0][0] == 0xEE and f[segs[0][1] + 4:segs[0][1] + 9] == b"Adobe" and f[segs[0][1] + 15] == 0  # APP14 right behind SOI, transform 0
    assert not any(m == 0xE0 for m, _, _ in segs)
    sof = next(a for m, a, _ in segs if m == 0xC0)
    assert f[sof + 9] == 4 and bytes(f[sof + 10 + 3 * c] for c in range(4)) == b"CMYK" and all(f[sof + 11 + 3 * c] == 0x11 for c in range(4))
    f = _rgb()
    sof = next(a for m, a, _ in cm.segments(f) if m == 0xC0)
    assert f[sof + 9] == 3 and bytes(f[sof + 10 + 3 * c] for c in range(3)) == b"RGB"


def test_what_the_rule_refuses():
    with pytest.raises(NotSupportedException):
        jl.identify_color(cm.patch_precision(_cmyk(), 12))
    with pytest.raises(NotSupportedException):
        jl.identify_color(cm.patch_precision(_ycc3(), 12))
    import encoder_arrangements as ea
    import encoder_model as em

    two = bytes(em.encode(ea.pixels(40, 24, 2, 13), ea.arrangement("F"))[0])
    with pytest.raises(NotSupportedException):
        jl.identify_color(two)
    for broken in (b"", b"\xff\xd8\xff\xd9", _cmyk()[:10]):  # no frame header: the library's usual header errors
        with pytest.raises(Exception) as e:
            jl.identify_color(broken)
        assert type(e.value).__name__ in ("InvalidOperationException", "InvalidDataException"), e.value
    with pytest.raises(InvalidOperationException):
        jl.identify_color(b"\xff\xd8\xff\xd9")
    kind = _capi.C.c_int(-7)
    assert _capi.lib.jpgpu_identify_color(None, 0, _capi.C.byref(kind)) == _capi.ERR_ARGUMENT and kind.value == -7
    assert _capi.lib.jpgpu_identify_color(b"\xff\xd8", 2, None) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_set_color_policy(None, 1) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_image_color(None, 0, _capi.C.byref(kind)) == _capi.ERR_ARGUMENT


def test_header_declarations_equal_exports_for_the_new_symbols():
    header = open(_capi.LIB_PATH.replace("jpeglibrary_amd/libjpgpu.so", "include/jpgpu.h")).read()
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert len(re.findall(r"^int %s\(" % name, header, re.M)) == 1, name
        assert name in bound and hasattr(_capi.lib, name), name
    assert re.search(r"JPGPU_COLOR_YCC = 0,.*\n\s*JPGPU_COLOR_FILE = 1", header)
    kinds = re.findall(r"JPGPU_COLOR_KIND_(\w+) = (\d)", header)
    assert [(k.lower(), int(v)) for k, v in kinds] == list(zip(_capi.COLOR_KINDS, range(5))) == list(zip(cm.KINDS, range(5)))
    assert _capi.lib.jpgpu_version() == 101
    for fenced in ("jpgpu_decoder_*", "jpgpu_decode_scan", "jpgpu_progressive_*", "jpgpu_multi_*"):  # the header says what is out of scope
        assert fenced in header[header.index("---- Colour"):header.index("typedef enum jpgpu_color_policy")]


# ------------------------------------------------------------------------------------------------ the arithmetic

def test_d_is_exact_rounding_of_x_over_255():
    x = np.arange(0, 65026, dtype=np.int64)
    exact = (2 * x + 255) // 510  # round half up; x / 255 is never a half (255 is odd), so this is round to nearest
    assert np.array_equal(cm.d(x), exact)
    assert np.array_equal(exact, np.rint(x / 255.0).astype(np.int64))


def test_the_cmyk_case_is_pillows_converter_on_every_pair():
    from PIL import Image

    a = np.arange(256, dtype=np.uint8)
    c, k = np.meshgrid(a, a, indexing="ij")
    ink = np.stack([c, c[::-1], c, k], axis=-1)  # Pillow's own convention: 0 = no ink
    want = np.asarray(Image.fromarray(ink, "CMYK").convert("RGB"))
    got = cm.model("cmyk", 255 - ink)  # the file's samples are the inverted inks (Adobe)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("quality", [75, 90, 100])
@pytest.mark.parametrize("name", list(MEASURED))
def test_the_model_on_oracle_samples_against_pillows_decode(name, quality):
    from PIL import Image

    from oracle import pyoracle

    f, kind = cm.kind_file(name, quality=quality)
    samples, _ = pyoracle.decode_8bit(f)
    assert samples.shape == (67, 45, 4 if "c" in kind else 3)
    want = np.asarray(Image.open(io.BytesIO(f)).convert("RGB")).astype(np.int64)
    diff = np.abs(cm.model(kind, samples).astype(np.int64) - want)
    print("%s Q%d: largest difference %d, %.3f %% of the samples off by more than 1" % (name, quality, diff.max(), 100.0 * (diff > 1).mean()))
    assert diff.max() <= MEASURED[name] + 1


# ------------------------------------------------------------------------------------------------ Python arguments

@pytest.mark.parametrize("bad", ["FILE", "rgb", "", None, 1, b"file", ("file",)])
def test_the_helpers_refuse_another_policy_before_any_library_call(bad):
    from jpeglibrary_amd import batch as jb

    with pytest.raises(ValueError, match="ycc"):
        jb._color_policy(bad)
    # (no context exists on this machine: a ValueError, not the NoDevice a library call would raise, shows the order)
    for call in (lambda: jl.decode_batch([b"x"], jl.FMT_RGB_U8, color=bad), lambda: jl.decode_to_tensors([b"x"], color=bad)):
        with pytest.raises(ValueError, match="ycc"):
            call()


def test_decode_resized_checks_the_policy_with_its_other_arguments():
    import torch

    with pytest.raises(ValueError, match="ycc"):
        jl.decode_resized([b"x"], (8, 8), torch.uint8, color="cmyk")


def test_the_policy_names_are_the_header_values():
    from jpeglibrary_amd import batch as jb

    assert jb._color_policy("ycc") == 0 and jb._color_policy("file") == 1
    assert jl.identify_color is jb.identify_color and "identify_color" in jl.__all__
