"""The device-input entries of the encoder, as far as they go without a GPU: the two C symbols, their refusal of a NULL encoder, and the
checks EncodeBatch.upload_tensors makes before it calls the library (so they need neither a context nor a device)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import encoder_arrangements as ea
import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi


def test_the_two_entries_exist_and_refuse_a_null_encoder():
    lib = _capi.lib
    declared = {name for name, _, _ in _capi.SYMBOLS}
    assert {"jpgpu_encoder_upload_device", "jpgpu_encoder_upload_described_device"} <= declared
    px = np.zeros(16 * 16 * 3, np.uint8)
    ptrs = (C.c_void_p * 1)(px.ctypes.data)
    layouts = (C.c_int32 * 1)(_capi.PIXELS_PLANAR)
    params = (_capi.EncodeParams * 1)(_capi.EncodeParams(16, 16, 3, 2, 2, 75, 1, 0, 0))
    assert lib.jpgpu_encoder_upload_device(None, ptrs, params, layouts, 1) == _capi.ERR_ARGUMENT
    assert lib.jpgpu_encoder_upload_device(None, ptrs, params, None, 1) == _capi.ERR_ARGUMENT
    descs = (_capi.EncodeDescription * 1)(ea.to_description(ea.arrangement("A"), 16, 16))
    assert lib.jpgpu_encoder_upload_described_device(None, ptrs, descs, layouts, 1) == _capi.ERR_ARGUMENT
    assert (_capi.PIXELS_INTERLEAVED, _capi.PIXELS_PLANAR) == (0, 1)
    assert callable(jl.encode_tensors) and "encode_tensors" in jl.__all__


@pytest.fixture
def batch():
    """An EncodeBatch that has no encoder behind it: every check below has to fire before the library is called"""
    b = object.__new__(jl.EncodeBatch)
    b.ctx = types.SimpleNamespace(device=0, _h=None)
    b._h, b._n, b._blocks, b._keep = C.c_void_p(), 0, [], None
    return b


CHW, HWC = torch.zeros((3, 16, 20), dtype=torch.uint8), torch.zeros((16, 20, 3), dtype=torch.uint8)
BAD = [
    ("cpu_chw", CHW, "chw", False, "context's device"),
    ("cpu_hwc", HWC, "hwc", False, "context's device"),
    ("cpu_default_layout", CHW, None, False, "context's device"),
    ("int16", CHW.to(torch.int16), "chw", False, "uint8"),
    ("float", HWC.float(), "hwc", False, "uint8"),
    ("permuted", HWC.permute(2, 0, 1), "chw", False, r"\.contiguous\(\)"),
    ("sliced", HWC[:, ::2], "hwc", False, r"\.contiguous\(\)"),
    ("rank_2_as_chw", HWC[..., 0].contiguous(), "chw", False, r"\(C, H, W\)"),
    ("rank_4", CHW[None], "chw", False, r"\(C, H, W\)"),
    ("rank_1", CHW.reshape(-1), "hwc", False, r"\(H, W, C\)"),
    ("hwc_read_as_planes", HWC, "chw", False, "samples per pixel"),
    ("two_channels", torch.zeros((16, 20, 2), dtype=torch.uint8), "hwc", False, "samples per pixel"),
    ("rgba_without_rgb", torch.zeros((16, 20, 4), dtype=torch.uint8), "hwc", False, "samples per pixel"),
    ("rgba_planes", torch.zeros((4, 16, 20), dtype=torch.uint8), "chw", True, "samples per pixel"),
    ("numpy", np.zeros((3, 16, 20), np.uint8), "chw", False, "torch tensor"),
    ("unknown_layout", CHW, "nchw", False, "layout"),
]


@pytest.mark.parametrize("tensor,layout,rgb,message", [c[1:] for c in BAD], ids=[c[0] for c in BAD])
def test_upload_tensors_raises_before_any_library_call(batch, tensor, layout, rgb, message):
    with pytest.raises(ValueError, match=message):
        batch.upload_tensors([tensor], (2, 2), 75, rgb, layout=layout)
    assert batch._keep is None and len(batch) == 0


def test_upload_described_tensors_raises_before_any_library_call(batch):
    desc = ea.to_description(ea.arrangement("A"), 20, 16)
    for tensor, layout, message in ((torch.zeros((4, 16, 20), dtype=torch.uint8), "chw", "context's device"),
                                    (torch.zeros((3, 16, 20), dtype=torch.uint8), "chw", "samples per pixel"),
                                    (torch.zeros((4, 16, 24), dtype=torch.uint8), "chw", "24 x 16 pixels"),
                                    (torch.zeros((16, 20, 4), dtype=torch.int8), "hwc", "uint8"),
                                    (torch.zeros((16, 4, 20), dtype=torch.uint8).permute(0, 2, 1), "hwc", r"\.contiguous\(\)")):
        with pytest.raises(ValueError, match=message):
            batch.upload_described_tensors([tensor], [desc], layout)
    with pytest.raises(ValueError, match="one description per image"):
        batch.upload_described_tensors([], [desc])
