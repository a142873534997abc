"""jpgpu_batch_upload_device as far as it goes without a GPU: the new C symbols, the size of the statistics struct, the refusal of a NULL
batch, and the checks Batch.upload_tensors makes before it calls the library (a module-level function that needs no device)."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeglibrary_amd as jl
from jpeglibrary_amd import _capi
from jpeglibrary_amd import batch as jb


def test_the_library_exports_the_new_symbols():
    declared = {name for name, _, _ in _capi.SYMBOLS}
    assert {"jpgpu_batch_upload_device", "jpgpu_batch_device_ingest_stats", "jpgpu_sizeof_device_ingest_stats"} <= declared
    for name in ("jpgpu_batch_upload_device", "jpgpu_batch_device_ingest_stats"):
        assert getattr(_capi.lib, name) is not None
    assert callable(jl.Batch.upload_tensors) and callable(jl.Batch.device_ingest_stats)


def test_the_statistics_mirror_has_the_size_the_library_reports():
    assert _capi.lib.jpgpu_sizeof_device_ingest_stats() == C.sizeof(_capi.DeviceIngestStats) == 40
    assert [k for k, _ in _capi.DeviceIngestStats._fields_] == ["files_gathered", "files_downloaded", "walker_giveups", "gather_ms", "bytes_gathered",
                                                                "head_bytes", "bytes_downloaded"]
    assert _capi.lib.jpgpu_batch_device_ingest_stats(None, C.byref(_capi.DeviceIngestStats())) == _capi.ERR_ARGUMENT
    assert 0 < _capi.DEVICE_HEAD_PAD <= 256


def test_a_null_batch_is_refused():
    data = np.zeros(16, np.uint8)
    ptrs, lens = (C.c_void_p * 1)(data.ctypes.data), (C.c_size_t * 1)(16)
    assert _capi.lib.jpgpu_batch_upload_device(None, ptrs, lens, 1, jl.FMT_INTERLEAVED_U8) == _capi.ERR_ARGUMENT
    assert _capi.lib.jpgpu_batch_upload_device(None, None, None, 0, jl.FMT_INTERLEAVED_U8) == _capi.ERR_ARGUMENT


def test_the_version_is_unchanged():
    assert _capi.lib.jpgpu_version() == 101


FILE = torch.arange(40, dtype=torch.uint8)
CPU = torch.device("cpu")
BAD = [
    ("a_tensor_instead_of_a_list", FILE, CPU, "list of tensors"),
    ("bytes_instead_of_a_list", b"\xff\xd8\xff\xd9", CPU, "list of tensors"),
    ("a_list_in_the_list", [[1, 2, 3]], CPU, "torch tensor"),
    ("bytes_in_the_list", [b"\xff\xd8\xff\xd9"], CPU, "torch tensor"),
    ("numpy", [np.zeros(8, np.uint8)], CPU, "torch tensor"),
    ("float", [FILE.float()], CPU, "uint8"),
    ("int8", [FILE.to(torch.int8)], CPU, "uint8"),
    ("two_dimensional", [FILE.reshape(4, 10)], CPU, "1-D"),
    ("zero_dimensional", [FILE[3]], CPU, "1-D"),
    ("strided_view", [FILE[::2]], CPU, r"\.contiguous\(\)"),
    ("cpu_tensor_for_a_device_context", [FILE], 0, "context's device cuda:0"),
    ("second_of_two", [FILE, FILE.float()], CPU, "file 1"),
]


@pytest.mark.parametrize("tensors,device,message", [c[1:] for c in BAD], ids=[c[0] for c in BAD])
def test_the_tensor_check_raises_before_any_library_call(tensors, device, message):
    with pytest.raises(ValueError, match=message):
        jb._tensor_files(tensors, device)


def test_a_well_formed_description_passes_through():
    view = FILE[3:29]  # a contiguous view at an odd address
    got = jb._tensor_files([FILE, view, FILE[:0]], CPU)
    assert got == [(FILE.data_ptr(), 40), (FILE.data_ptr() + 3, 26), (None, 0)]
    assert jb._tensor_files((), 0) == []


def test_a_list_is_all_bytes_or_all_tensors():
    assert jb._all_tensors([FILE, FILE]) is True and jb._all_tensors([b"ab", bytearray(2), np.zeros(2, np.uint8)]) is False
    assert jb._all_tensors([]) is False
    with pytest.raises(ValueError, match="mix"):
        jb._all_tensors([b"ab", FILE])
