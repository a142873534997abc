"""jpeglibrary_amd -- MI355X-native baseline-JPEG decode path behind the JpegLibrary decoder API.

Importing the package loads the in-tree HIP library (libjpgpu.so); it raises if the library is missing.
There is no CPU fallback: creating a context without a GPU raises NoDeviceError.
"""
from . import _capi  # noqa: F401  (loads libjpgpu.so, fails loudly when absent)
from . import sharding  # noqa: F401
from .batch import FMT_EXTENDED_U16, FMT_INTERLEAVED_U8, FMT_INTERLEAVED_U8_SCALED, FMT_PLANAR_I16, FMT_PLANAR_U8, FMT_RGB_PLANAR_F16, FMT_RGB_PLANAR_F32, FMT_RGB_PLANAR_U8, FMT_RGB_U8, FMT_RGBA_U8, Batch, affine_from_mean_std, decode_batch, decode_resized, decode_to_tensors, identify_color, identify_orientation
from .context import Context, default_context, device_count
from .encoder import EncodeBatch, encode_batch, encode_tensors
from .optimizer import JpegOptimizer, OptimizeBatch, TransformPlan, build_optimal_huffman_table, optimize_batch, plan_transform
from .decoder import (JpegBlockOutputWriter, JpegBufferOutputWriter8Bit, JpegBufferOutputWriterGreaterThan8Bit, JpegBufferOutputWriterLessThan8Bit, JpegDecoder, JpegExtendingOutputWriter, JpegFrameComponentSpecificationParameters,
                      JpegFrameHeader, JpegGpuProgressiveScanDecoder, JpegHuffmanDecodingTable, JpegScanComponentSpecificationParameters, JpegScanHeader)
from .jpeg_encoder import (JpegBufferInputReader, JpegEncoder, JpegHuffmanCanonicalCode, JpegHuffmanEncodingTable, JpegHuffmanEncodingTableBuilder, JpegQuantizationTable, JpegStandardHuffmanEncodingTable,
                           JpegStandardQuantizationTable)
from .multi import MultiDecoder
from .errors import (ArgumentException, DeviceError, InvalidDataException, InvalidOperationException, JpegError,
                     NoDeviceError, NotSupportedException)

__all__ = [
    "Batch", "decode_batch", "decode_to_tensors", "decode_resized", "MultiDecoder", "JpegEncoder", "JpegQuantizationTable", "JpegStandardQuantizationTable", "JpegHuffmanEncodingTable", "JpegHuffmanCanonicalCode", "JpegHuffmanEncodingTableBuilder",
    "JpegStandardHuffmanEncodingTable", "JpegBufferInputReader", "EncodeBatch", "encode_batch", "encode_tensors", "JpegOptimizer", "OptimizeBatch", "optimize_batch", "build_optimal_huffman_table", "plan_transform", "TransformPlan", "Context", "default_context", "device_count", "JpegDecoder", "JpegBlockOutputWriter",
    "JpegBufferOutputWriter8Bit", "JpegExtendingOutputWriter", "JpegFrameHeader", "JpegFrameComponentSpecificationParameters", "JpegScanHeader",
    "JpegScanComponentSpecificationParameters", "JpegHuffmanDecodingTable", "JpegGpuProgressiveScanDecoder", "FMT_INTERLEAVED_U8", "FMT_PLANAR_U8", "FMT_PLANAR_I16", "FMT_RGB_U8", "FMT_RGBA_U8", "FMT_EXTENDED_U16",
    "FMT_INTERLEAVED_U8_SCALED", "FMT_RGB_PLANAR_U8", "FMT_RGB_PLANAR_F16", "FMT_RGB_PLANAR_F32", "affine_from_mean_std", "identify_color", "identify_orientation", "JpegBufferOutputWriterGreaterThan8Bit", "JpegBufferOutputWriterLessThan8Bit",
    "JpegError", "InvalidDataException", "InvalidOperationException", "NotSupportedException", "ArgumentException",
    "DeviceError", "NoDeviceError",
]
