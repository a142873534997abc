"""Device-resident batch decode (include/jpgpu.h level 1: jpgpu_batch_*).

Replaces, for a set of files at once, the canonical reference sequence
    new JpegDecoder(); SetInput; Identify; SetOutputWriter(JpegBufferOutputWriter8Bit); Decode()
(ref: apps/JpegDecode/DecodeAction.cs:26-56, tests/JpegLibrary.Benchmarks/DecoderBenchmark.cs:51-73).
"""
import ctypes as C

import numpy as np

from . import _capi
from .context import Context, default_context
from .errors import raise_for_status

_lib = _capi.lib
FMT_INTERLEAVED_U8, FMT_PLANAR_U8, FMT_PLANAR_I16 = _capi.FMT_INTERLEAVED_U8, _capi.FMT_PLANAR_U8, _capi.FMT_PLANAR_I16
FMT_RGB_U8, FMT_RGBA_U8, FMT_EXTENDED_U16 = _capi.FMT_RGB_U8, _capi.FMT_RGBA_U8, _capi.FMT_EXTENDED_U16
FMT_INTERLEAVED_U8_SCALED = _capi.FMT_INTERLEAVED_U8_SCALED
FMT_RGB_PLANAR_U8 = _capi.FMT_RGB_PLANAR_U8
FMT_RGB_PLANAR_F16, FMT_RGB_PLANAR_F32 = _capi.FMT_RGB_PLANAR_F16, _capi.FMT_RGB_PLANAR_F32
# the sample type of the formats that are one dense array per image: numpy dtype and the typestr of __cuda_array_interface__
_SAMPLE_DTYPES = {FMT_RGB_PLANAR_F16: np.float16, FMT_RGB_PLANAR_F32: np.float32}
_RGB_PLANES = (FMT_RGB_PLANAR_U8, FMT_RGB_PLANAR_F16, FMT_RGB_PLANAR_F32)


def _typestr(fmt):
    """__cuda_array_interface__ typestr of a format's samples: "|u1", or "<f2" / "<f4" for RGB_PLANAR_F16 / _F32"""
    return np.dtype(_SAMPLE_DTYPES.get(fmt, np.uint8)).str


def affine_from_mean_std(mean, std):
    """The constants of Batch.set_output_affine that make RGB_PLANAR_F16 / _F32 hold (u / 255 - mean[c]) / std[c]: mean and std per channel
    (R, G, B) in 0..1 units, as model code states them.  scale = 1 / (255 * std), bias = -mean / std, computed in float64 and rounded once
    to float32.  -> (scale, bias), two float32[3] arrays."""
    mean, std = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(std, dtype=np.float64).reshape(-1)
    if mean.shape != (3,) or std.shape != (3,):
        raise ValueError("mean and std are three values each, one per channel (R, G, B)")
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std))) or np.any(std == 0):
        raise ValueError("mean and std must be finite and std non-zero")
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def _resize_setting(size, dtype):
    """The checks of Batch.set_resize / decode_resized, before any library call: size = (oh, ow), two integers in 1..65535; dtype = torch.uint8,
    torch.float16 or torch.float32.  -> (oh, ow, format of the samples, numpy dtype)"""
    import numbers

    import torch  # (here: the package imports without torch)

    by_dtype = {torch.uint8: (FMT_RGB_PLANAR_U8, np.uint8), torch.float16: (FMT_RGB_PLANAR_F16, np.float16), torch.float32: (FMT_RGB_PLANAR_F32, np.float32)}
    if dtype not in by_dtype:
        raise ValueError("resize: dtype is torch.uint8, torch.float16 or torch.float32, not %s" % (dtype,))
    try:
        vals = tuple(size)
    except TypeError:
        raise ValueError("resize: size is (height, width), not %s" % type(size).__name__) from None
    if len(vals) != 2 or not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and 1 <= v <= 65535 for v in vals):
        raise ValueError("resize: size is (height, width), two integers in 1..65535, not %r" % (size,))
    return (int(vals[0]), int(vals[1])) + by_dtype[dtype]


IDCT_LAYOUT_CLASSES = 6  # JPGPU_IDCT_LAYOUT_CLASSES: generic, YCbCr 1x1 / 2x1 / 2x2, gray, store holding samples


class _BorrowedContext:
    def __init__(self, handle):
        self._h = C.c_void_p(handle)


class _DeviceView:
    """What torch.as_tensor wraps without a copy: a span of a batch's output buffer described by __cuda_array_interface__ (version 2).
    torch holds a reference to this object for as long as any tensor made from it lives, and this object holds the batch."""

    def __init__(self, batch, ptr, shape, typestr="|u1"):
        self._batch = batch
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}


def _tensor_files(tensors, device):
    """The checks of Batch.upload_tensors, before any library call (they need neither a context nor a device): [(data_ptr, bytes)] for
    1-D contiguous uint8 torch tensors on `device` (a CUDA device index, or a torch.device), one per file.  An empty tensor is the
    empty file (no pointer)."""
    import torch  # (here: the package imports without torch)

    want = device if isinstance(device, torch.device) else torch.device("cuda", device)

    if isinstance(tensors, (torch.Tensor, bytes, bytearray, memoryview)):
        raise ValueError("a list of tensors is expected, one per file, not %s" % type(tensors).__name__)
    out = []
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor):
            raise ValueError("file %d: a torch tensor is expected, not %s (bytes and numpy arrays go to upload())" % (i, type(t).__name__))
        if t.dtype != torch.uint8:
            raise ValueError("file %d: a uint8 tensor is expected, not %s" % (i, t.dtype))
        if t.dim() != 1:
            raise ValueError("file %d: a 1-D tensor of the file's bytes is expected, not shape %s" % (i, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("file %d: the tensor is not contiguous; call .contiguous() (nothing is copied silently)" % i)
        if t.device != want:
            raise ValueError("file %d: the tensor is on %s, not on the context's device %s" % (i, t.device, want))
        out.append((t.data_ptr() if t.numel() else None, t.numel()))
    return out


def _all_tensors(files):
    """decode_batch / decode_to_tensors: is `files` a list of device files (torch tensors)?  A list that mixes them with bytes raises."""
    import sys

    torch = sys.modules.get("torch")  # (a tensor cannot exist without it; the package imports without torch)
    kinds = {torch is not None and isinstance(f, torch.Tensor) for f in files}
    if kinds == {True, False}:
        raise ValueError("files are all bytes-like (host memory) or all torch tensors (device memory), not a mix")
    return kinds == {True}


def _window_rects(rects, n_files=None):
    """The checks of Batch.set_windows / decode_batch(windows=...), before any library call: [(x, y, w, h)] of four non-negative integers
    below 2^32 each, one per file ((0, 0, 0, 0) = the whole frame); n_files: the count they must match.  None -> None."""
    import numbers

    if rects is None:
        return None
    out = []
    for i, r in enumerate(rects):
        try:
            vals = tuple(r)
        except TypeError:
            raise ValueError("window %d: (x, y, w, h) is expected, not %s" % (i, type(r).__name__)) from None
        if len(vals) != 4 or not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and 0 <= v < 2 ** 32 for v in vals):
            raise ValueError("window %d: (x, y, w, h) are four non-negative integers below 2^32, not %r" % (i, r))
        out.append(tuple(int(v) for v in vals))
    if n_files is not None and len(out) != n_files:
        raise ValueError("%d windows for %d files: one per file ((0, 0, 0, 0) = the whole frame)" % (len(out), n_files))
    return out


def _color_policy(color, who="color"):
    """The check of Batch.set_color_policy / decode_batch(color=...), before any library call: "ycc" or "file" -> the jpgpu_color_policy value"""
    if not isinstance(color, str) or color not in _capi.COLOR_POLICIES:
        raise ValueError('%s is "ycc" (1 component = grey, 3 = YCbCr) or "file" (what the file declares), not %r' % (who, color))
    return _capi.COLOR_POLICIES.index(color)


def identify_color(data):
    """What a JPEG file's headers declare its samples to be: "gray", "ycbcr", "rgb", "cmyk" or "ycck" -- libjpeg's rule over the JFIF and Adobe
    markers and the component ids (include/jpgpu.h, "Colour"), the kind Batch.color(i) reports under the "file" policy.  Host only: no
    device, no context.  Raises as the decoder does for a file without a frame header, and NotSupported for 2 or more than 4 components or a
    precision other than 8."""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    kind = C.c_int()
    raise_for_status(_lib.jpgpu_identify_color(a.ctypes.data, a.size, C.byref(kind)), b"jpgpu_identify_color: the headers give no colour kind")
    return _capi.COLOR_KINDS[kind.value]


def _orientation_policy(orientation, who="orientation"):
    """The check of Batch.set_orientation_policy / decode_batch(orientation=...), before any library call: "stored" or "file" -> the
    jpgpu_orientation_policy value"""
    if not isinstance(orientation, str) or orientation not in _capi.ORIENTATION_POLICIES:
        raise ValueError('%s is "stored" (as the file stores the pixels) or "file" (as its Exif orientation says), not %r' % (who, orientation))
    return _capi.ORIENTATION_POLICIES.index(orientation)


def _upsampling_policy(upsampling, who="upsampling"):
    """The check of Batch.set_upsampling_policy / decode_batch(upsampling=...), before any library call: "replicate" or "fancy" -> the
    jpgpu_upsampling_policy value"""
    if not isinstance(upsampling, str) or upsampling not in _capi.UPSAMPLING_POLICIES:
        raise ValueError('%s is "replicate" (a chroma sample repeated over its pixels) or "fancy" (libjpeg\'s triangle filter), not %r' % (who, upsampling))
    return _capi.UPSAMPLING_POLICIES.index(upsampling)


def _arithmetic_policy(arithmetic, who="arithmetic"):
    """The check of Batch.set_arithmetic_policy / decode_batch(arithmetic=...), before any library call: "reference" or "libjpeg" -> the
    jpgpu_arithmetic_policy value"""
    if not isinstance(arithmetic, str) or arithmetic not in _capi.ARITHMETIC_POLICIES:
        raise ValueError('%s is "reference" (the reference\'s float transform and constants) or "libjpeg" (its integer transform and colour constants), not %r' % (who, arithmetic))
    return _capi.ARITHMETIC_POLICIES.index(arithmetic)


def _scale_setting(scale, arithmetic="libjpeg", fit=False, windows=None, who="scale"):
    """The check of Batch.set_scale_policy / decode_to_tensors(scale=...) / decode_resized(scale=...), before any library call: 1, 2, 4 or 8,
    or "fit" where fit is allowed; anything but 1 needs arithmetic="libjpeg" (the reduced transforms are libjpeg's), and "fit" takes no windows."""
    is_fit = fit and isinstance(scale, str) and scale == "fit"
    if not is_fit and (isinstance(scale, bool) or not isinstance(scale, int) or scale not in _capi.SCALE_DENOMINATORS):
        raise ValueError('%s is 1, 2, 4 or 8%s, not %r' % (who, ' or "fit"' if fit else "", scale))
    if scale != 1 and arithmetic != "libjpeg":
        raise ValueError('%s=%r needs arithmetic="libjpeg": the reduced transforms are libjpeg\'s, the reference has none' % (who, scale))
    if is_fit and windows is not None:
        raise ValueError('%s="fit" takes no windows: each image picks its own scale, and a window is in pixels of the reduced frame' % who)
    return scale


def _channels_policy(mode, fmt=None, who="mode"):
    """The check of Batch.set_channels_policy / decode_batch(mode=...), before any library call: "rgb" or "gray" -> the jpgpu_channels_policy
    value.  fmt: the format "gray" is asked for with; only RGB_PLANAR_U8 / _F16 / _F32 have a one-plane form."""
    if not isinstance(mode, str) or mode not in _capi.CHANNELS_POLICIES:
        raise ValueError('%s is "rgb" (three planes) or "gray" (one plane: the luma samples, or L of a CMYK or RGB file), not %r' % (who, mode))
    if mode == "gray" and fmt is not None and fmt not in _RGB_PLANES:
        raise ValueError('%s="gray" needs RGB_PLANAR_U8, RGB_PLANAR_F16 or RGB_PLANAR_F32; format %d has no one-plane form' % (who, fmt))
    return _capi.CHANNELS_POLICIES.index(mode)


def _gray_mean_std(mean, std):
    """mean and std of a one-plane decode: a number or a sequence of one, each -> three equal values for affine_from_mean_std (only
    scale[0] and bias[0] are read)"""
    def one(v, name):
        a = np.asarray(v, dtype=np.float64).reshape(-1)
        if a.shape != (1,):
            raise ValueError('%s under mode="gray" is one value (a number or a sequence of one), not %r' % (name, v))
        return [float(a[0])] * 3
    return one(mean, "mean"), one(std, "std")


def _orientation_list(orientations, n_files=None):
    """The checks of Batch.set_orientations / decode_batch(orientations=...), before any library call: integers 0..8, one per file (0 = what
    the policy gives); n_files: the count they must match.  None -> None."""
    import numbers

    if orientations is None:
        return None
    out = []
    for i, o in enumerate(orientations):
        if not isinstance(o, numbers.Integral) or isinstance(o, bool) or not 0 <= o <= 8:
            raise ValueError("orientation %d: an integer 1..8 (the Exif values), or 0 for what the policy gives, not %r" % (i, o))
        out.append(int(o))
    if n_files is not None and len(out) != n_files:
        raise ValueError("%d orientations for %d files: one per file (0 = what the policy gives)" % (len(out), n_files))
    return out


def identify_orientation(data):
    """The Exif orientation a JPEG file declares, 1..8 -- the Orientation tag in IFD0 of the first Exif APP1 in front of the first scan
    (include/jpgpu.h, "Orientation"), what Batch.orientation(i) reports under the "file" policy; 1 for a file without the tag or with a
    broken Exif block.  Host only: no device, no context.  Raises as the decoder does for a file without a frame header."""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    o = C.c_int()
    raise_for_status(_lib.jpgpu_identify_orientation(a.ctypes.data, a.size, C.byref(o)), b"jpgpu_identify_orientation: the headers could not be read")
    return o.value


def _upload_any(batch, files, fmt):
    """decode_batch / decode_to_tensors: upload() for bytes-like files, upload_tensors() for a list of torch tensors"""
    files = list(files)
    return batch.upload_tensors(files, fmt) if _all_tensors(files) else batch.upload(files, fmt)


class Batch:
    def __init__(self, ctx: Context = None):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        raise_for_status(_lib.jpgpu_batch_create(self.ctx._h, C.byref(self._h)), b"jpgpu_batch_create failed")
        self.format = FMT_INTERLEAVED_U8
        self._keep = None
        self._resize = self._resized_as = None

    def _check(self, rc):
        raise_for_status(rc, _lib.jpgpu_last_error(self.ctx._h))

    def upload(self, files, fmt=FMT_INTERLEAVED_U8):
        """files: list of bytes-like objects or of (numpy uint8 array) views. Host parse + H2D."""
        n = len(files)
        ptrs = (C.c_void_p * n)()
        lens = (C.c_size_t * n)()
        keep = []
        for i, f in enumerate(files):
            a = np.frombuffer(f, dtype=np.uint8) if not isinstance(f, np.ndarray) else f
            if not a.flags["C_CONTIGUOUS"]:
                a = np.ascontiguousarray(a)
            keep.append(a)
            ptrs[i] = a.ctypes.data
            lens[i] = a.size
        self._check(_lib.jpgpu_batch_upload(self._h, ptrs, lens, n, fmt))
        self.format = fmt
        return self

    def upload_segments(self, files, fmt=FMT_INTERLEAVED_U8, pinned=False, arena=False):
        """files: list of files, each a LIST of bytes-like / uint8-array segments (the ReadOnlySequence<byte> a reference
        caller hands to SetInput, read in place).  pinned=True: every segment lies in page-locked memory
        (Context.host_alloc / host_register) and is DMA'd to HBM from where it lies.  arena=True (JPGPU_UPLOAD_PINNED_ARENA): all
        of them are views into ONE page-locked array, every file contiguous -- the span travels as a few large DMAs."""
        keep, segs, per = [], [], []
        for f in files:
            parts = f if isinstance(f, (list, tuple)) else [f]
            per.append(len(parts))
            for part in parts:
                a = np.frombuffer(part, dtype=np.uint8) if not isinstance(part, np.ndarray) else part
                if not a.flags["C_CONTIGUOUS"]:
                    if pinned or arena:
                        raise ValueError("a pinned segment must be contiguous (a copy would leave the page-locked memory)")
                    a = np.ascontiguousarray(a)
                keep.append(a)
                segs.append((a.ctypes.data if a.size else None, a.size))
        arr = (_capi.Segment * max(1, len(segs)))(*[_capi.Segment(d, n) for d, n in segs])
        cnt = (C.c_int * max(1, len(per)))(*per)
        self._check(_lib.jpgpu_batch_upload_segments(self._h, arr, cnt, len(per), fmt, (_capi.UPLOAD_PINNED_ARENA if arena else 0) | (_capi.UPLOAD_PINNED if pinned else 0)))
        self.format = fmt
        return self

    def upload_tensors(self, tensors, fmt=FMT_INTERLEAVED_U8):
        """upload() for files that are in device memory already (jpgpu_batch_upload_device): 1-D contiguous torch.uint8 tensors on the
        context's device, one per file -- an EncodeBatch.output_tensor(i), bytes a storage stack delivered into HBM.  The files are copied
        into the batch on the device; only their headers cross the host link (and, whole, the files that need the full marker walks).
        ValueError, before the library is called, for anything that is not such a tensor.  torch's current stream on the device is
        synchronised first, so whatever produced the bytes has finished.  The batch owns a copy when this returns: no reference to the
        tensors is kept, they may be overwritten or freed."""
        import torch

        tensors = list(tensors) if isinstance(tensors, (list, tuple)) else tensors
        files = _tensor_files(tensors, self.ctx.device)
        n = len(files)
        ptrs = (C.c_void_p * max(1, n))(*[p for p, _ in files])
        lens = (C.c_size_t * max(1, n))(*[m for _, m in files])
        # the library reads the tensors on its own stream: what torch has queued on its current one must have happened
        torch.cuda.current_stream(self.ctx.device).synchronize()
        self._check(_lib.jpgpu_batch_upload_device(self._h, ptrs, lens, n, fmt))
        self.format = fmt
        return self

    def upload_frames(self, frames, quant_tables, fmt=FMT_INTERLEAVED_U8):
        """Coefficient hand-off (progressive images, BASELINE config 5): frames = list of dicts
        {width, height, precision, components: [(id, h, v, tq), ...]}, quant_tables = uint16[n][4][64] (zig-zag order).
        Follow with set_coefficients(i, blocks in MCU scan order) and run_idct()."""
        n = len(frames)
        arr = (_capi.Frame * n)()
        for i, f in enumerate(frames):
            arr[i].width, arr[i].height, arr[i].precision = f["width"], f["height"], f["precision"]
            arr[i].num_components = len(f["components"])
            arr[i].sof = f.get("sof", 0xC2)
            for c, (cid, h, v, tq) in enumerate(f["components"]):
                arr[i].comp[c] = _capi.FrameComponent(cid, h, v, tq)
        qt = np.ascontiguousarray(quant_tables, dtype=np.uint16).reshape(n, 4, 64)
        self._check(_lib.jpgpu_batch_upload_frames(self._h, arr, qt.ctypes.data, n, fmt))
        self.format = fmt
        return self

    def set_windows(self, rects):
        """The windows of the NEXT upload(), upload_segments() or upload_tensors(): an iterable of (x, y, w, h) in pixels of the frame, one per
        file ((0, 0, 0, 0) = the whole frame), or None to withdraw pending ones.  Image i is then decoded into an output of its window's size
        -- the slice [y : y + h, x : x + w] of the whole decode, sample for sample -- and the output stage transforms only the MCUs the window
        touches.  Whole-pixel formats only.  The windows are consumed by that upload; the one after it decodes whole frames again.
        ValueError, before the library is called, for a rect that is not four non-negative integers below 2^32."""
        rects = _window_rects(rects)
        n = len(rects) if rects else 0
        arr = (_capi.Rect * max(1, n))(*[_capi.Rect(*r) for r in (rects or [])])
        self._check(_lib.jpgpu_batch_set_windows(self._h, arr, n))
        return self

    def set_color_policy(self, color):
        """How the RGB formats (RGB_U8, RGBA_U8, RGB_PLANAR_U8 / _F16 / _F32) read a file's colour from the next upload on: "ycc", the default
        -- 1 component is grey, 3 are YCbCr, anything else fails -- or "file": what the file declares (identify_color), so CMYK and YCCK files
        come out as RGB the way Pillow converts them and Adobe-RGB files keep their samples.  State of the batch: it holds until set again.
        ValueError, before the library is called, for any other value."""
        self._check(_lib.jpgpu_batch_set_color_policy(self._h, _color_policy(color)))
        return self

    def color(self, i):
        """"gray", "ycbcr", "rgb", "cmyk" or "ycck": the kind image i was planned with ("gray" / "ycbcr" under the "ycc" policy and under a
        format that does not read the policy)"""
        kind = C.c_int()
        raise_for_status(_lib.jpgpu_batch_image_color(self._h, i, C.byref(kind)), b"jpgpu_batch_image_color: no such image")
        return _capi.COLOR_KINDS[kind.value]

    def set_orientation_policy(self, orientation):
        """How the RGB formats (RGB_U8, RGBA_U8, RGB_PLANAR_U8 / _F16 / _F32) turn an image from the next upload on: "stored", the default -- as
        the file stores its pixels -- or "file": as its Exif orientation says (identify_orientation), the way ImageOps.exif_transpose does, so
        a portrait phone photo comes out upright, [3, W, H] for the values 5..8.  State of the batch: it holds until set again.  ValueError,
        before the library is called, for any other value."""
        self._check(_lib.jpgpu_batch_set_orientation_policy(self._h, _orientation_policy(orientation)))
        return self

    def set_orientations(self, orientations):
        """The orientations of the NEXT upload(), upload_segments() or upload_tensors(): one integer per file, 1..8 (the Exif values: 2 is the
        horizontal flip of the usual augmentation pair) used as given whatever the file says, or 0 for what the policy gives; None withdraws
        a pending list.  Consumed by that upload like windows.  RGB formats only.  ValueError, before the library is called, for anything
        that is not such an integer."""
        vals = _orientation_list(orientations)
        n = len(vals) if vals else 0
        arr = (C.c_uint8 * max(1, n))(*(vals or []))
        self._check(_lib.jpgpu_batch_set_orientations(self._h, arr, n))
        return self

    def orientation(self, i):
        """1..8: the orientation image i was planned with (1 under a format that does not read it)"""
        o = C.c_int()
        raise_for_status(_lib.jpgpu_batch_image_orientation(self._h, i, C.byref(o)), b"jpgpu_batch_image_orientation: no such image")
        return o.value

    def set_upsampling_policy(self, upsampling):
        """How the RGB formats (RGB_U8, RGBA_U8, RGB_PLANAR_U8 / _F16 / _F32) expand sub-sampled chroma from the next upload on: "replicate",
        the default -- every chroma sample repeated over the pixels it covers, as the reference does -- or "fancy": libjpeg's triangle filter
        for 4:2:2, 4:2:0 and 4:4:0 YCbCr images (include/jpgpu.h, "Chroma upsampling"), the chroma Pillow, torchvision and OpenCV deliver.
        State of the batch: it holds until set again.  ValueError, before the library is called, for any other value."""
        self._check(_lib.jpgpu_batch_set_upsampling_policy(self._h, _upsampling_policy(upsampling)))
        return self

    def upsampling(self, i):
        """1 where image i was planned with the "fancy" filter, else 0 (grey, 4:4:4, other ratios and kinds, planes two samples wide, a format
        that does not read the policy)"""
        a = C.c_int()
        raise_for_status(_lib.jpgpu_batch_image_upsampling(self._h, i, C.byref(a)), b"jpgpu_batch_image_upsampling: no such image")
        return a.value

    def upsampling_ms(self):
        """device time of this upload's last K3U call, from an event pair of its own (synchronises); only for an upload made under
        JPGPU_TIME_UPSAMPLE=1 that has a filtered image and was decoded -- a measuring aid (tools/bench_decode_upsample.py)"""
        ms = C.c_float()
        self._check(_lib.jpgpu_batch_upsampling_ms(self._h, C.byref(ms)))
        return ms.value

    def set_arithmetic_policy(self, arithmetic):
        """Which arithmetic the RGB formats decode with from the next upload on: "reference", the default -- the reference's float transform and
        colour constants, as ever -- or "libjpeg": jpeg_idct_islow, libjpeg's integer transform, and its colour constants (include/jpgpu.h,
        "Arithmetic"), bit for bit what Pillow, torchvision and OpenCV compute; with set_upsampling_policy("fancy") the pixels are theirs.
        Every other format ignores it.  State of the batch: it holds until set again.  ValueError, before the library is called, for any
        other value."""
        self._check(_lib.jpgpu_batch_set_arithmetic_policy(self._h, _arithmetic_policy(arithmetic)))
        return self

    def arithmetic(self, i):
        """1 where image i was planned with libjpeg's integer transform, else 0 (the policy unset, a format that does not read it, a 12-bit
        frame or another image outside the rule of include/jpgpu.h)"""
        a = C.c_int()
        raise_for_status(_lib.jpgpu_batch_image_arithmetic(self._h, i, C.byref(a)), b"jpgpu_batch_image_arithmetic: no such image")
        return a.value

    def set_scale_policy(self, denom):
        """The size the RGB formats decode at from the next upload on: 1, the default, or 2, 4, 8 -- the picture at 1/2, 1/4, 1/8 size through
        libjpeg's reduced transforms (include/jpgpu.h, "Scaled decode"), ceil(W / denom) x ceil(H / denom) pixels, bit for bit Pillow's
        draft() decode.  Only images that take libjpeg's transform (set_arithmetic_policy("libjpeg"); arithmetic(i) == 1) take it; every other
        image keeps full size, and scale(i) says which.  Windows are then in pixels of the reduced frame.  State of the batch: it holds until
        set again.  ValueError, before the library is called, for any other value."""
        self._check(_lib.jpgpu_batch_set_scale_policy(self._h, _scale_setting(denom, who="denom")))
        return self

    def set_scale_fit(self, size):
        """Pillow's draft() rule from the next upload on: size = (h, w), the least size wanted -- every image takes the largest of 1/8, 1/4,
        1/2 that leaves its oriented frame at least that large, or full size (k = min(W // w, H // h): 8 if k >= 8, else 4, else 2, else 1).
        While set it overrides set_scale_policy; None switches it off.  ValueError, before the library is called, for anything else."""
        if size is None:
            h = w = 0
        else:
            try:
                h, w = size
            except (TypeError, ValueError):
                raise ValueError("set_scale_fit: size is (h, w) or None, not %r" % (size,))
            if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 or v > 0xFFFFFFFF for v in (h, w)):
                raise ValueError("set_scale_fit: size is two positive integers (h, w), not %r" % (size,))
        self._check(_lib.jpgpu_batch_set_scale_fit(self._h, w, h))
        return self

    def scale(self, i):
        """The denominator image i was planned with: 1, 2, 4 or 8"""
        d = C.c_int()
        raise_for_status(_lib.jpgpu_batch_image_scale(self._h, i, C.byref(d)), b"jpgpu_batch_image_scale: no such image")
        return d.value

    def set_channels_policy(self, mode):
        """How many planes RGB_PLANAR_U8 / _F16 / _F32 deliver from the next upload on: "rgb", the default -- three, as ever -- or "gray": ONE
        tight plane [1, H, W] of the oriented frame or its window (include/jpgpu.h, "Grey output") -- component 0's samples for grey and
        YCbCr files, Pillow's convert("L") of the RGB bytes for the CMYK, YCCK and Adobe-RGB files of color="file".  The float forms take
        scale[0] and bias[0] of set_output_affine.  Every other format ignores it.  State of the batch: it holds until set again.
        ValueError, before the library is called, for any other value."""
        self._check(_lib.jpgpu_batch_set_channels_policy(self._h, _channels_policy(mode)))
        return self

    def channels(self, i):
        """1 where image i was planned with one plane ("gray" under an RGB_PLANAR_* format), else 3"""
        c = C.c_int()
        raise_for_status(_lib.jpgpu_batch_image_channels(self._h, i, C.byref(c)), b"jpgpu_batch_image_channels: no such image")
        return c.value

    def luma_work(self):
        """(images on the fast road, images on the scratch road) of this upload under "gray": which kernel forms each one's plane"""
        counts = (C.c_int32 * 2)()
        self._check(_lib.jpgpu_batch_luma_work(self._h, counts))
        return (counts[0], counts[1])

    def window(self, i):
        """(x, y, w, h): the window image i was planned with, in pixels of the oriented frame; (0, 0, W, H) of that frame for a whole one"""
        r = _capi.Rect()
        raise_for_status(_lib.jpgpu_batch_image_window(self._h, i, C.byref(r)), b"jpgpu_batch_image_window: no such image")
        return (r.x, r.y, r.width, r.height)

    def decode(self):
        self._check(_lib.jpgpu_batch_decode(self._h))
        self._resized_as = getattr(self, "_resize", None)
        return self

    def run_entropy(self):
        self._check(_lib.jpgpu_batch_run_entropy(self._h))
        return self

    def run_idct(self):
        self._check(_lib.jpgpu_batch_run_idct(self._h))
        self._resized_as = getattr(self, "_resize", None)
        return self

    def set_resize(self, size, dtype=None):
        """The resize stage: from the next decode() / run_idct() on, every image of an RGB_PLANAR_U8 upload (its window, if it has one) is also
        resampled to size = (oh, ow) -- antialiased bilinear, the fixed function include/jpgpu.h states -- into ONE dense [N, 3, oh, ow] buffer of
        dtype (torch.uint8, the default, torch.float16 or torch.float32; the float samples take the constants of set_output_affine), in one
        launch behind the output stage.  The per-image outputs stay what they are.  Launch state like the constants: it holds until set again;
        None withdraws it, and with it what an earlier decode left.  A decode of an upload of another format is refused while it is set.
        ValueError, before the library is called, for anything that is not such a size or dtype."""
        if size is None:
            self._check(_lib.jpgpu_batch_set_resize(self._h, 0, 0, 0))
            self._resize = self._resized_as = None
            return self
        if dtype is None:
            import torch

            dtype = torch.uint8
        oh, ow, fmt, np_dtype = _resize_setting(size, dtype)
        self._check(_lib.jpgpu_batch_set_resize(self._h, ow, oh, fmt))
        self._resize = (oh, ow, fmt, np_dtype)
        return self

    def _resized_span(self):
        """(device pointer, (N, 3, oh, ow), format, numpy dtype) of the resized buffer -- (N, 1, oh, ow) for an upload made under "gray" --;
        raises when no decode with a resize set has run"""
        ptr, total = C.c_void_p(), C.c_uint64()
        self._check(_lib.jpgpu_batch_resized_device(self._h, C.byref(ptr), C.byref(total)))
        made = getattr(self, "_resized_as", None)
        if made is None:
            raise ValueError("resized: the resize was not set through this object (Batch.set_resize)")
        oh, ow, fmt, np_dtype = made
        one_plane = len(self) * oh * ow * np.dtype(np_dtype).itemsize  # (the library sizes the slabs by the upload's plane count)
        shape = (len(self), 1 if total.value == one_plane and one_plane != 0 else 3, oh, ow)
        if total.value != int(np.prod(shape, dtype=np.int64)) * np.dtype(np_dtype).itemsize:
            raise ValueError("resized: the buffer holds %d bytes, not %s of %s" % (total.value, shape, np.dtype(np_dtype)))
        return ptr.value, shape, fmt, np_dtype

    def resized(self):
        """Downloads the resized images: a numpy array [N, 3, oh, ow] of the dtype that was set (an image that failed reads as zeros)."""
        _, shape, _, np_dtype = self._resized_span()
        out = np.empty(shape, dtype=np_dtype)
        for i in range(shape[0]):
            self._check(_lib.jpgpu_batch_download_resized(self._h, i, out[i].ctypes.data, out[i].nbytes))
        return out

    def resized_tensor(self):
        """The resized images as ONE torch tensor [N, 3, oh, ow] on the context's device that ALIASES the batch's resized buffer -- no copy:
        data_ptr() is jpgpu_batch_resized_device's pointer.  output_tensor's rules: sync() is called first, the tensor keeps the batch alive,
        a borrowed batch raises, and the next upload(), decode(), set_resize(None) or close() invalidates it."""
        import torch  # (here: the package imports without torch)

        if not getattr(self, "_owned", True):
            raise ValueError("resized_tensor: a borrowed batch (a MultiDecoder shard) is recycled by its owner; use resized()")
        ptr, shape, fmt, _ = self._resized_span()
        self.sync()
        if not ptr or 0 in shape:
            raise ValueError("resized_tensor: the batch has no resized buffer")
        return torch.as_tensor(_DeviceView(self, ptr, shape, _typestr(fmt)), device=torch.device("cuda", self.ctx.device))

    def resize_ms(self):
        """Device time (ms) of the last resize launch, from an event pair of its own; stage_ms() does not include it."""
        ms = C.c_float()
        self._check(_lib.jpgpu_batch_resize_ms(self._h, C.byref(ms)))
        return ms.value

    def set_output_affine(self, scale, bias):
        """RGB_PLANAR_F16 / _F32: sample = float32(byte) * scale[c] + bias[c] per channel c (R, G, B); the default is scale 1, bias 0.  The
        constants belong to the batch, not to an upload: they hold from the next decode() / run_idct() on.  ArgumentException for a constant
        that is not finite (the ones in force stay).  The other formats never read them."""
        s, b = np.asarray(scale, dtype=np.float32).reshape(-1), np.asarray(bias, dtype=np.float32).reshape(-1)
        if s.shape != (3,) or b.shape != (3,):
            raise ValueError("scale and bias are three values each, one per channel (R, G, B)")
        self._check(_lib.jpgpu_batch_set_output_affine(self._h, (C.c_float * 3)(*s.tolist()), (C.c_float * 3)(*b.tolist())))
        return self

    def sync(self):
        self._check(_lib.jpgpu_batch_sync(self._h))
        return self

    def __len__(self):
        return _lib.jpgpu_batch_size(self._h)

    def image_info(self, i) -> _capi.ImageInfo:
        info = _capi.ImageInfo()
        self._check(_lib.jpgpu_batch_image_info(self._h, i, C.byref(info)))
        return info

    def result(self, i) -> _capi.ImageResult:
        res = _capi.ImageResult()
        self._check(_lib.jpgpu_batch_result(self._h, i, C.byref(res)))
        return res

    def stage_ms(self):
        ms = (C.c_float * 4)()
        self._check(_lib.jpgpu_batch_stage_ms(self._h, ms))
        return {"marker_index": ms[0], "huffman": ms[1], "idct": ms[2], "total": ms[3]}

    def ingest_stats(self):
        """What the last upload() did: files planned from their headers alone vs full host walks, and where the time went."""
        st = _capi.IngestStats()
        self._check(_lib.jpgpu_batch_ingest_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _capi.IngestStats._fields_}

    def device_ingest_stats(self):
        """What the last upload_tensors() moved: files_gathered / bytes_gathered (device to device), head_bytes (the headers, D2H),
        files_downloaded / bytes_downloaded (files fetched whole for the full marker walks), walker_giveups, gather_ms (device time of the
        gather).  Zero behind any other upload."""
        st = _capi.DeviceIngestStats()
        self._check(_lib.jpgpu_batch_device_ingest_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _capi.DeviceIngestStats._fields_}

    def plan_stats(self):
        """How the last upload() planned the entropy stage (K2's plain list and pools, K2S's final-pass list, pools and table
        sets, k2s_subs_per_lane = subsequences a lane of the final pass takes, k2s_sub_shift = log2 of the subsequence length in bits,
        0 without K2S scans, k2s_subs = subsequences over all K2S scans) and K3: idct_work = work entries per output layout class (generic, YCbCr 1x1, 2x1, 2x2, gray, store of samples),
        idct_split_work = those of them that belong to scans handed over as half-line planes, idct_listed_mcus = the MCUs all of K3's work
        entries list (under windows: the MCUs the windows touch)."""
        st = _capi.PlanStats()
        self._check(_lib.jpgpu_batch_plan_stats(self._h, C.byref(st)))
        work = (C.c_int32 * IDCT_LAYOUT_CLASSES)()
        self._check(_lib.jpgpu_batch_idct_work(self._h, work, IDCT_LAYOUT_CLASSES))
        split = (C.c_int32 * IDCT_LAYOUT_CLASSES)()
        self._check(_lib.jpgpu_batch_idct_split_work(self._h, split, IDCT_LAYOUT_CLASSES))
        listed = C.c_uint64()
        self._check(_lib.jpgpu_batch_idct_listed_mcus(self._h, C.byref(listed)))
        return dict({k: getattr(st, k) for k, _ in _capi.PlanStats._fields_}, idct_work=list(work), idct_split_work=list(split),
                    idct_listed_mcus=listed.value)

    def progressive_fallbacks(self):
        """Times the single-launch progressive path timed out and the step was re-issued level by level."""
        return _lib.jpgpu_batch_progressive_fallbacks(self._h)

    def progressive_plan(self):
        """How the last upload() planned the scans of its progressive frames (scans, levels, max_deps, pipelined, chains_ok,
        pipe_waves, wave_tails, lane_work, chain_scans[5]) and launch_form: what the last decode() / run_entropy() launched for
        them -- "pipelined_gated", "pipelined_forced", "chains", "by_level" or "none"."""
        st = _capi.ProgressivePlan()
        self._check(_lib.jpgpu_batch_progressive_plan(self._h, C.byref(st)))
        d = {k: getattr(st, k) for k, _ in _capi.ProgressivePlan._fields_}
        return dict(d, pipelined=bool(st.pipelined), chains_ok=bool(st.chains_ok), chain_scans=list(st.chain_scans),
                    launch_form=_capi.PROG_LAUNCH_NAMES[st.launch_form])

    def subseq_rounds(self):
        """Synchronisation rounds the DRI = 0 subsequence decoder needed in the last decode (0 = not used)."""
        return _lib.jpgpu_batch_subseq_rounds(self._h)

    def set_partial_flush(self, on=True):
        """Failing progressive files: reproduce the reference's partial flush (default) or leave those frames' outputs unspecified."""
        self._check(_lib.jpgpu_batch_set_partial_flush(self._h, 1 if on else 0))
        return self

    def progressive_replays(self):
        """Times a partial-flush replay was issued for this batch."""
        return _lib.jpgpu_batch_progressive_replays(self._h)

    def marker_fallbacks(self):
        """Waits behind which a group of the one-pass marker index had run out of patience and counted its predecessors itself (expected: 0)."""
        return _lib.jpgpu_batch_marker_fallbacks(self._h)

    def subseq_fallbacks(self):
        """Times the enqueued K2S rounds did not converge and the step was issued again with host-checked rounds."""
        return _lib.jpgpu_batch_subseq_fallbacks(self._h)

    def totals(self):
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.jpgpu_batch_totals(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return {"compressed_bytes": a.value, "blocks": b.value, "pixels": c.value, "output_bytes": d.value}

    def output_device_ptr(self):
        total = C.c_uint64()
        p = _lib.jpgpu_batch_output_device(self._h, C.byref(total))
        return p, total.value

    def output(self, i):
        """Downloads image i. INTERLEAVED_U8 / INTERLEAVED_U8_SCALED -> uint8[H,W,C]; RGB_U8 / RGBA_U8 -> uint8[H,W,3|4]; RGB_PLANAR_U8 -> uint8[3,H,W];
        RGB_PLANAR_F16 / _F32 -> float16 / float32 [3,H,W]; EXTENDED_U16 -> uint16[H,W,4]; PLANAR_* -> list of per-component 2-D arrays (padded)."""
        info = self.image_info(i)
        raise_for_status(info.status, _lib.jpgpu_last_error(self.ctx._h))
        raw = np.empty(info.out_bytes, dtype=np.uint8)
        self._check(_lib.jpgpu_batch_download_output(self._h, i, raw.ctypes.data, raw.size))
        _, _, w, h = self.window(i)  # (the whole oriented frame's W, H without a window)
        if self.format in (FMT_INTERLEAVED_U8, FMT_INTERLEAVED_U8_SCALED):
            return raw.reshape(h, w, info.num_components)
        if self.format in (FMT_RGB_U8, FMT_RGBA_U8):
            return raw.reshape(h, w, 4 if self.format == FMT_RGBA_U8 else 3)
        if self.format in _RGB_PLANES:  # three tight planes R, G, B, or the one plane of "gray" (Batch.set_channels_policy)
            return raw.view(_SAMPLE_DTYPES.get(self.format, np.uint8)).reshape(self._planes(info), h, w)
        if self.format == FMT_EXTENDED_U16:  # the reference tests' JpegExtendingOutputWriter buffer: ushort x 4 per pixel
            return raw.view(np.uint16).reshape(info.height, info.width, 4)
        dt = np.int16 if self.format == FMT_PLANAR_I16 else np.uint8
        planes = []
        for c in range(info.num_components):
            p = info.plane[c]
            nbytes = p.pitch * p.height * np.dtype(dt).itemsize
            planes.append(raw[p.offset:p.offset + nbytes].view(dt).reshape(p.height, p.pitch)[:, :p.width])
        return planes

    @staticmethod
    def _planes(info):
        """planes of an RGB_PLANAR_* image: 1 where it was planned under "gray" (plane[1] and plane[2] are zero), else 3"""
        return 1 if info.plane[0].width != 0 and info.plane[1].width == 0 and info.plane[1].pitch == 0 else 3

    def _tensor_shape(self, info, hw=None):
        """hw: the (h, w) of the image's window (Batch.window), which is the oriented frame's without one; None: the stored frame's"""
        h, w = hw if hw is not None else (info.height, info.width)
        if self.format in (FMT_INTERLEAVED_U8, FMT_INTERLEAVED_U8_SCALED):
            return (h, w, info.num_components)
        if self.format in (FMT_RGB_U8, FMT_RGBA_U8):
            return (h, w, 4 if self.format == FMT_RGBA_U8 else 3)
        if self.format in _RGB_PLANES:
            return (self._planes(info), h, w)
        raise ValueError("output_tensor: format %d is not one dense uint8 array per image (MCU-padded planes, or uint16 pixels); use output()" % self.format)

    def output_tensor(self, i):
        """Image i as a torch uint8 tensor on the context's device that ALIASES the batch's output buffer -- no copy, no download:
        data_ptr() == output_device_ptr()[0] + image_info(i).out_offset.  RGB_PLANAR_U8 -> (3, H, W); RGB_PLANAR_F16 / _F32 -> a torch.float16 /
        float32 (3, H, W) tensor; INTERLEAVED_U8 / INTERLEAVED_U8_SCALED /
        RGB_U8 -> (H, W, C); RGBA_U8 -> (H, W, 4).  The MCU-padded PLANAR_* formats and EXTENDED_U16 raise ValueError; an image that failed
        raises as output() does.  sync() is called first, so the tensor may be used on any torch stream.  The tensor keeps the batch alive.
        One rule remains: the next upload() on this batch, or an explicit close(), invalidates every tensor made from it."""
        import torch  # (here: the package imports without torch)

        info = self.image_info(i)
        raise_for_status(info.status, _lib.jpgpu_last_error(self.ctx._h))
        win = self.window(i)
        shape = self._tensor_shape(info, (win[3], win[2]))
        if not getattr(self, "_owned", True):
            raise ValueError("output_tensor: a borrowed batch (a MultiDecoder shard) is recycled by its owner; use output()")
        self.sync()
        base, total = self.output_device_ptr()
        if not base or info.out_offset + info.out_bytes > total:
            raise ValueError("output_tensor: the batch has no output buffer for image %d" % i)
        view = _DeviceView(self, base + info.out_offset, shape, _typestr(self.format))
        return torch.as_tensor(view, device=torch.device("cuda", self.ctx.device))

    def coefficients(self, i):
        """int16[blocks, 64] zig-zag order, MCU scan order (the buffer between the Huffman and IDCT stages)."""
        info = self.image_info(i)
        raise_for_status(info.status, _lib.jpgpu_last_error(self.ctx._h))
        out = np.empty((info.total_blocks, 64), dtype=np.int16)
        self._check(_lib.jpgpu_batch_download_coefficients(self._h, i, out.ctypes.data, info.total_blocks))
        return out

    def set_coefficients(self, i, coefs):
        coefs = np.ascontiguousarray(coefs, dtype=np.int16).reshape(-1, 64)
        self._check(_lib.jpgpu_batch_upload_coefficients(self._h, i, coefs.ctypes.data, coefs.shape[0]))

    @classmethod
    def _borrowed(cls, handle, ctx_handle, fmt):
        """A view on a batch some other object owns (MultiDecoder's shards): same accessors, close() leaves it alone."""
        self = cls.__new__(cls)
        self.ctx = _BorrowedContext(ctx_handle)
        self._h = C.c_void_p(handle)
        self.format = fmt
        self._keep = None
        self._resize = self._resized_as = None
        self._owned = False
        return self

    def close(self):
        if self._h and getattr(self, "_owned", True):
            _lib.jpgpu_batch_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_batch(files, fmt=FMT_INTERLEAVED_U8, ctx=None, windows=None, color="ycc", orientation="stored", orientations=None, upsampling="replicate", mode="rgb", arithmetic="reference"):
    """One-call helper: returns (outputs, results).  files: bytes-like objects, or 1-D uint8 torch tensors on the context's device.
    windows: one (x, y, w, h) per file (Batch.set_windows): outputs[i] is that rectangle of image i.
    color: "ycc" or "file" (Batch.set_color_policy): under "file" the RGB formats deliver RGB for CMYK, YCCK and Adobe-RGB files.
    orientation: "stored" or "file" (Batch.set_orientation_policy); orientations: one value 0..8 per file (Batch.set_orientations).  Windows
    are then in pixels of the oriented frame.
    upsampling: "replicate" or "fancy" (Batch.set_upsampling_policy): under "fancy" the RGB formats filter 4:2:2 / 4:2:0 / 4:4:0 chroma as libjpeg does.
    mode: "rgb" or "gray" (Batch.set_channels_policy): under "gray" RGB_PLANAR_U8 / _F16 / _F32 give one plane, [1, H, W]; ValueError for another fmt.
    arithmetic: "reference" or "libjpeg" (Batch.set_arithmetic_policy): under "libjpeg" the RGB formats decode with libjpeg's integer transform and constants."""
    files = list(files)
    windows = _window_rects(windows, len(files))
    _color_policy(color)
    _orientation_policy(orientation)
    _upsampling_policy(upsampling)
    _arithmetic_policy(arithmetic)
    _channels_policy(mode, fmt)
    orientations = _orientation_list(orientations, len(files))
    b = Batch(ctx)
    b.set_color_policy(color)
    b.set_orientation_policy(orientation)
    b.set_upsampling_policy(upsampling)
    b.set_arithmetic_policy(arithmetic)
    b.set_channels_policy(mode)
    if orientations is not None:
        b.set_orientations(orientations)
    if windows is not None:
        b.set_windows(windows)
    b = _upload_any(b, files, fmt).decode().sync()
    outs, results = [], []
    for i in range(len(b)):
        r = b.result(i)
        results.append(r)
        outs.append(b.output(i) if b.image_info(i).status == 0 else None)
    b.close()
    return outs, results


def decode_to_tensors(files, fmt=FMT_RGB_PLANAR_U8, dtype=None, mean=None, std=None, ctx=None, windows=None, color="ycc", orientation="stored", orientations=None, upsampling="replicate", mode="rgb", arithmetic="reference", scale=1):
    """One-call helper for torch consumers: returns (tensors, results), tensors[i] = Batch.output_tensor(i) -- uint8[3, H, W] on the
    context's device by default -- or None for an image that failed.  Nothing is downloaded.  The batch is not closed: its output
    buffer is the tensors' memory and is freed with the last of them.  files: bytes-like objects, or 1-D uint8 torch tensors on the
    context's device (Batch.upload_tensors: e.g. EncodeBatch.output_tensor(i) -- the streams never leave the device).
    dtype=torch.float16 / torch.float32 selects RGB_PLANAR_F16 / _F32: float [3, H, W] tensors written by the decoder's output stage itself.
    mean / std (per channel, 0..1 units; both or neither) then make them (u / 255 - mean) / std through affine_from_mean_std; without them
    a sample is the byte as a float.
    windows: one (x, y, w, h) per file (Batch.set_windows): tensors[i] is [3, h, w], that rectangle of image i, decoded without the rest.
    color: "ycc" or "file" (Batch.set_color_policy): under "file" CMYK, YCCK and Adobe-RGB files come out as RGB instead of failing or
    taking the YCbCr matrix.
    orientation: "stored" or "file" (Batch.set_orientation_policy): under "file" an image is turned as its Exif orientation says, so
    tensors[i] is [3, W, H] for the values 5..8; orientations: one value 0..8 per file (Batch.set_orientations), e.g. 2 for a horizontal flip.
    Windows are then in pixels of the oriented frame.
    upsampling: "replicate" or "fancy" (Batch.set_upsampling_policy): under "fancy" sub-sampled chroma (4:2:2, 4:2:0, 4:4:0) is expanded with
    libjpeg's triangle filter, as Pillow, torchvision and OpenCV deliver it, instead of repeated; windows, orientation and dtype compose on it.
    mode: "rgb" or "gray" (Batch.set_channels_policy): under "gray" tensors[i] is [1, H, W] -- the luma samples of a grey or YCbCr file, decoded
    without touching its chroma, or Pillow's convert("L") of a CMYK, YCCK or Adobe-RGB file under color="file".  mean and std are then a number or
    a sequence of one; every other argument composes, and upsampling="fancy" changes nothing (no chroma is read).  ValueError for a fmt that is
    not RGB_PLANAR_*.
    arithmetic: "reference" or "libjpeg" (Batch.set_arithmetic_policy): under "libjpeg" the samples come from libjpeg's integer transform
    (jpeg_idct_islow) and its colour constants; with upsampling="fancy" tensors[i] holds exactly the pixels Pillow and torchvision decode.
    Everything else composes on it.
    scale: 1, 2, 4 or 8 (Batch.set_scale_policy): with arithmetic="libjpeg", tensors[i] is the picture at 1 / scale size, [3, ceil(H / scale),
    ceil(W / scale)], through libjpeg's reduced transforms -- Pillow's draft() decode; windows are in pixels of that picture.  ValueError for
    another value, or for a scale other than 1 without arithmetic="libjpeg"."""
    files = list(files)
    windows = _window_rects(windows, len(files))
    _color_policy(color)
    _orientation_policy(orientation)
    _upsampling_policy(upsampling)
    _arithmetic_policy(arithmetic)
    _scale_setting(scale, arithmetic)
    orientations = _orientation_list(orientations, len(files))
    if dtype is not None:
        import torch

        by_dtype = {torch.float16: FMT_RGB_PLANAR_F16, torch.float32: FMT_RGB_PLANAR_F32, torch.uint8: fmt}
        if dtype not in by_dtype:
            raise ValueError("decode_to_tensors: dtype is torch.float16, torch.float32 or torch.uint8, not %s" % (dtype,))
        if dtype != torch.uint8 and fmt not in _RGB_PLANES:
            raise ValueError("decode_to_tensors: float samples come as three planes (3, H, W) only; leave fmt at its default")
        fmt = by_dtype[dtype]
    if (mean is None) != (std is None):
        raise ValueError("decode_to_tensors: mean and std go together")
    if mean is not None and fmt not in _SAMPLE_DTYPES:
        raise ValueError("decode_to_tensors: mean / std apply to float samples; pass dtype=torch.float16 or torch.float32")
    _channels_policy(mode, fmt)
    if mean is not None and mode == "gray":
        mean, std = _gray_mean_std(mean, std)
    consts = affine_from_mean_std(mean, std) if mean is not None else None
    b = Batch(ctx)
    b.set_color_policy(color)
    b.set_orientation_policy(orientation)
    b.set_upsampling_policy(upsampling)
    b.set_arithmetic_policy(arithmetic)
    b.set_scale_policy(scale)
    b.set_channels_policy(mode)
    if orientations is not None:
        b.set_orientations(orientations)
    if consts is not None:
        b.set_output_affine(*consts)
    if windows is not None:
        b.set_windows(windows)
    b = _upload_any(b, files, fmt).decode().sync()
    tensors, results = [], []
    for i in range(len(b)):
        results.append(b.result(i))
        tensors.append(b.output_tensor(i) if b.image_info(i).status == 0 and results[-1].status == 0 else None)
    return tensors, results


def decode_resized(files, size, dtype=None, mean=None, std=None, windows=None, ctx=None, color="ycc", orientation="stored", orientations=None, upsampling="replicate", mode="rgb", arithmetic="reference", scale=1):
    """One-call helper for fixed-size consumers: returns (tensor, results), tensor = Batch.resized_tensor() -- ONE [N, 3, oh, ow] tensor on the
    context's device, size = (oh, ow), dtype torch.float16 (the default), torch.float32 or torch.uint8 -- every image decoded to RGB and
    resampled to that size (antialiased bilinear) in one launch behind the output stage; the slab of an image that failed is zero and
    results[i] says why.  Nothing is downloaded, and the batch is not closed: its buffer is the tensor's memory and is freed with it.
    files: bytes-like objects, or 1-D uint8 torch tensors on the context's device, as in decode_to_tensors.  mean / std (per channel, 0..1
    units; both or neither) make the float samples (v / 255 - mean) / std through affine_from_mean_std; they are refused for torch.uint8.
    windows: one (x, y, w, h) per file (Batch.set_windows): that rectangle of image i is what is resampled -- a RandomResizedCrop's crop.
    color: "ycc" or "file" (Batch.set_color_policy), orientation and orientations (Batch.set_orientation_policy / set_orientations), as in
    decode_to_tensors: the oriented image is what is resampled.  upsampling: "replicate" or "fancy" (Batch.set_upsampling_policy): under "fancy"
    the image that is resampled has libjpeg's filtered chroma.  mode: "rgb" or "gray" (Batch.set_channels_policy): under "gray" the tensor is
    [N, 1, oh, ow], the grey plane of decode_to_tensors(mode="gray") resampled by the same function; mean and std are a number or a sequence of one.
    arithmetic: "reference" or "libjpeg" (Batch.set_arithmetic_policy): under "libjpeg" the image that is resampled is libjpeg's decode.
    scale: 1, 2, 4, 8 (Batch.set_scale_policy) or "fit" (Batch.set_scale_fit(size)): with arithmetic="libjpeg" the image that is resampled is
    decoded at 1 / scale size first -- under "fit" at the smallest of 1/1 .. 1/8, per image, that is still at least `size`, Pillow's draft()
    rule --, so a large file costs the output stage and the resize a fraction of its pixels.  "fit" together with windows is a ValueError."""
    import torch

    files = list(files)
    windows = _window_rects(windows, len(files))
    _color_policy(color)
    _orientation_policy(orientation)
    _upsampling_policy(upsampling)
    _arithmetic_policy(arithmetic)
    _scale_setting(scale, arithmetic, fit=True, windows=windows, who="decode_resized: scale")
    orientations = _orientation_list(orientations, len(files))
    dtype = torch.float16 if dtype is None else dtype
    _resize_setting(size, dtype)
    _all_tensors(files)  # (a list that mixes bytes and tensors raises here, before a batch exists)
    if (mean is None) != (std is None):
        raise ValueError("decode_resized: mean and std go together")
    if mean is not None and dtype == torch.uint8:
        raise ValueError("decode_resized: mean / std apply to float samples; pass dtype=torch.float16 or torch.float32")
    _channels_policy(mode)
    if mean is not None and mode == "gray":
        mean, std = _gray_mean_std(mean, std)
    consts = affine_from_mean_std(mean, std) if mean is not None else None
    b = Batch(ctx)
    b.set_color_policy(color)
    b.set_orientation_policy(orientation)
    b.set_upsampling_policy(upsampling)
    b.set_arithmetic_policy(arithmetic)
    if scale == "fit":
        b.set_scale_fit(tuple(size))
    else:
        b.set_scale_policy(scale)
    b.set_channels_policy(mode)
    if orientations is not None:
        b.set_orientations(orientations)
    if consts is not None:
        b.set_output_affine(*consts)
    b.set_resize(size, dtype)
    if windows is not None:
        b.set_windows(windows)
    b = _upload_any(b, files, FMT_RGB_PLANAR_U8).decode().sync()
    results = [b.result(i) for i in range(len(b))]
    return b.resized_tensor(), results
