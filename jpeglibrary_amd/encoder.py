"""Batch encode on the GPU: the reference's JpegEncoder.Encode() with the EncodeAction call sequence
(ref: src/JpegLibrary/JpegEncoder.cs:255-291, apps/JpegEncode/EncodeAction.cs:38-63) for a set of images at once.

    encoder.SetQuantizationTable(ScaleByQuality(luminance / chrominance, quality)); SetHuffmanTable(standard tables);
    AddComponent(1, 0, 0, 0, h, v); AddComponent(2, 1, 1, 1, 1, 1); AddComponent(3, 1, 1, 1, 1, 1);
    SetInputReader(JpegBufferInputReader(width, height, components, pixels)); SetOutput(writer); Encode()
"""
import ctypes as C

import numpy as np

from . import _capi
from .batch import _DeviceView, _arithmetic_policy
from .context import Context, default_context
from .errors import raise_for_status

_lib = _capi.lib


def describe(width, height, components, quant_tables, huffman_tables, in_components=None, input_rgb=0, restart_interval=0,
             most_optimal_coding=False):
    """A jpgpu_encode_description: the encoder's state after the caller's Set* / AddComponent sequence (include/jpgpu.h, 4b).
    components: (component_index, h, v, tq, td, ta, captured 64 zig-zag elements) in AddComponent order;
    quant_tables: (identifier, 64 zig-zag elements) in SetQuantizationTable order;
    huffman_tables: (table_class, identifier, codes) in SetHuffmanTable order, codes = None (built from the image) or the
    JpegHuffmanCanonicalCode[] as (symbol, code, length) triples."""
    if len(components) > _capi.ENC_MAX_COMPONENTS:
        raise ValueError("at most four components can be described")
    if len(quant_tables) > _capi.ENC_MAX_TABLES or len(huffman_tables) > _capi.ENC_MAX_TABLES:
        raise ValueError("at most eight tables of a kind can be described")
    d = _capi.EncodeDescription()
    d.width, d.height = int(width), int(height)
    d.in_components = len(components) if in_components is None else int(in_components)
    d.input_rgb, d.restart_interval, d.most_optimal_coding = int(input_rgb), int(restart_interval), int(bool(most_optimal_coding))
    d.num_components, d.num_quant_tables, d.num_huffman_tables = len(components), len(quant_tables), len(huffman_tables)
    for k, (index, h, v, tq, td, ta, quant) in enumerate(components):
        c = d.components[k]
        c.component_index, c.h, c.v, c.tq, c.td, c.ta = int(index), int(h), int(v), int(tq), int(td), int(ta)
        c.quant[:] = [int(q) for q in quant]
    for k, (identifier, elements) in enumerate(quant_tables):
        d.quant_tables[k].identifier = int(identifier)
        d.quant_tables[k].elements[:] = [int(q) for q in elements]
    for k, (table_class, identifier, codes) in enumerate(huffman_tables):
        t = d.huffman_tables[k]
        t.table_class, t.identifier, t.given = int(table_class), int(identifier), 0 if codes is None else 1
        if codes is not None:
            if len(codes) > 256:
                raise ValueError("a Huffman table holds at most 256 codes")
            t.num_codes = len(codes)
            for j, (symbol, code, length) in enumerate(codes):
                t.symbol[j], t.code[j], t.length[j] = int(symbol), int(code), int(length)
    return d


def description_header(desc):
    """Host only: (status, message, SOI..SOS bytes of the WriteScanData path) for a description, no device needed."""
    n = C.c_size_t(0)
    buf = C.create_string_buffer(4096)
    msg = C.create_string_buffer(512)
    rc = _lib.jpgpu_encode_description_header(C.byref(desc), buf, len(buf), C.byref(n), msg, len(msg))
    return rc, msg.value.decode("utf-8", "replace"), buf.raw[:n.value] if rc == 0 else b""


def _coding_policy(coding, who="coding"):
    """The check of EncodeBatch.set_coding_policy / encode_batch(coding=...), before any library call: the jpgpu_coding_policy value"""
    if coding not in _capi.CODING_POLICIES:
        raise ValueError("%s is 'standard', 'optimized' or 'progressive', not %r" % (who, coding))
    return _capi.CODING_POLICIES.index(coding)


def libjpeg_optimal_table(freq):
    """Host only: libjpeg's jpeg_gen_optimal_table for 256 symbol counts -> (bits[16], values) of the DHT (jpgpu_libjpeg_optimal_table).
    Counts that are all zero give the empty table, ([0] * 16, [])."""
    f = np.ascontiguousarray(freq, dtype=np.uint32).reshape(256)
    bits, values, n = (C.c_uint8 * 16)(), (C.c_uint8 * 256)(), C.c_int(0)
    raise_for_status(_lib.jpgpu_libjpeg_optimal_table(f.ctypes.data, bits, values, C.byref(n)), b"jpgpu_libjpeg_optimal_table: bad argument")
    return list(bits), list(values)[:n.value]


def _blocks_of(w, h, luma, components):
    return (-(-w // (8 * luma[0]))) * (-(-h // (8 * luma[1]))) * (luma[0] * luma[1] + (2 if components == 3 else 0))


def _tensor_pixels(tensors, layout, device, shape_ok):
    """The checks of upload_tensors / upload_described_tensors, before any library call: [(data_ptr, width, height, channels)] and the
    C ABI's pixel layout.  shape_ok(i, width, height, channels) says whether image i may have that size and that many samples per pixel."""
    import torch  # (here: the package imports without torch)

    layout = "chw" if layout is None else layout
    if layout not in ("chw", "hwc"):
        raise ValueError("layout is 'chw' (planes, the default) or 'hwc' (interleaved pixels), not %r" % (layout,))
    out = []
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor):
            raise ValueError("image %d: a torch tensor is expected, not %s (numpy arrays go to upload())" % (i, type(t).__name__))
        if t.dtype != torch.uint8:
            raise ValueError("image %d: a uint8 tensor is expected, not %s" % (i, t.dtype))
        if layout == "chw":
            if t.dim() != 3:
                raise ValueError("image %d: layout 'chw' takes (C, H, W) tensors, not %s" % (i, tuple(t.shape)))
            c, h, w = t.shape
        else:
            if t.dim() not in (2, 3):
                raise ValueError("image %d: layout 'hwc' takes (H, W, C) or (H, W) tensors, not %s" % (i, tuple(t.shape)))
            h, w = t.shape[:2]
            c = t.shape[2] if t.dim() == 3 else 1
        if not shape_ok(i, w, h, c):
            raise ValueError("image %d: %d x %d pixels, %d samples per pixel in a %s tensor of layout '%s'" % (i, w, h, c, tuple(t.shape), layout))
        if h < 1 or w < 1:
            raise ValueError("image %d: an empty tensor %s" % (i, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("image %d: the tensor is not contiguous (strides %s): call .contiguous() -- nothing is copied here" % (i, tuple(t.stride())))
        if not t.is_cuda or t.device.index != device:
            raise ValueError("image %d: the tensor is on %s, not on the context's device cuda:%d" % (i, t.device, device))
        out.append((t.data_ptr(), int(w), int(h), int(c)))
    return out, (_capi.PIXELS_PLANAR if layout == "chw" else _capi.PIXELS_INTERLEAVED)


class EncodeBatch:
    def __init__(self, ctx: Context = None):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        raise_for_status(_lib.jpgpu_encoder_create(self.ctx._h, C.byref(self._h)), b"jpgpu_encoder_create failed")
        self._n = 0
        self._blocks = []
        self._keep = None
        self._libjpeg = False

    def _check(self, rc):
        raise_for_status(rc, _lib.jpgpu_last_error(self.ctx._h))

    def set_arithmetic_policy(self, arithmetic):
        """Which arithmetic upload() and upload_tensors() plan with from here on: "reference", the default -- the reference's float transform,
        zero padding and header, every stream the bytes it always was -- or "libjpeg": jpeg_fdct_islow, libjpeg's colour constants, edge
        replication, dummy blocks and header (include/jpgpu.h, 4d), byte for byte the file Pillow's Image.save(f, "JPEG", quality=q,
        subsampling=s) writes for the same pixels.  Under "libjpeg" optimize_coding and luma factors other than (1, 1), (2, 1), (2, 2) raise
        ArgumentException, the described uploads InvalidOperationException; a grey image is planned (1, 1) whatever luma says.  State of the
        batch: it holds until set again.  ValueError, before the library is called, for any other value."""
        policy = _arithmetic_policy(arithmetic)
        self._check(_lib.jpgpu_encoder_set_arithmetic_policy(self._h, policy))
        self._libjpeg = policy == 1
        return self

    def set_coding_policy(self, coding):
        """Which entropy coding upload() and upload_tensors() plan with from here on, under arithmetic "libjpeg" only: "standard", the default
        -- the Annex K tables, every stream what it was --, "optimized" -- byte for byte Pillow's Image.save(..., optimize=True): sequential,
        Huffman tables built from the image by libjpeg's rule; takes restart_interval -- or "progressive" -- byte for byte Image.save(...,
        progressive=True): SOF2, libjpeg's simple progression, a table built per scan (include/jpgpu.h, 4e).  An upload under "reference" with
        another coding than "standard", and "progressive" with a restart interval, raise ArgumentException and leave the batch usable.  State
        of the batch: it holds until set again.  ValueError, before the library is called, for any other value."""
        self._check(_lib.jpgpu_encoder_set_coding_policy(self._h, _coding_policy(coding)))
        return self

    def coding(self, i):
        """"standard", "optimized" or "progressive": what image i of the last upload was planned with"""
        a = C.c_int()
        raise_for_status(_lib.jpgpu_encoder_image_coding(self._h, i, C.byref(a)), b"jpgpu_encoder_image_coding: no such image")
        return _capi.CODING_POLICIES[a.value]

    def arithmetic(self, i):
        """1 where image i of the last upload was planned with libjpeg's integer transform, else 0"""
        a = C.c_int()
        raise_for_status(_lib.jpgpu_encoder_image_arithmetic(self._h, i, C.byref(a)), b"jpgpu_encoder_image_arithmetic: no such image")
        return a.value

    def _planned_luma(self, luma, components):
        # (libjpeg: one component is a non-interleaved scan of single blocks, see jpgpu.h 4d)
        return (1, 1) if self._libjpeg and components == 1 else (luma[0], luma[1])

    def upload(self, images, luma=(2, 2), quality=75, rgb=False, optimize_coding=False, restart_interval=0, arithmetic=None, coding=None):
        """images: list of uint8 arrays (H, W, 3) or (H, W) / (H, W, 1); with rgb=True also (H, W, 4) = Rgba32 pixels, the alpha byte
        stepped over like ConvertRgba32ToYCbCr8 does (the reference's EncoderBenchmark).  luma = sampling factors of the first component.
        optimize_coding = EncodeAction's switch: Huffman tables built from each image's own statistics.
        restart_interval = MCUs between restart markers (0 = none, as the reference's encoder; an extension, see jpgpu.h).
        arithmetic = "reference" or "libjpeg": set_arithmetic_policy() first (None: the batch's policy as it stands).
        coding = "standard", "optimized" or "progressive": set_coding_policy() first (None: as it stands)."""
        if arithmetic is not None:
            self.set_arithmetic_policy(arithmetic)
        if coding is not None:
            self.set_coding_policy(coding)
        n = len(images)
        ptrs = (C.c_void_p * n)()
        params = (_capi.EncodeParams * n)()
        keep = []
        self._blocks = []
        for i, im in enumerate(images):
            a = np.ascontiguousarray(im, dtype=np.uint8)
            if a.ndim == 2:
                a = a.reshape(a.shape[0], a.shape[1], 1)
            keep.append(a)
            ptrs[i] = a.ctypes.data
            h, w, c = a.shape
            mode = 1 if rgb else 0
            if c == 4:
                if not rgb:
                    raise ValueError("four bytes per pixel are Rgba32 pixels: rgb=True")
                c, mode = 3, 2
            params[i] = _capi.EncodeParams(w, h, c, luma[0], luma[1], quality, mode, int(optimize_coding), int(restart_interval))
            self._blocks.append(_blocks_of(w, h, self._planned_luma(luma, c), c))
        self._keep = None
        self._check(_lib.jpgpu_encoder_upload(self._h, ptrs, params, n))
        self._n = n
        return self

    def _device_upload(self, entry, tensors, pixels, pixel_layout, records):
        import torch

        n = len(pixels)
        ptrs = (C.c_void_p * n)(*[p[0] for p in pixels])
        layouts = (C.c_int32 * n)(*([pixel_layout] * n))
        # the library reads the tensors on its own stream: what torch has queued on its current one must have happened
        torch.cuda.current_stream(self.ctx.device).synchronize()
        self._n = 0
        self._keep = list(tensors)  # the encoder reads this memory in encode(): held until the next upload or close()
        self._check(entry(self._h, ptrs, records, layouts, n))
        self._n = n
        return self

    def upload_tensors(self, tensors, luma=(2, 2), quality=75, rgb=False, optimize_coding=False, restart_interval=0, layout=None, arithmetic=None,
                       coding=None):
        """upload() for pixels that are on the device already: torch uint8 tensors on the context's device, read where they are --
        no download, no permute, no copy (jpgpu_encoder_upload_device).  layout='chw' (the default: what decode_to_tensors returns) takes
        (3, H, W) or (1, H, W); layout='hwc' takes (H, W, 3), (H, W), (H, W, 1) and, with rgb=True, (H, W, 4) = Rgba32.  The other arguments
        are upload()'s.  ValueError, before the library is called, for a tensor that is not uint8, has another rank or channel count, is
        not contiguous (call .contiguous(): nothing is copied silently) or is not on the context's device.
        torch's current stream on that device is synchronised first, so whatever produced the tensors has finished; the batch keeps
        references to the tensors until the next upload or close(), and they must not be written before encode() has returned."""
        if arithmetic is not None:
            self.set_arithmetic_policy(arithmetic)
        if coding is not None:
            self.set_coding_policy(coding)
        tensors = list(tensors)
        hwc = (layout or "chw") == "hwc"
        pixels, pixel_layout = _tensor_pixels(tensors, layout, self.ctx.device, lambda i, w, h, c: c in (1, 3) or (c == 4 and hwc and rgb))
        params = (_capi.EncodeParams * len(pixels))()
        self._blocks = []
        for i, (_, w, h, c) in enumerate(pixels):
            mode = 1 if rgb else 0
            if c == 4:
                c, mode = 3, 2
            params[i] = _capi.EncodeParams(w, h, c, luma[0], luma[1], quality, mode, int(optimize_coding), int(restart_interval))
            self._blocks.append(_blocks_of(w, h, self._planned_luma(luma, c), c))
        return self._device_upload(_lib.jpgpu_encoder_upload_device, tensors, pixels, pixel_layout, params)

    def upload_described_tensors(self, tensors, descriptions, layout=None):
        """upload_described() for torch uint8 tensors on the context's device (jpgpu_encoder_upload_described_device): layout='chw'
        (the default) takes (in_components, H, W), e.g. CMYK as (4, H, W); layout='hwc' takes (H, W, in_components), or (H, W) for one.
        Checks, synchronisation and lifetime as in upload_tensors."""
        tensors = list(tensors)
        if len(descriptions) != len(tensors):
            raise ValueError("one description per image")
        descs = (_capi.EncodeDescription * len(tensors))(*descriptions)
        chw = (layout or "chw") == "chw"

        def as_described(i, w, h, c):
            d = descs[i]
            return (w, h, c) == (d.width, d.height, d.in_components) and not (chw and d.input_rgb == 2)

        pixels, pixel_layout = _tensor_pixels(tensors, layout, self.ctx.device, as_described)
        self._blocks = []
        for i in range(len(pixels)):
            d = descs[i]
            comps = [d.components[k] for k in range(d.num_components)]
            mh, mv = max([c.h for c in comps] or [1]), max([c.v for c in comps] or [1])
            self._blocks.append((-(-d.width // (8 * mh))) * (-(-d.height // (8 * mv))) * sum(c.h * c.v for c in comps))
        return self._device_upload(_lib.jpgpu_encoder_upload_described_device, tensors, pixels, pixel_layout, descs)

    def upload_described(self, images, descriptions):
        """images: uint8 arrays (H, W, in_components) or (H, W); descriptions: describe(...) per image.  An arrangement the device
        path refuses is that image's status (image_status / output raise it); the other images of the upload are unaffected."""
        n = len(images)
        if len(descriptions) != n:
            raise ValueError("one description per image")
        ptrs = (C.c_void_p * n)()
        descs = (_capi.EncodeDescription * n)(*descriptions)
        keep = []
        self._blocks = []
        for i, im in enumerate(images):
            a = np.ascontiguousarray(im, dtype=np.uint8)
            d = descs[i]
            if a.size != d.width * d.height * d.in_components:
                raise ValueError("image %d: %d samples for %d x %d x %d" % (i, a.size, d.height, d.width, d.in_components))
            keep.append(a)
            ptrs[i] = a.ctypes.data
            comps = [d.components[k] for k in range(d.num_components)]
            mh, mv = max([c.h for c in comps] or [1]), max([c.v for c in comps] or [1])
            self._blocks.append((-(-d.width // (8 * mh))) * (-(-d.height // (8 * mv))) * sum(c.h * c.v for c in comps))
        self._keep = None
        self._check(_lib.jpgpu_encoder_upload_described(self._h, ptrs, descs, n))
        self._n = n
        return self

    def image_status(self, i):
        """JPGPU_OK or the status Encode() of image i reports, as known so far."""
        return _lib.jpgpu_encoder_image_status(self._h, i)

    def set_quantization_table(self, i, identifier, zigzag64):
        """SetQuantizationTable for image i: the caller's own table (zig-zag order, 1..255) instead of the scaled standard one."""
        q = np.ascontiguousarray(zigzag64, dtype=np.uint16).reshape(64)
        self._check(_lib.jpgpu_encoder_set_quantization_table(self._h, i, identifier, q.ctypes.data))
        return self

    def encode(self):
        self._check(_lib.jpgpu_encoder_encode(self._h))
        return self

    def __len__(self):
        return self._n

    def emit_passes(self):
        """(calls of encode() whose entropy stage ran as ONE pass over the blocks, those of them that fell back to the two kernels)."""
        a, b = C.c_int(0), C.c_int(0)
        self._check(_lib.jpgpu_encoder_emit_passes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def stage_ms(self):
        """Device time of the last encode() by stage (HIP events)."""
        ms = (C.c_float * 5)()
        self._check(_lib.jpgpu_encoder_stage_ms(self._h, ms))
        return {"fdct_quant": ms[0], "block_bits": ms[1], "emit": ms[2], "stuff": ms[3], "total": ms[4]}

    def output(self, i) -> bytes:
        size = C.c_size_t()
        self._check(_lib.jpgpu_encoder_encoded_size(self._h, i, C.byref(size)))
        out = np.empty(size.value, np.uint8)
        self._check(_lib.jpgpu_encoder_download(self._h, i, out.ctypes.data, out.size))
        return out.tobytes()

    def output_tensor(self, i):
        """Stream i of the last encode() as a 1-D torch uint8 tensor on the context's device that ALIASES the encoder's output buffer
        (jpgpu_encoder_output_device) -- no download.  An image whose encode failed raises as output() does.  encode() has synchronised
        the context's stream, so the tensor may be used on any torch stream.  The tensor keeps the batch alive.  One rule remains: the
        next upload or encode() on this batch, or an explicit close(), invalidates every tensor made from it."""
        import torch  # (here: the package imports without torch)

        size = C.c_size_t()
        self._check(_lib.jpgpu_encoder_encoded_size(self._h, i, C.byref(size)))
        ptr = _lib.jpgpu_encoder_output_device(self._h, i, C.byref(size))
        if not ptr:
            raise ValueError("output_tensor: no encode() has produced stream %d" % i)
        return torch.as_tensor(_DeviceView(self, ptr, (size.value,)), device=torch.device("cuda", self.ctx.device))

    def coefficients(self, i):
        out = np.empty((self._blocks[i], 64), np.int16)
        self._check(_lib.jpgpu_encoder_download_coefficients(self._h, i, out.ctypes.data, out.shape[0]))
        return out

    def close(self):
        if self._h:
            _lib.jpgpu_encoder_destroy(self._h)
            self._h = C.c_void_p()
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def encode_batch(images, luma=(2, 2), quality=75, rgb=False, ctx=None, optimize_coding=False, restart_interval=0, arithmetic="reference",
                 coding="standard"):
    """One-call helper: list of JPEG byte strings.  arithmetic="libjpeg": the files Pillow writes (EncodeBatch.set_arithmetic_policy);
    with coding="optimized" / "progressive" those of optimize=True / progressive=True (EncodeBatch.set_coding_policy)."""
    _arithmetic_policy(arithmetic)  # (ValueError before a context is made)
    _coding_policy(coding)
    b = EncodeBatch(ctx).upload(images, luma, quality, rgb, optimize_coding, restart_interval, arithmetic, coding).encode()
    outs = [b.output(i) for i in range(len(b))]
    b.close()
    return outs


def encode_tensors(tensors, luma=(2, 2), quality=75, rgb=True, ctx=None, optimize_coding=False, restart_interval=0, layout=None, arithmetic="reference",
                   coding="standard"):
    """One-call helper for torch producers: uint8 tensors on the context's device (layout 'chw' by default: decode_to_tensors' output,
    R,G,B planes) -> list of JPEG byte strings.  The pixels are never downloaded; see EncodeBatch.upload_tensors.  arithmetic="libjpeg": the
    files Pillow writes (EncodeBatch.set_arithmetic_policy), coding as in encode_batch."""
    _arithmetic_policy(arithmetic)  # (ValueError before a context is made)
    _coding_policy(coding)
    b = EncodeBatch(ctx).upload_tensors(tensors, luma, quality, rgb, optimize_coding, restart_interval, layout, arithmetic, coding).encode()
    outs = [b.output(i) for i in range(len(b))]
    b.close()
    return outs
