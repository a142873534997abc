"""Batch JpegOptimizer on the GPU (ref: src/JpegLibrary/JpegOptimizer.cs): for every file

    optimizer = JpegOptimizer(); optimizer.SetInput(bytes); optimizer.Scan(); optimizer.SetOutput(buffer); optimizer.Optimize(strip)

i.e. the Huffman tables are rebuilt from the file's own symbol statistics and the scan is re-written symbol by symbol
(no coefficients are reconstructed).  Single-scan baseline files; see include/jpgpu.h section (5).
"""
import collections
import ctypes as C

import numpy as np

from . import _capi
from .batch import _window_rects
from .context import Context, default_context
from .errors import raise_for_status

_lib = _capi.lib

ORIENT_STORED, ORIENT_FILE = 0, 1
EDGE_REFUSE, EDGE_TRIM = 0, 1
_POLICIES = {None: ORIENT_STORED, "stored": ORIENT_STORED, "file": ORIENT_FILE}
ORIGIN_REFUSE, ORIGIN_EXPAND = 0, 1
_EDGES = {"refuse": EDGE_REFUSE, "trim": EDGE_TRIM}
_ORIGINS = {"refuse": ORIGIN_REFUSE, "expand": ORIGIN_EXPAND}

# what an image is turned by (include/jpgpu.h, "Lossless transform"): factors = [(h, v)] of the output, frame order; window = (x, y, w, h) as
# applied, in pixels of the turned frame ((0, 0, width, height) without one: the field defaults so, and width x height is the OUTPUT's size)
class TransformPlan(collections.namedtuple("TransformPlan", "orientation width height trimmed factors window")):
    __slots__ = ()

    def __new__(cls, orientation, width, height, trimmed, factors, window=None):
        return super().__new__(cls, orientation, width, height, trimmed, factors, (0, 0, width, height) if window is None else tuple(window))


def _policy(orientation):
    if orientation not in _POLICIES:
        raise ValueError("orientation is None, 'stored' or 'file' (a value per file goes into orientations=): %r" % (orientation,))
    return _POLICIES[orientation]


def _edge(edge):
    if edge not in _EDGES:
        raise ValueError("edge is 'refuse' or 'trim': %r" % (edge,))
    return _EDGES[edge]


def _origin(origin):
    if origin not in _ORIGINS:
        raise ValueError("origin is 'refuse' or 'expand': %r" % (origin,))
    return _ORIGINS[origin]


def _plan_of(info, window=None):
    return TransformPlan(info.orientation, info.width, info.height, bool(info.trimmed), [(info.h[c], info.v[c]) for c in range(info.num_components)],
                         None if window is None else (window.x, window.y, window.width, window.height))


class OptimizeBatch:
    def __init__(self, ctx: Context = None):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        raise_for_status(_lib.jpgpu_optimizer_create(self.ctx._h, C.byref(self._h)), b"jpgpu_optimizer_create failed")
        self._n = 0
        self._keep = None

    def _check(self, rc):
        raise_for_status(rc, _lib.jpgpu_last_error(self.ctx._h))

    def set_most_optimal_coding(self, on=True):
        """JpegOptimizer.MostOptimalCoding"""
        self._check(_lib.jpgpu_optimizer_set_most_optimal_coding(self._h, 1 if on else 0))
        return self

    def set_orientation_policy(self, orientation):
        """None / "stored" (the default): images stay as stored; "file": every image is turned the way its Exif block says."""
        self._check(_lib.jpgpu_optimizer_set_orientation_policy(self._h, _policy(orientation)))
        return self

    def set_orientations(self, orientations):
        """One value per file of the NEXT upload: 1..8 as given, 0 = what the policy gives; None or [] withdraws a pending list."""
        values = [int(o) for o in (orientations or [])]
        if any(o < 0 or o > 8 for o in values):
            raise ValueError("an orientation is 1..8, or 0 for what the policy gives")
        arr = (C.c_uint8 * max(1, len(values)))(*values)
        self._check(_lib.jpgpu_optimizer_set_orientations(self._h, arr, len(values)))
        return self

    def set_edge_policy(self, edge):
        """ "refuse" (the default; jpegtran -perfect) or "trim" (jpegtran -trim) for a mirrored axis that is no whole number of MCUs"""
        self._check(_lib.jpgpu_optimizer_set_edge_policy(self._h, _edge(edge)))
        return self

    def set_windows(self, rects):
        """One (x, y, w, h) per file of the NEXT upload, in pixels of the turned frame ((0, 0, 0, 0) = none); None or [] withdraws a pending
        list.  The image is cut in the coefficient domain (include/jpgpu.h, "Window"): its output decodes to that slice of the whole picture,
        sample for sample.  ValueError, before the library is called, for a rect that is not four non-negative integers below 2^32."""
        rects = _window_rects(rects) or []
        arr = (_capi.Rect * max(1, len(rects)))(*[_capi.Rect(*r) for r in rects])
        self._check(_lib.jpgpu_optimizer_set_windows(self._h, arr, len(rects)))
        return self

    def set_origin_policy(self, origin):
        """ "refuse" (the default; jpegtran -perfect): a window whose x or y is no multiple of the MCU size refuses the image; "expand"
        (jpegtran's default): it is moved up and left to the MCU boundary and grows by as much"""
        self._check(_lib.jpgpu_optimizer_set_origin_policy(self._h, _origin(origin)))
        return self

    def transform(self, i) -> TransformPlan:
        """What image i of the last upload was planned with (width x height: the output's, the window's where there is one)."""
        info = _capi.TransformInfo()
        self._check(_lib.jpgpu_optimizer_image_transform(self._h, i, C.byref(info)))
        r = _capi.Rect()
        self._check(_lib.jpgpu_optimizer_image_window(self._h, i, C.byref(r)))
        return _plan_of(info, r)

    def window(self, i):
        """(x, y, w, h): the window image i was planned with, behind the origin policy; (0, 0, W, H) of the turned frame without one"""
        r = _capi.Rect()
        self._check(_lib.jpgpu_optimizer_image_window(self._h, i, C.byref(r)))
        return (r.x, r.y, r.width, r.height)

    def turn_sources(self) -> int:
        """How many files the coefficient road of the last upload entropy-decoded: entries that are the same file are decoded once."""
        n = C.c_int()
        self._check(_lib.jpgpu_optimizer_turn_sources(self._h, C.byref(n)))
        return n.value

    def turn_ms(self) -> float:
        """Device time of the turn kernel (KX) alone in the last run; 0 when nothing was turned."""
        return self.turn_stage_ms()[0]

    def turn_stage_ms(self):
        """(KX alone, the entropy decode in front of it, the dense copy of split scans) of the last run, in ms; zeros when nothing was turned."""
        ms = (C.c_float * 3)()
        _lib.jpgpu_optimizer_turn_ms(self._h, C.byref(ms))
        return tuple(ms)

    def upload(self, files, strip=True):
        n = len(files)
        ptrs = (C.c_void_p * n)()
        lens = (C.c_size_t * n)()
        keep, seen = [], {}  # (entries that are the same object share one buffer: the coefficient road decodes such a file once)
        for i, f in enumerate(files):
            buf = seen.get(id(f))
            if buf is None:
                buf = seen[id(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
            keep.append(buf)
            ptrs[i] = buf.ctypes.data if buf.size else None
            lens[i] = buf.size
        self._keep = keep
        self._check(_lib.jpgpu_optimizer_upload(self._h, ptrs, lens, n, 1 if strip else 0))
        self._n = n
        return self

    def run(self):
        self._check(_lib.jpgpu_optimizer_run(self._h))
        return self

    def __len__(self):
        return self._n

    def result(self, i):
        res = _capi.ImageResult()
        size = C.c_size_t()
        self._check(_lib.jpgpu_optimizer_result(self._h, i, C.byref(res), C.byref(size)))
        return res, size.value

    def output(self, i) -> bytes:
        """The bytes Optimize() wrote for file i; raises the reference's exception class when the file failed."""
        res, size = self.result(i)
        raise_for_status(res.status, _lib.jpgpu_last_error(self.ctx._h))
        out = np.empty(size, np.uint8)
        self._check(_lib.jpgpu_optimizer_download(self._h, i, out.ctypes.data, out.size))
        return out.tobytes()

    def statistics(self, i):
        """[(table_class, identifier, counts[256])] as Scan() collected them, in builder-creation order."""
        tables = []
        for t in range(8):
            cls = C.c_uint8()
            ident = C.c_uint8()
            counts = np.zeros(256, np.uint32)
            if _lib.jpgpu_optimizer_statistics(self._h, i, t, C.byref(cls), C.byref(ident), counts.ctypes.data) != 0:
                break
            tables.append((cls.value, ident.value, counts))
        return tables

    def last_ms(self) -> float:
        ms = C.c_float()
        _lib.jpgpu_optimizer_last_ms(self._h, C.byref(ms))
        return ms.value

    def close(self):
        if self._h:
            _lib.jpgpu_optimizer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JpegOptimizer:
    """The reference's class surface (src/JpegLibrary/JpegOptimizer.cs:16-70, 523-548) over a one-file batch:

        optimizer = JpegOptimizer(); optimizer.SetInput(bytes); optimizer.Scan(); optimizer.SetOutput(buffer); optimizer.Optimize(strip)

    `buffer` is anything with `write(bytes)` (an IBufferWriter<byte> stand-in, e.g. io.BytesIO) or a bytearray."""

    def __init__(self, ctx: Context = None):
        self._ctx = ctx
        self._input = None
        self._output = None
        self._scanned = False
        self.MostOptimalCoding = False

    def SetInput(self, data):
        self._input = bytes(data)
        self._scanned = False

    def Scan(self):
        if not self._input:
            from .errors import InvalidOperationException
            raise InvalidOperationException("Input buffer is not specified.")
        self._scanned = True  # the symbol pass runs with Optimize(): both need the device, and Scan() alone has no observable result

    def SetOutput(self, output):
        if output is None:
            raise TypeError("output")
        self._output = output

    def Optimize(self, strip=True):
        from .errors import InvalidOperationException
        if not self._scanned or self._output is None:
            raise InvalidOperationException("Operation is not valid due to the current state of the object.")
        data = optimize_batch([self._input], strip, self._ctx, self.MostOptimalCoding)[0]
        if isinstance(self._output, bytearray):
            self._output += data
        else:
            self._output.write(data)


def optimize_batch(files, strip=True, ctx=None, most_optimal=False, orientation=None, orientations=None, edge="refuse", windows=None, origin="refuse"):
    """One-call helper: the optimized bytes of every file (raises on the first failing file).  orientation="file" bakes every file's Exif
    orientation into its coefficients, orientations=[...] turns file i by orientations[i] (1..8; 0 = by the policy); edge="trim" drops the
    partial MCU column or row of a mirrored axis where the default refuses the image (include/jpgpu.h, "Lossless transform").
    windows=[(x, y, w, h), ...] cuts file i to that window of its turned frame without recompressing ((0, 0, 0, 0) = none); origin="expand"
    moves an x or y that is no multiple of the MCU size to the boundary below where the default refuses the image ("Window")."""
    policy, edge_policy, origin_policy = _policy(orientation), _edge(edge), _origin(origin)
    if orientations is not None and len(orientations) != len(files):
        raise ValueError("orientations holds one value per file")
    windows = _window_rects(windows, len(files))
    b = OptimizeBatch(ctx)
    try:
        b.set_most_optimal_coding(most_optimal)
        if policy != ORIENT_STORED:
            b.set_orientation_policy(orientation)
        if edge_policy != EDGE_REFUSE:
            b.set_edge_policy(edge)
        if origin_policy != ORIGIN_REFUSE:
            b.set_origin_policy(origin)
        if orientations is not None:
            b.set_orientations(orientations)
        if windows is not None:
            b.set_windows(windows)
        b.upload(files, strip).run()
        return [b.output(i) for i in range(len(b))]
    finally:
        b.close()


def plan_transform(file, orientation=None, orientations=None, edge="refuse", window=None, origin="refuse") -> TransformPlan:
    """Host only (no device): what optimize_batch([file], orientation=..., orientations=[...], edge=..., windows=[window], origin=...) would
    turn and cut the file by.  Raises NotSupportedException with the refusal's text where the image would be refused, ArgumentException for
    a window outside the turned frame or with one zero side."""
    if orientations is not None and len(orientations) != 1:
        raise ValueError("orientations holds one value per file")
    given = int(orientations[0]) if orientations is not None else 0
    if given < 0 or given > 8:
        raise ValueError("an orientation is 1..8, or 0 for what the policy gives")
    rect = _capi.Rect(*(_window_rects([window])[0] if window is not None else (0, 0, 0, 0)))
    buf = np.frombuffer(bytes(file), dtype=np.uint8)
    info, applied = _capi.TransformInfo(), _capi.Rect()
    msg = C.create_string_buffer(512)
    rc = _lib.jpgpu_transform_plan_window(buf.ctypes.data if buf.size else None, buf.size, given, _policy(orientation), _edge(edge), C.byref(rect),
                                          _origin(origin), C.byref(info), C.byref(applied), msg, 512)
    raise_for_status(rc, msg.value or b"jpgpu_transform_plan_window failed")
    return _plan_of(info, applied)


def build_optimal_huffman_table(counts, most_optimal=False):
    """JpegHuffmanEncodingTableBuilder.Build(most_optimal) (host code of the optimizer path): (bits[16], values[n], code[256], length[256])."""
    f = np.ascontiguousarray(counts, dtype=np.uint32).reshape(256)
    bits = np.zeros(16, np.uint8)
    values = np.zeros(256, np.uint8)
    code = np.zeros(256, np.uint16)
    length = np.zeros(256, np.uint8)
    n = C.c_int()
    rc = _lib.jpgpu_build_optimal_huffman_table(f.ctypes.data, 1 if most_optimal else 0, bits.ctypes.data, values.ctypes.data, C.byref(n),
                                                code.ctypes.data, length.ctypes.data)
    raise_for_status(rc, b"No symbol is recorded.")
    return bits, values[:n.value].copy(), code, length
