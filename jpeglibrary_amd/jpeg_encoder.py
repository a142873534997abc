"""Mirror of the reference's public encoder surface (src/JpegLibrary/JpegEncoder.cs, JpegQuantizationTable.cs,
JpegStandardQuantizationTable.cs, JpegStandardHuffmanEncodingTable.cs; apps/JpegEncode/JpegBufferInputReader.cs) over the
GPU encoder, so that a test can be written like the reference's own callers (apps/JpegEncode/EncodeAction.cs:38-63):

    encoder = JpegEncoder()
    encoder.SetQuantizationTable(JpegStandardQuantizationTable.ScaleByQuality(JpegStandardQuantizationTable.GetLuminanceTable(0, 0), quality))
    encoder.SetQuantizationTable(JpegStandardQuantizationTable.ScaleByQuality(JpegStandardQuantizationTable.GetChrominanceTable(0, 1), quality))
    encoder.SetHuffmanTable(True, 0, JpegStandardHuffmanEncodingTable.GetLuminanceDCTable())   # or SetHuffmanTable(True, 0): built from the image
    ...
    encoder.AddComponent(1, 0, 0, 0, 2, 2); encoder.AddComponent(2, 1, 1, 1, 1, 1); encoder.AddComponent(3, 1, 1, 1, 1, 1)
    encoder.SetInputReader(JpegBufferInputReader(width, height, 3, ycbcr)); encoder.SetOutput(writer); encoder.Encode()

Same names, argument meaning and exceptions.  The device path takes every arrangement AddComponent accepts: one to four
components with sampling factors 1, 2 or 4 each, any component identifiers, quantisation tables of the caller's choice under any
identifier (the stream's DQT holds the tables as they are at Encode(), a component quantises with the one it captured), Huffman
tables given (the standard ones, JpegHuffmanEncodingTable(codes), a JpegHuffmanEncodingTableBuilder's result) or left to be
built from the image, table by table.  Encode() hands the state to the device as one described image (jpgpu_encode_description);
an EncodeAction arrangement takes the fused kernels it always took.  NotSupportedException remains for two things: more components
than the input holds samples per pixel, and an arrangement without a component at the maximum sampling factors in both directions
(DESIGN.md section 5).  A second Encode() on one object is not mirrored.  Nothing touches the device before Encode().
"""
import numpy as np

from .errors import ArgumentException, InvalidOperationException, NotSupportedException

# ref: JpegStandardQuantizationTable.cs:12-34 (zig-zag order)
_STD_LUMINANCE = (16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
                  56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101,
                  103, 99)
_STD_CHROMINANCE = (17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66) + (99,) * 50


class JpegQuantizationTable:
    """ref: JpegQuantizationTable.cs:22-33 -- elements in zig-zag order; element precision 0 = 8 bit, 1 = 12 bit."""

    def __init__(self, elementPrecision=0, identifier=0, elements=None):
        if elements is None:
            self.ElementPrecision, self.Identifier, self.Elements = 0, 0, None  # default(JpegQuantizationTable)
            return
        if len(elements) != 64:
            raise ArgumentException("The length of elements must be 64.")
        self.ElementPrecision = int(elementPrecision)
        self.Identifier = int(identifier)
        self.Elements = tuple(int(e) for e in elements)

    @property
    def IsEmpty(self):
        return self.Elements is None


class JpegStandardQuantizationTable:
    @staticmethod
    def GetLuminanceTable(elementPrecision, identifier):  # :42-45
        return JpegQuantizationTable(elementPrecision, identifier, _STD_LUMINANCE)

    @staticmethod
    def GetChrominanceTable(elementPrecision, identifier):  # :53-56
        return JpegQuantizationTable(elementPrecision, identifier, _STD_CHROMINANCE)

    @staticmethod
    def ScaleByQuality(quantizationTable, quality):  # :64-87
        if quantizationTable.IsEmpty:
            raise ArgumentException("Quantization table is not initialized. (Parameter 'quantizationTable')")
        if quality < 0 or quality > 100:
            raise ArgumentException("Specified argument was out of the range of valid values. (Parameter 'quality')")
        scale = 5000 // quality if quality < 50 else 200 - quality * 2  # quality 0: DivideByZeroException there, ZeroDivisionError here
        return JpegQuantizationTable(quantizationTable.ElementPrecision, quantizationTable.Identifier,
                                     [min(max((x * scale + 50) // 100, 1), 255) for x in quantizationTable.Elements])


class JpegHuffmanCanonicalCode:
    """ref: JpegHuffmanCanonicalCode.cs -- one entry of an encoding table."""

    def __init__(self, symbol=0, code=0, codeLength=0):
        self.Symbol, self.Code, self.CodeLength = int(symbol) & 0xFF, int(code) & 0xFFFF, int(codeLength) & 0xFF


class JpegHuffmanEncodingTable:
    """ref: JpegHuffmanEncodingTable.cs:21-37 -- whatever array of codes the caller hands over.  TryWrite (:50-86) writes its last
    `code count` entries (those with a length), GetCode (:94-100) answers a symbol the table does not hold with entry 0."""

    def __init__(self, codes):
        if codes is None:
            raise ArgumentException("Value cannot be null. (Parameter 'codes')")
        self._codes = list(codes)

    @property
    def BytesRequired(self):  # :42
        return (16 + sum(1 for c in self._codes if c.CodeLength != 0)) & 0xFFFF

    def GetCode(self, symbol):  # :94-100 -> (code, codeLength)
        index = 0
        for i, c in enumerate(self._codes):
            if c.CodeLength != 0 and c.Symbol == symbol:
                index = i & 0xFF
        c = self._codes[index]
        return c.Code, c.CodeLength


class JpegHuffmanEncodingTableBuilder:
    """ref: JpegHuffmanEncodingTableBuilder.cs:14-65 -- counts symbols, Build() gives the table the encoder would have built."""

    def __init__(self):
        self._frequencies = [0] * 256

    def IncrementCodeCount(self, symbol):  # :30-34
        self._frequencies[symbol] += 1

    def Reset(self):  # :39-42
        self._frequencies = [0] * 256

    def Build(self, optimal=False):  # :62-65; InvalidOperationException("No symbol is recorded.") without symbols
        from .optimizer import build_optimal_huffman_table

        _, values, code, length = build_optimal_huffman_table(self._frequencies, optimal)
        return JpegHuffmanEncodingTable([JpegHuffmanCanonicalCode(v, code[v], length[v]) for v in values.tolist()])


# ref: JpegStandardHuffmanEncodingTable.cs:14-83 (ITU-T T.81 Annex K.3): code counts by length, symbols
_STD_DC_LUMINANCE = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
_STD_DC_CHROMINANCE = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
_STD_AC_LUMINANCE = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
_STD_AC_CHROMINANCE = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))


def _build_canonical_code(bits, values):
    """ref: JpegStandardHuffmanEncodingTable.BuildCanonicalCode (:85-131)."""
    lengths = [n + 1 for n, count in enumerate(bits) for _ in range(count)]
    codes, code, current = [], 0, lengths[0]
    for i, (symbol, length) in enumerate(zip(values, lengths)):
        if i > 0:
            code += 1
            if length > current:
                code <<= length - current
                current = length
        codes.append(JpegHuffmanCanonicalCode(symbol, code, length))
    return JpegHuffmanEncodingTable(codes)


class JpegStandardHuffmanEncodingTable:  # ref: JpegStandardHuffmanEncodingTable.cs:142-195
    _tables = [_build_canonical_code(*t) for t in (_STD_DC_LUMINANCE, _STD_AC_LUMINANCE, _STD_DC_CHROMINANCE, _STD_AC_CHROMINANCE)]

    @classmethod
    def GetLuminanceDCTable(cls):
        return cls._tables[0]

    @classmethod
    def GetLuminanceACTable(cls):
        return cls._tables[1]

    @classmethod
    def GetChrominanceDCTable(cls):
        return cls._tables[2]

    @classmethod
    def GetChrominanceACTable(cls):
        return cls._tables[3]


class JpegBufferInputReader:
    """ref: apps/JpegEncode/JpegBufferInputReader.cs:14-20 -- interleaved 8-bit samples, componentCount per pixel."""

    def __init__(self, width, height, componentCount, buffer):
        self.Width, self.Height, self.ComponentCount = int(width), int(height), int(componentCount)
        self.buffer = np.frombuffer(buffer, dtype=np.uint8) if not isinstance(buffer, np.ndarray) else np.ascontiguousarray(buffer, dtype=np.uint8).reshape(-1)
        if self.buffer.size < self.Width * self.Height * self.ComponentCount:
            raise ArgumentException("The buffer is too small for the image.")


class JpegEncoder:
    def __init__(self, ctx=None):
        self._ctx = ctx
        self.MostOptimalCoding = False  # :43
        self._input = None
        self._output = None
        self._quant = []        # SetQuantizationTable order (:102-126)
        self._huffman = {}      # (class, identifier & 0xff) -> table or None (= to be built), in SetHuffmanTable order
        self._components = []   # AddComponent order
        self.restart_interval = 0  # extension (see jpgpu_encode_params): 0 = what the reference writes

    # ---- setters, with the reference's checks and messages
    def SetInputReader(self, inputReader):  # :84-87
        if inputReader is None:
            raise ArgumentException("Value cannot be null. (Parameter 'inputReader')")
        self._input = inputReader

    def SetOutput(self, output):  # :93-96
        if output is None:
            raise ArgumentException("Value cannot be null. (Parameter 'output')")
        self._output = output

    def SetQuantizationTable(self, table):  # :102-126
        if table.IsEmpty:
            raise ArgumentException("Quantization table is not initialized. (Parameter 'table')")
        if table.ElementPrecision != 0:
            raise InvalidOperationException("Only baseline JPEG is supported.")
        for k, t in enumerate(self._quant):
            if t.Identifier == table.Identifier:
                self._quant[k] = table
                return
        self._quant.append(table)

    def SetHuffmanTable(self, isDcTable, identifier, table=None):  # :137-148; no table = built from the image's statistics
        key = (0 if isDcTable else 1, int(identifier) & 0xFF)
        if key in self._huffman:  # AddTable (JpegHuffmanEncodingTableCollection.cs:82-88)
            raise InvalidOperationException("Operation is not valid due to the current state of the object.")
        self._huffman[key] = table

    def AddComponent(self, componentIndex, quantizationTableIdentifier, huffmanDcTableIdentifier, huffmanAcTableIdentifier, horizontalSubsampling,
                     verticalSubsampling):  # :175-239
        if horizontalSubsampling not in (1, 2, 4):
            raise ArgumentException("Subsampling factor can only be 1, 2 or 4. (Parameter 'horizontalSubsampling')")
        if verticalSubsampling not in (1, 2, 4):
            raise ArgumentException("Subsampling factor can only be 1, 2 or 4. (Parameter 'verticalSubsampling')")
        if any(c[0] == componentIndex for c in self._components):
            raise ArgumentException("The component index is already used by another component. (Parameter 'componentIndex')")
        if not any(t.Identifier == quantizationTableIdentifier for t in self._quant):
            raise ArgumentException("Quantization table is not defined. (Parameter 'quantizationTableIdentifier')")
        if (0, huffmanDcTableIdentifier) not in self._huffman:
            raise ArgumentException("Huffman table is not defined. (Parameter 'huffmanDcTableIdentifier')")
        if (1, huffmanAcTableIdentifier) not in self._huffman:
            raise ArgumentException("Huffman table is not defined. (Parameter 'huffmanAcTableIdentifier')")
        # the component captures the quantisation table as it is NOW (:226: a later SetQuantizationTable does not reach it)
        quant = next(t for t in self._quant if t.Identifier == quantizationTableIdentifier)
        self._components.append((int(componentIndex), quant, int(huffmanDcTableIdentifier), int(huffmanAcTableIdentifier), int(horizontalSubsampling),
                                 int(verticalSubsampling)))

    # ---- Encode (:255-291)
    def Encode(self):
        from .encoder import EncodeBatch  # the device is only needed from here on

        if self._output is None:
            raise InvalidOperationException("Output is not specified.")
        if self._input is None:
            raise InvalidOperationException("Input is not specified.")
        if not self._components:
            raise InvalidOperationException("No component is specified.")
        comps = self._components
        reader = self._input
        if reader.ComponentCount < len(comps):  # (the reference's reader would run past its pixels)
            raise NotSupportedException("The input holds fewer samples per pixel than components were added.")
        if len(comps) > 4 or len(self._quant) > 8 or len(self._huffman) > 8:
            raise NotSupportedException("Up to four components and eight tables of a kind are supported.")
        from .encoder import describe

        desc = describe(reader.Width, reader.Height,
                        [(c[0], c[4], c[5], c[1].Identifier, c[2], c[3], c[1].Elements) for c in comps],
                        [(t.Identifier, t.Elements) for t in self._quant],  # the tables as they are NOW (WriteQuantizationTables :305-330)
                        [(k[0], k[1], None if t is None else [(c.Symbol, c.Code, c.CodeLength) for c in t._codes]) for k, t in self._huffman.items()],
                        in_components=reader.ComponentCount, restart_interval=self.restart_interval, most_optimal_coding=self.MostOptimalCoding)
        pixels = reader.buffer[:reader.Width * reader.Height * reader.ComponentCount].reshape(reader.Height, reader.Width, reader.ComponentCount)
        batch = EncodeBatch(self._ctx)
        try:
            batch.upload_described([pixels], [desc])
            batch.encode()
            data = batch.output(0)  # (raises what Encode() of this image reports)
        finally:
            batch.close()
        out = self._output
        if hasattr(out, "extend"):
            out.extend(data)
        elif hasattr(out, "write"):
            out.write(data)
        else:
            raise ArgumentException("output: a bytearray-like (extend) or file-like (write) object")
