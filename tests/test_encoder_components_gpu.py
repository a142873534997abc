"""Every component arrangement JpegEncoder.AddComponent accepts, on the GPU: stream and coefficients byte for byte against the serial
model (encoder_model.py), through the C-level described upload and through the JpegEncoder mirror."""
import numpy as np
import pytest

import encoder_arrangements as ea
import encoder_model as em
import jpeglibrary_amd as jl

pytestmark = pytest.mark.gpu


def _gpu(images, arrs, in_components=None):
    """One described upload: [(stream, coefficients) | raised exception] per image."""
    descs = [ea.to_description(a, im.shape[1], im.shape[0], in_components) for im, a in zip(images, arrs)]
    batch = jl.EncodeBatch().upload_described(images, descs)
    try:
        statuses = [batch.image_status(i) for i in range(len(images))]
        batch.encode()
        out = []
        for i in range(len(images)):
            try:
                out.append((batch.output(i), batch.coefficients(i)))
            except jl.JpegError as e:
                assert statuses[i] != 0, "a refusal is known at upload"
                out.append(e)
        return out
    finally:
        batch.close()


def _mirror(px, arr):
    """The arrangement as the reference's caller would set it up, call by call."""
    enc = jl.JpegEncoder()
    captured = {c.quant_id: c.quant for c in arr.components}
    for identifier, elements in arr.quant_tables:
        enc.SetQuantizationTable(jl.JpegQuantizationTable(0, identifier, captured.get(identifier, elements)))
    for table_class, identifier, codes in arr.huffman_tables:
        table = None if codes is None else jl.JpegHuffmanEncodingTable([jl.JpegHuffmanCanonicalCode(*c) for c in codes])
        enc.SetHuffmanTable(table_class == 0, identifier, table)
    for c in arr.components:
        enc.AddComponent(c.component_index, c.quant_id, c.dc_id, c.ac_id, c.h, c.v)
    for identifier, elements in arr.quant_tables:  # a table replaced after AddComponent captured it
        if identifier in captured and list(captured[identifier]) != list(elements):
            enc.SetQuantizationTable(jl.JpegQuantizationTable(0, identifier, elements))
    enc.MostOptimalCoding = arr.most_optimal
    enc.restart_interval = arr.restart_interval
    enc.SetInputReader(jl.JpegBufferInputReader(px.shape[1], px.shape[0], px.shape[2], px))
    out = bytearray()
    enc.SetOutput(out)
    enc.Encode()
    return bytes(out)


def _check(px, arr, what, mirror=True, in_components=None):
    ref, ref_coefs, in_grid = em.encode(px, arr)
    (got, coefs), = _gpu([px], [arr], in_components)
    assert coefs.shape == ref_coefs.shape, what
    bad = np.flatnonzero((coefs != ref_coefs).any(axis=1) & in_grid)
    assert bad.size == 0, f"{what}: {bad.size} blocks differ, first {bad[:8]}"
    assert got == ref, f"{what}: streams differ ({len(got)} / {len(ref)} bytes)"
    if mirror:
        assert _mirror(px, arr) == ref, f"{what}: the JpegEncoder mirror"
    return got, coefs


CASES = [(name, size) for name in "ACDEJ" for size in ea.SIZES[name]]


@pytest.mark.parametrize("built", [False, True], ids=["given", "built"])
@pytest.mark.parametrize("name,size", CASES, ids=[f"{n}-{s[0]}x{s[1]}" for n, s in CASES])
def test_arrangement_equals_the_model(name, size, built):
    px = ea.pixels(size[0], size[1], len(ea.SAMPLING[name]), 11)
    _check(px, ea.arrangement(name, built), (name, size, built))


@pytest.mark.parametrize("built", [False, True], ids=["given", "built"])
def test_encode_action_arrangement_through_the_described_upload_is_the_old_entry(built):
    """B: the anchor.  Described, it takes the kernels jpgpu_encoder_upload takes and writes the same bytes."""
    px = ea.pixels(90, 41, 3, 12)
    old = jl.encode_batch([px], (2, 2), 75, optimize_coding=built)[0]
    got, _ = _check(px, ea.arrangement("B", built), ("B", built))
    assert got == old


def test_the_two_paths_read_a_middle_factor_at_different_pixels():
    """D: h = 2 under maxH = 4 -- WriteScanData reads the middle component's two blocks 8 pixels apart (overlapping 16-pixel
    windows) and on top of the block before, TransformBlocks 16 apart from zeros: the paths differ there and agree on the
    full-resolution blocks; each equals the model (test above)."""
    px = ea.pixels(100, 50, 3, 11)
    (_, given), (_, built) = _gpu([px, px], [ea.arrangement("D"), ea.arrangement("D", True)])
    assert np.array_equal(given[:8], built[:8])  # MCU 0 lies inside the image: its eight 4 x 2 blocks
    assert not np.array_equal(given[8], built[8]) and not np.array_equal(given[9], built[9])


@pytest.mark.parametrize("built", [False, True], ids=["given", "built"])
def test_arrangement_without_a_full_resolution_component_is_refused(built):
    """F: 2 x 1 beside 1 x 2.  NotSupportedException for that image at upload, the rest of the upload as if it were alone."""
    f = ea.pixels(40, 24, 2, 13)
    a = ea.pixels(37, 29, 4, 11)
    descs = [ea.to_description(ea.arrangement("A", built), 37, 29), ea.to_description(ea.arrangement("F", built), 40, 24),
             ea.to_description(ea.arrangement("A", built), 37, 29)]
    batch = jl.EncodeBatch().upload_described([a, f, a], descs)
    assert [batch.image_status(i) for i in range(3)] == [0, 3, 0]
    batch.encode()
    ref = em.encode(a, ea.arrangement("A", built))[0]
    assert batch.output(0) == ref and batch.output(2) == ref
    with pytest.raises(jl.NotSupportedException, match="maximum sampling factors"):
        batch.output(1)
    batch.close()
    with pytest.raises(jl.NotSupportedException, match="maximum sampling factors"):
        _mirror(f, ea.arrangement("F", built))


@pytest.mark.parametrize("name", ["B", "C"])
def test_huffman_tables_table_by_table(name):
    """G: shared tables add their counts up; DC given with AC built; a builder nobody feeds; a given table that lacks symbols."""
    px = ea.pixels(90, 41, 3, 14)
    _check(px, ea.shared_tables(name), (name, "shared"))
    _check(px, ea.dc_given_ac_built(name), (name, "dc given, ac built"))
    # a builder no component uses: Build throws, for that image alone
    res = _gpu([px, px], [ea.unused_builder(name), ea.arrangement(name)])
    assert isinstance(res[0], jl.InvalidOperationException) and "No symbol is recorded." in str(res[0])
    assert res[1][0] == em.encode(px, ea.arrangement(name))[0]
    with pytest.raises(jl.InvalidOperationException, match="No symbol is recorded."):
        _mirror(px, ea.unused_builder(name))
    # an AC table built (with the builder mirror) from a flat image, used on a noisy one: GetCode answers the symbols it lacks
    # with entry 0's code.  The model's bytes are the truth; nobody is asked to decode them.
    builder = jl.JpegHuffmanEncodingTableBuilder()
    for symbol in (0x00, 0x00, 0x00, 0x01, 0x01, 0x11):
        builder.IncrementCodeCount(symbol)
    table = builder.Build()
    codes = [(c.Symbol, c.Code, c.CodeLength) for c in table._codes]
    assert len(codes) == 3
    arr = ea.arrangement(name)
    arr.huffman_tables[1] = (1, 0, codes)
    _check(px, arr, (name, "a given table that lacks symbols"))


@pytest.mark.parametrize("name", ["B", "C"])
@pytest.mark.parametrize("built", [False, True], ids=["given", "built"])
def test_identifiers_are_the_callers(name, built):
    """H: component identifiers 7, 9, 200; quantisation identifiers 2, 3 and an unused table in the DQT; Huffman identifiers 3 and 1,
    AC set before DC; a quantisation table replaced after AddComponent (the DQT has the new one, the coefficients the old one's)."""
    px = ea.pixels(90, 41, 3, 15)
    arr = ea.identifiers(name, built)
    got, coefs = _check(px, arr, (name, "identifiers", built))
    at = got.index(b"\xff\xdb")
    assert got[at + 4] == 2 and list(got[at + 5:at + 69]) == list(ea.LUM40) and got[at + 2:at + 4] == bytes((0, 2 + 3 * 65))
    # quantised with the captured table (quality 75), not with the DQT's (quality 40)
    first = px[:8, :8, 0].astype(np.int16).reshape(64)
    if not built:
        assert np.array_equal(coefs[0], em.pyoracle.fdct_quantize_block(first, ea.LUM75)[0])
        assert not np.array_equal(coefs[0], em.pyoracle.fdct_quantize_block(first, ea.LUM40)[0])


@pytest.mark.parametrize("name,size", [("E", (264, 136)), ("C", (90, 41))])
@pytest.mark.parametrize("interval", [1, 3])
def test_restart_intervals_on_general_arrangements(name, size, interval):
    """K: the restart extension cuts the DC prediction, not the block buffer."""
    px = ea.pixels(size[0], size[1], 3, 16)
    for built in (False, True):
        _check(px, ea.arrangement(name, built, restart_interval=interval), (name, interval, built), mirror=not built)


def test_one_upload_mixes_both_kinds_of_image():
    """L: B, A, E, D, J and a plain 4:2:0 image in one upload, each stream what the image gives alone."""
    names = ["B", "A", "E", "D", "J", "B"]
    sizes = [(90, 41), (37, 29), (264, 136), (100, 50), (70, 40), (150, 98)]
    for built in (False, True):
        images = [ea.pixels(w, h, len(ea.SAMPLING[n]), 17 + k) for k, (n, (w, h)) in enumerate(zip(names, sizes))]
        arrs = [ea.arrangement(n, built) for n in names]
        res = _gpu(images, arrs)
        for k, (px, arr) in enumerate(zip(images, arrs)):
            assert res[k][0] == em.encode(px, arr)[0], (names[k], built)
        assert res[5][0] == jl.encode_batch([images[5]], (2, 2), 75, optimize_coding=built)[0]


@pytest.mark.parametrize("name,size", [("E", (264, 136)), ("D", (200, 100))])
def test_work_list_boundaries(name, size):
    """9 and 11 blocks per MCU, more than 256 blocks and no multiple of 256: lanes of one workgroup in different MCU positions."""
    px = ea.pixels(size[0], size[1], 3, 18)
    blocks = em.encode(px, ea.arrangement(name))[1].shape[0]
    assert blocks > 256 and blocks % 256 != 0 and blocks % {"E": 9, "D": 11}[name] == 0
    for built in (False, True):
        _check(px, ea.arrangement(name, built), (name, size, built), mirror=False)


def test_components_read_the_sample_at_their_position():
    """Four samples per pixel, two components added: samples 0 and 1 are read, whatever the identifiers say."""
    px = ea.pixels(61, 35, 4, 19)
    std = em.standard_tables()
    for built in (False, True):
        t = [None] * 4 if built else std
        arr = em.Arrangement([em.Component(9, 0, 0, 0, 2, 1, ea.LUM75), em.Component(4, 1, 1, 1, 1, 1, ea.CHR75)], [(0, ea.LUM75), (1, ea.CHR75)],
                             [(0, 0, t[0]), (1, 0, t[1]), (0, 1, t[2]), (1, 1, t[3])])
        _check(px, arr, ("in_components 4", built), in_components=4)
    with pytest.raises(jl.NotSupportedException, match="fewer samples per pixel"):
        _mirror(px[:, :, :1].copy(), arr)


def test_the_quantization_setter_belongs_to_the_parameter_upload():
    """jpgpu_encoder_set_quantization_table patches the two tables of a jpgpu_encoder_upload image; a described image carries its
    tables, so behind a described upload the call is refused for every image -- EncodeAction arrangement, general one, refused one --
    and changes nothing."""
    b, a, f = ea.pixels(90, 41, 3, 20), ea.pixels(37, 29, 4, 20), ea.pixels(40, 24, 2, 20)
    arrs = [ea.arrangement("B"), ea.arrangement("A"), ea.arrangement("F")]
    descs = [ea.to_description(arr, im.shape[1], im.shape[0]) for im, arr in zip((b, a, f), arrs)]
    batch = jl.EncodeBatch().upload_described([b, a, f], descs)
    for i in range(3):
        for identifier in (0, 1):
            with pytest.raises(jl.InvalidOperationException, match="a described image carries its tables"):
                batch.set_quantization_table(i, identifier, np.full(64, 3))
    batch.encode()
    assert batch.output(0) == em.encode(b, arrs[0])[0] and batch.output(1) == em.encode(a, arrs[1])[0]
    # the same handle takes the parameter upload again, setter included
    batch.upload([b], (2, 2), 75)
    batch.set_quantization_table(0, 0, np.full(64, 3))
    batch.encode()
    from oracle import pyoracle

    assert batch.output(0) == pyoracle.encode_8bit(b, 2, 2, 75, quant_tables=(np.full(64, 3), ea.CHR75))
    batch.close()
