"""The marker index (K1, jpeglibrary_amd/csrc/k1_markers.hip) restated byte by byte, and the writer of the files its tests run on.

model() follows the reference's bit reader (JpegBitReader.FillBuffer, src/JpegLibrary/JpegBitReader.cs:95-138) and the hand-off
rules K1's head comment and DevScanStatus (common.h) state; it knows nothing of lanes, chunks or groups.

The case writer makes baseline gray files (SOF0, the standard tables, 8 x 8 MCUs) around an ARBITRARY entropy segment: K1 is a pure
function of (bytes, DRI, interval count), it never decodes a Huffman symbol.  A segment is an FF-free random background with pattern
instances at chosen places RELATIVE TO THE SEGMENT'S 16-BYTE-ALIGNED BASE -- the origin K1's lanes count from: lane l of chunk c
holds bytes [4096 c + 16 l, + 16) from there, a wave 1 KiB, a chunk 4 KiB, a group of the one-pass form 16 KiB.  A COM segment in
front of the frame header sets data_off & 15.  The corpus is a fixed list (no case is made or dropped at run time)."""
import bisect
import functools
import zlib

import numpy as np

LANE, WAVE, CHUNK, GROUP = 16, 1024, 4096, 16384
LANE_EDGE = 5 * LANE  # a lane edge inside a wave, far enough from the segment's head for the longest pattern in front of it
EOI = b"\xff\xd9"


# ------------------------------------------------------------------------------------------------ the restatement

def model(data, dri, n_intervals, total_mcus, with_marks=False):
    """What K1 owes for one scan: dict(udata, ends, ends_u, n_ends, terminator, decoded_mcus, end_pos, ulen).  udata runs up to and
    including the FF FF of the closing entry (ulen = its position); nothing behind the closing entry is specified."""
    data = bytes(data)
    n = len(data)
    out, ends, ends_u, marks = bytearray(), [], [], []
    terminator, end_pos, p = 0, None, 0
    while p < n:
        if data[p] != 0xFF:
            q = data.find(b"\xff", p)  # (bytes other than FF are emitted as they are: a run of them at once)
            q = n if q < 0 else q
            out += data[p:q]
            p = q
            continue
        marks.append((len(out), p))
        if p + 1 >= n:  # FF with nothing behind it: dropped, the data has run out
            p += 1
            break
        x = data[p + 1]
        if x == 0x00:
            out.append(0xFF)
            p += 2
        elif x == 0xFF:  # fill: the first FF goes, the second is looked at again
            p += 1
        else:
            ends.append(p)
            ends_u.append(len(out))
            out += b"\xff\xff"
            if dri != 0 and 0xD0 <= x <= 0xD7 and len(ends) < n_intervals:
                p += 2
                continue
            terminator, end_pos = x, p  # the n_intervals-th RST, or any other marker (every marker when DRI == 0)
            break
    if end_pos is None:  # the data ran out: a pseudo entry at its end, sixteen one-bits behind the copied bytes
        ends.append(n)
        ends_u.append(len(out))
        out += b"\xff\xff"
        end_pos = n
    res = dict(udata=bytes(out), ends=ends, ends_u=ends_u, n_ends=len(ends), terminator=terminator,
               decoded_mcus=min(len(ends) * (dri or total_mcus), total_mcus), end_pos=end_pos, ulen=ends_u[-1])
    if with_marks:
        res["marks"] = marks
    return res


def raw_position(marks, u):
    """raw offset of the byte that udata[u] came from (marks: (udata length, raw offset) at every FF the model met)"""
    k = bisect.bisect_right(marks, (u, 1 << 62)) - 1
    return u if k < 0 else marks[k][1] + (u - marks[k][0])


# ------------------------------------------------------------------------------------------------ the file writer

@functools.lru_cache(maxsize=None)
def _template():
    """the marker segments of a gray baseline file of the generator (APP0, DQT, SOF0, DHT with the standard tables, DRI, SOS)"""
    from tools import jpegsynth

    f = bytes(jpegsynth.encode(8, 8, "gray", 75, 1, seed=1))
    segs, i = {}, 2
    while True:
        m, ln = f[i + 1], int.from_bytes(f[i + 2:i + 4], "big")
        segs[m] = f[i:i + 2 + ln]
        i += 2 + ln
        if m == 0xDA:
            return segs


def header(width, height, dri, misalign):
    """SOI .. SOS header; its length is `misalign` modulo 16 (the COM segment's payload makes it so)"""
    t = _template()
    sof = bytearray(t[0xC0])
    sof[5:7], sof[7:9] = height.to_bytes(2, "big"), width.to_bytes(2, "big")
    rest = t[0xE0] + t[0xDB] + bytes(sof) + t[0xC4] + (b"\xff\xdd\x00\x04" + dri.to_bytes(2, "big") if dri else b"") + t[0xDA]
    pad = (misalign - (2 + 4 + len(rest))) % 16
    h = b"\xff\xd8" + b"\xff\xfe" + (pad + 2).to_bytes(2, "big") + bytes([0x20] * pad) + rest
    assert len(h) % 16 == misalign
    return h


def frame_for(dri, n_intervals):
    """(width, height) of a frame of 8 x 8 MCUs with that many restart intervals (DRI 0: one MCU, one interval)"""
    if dri == 0:
        assert n_intervals == 1
        return 8, 8
    mcus = n_intervals * dri
    if mcus <= 4000:
        return 8 * mcus, 8
    assert mcus % 200 == 0
    return 1600, 8 * (mcus // 200)


class Case:
    """One file.  instances: [(name, at, bytes)], `at` counted from the segment's aligned base (= data offset + misalign)."""

    def __init__(self, name, family, seg, tail, dri, n_intervals, misalign, instances, identify_ok=True, jobs=1):
        self.name, self.family, self.dri, self.n_intervals, self.misalign = name, family, dri, n_intervals, misalign
        self.instances, self.identify_ok, self.jobs = instances, identify_ok, jobs
        self.width, self.height = frame_for(dri, n_intervals)
        self.total_mcus = (self.width // 8) * (self.height // 8)
        h = header(self.width, self.height, dri, misalign)
        self.data_pos, self.seg_len = len(h), len(seg)
        self.file = h + bytes(seg) + tail

    @property
    def data(self):
        return self.file[self.data_pos:]

    def instance_near(self, raw):
        """the instance nearest raw offset `raw` of the data"""
        if not self.instances:
            return None
        return min(self.instances, key=lambda it: min(abs(it[1] - self.misalign - raw), abs(it[1] + len(it[2]) - 1 - self.misalign - raw)))[:2]

    def check_instances(self):
        """the pattern bytes lie where the case says, in the file the writer returned"""
        base = self.data_pos - self.misalign
        assert base % 16 == 0
        for name, at, pat in self.instances:
            assert self.file[base + at:base + at + len(pat)] == pat, (self.name, name, at)


def background(n, seed):
    return bytearray(np.random.default_rng(seed).integers(0, 255, n, dtype=np.uint8).tobytes())  # 0 .. 254: no FF


def make_case(name, family, end_at, places, tail, dri, n_intervals, misalign, **kw):
    """A segment whose last byte lies at `end_at` - 1 from the aligned base; places: [(name, at, bytes)] in rising order, 64 bytes
    of background between them (the last one may end the segment)."""
    seg = background(end_at - misalign, zlib.crc32(name.encode()))  # (the same bytes whatever is built first)
    prev_end = None
    for iname, at, pat in places:
        assert at - misalign >= 0 and at + len(pat) <= end_at, (name, iname, at)
        assert prev_end is None or at - prev_end >= 64, (name, iname, at, prev_end)
        seg[at - misalign:at - misalign + len(pat)] = pat
        prev_end = at + len(pat)
    return Case(name, family, seg, tail, dri, n_intervals, misalign, list(places), **kw)


# ------------------------------------------------------------------------------------------------ the corpus

KS = (1, 2, 3, 15, 16, 17, 33)  # fill runs: from 16 on a lane holds nothing but dropped bytes
RST8 = b"".join(b"\xff" + bytes([0xD0 + i]) for i in range(8))
STUFFED = [("ff00", b"\xff\x00"), ("ff00x8", b"\xff\x00" * 8), ("ff00x24", b"\xff\x00" * 24)] + [("ff%d_00" % k, b"\xff" * k + b"\x00") for k in KS]
ENTRIES = [("rst", b"\xff\xd3"), ("rstx8", RST8)] + [("ff%d_rst" % k, b"\xff" * k + b"\xd5") for k in KS]
# Marker-free patterns in a DRI = 0 scan: the restart interval only decides how a marker's code byte is classed, so the longest
# of them (ff00x24, the fill runs of 15, 17 and 33) are left to the DRI = 1 leg -- the corpus stays near 30 MiB.
STUFFED_DRI0 = [p for p in STUFFED if p[0] in ("ff00", "ff00x8", "ff1_00", "ff2_00", "ff3_00", "ff16_00")]
PLAIN_EDGES = (("lane", LANE_EDGE), ("wave", WAVE), ("chunk", CHUNK), ("group0|1", GROUP), ("group1|2", 2 * GROUP), ("group2|closing", 3 * GROUP))
TERM_EDGES = PLAIN_EDGES[:5]
TERM_KS = (2, 16, 17, 33)  # fill in front of the terminator (ff1_eoi would be EOI itself): 33 is two lanes of nothing but dropped bytes
SOS2 = b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"


def _mis(i):
    return (i * 7 + 3) % 16


@functools.lru_cache(maxsize=None)
def plain_cases(dri):
    """families a, b, c: patterns that do not end the scan, one instance on every edge kind per file -- groups 1 and 2 of the
    one-pass form are plain (tile writer), group 0 and the closing group 3 take the per-chunk writer"""
    out = []
    for pname, pat in (STUFFED + ENTRIES if dri else STUFFED_DRI0):
        for delta in range(-len(pat), 2):
            places = [("%s@%s%+d" % (pname, ename, delta), b + delta, pat) for ename, b in PLAIN_EDGES]
            n_entries = sum(1 for i in range(len(pat) - 1) if pat[i] == 0xFF and 0xD0 <= pat[i + 1] <= 0xD7) * len(places)
            out.append(make_case("plain/%s%+d/dri%d" % (pname, delta, dri), "plain_dri%d" % dri, 3 * GROUP + 192, places, EOI, dri,
                                 n_entries + 3 if dri else 1, _mis(len(out))))
    return out


@functools.lru_cache(maxsize=None)
def terminator_cases():
    """families d and c: what ends the scan, every byte of it once on each side of every edge kind"""
    out = []
    for dri in (1, 0):
        terms = [("eoi", b"\xff\xd9", b""), ("com_eoi", b"\xff\xfe", b"\x00\x04\x11\x22" + EOI), ("sos2", b"\xff\xda", SOS2[2:] + bytes(range(40)) + EOI)]
        if dri == 0:
            terms.append(("rst_dri0", b"\xff\xd4", bytes(range(1, 41)) + EOI))  # any marker ends a DRI = 0 scan
        terms += [("ff%d_eoi" % k, b"\xff" * k + b"\xd9", b"") for k in TERM_KS]
        for tname, pat, trail in terms:
            for ename, b in TERM_EDGES:
                for delta in range(-len(pat), 2):
                    at = b + delta
                    places = []
                    if dri and b >= CHUNK:  # a few intervals in front
                        places = [("rst_front", 300, b"\xff\xd0"), ("rst_front", 2000, b"\xff\xd1")]
                    places.append(("%s@%s%+d" % (tname, ename, delta), at, pat))
                    out.append(make_case("term/%s@%s%+d/dri%d" % (tname, ename, delta, dri), "term", at + len(pat), places, trail, dri,
                                         8 if dri else 1, min(_mis(len(out)), 15 if b > LANE_EDGE else 8), jobs=2 if tname == "sos2" else 1))
    return out


@functools.lru_cache(maxsize=None)
def behind_and_cap_cases():
    """family d: entries and stuffed bytes BEHIND the terminator (same lane, same chunk, a later group) do not count;
    family e: the interval cap -- the n_intervals-th RST closes the scan and is its terminator"""
    out = []
    junk = b"\xff\xd1\xff\x00\x55\xff\xd2"
    for dri in (1, 0):
        for tname, pat in (("eoi", EOI), ("com", b"\xff\xfe\x00\x02")) + ((("rst_dri0", b"\xff\xd6"),) if dri == 0 else ()):
            for at0 in (1000, 1006, GROUP + 8):  # the terminator in the middle of a lane / with the junk in the next lane
                places = [("%s_then_junk" % tname, at0, pat + junk), ("junk_same_chunk", at0 + 512, junk), ("junk_later_group", at0 + 20000, junk),
                          ("junk_later_group", at0 + 40000, junk)]
                out.append(make_case("behind/%s@%d/dri%d" % (tname, at0, dri), "behind_cap", at0 + 40100, places, EOI, dri, 9 if dri else 1, _mis(len(out))))
    # n - 1 entries, then EOI; exactly n entries (the last one's code byte is the terminator), data behind it
    for n in (1, 2, 5):
        rsts = [("rst%d" % i, 100 + 150 * i, b"\xff" + bytes([0xD0 + i % 8])) for i in range(n)]
        out.append(make_case("cap/%d_of_%d_then_eoi" % (n - 1, n), "behind_cap", 100 + 150 * n, rsts[:n - 1], EOI, 1, n, _mis(len(out))))
        out.append(make_case("cap/%d_of_%d" % (n, n), "behind_cap", 100 + 150 * n + 64, rsts, EOI, 1, n, _mis(len(out))))
    # n + 3 entries: the closing one at every place around a chunk edge and the group edges, three more behind it (the next two
    # bytes, the same chunk, a later group)
    for ename, b in (("chunk", CHUNK), ("group0|1", GROUP), ("group1|2", 2 * GROUP), ("group2|closing", 3 * GROUP)):
        for delta in range(-2, 2):
            at = b + delta
            front = [("rst_front%d" % i, x, b"\xff" + bytes([0xD0 + i])) for i, x in enumerate((100, 1500, b // 2, b - 900, b - 200))]
            places = front + [("closing_rst@%s%+d" % (ename, delta), at, b"\xff\xd5\xff\xd6"), ("rst_behind", at + 500, b"\xff\xd7"),
                              ("rst_behind", at + 17000, b"\xff\xd0")]
            out.append(make_case("cap/closing@%s%+d" % (ename, delta), "behind_cap", at + 20000, places, EOI, 1, 6, _mis(len(out))))
    return out


CUT_ENDINGS = (("xx", b"\x41"), ("ff", b"\xff"), ("ffff", b"\xff\xff"), ("ff00", b"\xff\x00"), ("ffd3", b"\xff\xd3"))


@functools.lru_cache(maxsize=None)
def cut_cases():
    """family f: the file is cut, nothing closes the scan.  The reference's Identify() walks the same bytes first and throws ("No
    marker found.") unless they end in a marker: such a file fails at upload, K1 never sees it, and the case says so
    (identify_ok False; the test asserts the failure).  A cut right behind an RST passes: with DRI != 0 that RST is an entry and the
    data runs out behind it."""
    out = []
    for dri in (1, 0):
        for ename, b in (("lane", LANE_EDGE), ("chunk", CHUNK), ("group0|1", GROUP)):
            for delta in range(-2, 3):
                for cname, pat in CUT_ENDINGS:
                    end = b + delta
                    places = [("rst_front", 20, b"\xff\xd0")] if dri and b > LANE_EDGE else []
                    places.append(("cut_%s@%s%+d" % (cname, ename, delta), end - len(pat), pat))
                    out.append(make_case("cut/%s@%s%+d/dri%d" % (cname, ename, delta, dri), "cut", end, places, b"", dri, 4 if dri else 1,
                                         min(_mis(len(out)), 15 if b > LANE_EDGE else 8), identify_ok=cname == "ffd3"))
    return out


@functools.lru_cache(maxsize=None)
def head_cases():
    """family g: patterns inside the first 16 bytes of the data at all 16 values of data_off & 15, and very short segments"""
    out = []
    for dri in (1, 0):
        pats = [("ff00", b"\xff\x00"), ("ff2_00", b"\xff\xff\x00"), ("ff00x7", b"\xff\x00" * 7)]
        if dri:
            pats += [("rst", b"\xff\xd2"), ("ff3_rst", b"\xff\xff\xff\xd1"), ("rstx7", RST8[:14])]
        for mis in range(16):
            for pname, pat in pats:
                for o in (0, 1, 16 - len(pat)):
                    out.append(make_case("head/%s+%d/mis%d/dri%d" % (pname, o, mis, dri), "heads", mis + 96, [("%s+%d" % (pname, o), mis + o, pat)], EOI, dri,
                                         12 if dri else 1, mis))
            for pname, pat in (("eoi", EOI), ("ff2_eoi", b"\xff\xff\xd9")):
                for o in (0, 1, 16 - len(pat)):
                    out.append(make_case("head/%s+%d/mis%d/dri%d" % (pname, o, mis, dri), "heads", mis + o + len(pat), [("%s+%d" % (pname, o), mis + o, pat)], b"",
                                         dri, 12 if dri else 1, mis))
            for n in (0, 1, 2, 15, 16, 17):
                out.append(make_case("head/len%d/mis%d/dri%d" % (n, mis, dri), "heads", mis + n, [], EOI, dri, 12 if dri else 1, mis))
    return out


LONG_BYTES = 66 * GROUP + 70000  # a little over 1.1 MiB


@functools.lru_cache(maxsize=None)
def long_case():
    """family h: at least 66 groups of random bytes (every FF stuffed), an entry every 40-300 bytes, a sprinkling of fill runs:
    look-back windows beyond 64 predecessors, running sums over many groups"""
    rng = np.random.default_rng(77)
    parts, total, entries = [], 0, 0
    while total < LONG_BYTES:
        run = rng.integers(0, 256, int(rng.integers(40, 301)), dtype=np.uint8).tobytes().replace(b"\xff", b"\xff\x00")
        fill = b"\xff" * int(rng.choice(KS)) if rng.random() < 0.08 else b""
        if rng.random() < 0.04:
            run = run[:len(run) // 2] + b"\xff" * int(rng.choice(KS)) + b"\x00" + run[len(run) // 2:]
        piece = run + fill + b"\xff" + bytes([0xD0 + entries % 8])
        parts.append(piece)
        total += len(piece)
        entries += 1
    seg = b"".join(parts) + background(50, 5)
    n = (entries + 10 + 199) // 200 * 200
    return Case("long", "long", seg, EOI, 1, n, 11, [])


def corpus():
    """every case of the direct tests, a fixed list"""
    return plain_cases(1) + plain_cases(0) + terminator_cases() + behind_and_cap_cases() + cut_cases() + head_cases() + [long_case()]


FAMILIES = ("plain_dri1", "plain_dri0", "term", "behind_cap", "cut", "heads", "long")


def family(name):
    return [c for c in corpus() if c.family == name]


@functools.lru_cache(maxsize=None)
def _expected(file, data_pos, dri, n_intervals, total_mcus):
    return model(file[data_pos:], dri, n_intervals, total_mcus, with_marks=True)


def expected(case, job=0):
    """the model's answer for scan job `job` of the case's file, computed once per file (job 1: the scan behind a second SOS)"""
    if job == 0:
        return _expected(case.file, case.data_pos, case.dri, case.n_intervals, case.total_mcus)
    at = case.file.index(SOS2, case.data_pos) + len(SOS2)
    return _expected(case.file, at, case.dri, case.n_intervals, case.total_mcus)


def segment_bytes():
    return sum(c.seg_len for c in corpus())


# ------------------------------------------------------------------------------------------------ fill in valid files

def insert_fill(data, seed, share=0.3):
    """`data`: a valid file.  Runs of 1-40 FF in front of about `share` of the stuffed FF 00 and the RSTs of its (last) scan, and
    always in front of its EOI -- fill the reference's bit reader and marker walk skip (JpegBitReader.cs:117-121, JpegReader.cs:131-135)."""
    data = bytes(data)
    rng = np.random.default_rng(seed)
    start = data.rindex(b"\xff\xda")
    start += 2 + int.from_bytes(data[start + 2:start + 4], "big")
    out, p = bytearray(data[:start]), start
    while p < len(data):
        if data[p] == 0xFF and p + 1 < len(data) and (data[p + 1] == 0 or 0xD0 <= data[p + 1] <= 0xD9) and (rng.random() < share or data[p + 1] == 0xD9):
            out += b"\xff" * int(rng.integers(1, 41))  # (the EOI always gets its run: the ingest's verdict is about that place)
        if data[p] == 0xFF:
            out += data[p:p + 2]
            p += 2
        else:
            out.append(data[p])
            p += 1
    return bytes(out)


def rebuild(m, data):
    """an entropy segment from the model's output: FF re-stuffed, the original marker bytes back at the entries"""
    out, u = bytearray(), 0
    for e, eu in zip(m["ends"], m["ends_u"]):
        out += m["udata"][u:eu].replace(b"\xff", b"\xff\x00")
        out += data[e:e + 2]
        u = eu + 2
    return bytes(out)
