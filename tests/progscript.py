"""A progressive (SOF2) JPEG writer driven by an arbitrary scan script, and the catalogue of scripts the suite decodes.

The writer works in the coefficient domain: the caller hands it the quantised zig-zag coefficients of every block of the padded
MCU grid and a list of scans, and gets a file whose decoded coefficient store is known in advance (expected_store).  T.81
Annex G (progressive Huffman coding) and K.2 (code lengths from frequencies, the all-ones code reserved) from the text.

  DC first / refinement; AC first pass with ZRL and EOBn runs (split at 32 767); AC refinement with buffered correction bits
  (flushed behind the EOBn symbol, and before the buffer passes 937 bits); runs and predictors reset at restart markers; a DRI
  segment whenever a scan's interval differs from the one in force; byte stuffing, 1-padding.

Table shapes of a scan: "optimal" (K.2 tables of the scan's own symbols, a DHT in front of the scan), "long16" (every symbol
the scan uses gets a 16-bit code 0x8000 + k, one symbol it never uses takes the 1-bit code), "shared" (all tables of the
file in ONE DHT segment in front of the first scan; scans pick identifiers 0-3 without redefining them).
"""
import functools
from typing import NamedTuple

import numpy as np

MAX_EOBRUN = 0x7FFF
MAX_CORRECTION_BITS = 937  # the buffer is flushed once it holds more than this (1000 - 64 + 1)


class Scan(NamedTuple):
    comps: tuple  # indices into the frame's component list
    ss: int
    se: int
    ah: int
    al: int
    dri: int = 0
    tid: int = 0  # table identifier: an AC scan uses tid, component j of a DC first pass (tid + j) & 3, a DC refinement tid
    shape: str = "optimal"


def S(comps, ss, se, ah, al, dri=0, tid=0, shape="optimal"):
    return Scan(tuple(comps), ss, se, ah, al, dri, tid, shape)


class Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, v, n):
        if n == 0:
            return
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def align(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)

    def marker(self, m):
        self.align()
        self.out += bytes([0xFF, m])


def optimal_table(freq):
    """K.2: code lengths <= 16 with the all-ones code reserved.  freq: {symbol: count}.  Returns (BITS[16], HUFFVAL)."""
    f = [0] * 257
    for s, c in freq.items():
        f[s] = c
    f[256] = 1
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, 1 << 62
        for i in range(257):
            if f[i] and f[i] <= v:
                v, c1 = f[i], i
        c2, v = -1, 1 << 62
        for i in range(257):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 64
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(63, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the reserved symbol 256 had the longest code
    vals = []
    for ln in range(1, 64):
        for s in range(256):
            if codesize[s] == ln:
                vals.append(s)
    return bits[1:17], vals


def long16_table(symbols, dc):
    """every used symbol a 16-bit code 0x8000 + k; a symbol the scan never uses takes the 1-bit code (for DC tables it must be
    <= 15 or libjpeg refuses the table)"""
    symbols = sorted(symbols)
    dummy = next(s for s in range(15 if dc else 255, -1, -1) if s not in symbols)
    return [1] + [0] * 14 + [len(symbols)], [dummy] + symbols


def code_map(bits, vals):
    """Annex C code assignment: {symbol: (code, length)}"""
    m, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            m[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return m


def seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def geometry(width, height, comps):
    """-> max_h, max_v, mcus_x, mcus_y, [(hblocks, vblocks) of each component's own grid]"""
    max_h, max_v = max(c[1] for c in comps), max(c[2] for c in comps)
    mcus_x, mcus_y = -(-width // (8 * max_h)), -(-height // (8 * max_v))
    hb, vb = (width + 7) // 8, (height + 7) // 8
    grids = []
    for (_, h, v, _) in comps:
        hs, vs = max_h // h, max_v // v
        grids.append((-(-hb // hs), -(-vb // vs)))
    return max_h, max_v, mcus_x, mcus_y, grids


def scan_symbols(coefs, comps, width, height, sc):
    """The scan as a token list: ("S", table key, symbol, extra bits, their count) | ("B", bit) | ("R",).
    coefs[ci]: int array [mcus_y * v, mcus_x * h, 64], zig-zag order.  The table key is the component index in a DC scan, 0 in
    an AC scan."""
    _, _, mcus_x, mcus_y, grids = geometry(width, height, comps)
    cis, ss, se, ah, al, dri = sc.comps, sc.ss, sc.se, sc.ah, sc.al, sc.dri
    out = []
    emit = out.append
    state = {"eobrun": 0, "be": [], "units": 0}

    def flush_eobrun():
        e = state["eobrun"]
        if e > 0:
            n = e.bit_length() - 1
            emit(("S", 0, n << 4, e & ((1 << n) - 1), n))
            state["eobrun"] = 0
        if state["be"]:
            for b in state["be"]:
                emit(("B", b))
            state["be"] = []

    pred = {ci: 0 for ci in cis}

    def unit_done(last):
        state["units"] += 1
        if dri and state["units"] % dri == 0 and not last:
            flush_eobrun()
            emit(("R",))
            for ci in cis:
                pred[ci] = 0

    def dc_block(ci, c0):
        if ah == 0:
            v = c0 >> al
            d = v - pred[ci]
            pred[ci] = v
            n = abs(d).bit_length()
            emit(("S", ci, n, (d if d >= 0 else d - 1) & ((1 << n) - 1), n))
        else:
            emit(("B", (c0 >> al) & 1))

    if ss == 0:
        assert se == 0, "a DC scan carries coefficient 0 only"
        dcs = [coefs[ci][..., 0].tolist() for ci in range(len(comps))]
        if len(cis) == 1:
            ci = cis[0]
            hcount, vcount = grids[ci]
            for by in range(vcount):
                for bx in range(hcount):
                    dc_block(ci, dcs[ci][by][bx])
                    unit_done(by == vcount - 1 and bx == hcount - 1)
        else:
            for my in range(mcus_y):
                for mx in range(mcus_x):
                    for ci in cis:
                        _, h, v, _ = comps[ci]
                        for y in range(v):
                            for x in range(h):
                                dc_block(ci, dcs[ci][my * v + y][mx * h + x])
                    unit_done(my == mcus_y - 1 and mx == mcus_x - 1)
        return out

    assert len(cis) == 1 and 1 <= ss <= se <= 63, "an AC scan has one component and a band inside 1..63"
    ci = cis[0]
    hcount, vcount = grids[ci]
    nblocks, nb = hcount * vcount, se - ss + 1
    band = np.ascontiguousarray(coefs[ci][:vcount, :hcount, ss:se + 1]).reshape(nblocks, nb)
    t = np.abs(band) >> al
    rows, cols = np.nonzero(t)  # (one vectorised test: all-zero bands of a block cost nothing below)
    starts = np.searchsorted(rows, np.arange(nblocks + 1)).tolist()
    tv = t[rows, cols].tolist()
    neg = (band[rows, cols] < 0).tolist()
    cols = cols.tolist()
    for b in range(nblocks):
        lo, hi = starts[b], starts[b + 1]
        if ah == 0:
            prev = -1
            for i in range(lo, hi):
                k = cols[i]
                r = k - prev - 1
                prev = k
                flush_eobrun()
                while r > 15:
                    emit(("S", 0, 0xF0, 0, 0))
                    r -= 16
                n = tv[i].bit_length()
                emit(("S", 0, (r << 4) | n, (~tv[i] if neg[i] else tv[i]) & ((1 << n) - 1), n))
            if prev != nb - 1:
                state["eobrun"] += 1
                if state["eobrun"] == MAX_EOBRUN:
                    flush_eobrun()
        else:
            eob = -1
            for i in range(lo, hi):
                if tv[i] == 1:
                    eob = cols[i]
            r, br, prev = 0, [], -1
            for i in range(lo, hi):
                k = cols[i]
                r += k - prev - 1
                prev = k
                while r > 15 and k <= eob:
                    flush_eobrun()
                    emit(("S", 0, 0xF0, 0, 0))
                    r -= 16
                    for x in br:
                        emit(("B", x))
                    br = []
                if tv[i] > 1:
                    br.append(tv[i] & 1)  # a coefficient with history: one correction bit
                    continue
                flush_eobrun()
                emit(("S", 0, (r << 4) | 1, 0 if neg[i] else 1, 1))
                for x in br:
                    emit(("B", x))
                br = []
                r = 0
            r += nb - 1 - prev
            if r > 0 or br:
                state["eobrun"] += 1
                state["be"] += br
                if state["eobrun"] == MAX_EOBRUN or len(state["be"]) > MAX_CORRECTION_BITS:
                    flush_eobrun()
        unit_done(b == nblocks - 1)
    flush_eobrun()
    return out


def _table_ids(sc):
    """{table key of scan_symbols: (class, identifier)}"""
    if sc.ss == 0:
        # (a DC refinement scan reads no symbol, but the reference wants the table its header names defined: the first one)
        return {ci: (0, (sc.tid + (j if sc.ah == 0 else 0)) & 3) for j, ci in enumerate(sc.comps)}
    return {0: (1, sc.tid & 3)}


def _frequencies(tokens):
    freq = {}
    for t in tokens:
        if t[0] == "S":
            f = freq.setdefault(t[1], {})
            f[t[2]] = f.get(t[2], 0) + 1
    return freq


def write(width, height, comps, qtabs, coefs, script, precision=8):
    """comps: [(id, h, v, tq)]; qtabs: {tq: uint16[64] zig-zag, every entry <= 255}; coefs: per component an integer array
    [mcus_y * v, mcus_x * h, 64] (the padded MCU grid); script: list of Scan."""
    coefs = [np.asarray(c, dtype=np.int64) for c in coefs]
    out = bytearray(b"\xff\xd8")
    for tq, q in qtabs.items():
        out += seg(0xDB, bytes([tq]) + bytes(int(x) for x in q))
    out += seg(0xC2, bytes([precision]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([len(comps)]) +
               b"".join(bytes([cid, (h << 4) | v, tq]) for cid, h, v, tq in comps))
    tokens = [scan_symbols(coefs, comps, width, height, sc) for sc in script]
    shared = {}  # (class, identifier) -> code map
    if any(sc.shape == "shared" for sc in script):
        assert all(sc.shape == "shared" for sc in script), "a file's tables are shared by all of its scans or by none"
        freq = {}
        for sc, tk in zip(script, tokens):
            ids = _table_ids(sc)
            for key, f in _frequencies(tk).items():
                acc = freq.setdefault(ids[key], {})
                for sym, n in f.items():
                    acc[sym] = acc.get(sym, 0) + n
        payload = b""
        for (cls, tid), f in sorted(freq.items()):
            bits, vals = optimal_table(f)
            payload += bytes([(cls << 4) | tid]) + bytes(bits) + bytes(vals)
            shared[(cls, tid)] = code_map(bits, vals)
        out += seg(0xC4, payload)
    cur_dri = 0
    for sc, tk in zip(script, tokens):
        dc_scan = sc.ss == 0
        ids = _table_ids(sc)
        maps = {}
        for key, f in sorted(_frequencies(tk).items()):
            if sc.shape == "shared":
                maps[key] = shared[ids[key]]
                continue
            bits, vals = long16_table(f.keys(), dc_scan) if sc.shape == "long16" else optimal_table(f)
            cls, tid = ids[key]
            out += seg(0xC4, bytes([(cls << 4) | tid]) + bytes(bits) + bytes(vals))
            maps[key] = code_map(bits, vals)
        if sc.dri != cur_dri:
            out += seg(0xDD, sc.dri.to_bytes(2, "big"))
            cur_dri = sc.dri
        hdr = bytes([len(sc.comps)])
        for ci in sc.comps:
            tid = ids[ci if dc_scan else 0][1]
            hdr += bytes([comps[ci][0], (tid << 4) if dc_scan else tid])
        hdr += bytes([sc.ss, sc.se, (sc.ah << 4) | sc.al])
        out += seg(0xDA, hdr)
        bw = Bits()
        put = bw.put
        rst = 0
        for t in tk:
            if t[0] == "S":
                code, ln = maps[t[1]][t[2]]
                put((code << t[4]) | t[3], ln + t[4])
            elif t[0] == "B":
                put(t[1], 1)
            else:
                bw.marker(0xD0 + rst)
                rst = (rst + 1) & 7
        bw.align()
        out += bw.out
    out += b"\xff\xd9"
    return bytes(out)


def expected_store(coefs, comps, width, height, script):
    """What the decoder's store must hold behind the script: per component int16 [vblocks, hblocks, 64] over the component's own
    grid -- DC (c >> Al) << Al, AC sign(c) * ((|c| >> Al) << Al) of the LAST scan that covered each (component, coefficient),
    zero where no scan did."""
    _, _, _, _, grids = geometry(width, height, comps)
    exp = [np.zeros((g[1], g[0], 64), np.int64) for g in grids]
    for sc in script:
        for ci in sc.comps:
            hbk, vbk = grids[ci]
            src = np.asarray(coefs[ci])[:vbk, :hbk].astype(np.int64)
            if sc.ss == 0:
                exp[ci][..., 0] = (src[..., 0] >> sc.al) << sc.al
            else:
                s, e = sc.ss, sc.se + 1
                exp[ci][..., s:e] = np.sign(src[..., s:e]) * ((np.abs(src[..., s:e]) >> sc.al) << sc.al)
    return [e.astype(np.int16) for e in exp]


def store_in_mcu_order(exp, comps, width, height):
    """expected_store's arrays as the batch keeps the store: int16 [blocks, 64], MCU raster, component order, block raster in the
    MCU; blocks outside a component's own grid are zero"""
    _, _, mcus_x, mcus_y, grids = geometry(width, height, comps)
    bpm = sum(h * v for _, h, v, _ in comps)
    out = np.zeros((mcus_y, mcus_x, bpm, 64), np.int16)
    base = 0
    for ci, (_, h, v, _) in enumerate(comps):
        hbk, vbk = grids[ci]
        full = np.zeros((mcus_y * v, mcus_x * h, 64), np.int16)
        full[:vbk, :hbk] = exp[ci]
        out[:, :, base:base + h * v] = full.reshape(mcus_y, v, mcus_x, h, 64).transpose(0, 2, 1, 3, 4).reshape(mcus_y, mcus_x, h * v, 64)
        base += h * v
    return out.reshape(-1, 64)


def planner_model(script):
    """What the product's planner must make of a script, restated from its documented rule: a scan waits for the
    earlier scans of its frame that may WRITE coefficients of a component it touches.  DC scans (interleaved, or Ss = 0) write
    coefficient 0; an AC first pass Ss..min(63, Se + 15), an AC refinement Ss..min(63, Se + 1).  Level = 1 + the highest level among
    them; DIRECT producers = those that no other one of them already waits for, transitively (the bookkeeping covers the first 64
    scans of a frame: from the 65th on a scan counts four more than it has).  Chain 0 = DC scans, 1 + min(3, c) = AC scans of
    component c.  -> dict(scans, levels, max_deps, chain_scans, deps: per scan the list of its direct producers)"""
    def written(sc):
        if len(sc.comps) != 1 or sc.ss == 0:
            return 0, 0
        return sc.ss, min(63, sc.se + (15 if sc.ah == 0 else 1))

    level, closure, deps, n_deps, chains = [], [], [], [], [0] * 5
    for i, sc in enumerate(script):
        lo, hi = written(sc)
        sharing = [j for j in range(i) if not (lo > written(script[j])[1] or written(script[j])[0] > hi) and set(sc.comps) & set(script[j].comps)]
        level.append(max([level[j] + 1 for j in sharing], default=0))
        mine = set()
        for j in sharing:
            if j < 64:
                mine |= closure[j] | {j}
        closure.append(mine)
        direct = [j for j in sharing if not any(k != j and k < 64 and j < 64 and j in closure[k] for k in sharing)]
        deps.append(direct)
        n_deps.append(len(direct) + (4 if i >= 64 else 0))
        chains[0 if (len(sc.comps) != 1 or sc.ss == 0) else 1 + min(3, sc.comps[0])] += 1
    return dict(scans=len(script), levels=max(level) + 1, max_deps=max(n_deps), chain_scans=chains, deps=deps)


def final_slots(script, ncomp):
    """The decoder's component slots as the script leaves them: scan component j goes into slot j (a single-component scan
    always takes slot 0).  None = a slot no scan ever filled."""
    slots = [None] * ncomp
    for sc in script:
        for j, ci in enumerate(sc.comps):
            slots[j] = ci
    return slots


def slots_map_one_to_one(script, ncomp):
    """Dispose() transforms the components the SLOTS name, one after the other: whether that is every component exactly once"""
    slots = final_slots(script, ncomp)
    return None not in slots and sorted(slots) == list(range(ncomp))


# ------------------------------------------------------------------------------------------------------------ coefficient recipes

def _shapes(width, height, comps):
    _, _, mcus_x, mcus_y, _ = geometry(width, height, comps)
    return [(mcus_y * v, mcus_x * h, 64) for (_, h, v, _) in comps]


def recipe_sparse(rng, width, height, comps, density=0.25, amp=40, dc_amp=600, ac_max=1023):
    """geometric magnitudes, fewer towards the high frequencies; the padding blocks of the MCU grid are filled like the others"""
    out = []
    for shape in _shapes(width, height, comps):
        mag = np.minimum(rng.geometric(1.0 / amp, shape), ac_max)
        c = mag * rng.choice([-1, 1], shape) * (rng.random(shape) < density * np.linspace(1.5, 0.2, 64))
        c[..., 0] = rng.integers(-dc_amp, dc_amp + 1, shape[:2])
        out.append(c.astype(np.int64))
    return out


def recipe_dense(rng, width, height, comps, amp=300, dc_amp=600):
    """63 nonzero AC coefficients in every block"""
    return recipe_sparse(rng, width, height, comps, density=5.0, amp=amp, dc_amp=dc_amp)


def recipe_sparse_gaps(rng, width, height, comps, gaps=()):
    """recipe_sparse with nothing but 0 and +-1 in the coefficient ranges `gaps` of component 0: no first pass of the script
    covers them, the refinement pass at Al = 0 brings them in as new coefficients"""
    out = recipe_sparse(rng, width, height, comps)
    for a, b in gaps:
        out[0][..., a:b + 1] = np.clip(out[0][..., a:b + 1], -1, 1)
    return out


def recipe_pm1(rng, width, height, comps, density=0.3):
    out = []
    for shape in _shapes(width, height, comps):
        c = rng.choice([-1, 1], shape) * (rng.random(shape) < density)
        c[..., 0] = rng.integers(-1, 2, shape[:2])
        out.append(c.astype(np.int64))
    return out


def recipe_limits(rng, width, height, comps):
    """8-bit category limits: AC +-1023 (category 10) beside +-1 and 0, DC alternating so that every difference is category 11"""
    out = []
    for shape in _shapes(width, height, comps):
        c = rng.choice([-1023, 1023, -1, 1, 0, 512, -512], shape)
        dc = np.where(np.arange(shape[0] * shape[1]).reshape(shape[:2]) % 2 == 0, -1000, 1000)  # (alternating in raster order)
        c[..., 0] = dc + rng.integers(-20, 21, shape[:2])
        out.append(c.astype(np.int64))
    return out


def recipe_history_only(rng, width, height, comps):
    """every coefficient at least 2 in magnitude: behind an Al = 1 first pass a refinement scan finds history everywhere and nothing
    new -- the whole scan is correction bits inside end-of-band runs"""
    out = []
    for shape in _shapes(width, height, comps):
        out.append(rng.choice([-6, -4, -2, 2, 4, 6, 3, 5, -7], shape).astype(np.int64))
    return out


def recipe_empty_high_band(rng, width, height, comps):
    """DC and coefficients 1-5 everywhere; 6-63 empty but for two coefficients: end-of-band runs longer than 32 767 blocks"""
    out = []
    for shape in _shapes(width, height, comps):
        c = np.zeros(shape, np.int64)
        c[..., 0] = rng.integers(-200, 200, shape[:2])
        c[..., 1:6] = rng.integers(-3, 4, shape[:2] + (5,))
        c[5, 7, 40] = 9
        c[shape[0] - 1, shape[1] - 1, 63] = -1
        out.append(c)
    return out


RECIPES = {"sparse": recipe_sparse, "sparse_gaps": recipe_sparse_gaps, "dense": recipe_dense, "pm1": recipe_pm1, "limits": recipe_limits,
           "history_only": recipe_history_only, "empty_high_band": recipe_empty_high_band}


# ------------------------------------------------------------------------------------------------------------------ the catalogue

YCC420 = [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
YCC444 = [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
YCC411 = [(1, 4, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
YCC440 = [(1, 1, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
GRAY = [(1, 1, 1, 0)]
CMYK = [(1, 1, 1, 0), (2, 1, 1, 0), (3, 1, 1, 0), (4, 1, 1, 0)]

CLEAN = "clean"
EXPECT_RESTART = ("InvalidOperationException", "Expect restart marker.")


class Entry(NamedTuple):
    comps: list
    width: int
    height: int
    script: list
    recipe: tuple  # (name in RECIPES, keyword arguments)
    outcome: object  # CLEAN, or (the checker's error kind, its message)
    row: str  # the row of the catalogue this entry belongs to (every row keeps at least one clean entry)
    precision: int = 8
    unit_quant: bool = False  # all-ones quantisation tables (large coefficients stay inside the sample range's neighbourhood)


def successive(ci, bands, top):
    """the bands of component ci at Al = top, then one refinement pass over them per bit down to Al = 0"""
    out = [S([ci], a, b, 0, top) for a, b in bands]
    for al in range(top - 1, -1, -1):
        out += [S([ci], a, b, al + 1, al) for a, b in bands]
    return out


def dc_successive(cis, top):
    return [S(cis, 0, 0, 0, top)] + [S(cis, 0, 0, a + 1, a) for a in range(top - 1, -1, -1)]


_SIMPLE_420 = [S([0, 1, 2], 0, 0, 0, 0), S([0], 1, 63, 0, 1), S([1], 1, 63, 0, 0), S([2], 1, 63, 0, 0), S([0], 1, 63, 1, 0)]
_DRI_HEAD = [S([0, 1, 2], 0, 0, 0, 1, dri=5), S([0], 1, 9, 0, 1, dri=7), S([0], 10, 63, 0, 1, dri=0), S([0], 1, 63, 1, 0, dri=11),
             S([1], 1, 63, 0, 0, dri=5), S([2], 1, 63, 0, 0, dri=1000)]
_SPARSE = ("sparse", {})

CATALOGUE = {
    # bands k-k for every k: 63 dependency levels, one-coefficient band masks; 64 scans, still pipelined
    "gray_single_coefficient_bands": Entry(GRAY, 67, 45, [S([0], 0, 0, 0, 0)] + [S([0], k, k, 0, 0) for k in range(1, 64)], _SPARSE, CLEAN,
                                           "single_coefficient_bands"),
    # 128 scans: n_deps = 4 from the 65th scan on; refinement in reverse band order
    "gray_single_bands_refined": Entry(GRAY, 41, 33, [S([0], 0, 0, 0, 1)] + [S([0], k, k, 0, 1) for k in range(1, 64)] +
                                       [S([0], 0, 0, 1, 0)] + [S([0], k, k, 1, 0) for k in range(63, 0, -1)], _SPARSE, CLEAN, "single_bands_refined"),
    "gray_deep_sa": Entry(GRAY, 90, 70, dc_successive([0], 5) + successive(0, [(1, 63)], 6), _SPARSE, CLEAN, "deep_sa"),
    "precision8_al13": Entry(GRAY, 64, 48, dc_successive([0], 13) + successive(0, [(1, 63)], 13), ("sparse", dict(amp=300, dc_amp=1000)), CLEAN,
                             "al13"),
    "precision12_al9": Entry(GRAY, 64, 48, dc_successive([0], 9) + successive(0, [(1, 20), (21, 63)], 9),
                             ("sparse", dict(amp=2000, dc_amp=16000, ac_max=16383)), CLEAN, "precision12", precision=12),
    # three first-pass bands and one refinement over all of them: three direct dependencies
    "three_bands_then_refinement": Entry(YCC420, 1024, 768, [S([0, 1, 2], 0, 0, 0, 0), S([1], 1, 63, 0, 0), S([2], 1, 63, 0, 0), S([0], 1, 5, 0, 1),
                                                             S([0], 6, 20, 0, 1), S([0], 21, 63, 0, 1), S([0], 1, 63, 1, 0)], _SPARSE, CLEAN,
                                         "three_bands"),
    # A first pass may write up to Se + 15 (a run that overshoots the band), so the planner orders a band behind every earlier band
    # of the component that begins at or below its Se + 15: the contiguous bands above follow EACH OTHER, and their refinement
    # waits for the last of them alone.  Bands more than 15 coefficients apart are independent: a refinement over all of them has
    # one direct producer per band -- three (all of DevScan::dep[3] live, still one pipelined launch) and four (one too many).
    # The coefficients between the bands are 0 or +-1 and new in the refinement.
    "three_separate_bands_then_refinement": Entry(YCC420, 1024, 768, [S([0, 1, 2], 0, 0, 0, 0), S([1], 1, 63, 0, 0), S([2], 1, 63, 0, 0),
                                                                      S([0], 1, 5, 0, 1), S([0], 21, 25, 0, 1), S([0], 41, 63, 0, 1), S([0], 1, 63, 1, 0)],
                                                  ("sparse_gaps", dict(gaps=((6, 20), (26, 40)))), CLEAN, "three_bands"),
    "four_separate_bands_then_refinement": Entry(YCC420, 83, 61, [S([0, 1, 2], 0, 0, 0, 0), S([1], 1, 63, 0, 0), S([2], 1, 63, 0, 0), S([0], 1, 1, 0, 1),
                                                                  S([0], 17, 17, 0, 1), S([0], 33, 33, 0, 1), S([0], 49, 63, 0, 1), S([0], 1, 63, 1, 0)],
                                                 ("sparse_gaps", dict(gaps=((2, 16), (18, 32), (34, 48)))), CLEAN, "five_bands"),
    # three DC first passes, one per component, and ONE interleaved refinement behind all of them: three direct producers
    "dc_three_producers": Entry(YCC420, 100, 75, [S([2], 0, 0, 0, 1), S([0], 0, 0, 0, 1), S([1], 0, 0, 0, 1), S([0], 1, 63, 0, 0), S([1], 1, 63, 0, 0),
                                                  S([2], 1, 63, 0, 0), S([0, 1, 2], 0, 0, 1, 0)], _SPARSE, CLEAN, "dc_per_component"),
    "five_bands_then_one_refinement": Entry(YCC420, 83, 61, [S([0, 1, 2], 0, 0, 0, 0), S([1], 1, 63, 0, 0), S([2], 1, 63, 0, 0)] +
                                            [S([0], a, b, 0, 1) for a, b in [(1, 2), (3, 5), (6, 20), (21, 40), (41, 63)]] + [S([0], 1, 63, 1, 0)], _SPARSE, CLEAN, "five_bands"),
    # DC scans per component, chroma first, refinement split differently; ends on a Cb scan behind an interleaved one:
    # slots (Cb, Cb, Cr) -- Cb transformed twice, Y never
    "dc_per_component_chroma_first": Entry(YCC420, 100, 75, [S([2], 0, 0, 0, 2), S([1], 0, 0, 0, 2), S([0], 0, 0, 0, 2), S([2], 1, 63, 0, 0),
                                                             S([1, 2], 0, 0, 2, 1), S([0], 0, 0, 2, 1), S([0], 1, 63, 0, 0), S([0, 1, 2], 0, 0, 1, 0),
                                                             S([1], 1, 63, 0, 0)], _SPARSE, CLEAN, "dc_per_component"),
    "two_component_dc_scans": Entry(YCC420, 77, 50, [S([0, 1], 0, 0, 0, 0), S([2], 0, 0, 0, 0), S([0], 1, 63, 0, 0)], _SPARSE,
                                    CLEAN, "two_component_dc"),
    "high_band_before_low": Entry(YCC444, 50, 50, [S([0, 1, 2], 0, 0, 0, 0), S([0], 32, 63, 0, 0), S([0], 1, 31, 0, 0), S([1], 33, 63, 0, 2),
                                                   S([1], 1, 32, 0, 2), S([1], 1, 32, 2, 1), S([1], 33, 63, 2, 1), S([1], 33, 63, 1, 0),
                                                   S([1], 1, 32, 1, 0)], _SPARSE, CLEAN, "high_band_first"),
    # a DRI segment in front of every scan, none dividing its scan's unit count (4:2:0 120 x 90: 48 MCUs, Y 180, Cb/Cr 48 blocks)
    "dri_changes_between_scans": Entry(YCC420, 120, 90, _DRI_HEAD + [S([1, 2], 0, 0, 1, 0, dri=11), S([0], 0, 0, 1, 0, dri=7)], _SPARSE, CLEAN,
                                       "dri_changes"),
    "dri_divides_in_last_scan": Entry(YCC420, 120, 90, _DRI_HEAD + [S([1, 2], 0, 0, 1, 0, dri=11), S([0], 0, 0, 1, 0, dri=12)], _SPARSE, CLEAN,
                                      "dri_divides"),
    "dri_divides_in_middle_scan": Entry(YCC420, 120, 90, _DRI_HEAD[:1] + [S([0], 1, 9, 0, 1, dri=6)] + _DRI_HEAD[2:], _SPARSE, EXPECT_RESTART,
                                        "dri_divides"),
    "layout_411": Entry(YCC411, 70, 30, _SIMPLE_420, _SPARSE, CLEAN, "layouts"),
    "layout_440": Entry(YCC440, 30, 70, _SIMPLE_420, _SPARSE, CLEAN, "layouts"),
    "cmyk": Entry(CMYK, 40, 24, [S([0, 1, 2, 3], 0, 0, 0, 1)] + [S([c], 1, 63, 0, 1) for c in range(4)] + [S([c], 1, 63, 1, 0) for c in (3, 1, 2, 0)] +
                  [S([0, 1, 2, 3], 0, 0, 1, 0)], _SPARSE, CLEAN, "layouts"),
    # 182 x 182 = 33 124 blocks: EOB14 with the run split at 32 767, first pass and refinement
    "eob_run_over_32767": Entry(GRAY, 1456, 1456, [S([0], 0, 0, 0, 0), S([0], 1, 5, 0, 0), S([0], 6, 63, 0, 1), S([0], 6, 63, 1, 0)],
                                ("empty_high_band", {}), CLEAN, "long_eob_run"),
    "corrections_inside_eob_runs": Entry(GRAY, 240, 240, [S([0], 0, 0, 0, 0), S([0], 1, 63, 0, 1), S([0], 1, 63, 1, 0)], ("history_only", {}), CLEAN,
                                         "corrections_in_eob_runs"),
    "dense_long16_gray": Entry(GRAY, 200, 120, [S([0], 0, 0, 0, 0, shape="long16"), S([0], 1, 63, 0, 2, shape="long16"),
                                                S([0], 1, 63, 2, 1, shape="long16"), S([0], 1, 63, 1, 0, shape="long16")], ("dense", {}), CLEAN,
                               "dense_long16", unit_quant=True),
    "dense_long16_420": Entry(YCC420, 130, 70, [S([0, 1, 2], 0, 0, 0, 1, shape="long16"), S([0], 1, 63, 0, 1, shape="long16"),
                                                S([1], 1, 63, 0, 0, shape="long16"), S([2], 1, 63, 0, 0, shape="long16"),
                                                S([0, 1, 2], 0, 0, 1, 0, shape="long16"), S([0], 1, 63, 1, 0, shape="long16")], ("dense", {}), CLEAN,
                              "dense_long16", unit_quant=True),
    # four DC and four AC tables in one DHT segment, the scans alternate between them
    "shared_tables_ids_0_to_3": Entry(CMYK, 56, 40, [S([c], 0, 0, 0, 1, tid=c, shape="shared") for c in range(4)] +
                                      [S([c], 1, 63, 0, 1, tid=(c + 1) & 3, shape="shared") for c in (2, 0, 3, 1)] +
                                      [S([c], 1, 63, 1, 0, tid=c, shape="shared") for c in range(4)] +
                                      [S([0, 1, 2, 3], 0, 0, 1, 0, shape="shared")], _SPARSE, CLEAN, "shared_tables"),
    "dc_only": Entry(YCC420, 33, 17, [S([0, 1, 2], 0, 0, 0, 0)], _SPARSE, CLEAN, "small_stores"),
    "one_pixel": Entry(YCC420, 1, 1, [S([0, 1, 2], 0, 0, 0, 0), S([1], 1, 63, 0, 0), S([2], 1, 63, 0, 0), S([0], 1, 63, 0, 0)],
                       _SPARSE, CLEAN, "small_stores"),
    "one_block_column": Entry(YCC420, 8, 400, _SIMPLE_420, _SPARSE, CLEAN, "small_stores"),
    "one_block_row": Entry(YCC420, 400, 8, _SIMPLE_420, _SPARSE, CLEAN, "small_stores"),
    # scripts that end on chroma scans: slots (Cb, Cb, Cr) -- Cb transformed twice, Y never; and, without any three-component
    # scan, slots (Cb, Cr, none) -- Cb and Cr once, Y never
    "ends_on_cb_transformed_twice": Entry(YCC420, 72, 56, [S([0, 1, 2], 0, 0, 0, 0), S([0], 1, 63, 0, 0), S([2], 1, 63, 0, 0), S([1], 1, 63, 0, 0)],
                                          _SPARSE, CLEAN, "ends_on_chroma"),
    "ends_on_chroma_pair_luma_never": Entry(YCC420, 72, 56, [S([0], 0, 0, 0, 0), S([1, 2], 0, 0, 0, 1), S([0], 1, 63, 0, 0), S([1], 1, 63, 0, 0),
                                                               S([2], 1, 63, 0, 0), S([1, 2], 0, 0, 1, 0)], _SPARSE, CLEAN, "ends_on_chroma"),
    # coefficient recipes of their own
    "plus_minus_one": Entry(YCC444, 48, 32, [S([0, 1, 2], 0, 0, 0, 0), S([1], 1, 10, 0, 0), S([1], 11, 63, 0, 0), S([2], 1, 63, 0, 0), S([0], 1, 63, 0, 0)],
                            ("pm1", {}), CLEAN, "recipes"),
    "category_limits": Entry(GRAY, 48, 32, [S([0], 0, 0, 0, 0), S([0], 1, 63, 0, 1), S([0], 1, 63, 1, 0)], ("limits", {}), CLEAN, "recipes",
                             unit_quant=True),
}

ROWS = sorted({e.row for e in CATALOGUE.values()})
# the entries whose decoded samples are also compared through the 16-bit sink
EXTENDED_U16_ENTRIES = ("precision12_al9", "gray_deep_sa", "cmyk")


class Built(NamedTuple):
    entry: Entry
    data: bytes
    coefs: list
    qtabs: dict
    expected: list  # expected_store


@functools.lru_cache(maxsize=None)
def build(name):
    """the catalogue entry as a file (fixed seeds: the same bytes in every session), with the coefficients it was made from"""
    e = CATALOGUE[name]
    rng = np.random.default_rng(1000 + sorted(CATALOGUE).index(name))
    fn, kw = e.recipe
    coefs = RECIPES[fn](rng, e.width, e.height, e.comps, **kw)
    tqs = sorted({c[3] for c in e.comps})
    qtabs = {tq: (np.ones(64, np.uint16) if e.unit_quant else rng.integers(1, 24, 64).astype(np.uint16)) for tq in tqs}
    data = write(e.width, e.height, e.comps, qtabs, coefs, e.script, precision=e.precision)
    return Built(e, data, coefs, qtabs, expected_store(coefs, e.comps, e.width, e.height, e.script))
