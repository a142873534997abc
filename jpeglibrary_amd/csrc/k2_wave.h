// jpeglibrary_amd/csrc/k2_wave.h -- the K2 wave: what k2_huffman.hip (K2) and the final pass of k2s_subseq.hip (K2S) are both made of,
// and nothing any other kernel file uses.  A wave of 64 lanes opens a ring-fed bit stream per lane, decodes one block per lane in
// lock-step into a swizzled 8 KB LDS staging, flushes 64 blocks as whole 128-byte lines and leaves the staging zero.
//   the lookups' format and their builders (lut_pool_kernel)     kK2LutBits .. k2_fast_entry
//   a lane's stream: ring, feed, position, the symbol step       K2Feed, K2Pos, k2_open_at_bit, k2_topup, k2_symbol, k2_slow_symbol
//   one block of a lane                                          k2_decode_dc, k2_decode_ac
//   the wave's staging                                           k2_wave_sync, k2_flush_dense
//   a workgroup's LDS and a pooled wave's work                   K2Group, k2_group_setup, k2_next_ticket
//   per-wave cycle counters of a -DJPGPU_K2_PROFILE build        K2_TICK, K2_PROF_ADD, K2_PROF_DEFINE
// Everything here is __forceinline__.
#pragma once
#include "kernels_device.h"

namespace jpgpu {

// K2: lanes of a wave decode block b of their MCU in lock-step into a shared LDS staging that is flushed per block as
// whole 128-byte lines of the coefficient buffer (zig-zag int16, MCU scan order).
//
// With 64 lanes in lock-step anything a lane does "rarely" happens in almost every iteration of the wave, so the symbol
// loop is written without per-lane state machines:
//  * the lane's bit source is a bit POSITION into a private 64-byte LDS ring of its unstuffed stream (17 words per lane:
//    16 ring words stored MSB-first + a mirror of word 0, so two consecutive words are always one ds_read2; stride 17
//    words keeps lanes on distinct banks).  Peeking 32 bits is bfe + address + ds_read2 + v_alignbit; consuming n bits is
//    one add.  The ring is topped up once per BLOCK (16 bytes, prefetched one block ahead into registers).
//  * one lookup of the next kK2LutBits bits returns total length (code + magnitude), code length, category and the
//    zig-zag advance in one 32-bit word; EOB and ZRL are ordinary entries whose "coefficient" is a zero stored where
//    nothing has been written yet, so the AC loop has no run/EOB branches.
//  * everything else -- codes longer than the lookup, the last bits of the interval where the reference's
//    "bits available" rules matter (JpegBitReader.cs:157-204), a ring that ran dry inside one block -- takes one
//    exec-masked exact path (k2_slow_symbol), the same decisions as ub_symbol.
constexpr int kK2RingStride = 68;                         // bytes per lane: 16 words + mirror of word 0
constexpr int kK2WaveBytes = 8192 + 64 * kK2RingStride;   // coefficient staging + rings
constexpr int kK2SmallBytes = 320;                        // maxcode[18] + valoffset[20] + values[256] + pad (round kernel's exact path)

// Lookups of the K2 family (K2, the K2S final pass), built once per upload for every table of the pool, as a DC and as an AC
// table (lut_pool_kernel), copied to LDS as they are:
//   L1  2^11 x u16, the next 11 bits:  AC  total bits | zig-zag advance << 6 | category << 12   (advance in coefficients: r + 1;
//                                          16 for any r != 0 with category 0; 63 = EOB, past the end from any position)
//                                      DC  total bits | category << 6
//                                      0 = not decided by 11 bits (a longer code); DC: 0x8000 = a category above 16
//   L2  256 x u16, the LONG codes:     entry j = the reference's maxcode walk on the 16 bits t16 + j, same format, 0 = no code.
//                                      Codes longer than the first level are the numerically largest ones of a canonical
//                                      table: for the standard tables the last 192 of the 65 536 16-bit values hold them all.
//                                      t16 = max(first value L1 does not decide, 65536 - 256).
//   header  t16
//   the reference's maxcode / valoffset / values (the exact walk: invalid codes, tables whose long codes leave the second level)
// Round 4: 32-bit entries took 34 KB of LDS for four tables and a long code cost the maxcode walk (six dependent LDS reads
// with 63 lanes waiting); now 19.8 KB, one more lookup for a long code, and the eleventh wave per workgroup.
// (Everything the symbol loop may touch stays in LDS: with the walk's arrays in global memory hipcc put a `s_waitcnt vmcnt(0)`
// at the head of the symbol loop -- every symbol waited for the previous block's coefficient stores: K2S final pass 7.8 -> 8.8 ms.)
constexpr int kK2LutBits = 11;
constexpr uint32_t kK2L1Bytes = 2u << kK2LutBits;
constexpr uint32_t kK2L2Entries = 256;
constexpr uint32_t kK2BadCat = 0x8000u;
constexpr uint32_t kK2TailBytes = 2u * kK2L2Entries + 16u + kK2SmallBytes;  // L2 | header | the reference's arrays
constexpr uint32_t kK2TabBytes = kK2L1Bytes + kK2TailBytes;  // the u16 image above (round 4-5 K2; still what the K2S ROUND kernel derives its lookups from)

// Round 6: the first level K2 and the K2S final pass keep in LDS carries the VALUES, and two symbols where two fit.
//   AC: 2^11 x u32, the next 11 bits;  DC: 2^9 x u32, the next 9 bits (the standard luminance DC codes end at 9 bits).
//   fast entry    n | nA << 4 | advA << 8 | advB << 14 | valA << 20 | valB << 26
//                 n = bits of everything the entry decodes (1..11), nA = bits of its FIRST symbol (code + magnitude), advA / advB =
//                 zig-zag advance of the first / second symbol in coefficients (r + 1; 16 for ZRL; 63 for EOB; advB = 0: the entry
//                 holds ONE symbol and valB = valA), valA / valB = the Extend()ed coefficients, six signed bits (categories 0..5:
//                 with the standard tables no longer symbol fits the index anyway).  A second symbol is only ever an AC symbol of the
//                 same table behind a first symbol that is not EOB; the lane checks that the first did not end the block.
//   medium entry  n = 0:  advA << 8 | category << 14 | (code + magnitude bits) << 19 -- the code fits the index, the magnitude does
//                 not (or is wider than six bits): one exec-masked stretch takes the value from the stream.
//   0x80000000    DC: a category above 16 (the exact path reports it);   0 = not decided by the index (a longer code: L2 / the walk).
// Image in the pool and in LDS: L1 | L2 (256 x u16, the old format: long codes) | header | the reference's arrays.
// Measured on the CPU before it was built (tools/microbench/k2_pairs/price_pairs_r06.txt): the wave's steps per block -- the
// longest of its 64 lanes' -- fall from 12.7 to 8.0 (Q75) and from 24.7 to 15.5 (Q90).
constexpr int kK2AcBits = 11, kK2DcBits = 9;
static_assert(kK2AcTabBytes == (4u << kK2AcBits) + kK2TailBytes && kK2DcTabBytes == (4u << kK2DcBits) + kK2TailBytes, "kernels.h holds the sizes for the host");
static_assert(kK2WaveLdsBytes == (uint32_t)kK2WaveBytes, "kernels.h holds the size for the host");
// pool, per table: the u16 images as an AC and as a DC table (round kernel), then the u32 images
constexpr uint32_t kPoolNewAc = 2u * kK2TabBytes, kPoolNewDc = kPoolNewAc + kK2AcTabBytes;
static_assert(kPoolNewDc + kK2DcTabBytes == kLutPoolBytesPerTable, "kernels.h sizes the pool");
constexpr uint32_t kK2MediumMask = 0xFFu;  // n | nA of an entry: zero = not a fast entry

struct K2Tab {
    const uint32_t *lut;
    const uint16_t *l2;
    const uint32_t *hdr;  // {t16, 0, 0, 0}
    const uint8_t *small;  // maxcode[18] | valoffset[20] | values[256]
    uint32_t shift;        // 32 - index bits
};

// off16: the table's LDS offset in 16-byte units (blk_info carries it: the images of a scan differ in size)
__device__ __forceinline__ K2Tab k2_tab_at(const uint8_t *tabs, uint32_t off16, bool is_dc) {
    const uint8_t *t = tabs + off16 * 16u;
    const uint32_t l1 = is_dc ? (4u << kK2DcBits) : (4u << kK2AcBits);
    K2Tab h;
    h.lut = reinterpret_cast<const uint32_t *>(t);
    h.l2 = reinterpret_cast<const uint16_t *>(t + l1);
    h.hdr = reinterpret_cast<const uint32_t *>(t + l1 + 2u * kK2L2Entries);
    h.small = t + l1 + 2u * kK2L2Entries + 16u;
    h.shift = is_dc ? 32u - kK2DcBits : 32u - kK2AcBits;
    return h;
}
// blk_info word: scan component | DC table offset << 8 | AC table offset << 20 (offsets in 16-byte units, 12 bits each)
__device__ __forceinline__ K2Tab k2_tab_dc(const uint8_t *tabs, uint32_t bi) { return k2_tab_at(tabs, (bi >> 8) & 0xFFFu, true); }
__device__ __forceinline__ K2Tab k2_tab_ac(const uint8_t *tabs, uint32_t bi) { return k2_tab_at(tabs, bi >> 20, false); }

// zig-zag advance (in int16 BYTES, i.e. 2 x coefficients) of an AC symbol: r + 1 coefficients for a non-zero category,
// 16 for ANY r != 0 with category 0 (ref: ...BaselineScanDecoder.cs:212-220), and "past the end" for EOB.
__device__ __forceinline__ uint32_t k2_ac_advance(uint32_t sym) {
    const uint32_t rr = sym >> 4;
    return (sym & 15u) ? 2u * (rr + 1u) : (rr ? 32u : 127u);
}

// next 32 bits of the lane's stream at bit position pm1 + 1
__device__ __forceinline__ uint32_t k2_window(const uint8_t *ring, int32_t pm1) {
    const uint32_t t = __builtin_amdgcn_ubfe((uint32_t)pm1, 5, 4);
    const uint32_t *p = reinterpret_cast<const uint32_t *>(ring + t * 4);
    return __builtin_amdgcn_alignbit(p[0], p[1], ~(uint32_t)pm1);
}

struct K2Feed {
    const uint8_t *gp;  // global address of the chunk after nx
    uint4 nx;           // chunk number `wr`, already loaded
    uint32_t wr;        // 16-byte chunks written to the ring so far (the ring holds chunks wr-4 .. wr-1)
};

__device__ __forceinline__ void k2_ring_write(uint8_t *ring, uint32_t slot, const uint4 &v) {
    uint32_t *rp = reinterpret_cast<uint32_t *>(ring + slot * 16);
    const uint32_t w0 = __builtin_bswap32(v.x);
    rp[0] = w0;
    rp[1] = __builtin_bswap32(v.y);
    rp[2] = __builtin_bswap32(v.z);
    rp[3] = __builtin_bswap32(v.w);
    if (slot == 0) reinterpret_cast<uint32_t *>(ring)[16] = w0;
}

// moves the prefetched chunk into the ring when the slot it replaces is no longer needed (the word before the current
// position must stay readable: k2_window reads it) and prefetches the next one
__device__ __forceinline__ void k2_topup(uint8_t *ring, K2Feed &f, int32_t pm1) {
    const int32_t rdc = (pm1 < 0 ? 0 : pm1) >> 7;
    if ((int32_t)f.wr < rdc + 4) {
        k2_ring_write(ring, f.wr & 3u, f.nx);
        f.wr++;
        __builtin_memcpy(&f.nx, f.gp, 16);
        f.gp += 16;
    }
}

// fast-path limit: a symbol of n bits at position pos may take the fast path when pos + n <= lim, which guarantees both
// "n real bits are available" and "the words the NEXT symbol reads (k2_symbol: up to 3 words past the one holding the bit
// before its position) are inside the ring"
__device__ __forceinline__ int32_t k2_limit(int32_t endpos, uint32_t wr) {
    const int32_t loaded = (int32_t)(wr * 128u) - 128;
    return endpos < loaded ? endpos : loaded;
}

// Exact symbol decode: DecodeHuffmanCode + ReceiveAndExtend with the reference's "bits available" rules (same decisions
// as ub_symbol).  ONE symbol, whatever the first-level entry holds.  Returns 0 or the failure detail; n = bits consumed, value,
// adv = zig-zag advance (AC, in coefficients).
__device__ __forceinline__ uint32_t k2_slow_symbol(uint8_t *ring, K2Feed &f, int32_t pm1, int32_t endpos, const K2Tab &h, bool is_dc,
                                                bool closed_by_marker, uint32_t &n, int32_t &value, uint32_t &adv) {
    const int32_t pos = pm1 + 1;
    while ((int32_t)(f.wr * 128u) < pos + 160) k2_topup(ring, f, pm1);  // always has room here
    const uint32_t hi = k2_window(ring, pm1);
    int32_t rem = endpos - pos;
    if (rem < 0) rem = 0;
    const uint32_t code16 = rem > 0 ? (hi >> 16) : 0xFFFFu;
    const uint32_t e = h.lut[code16 >> (h.shift - 16u)];
    uint32_t size, s;
    adv = 0;
    if ((e & 15u) != 0) {
        // a fast entry: its FIRST symbol.  The category of an Extend()ed value is the length of its magnitude.
        const int32_t va = (int32_t)__builtin_amdgcn_sbfe(e, 20, 6);
        s = va == 0 ? 0u : 32u - (uint32_t)__builtin_clz((uint32_t)(va < 0 ? -va : va));
        size = ((e >> 4) & 15u) - s;
        adv = (e >> 8) & 63u;
    } else if (e != 0 && (e >> 31) == 0) {  // the code fits the index, the magnitude does not
        s = (e >> 14) & 31u;
        size = ((e >> 19) & 63u) - s;
        adv = (e >> 8) & 63u;
    } else if (e != 0) {
        return kDetailInvalidHuffmanCode;  // DC categories above 16 are outside the verified envelope
    } else {
        uint32_t e2 = 0;
        const uint32_t t16 = h.hdr[0];
        if (code16 >= t16) {  // a long code: the second level (t16 >= 65536 - 256)
            e2 = h.l2[code16 - t16];
            if (is_dc && (e2 & kK2BadCat) != 0) return kDetailInvalidHuffmanCode;
        }
        if (e2 == 0) {
            // longer than the first level decides and not in the second: the reference's walk (an entry of the first level is empty
            // exactly when the code has more bits than the index, so the walk may start there)
            const uint16_t *maxcode = reinterpret_cast<const uint16_t *>(h.small);
            size = 33u - h.shift;
            while (code16 > maxcode[size]) size++;  // maxcode[17] = 0xFFFF terminates
            if (size > 16) return kDetailInvalidHuffmanCode;
            const uint32_t sym = h.small[56 + ((h.small[36 + size] + (code16 >> (16 - size))) & 0xFF)];
            s = is_dc ? sym : (sym & 15u);
            adv = (sym & 15u) ? (sym >> 4) + 1u : ((sym >> 4) ? 16u : 63u);
            if (s > 16u) return kDetailInvalidHuffmanCode;
        } else {
            s = is_dc ? ((e2 >> 6) & 31u) : (e2 >> 12);
            size = (e2 & 63u) - s;
            adv = (e2 >> 6) & 63u;
        }
    }
    rem = rem > (int32_t)size ? rem - (int32_t)size : 0;  // advance Math.Min(entry.CodeSize, bitsRead)
    value = 0;
    if (s != 0) {
        if ((int32_t)s > rem) return (rem == 0 && closed_by_marker) ? kDetailMarkerInData : kDetailStreamEnded;
        const int32_t v = (int32_t)__builtin_amdgcn_ubfe(hi, 32u - size - s, s);
        value = v - ((((v + v) >> s) - 1) & ((1 << s) - 1));  // Extend(v, nbits)
    }
    n = size + s;
    return 0;
}

// The lane's position and the three stream words around it: w0 holds the bit BEFORE the position (word q = pm1 >> 5),
// w1 and w2 follow.  A symbol is at most 32 bits, so q advances by at most one word per symbol; the word that would then
// be missing (q + 3) is read from the ring at the START of the step, off the dependency chain.
struct K2Pos {
    int32_t pm1;  // bit position - 1, relative to the lane's 4-byte aligned origin
    uint32_t w0, w1, w2;
};

__device__ __forceinline__ void k2_pos_init(K2Pos &p, const uint8_t *ring, int32_t pm1) {
    const uint32_t *r = reinterpret_cast<const uint32_t *>(ring);
    const int32_t q = pm1 >> 5;
    p.pm1 = pm1;
    p.w0 = r[q & 15];
    p.w1 = r[(q + 1) & 15];
    p.w2 = r[(q + 2) & 15];
}

// One STEP of a lane -- one symbol, or the two symbols of a pair entry --, fast path for every lane, then ONE branch the wave skips
// unless some lane needs more: a magnitude the index does not hold (medium), a long code (second level), the last bits of the
// interval, a ring that ran dry, a pair whose first symbol ended the block (exact path, one symbol); advances the position.
// i2 = 2 x zig-zag index of the next coefficient.  Out: ia = i2 + 2 x the first symbol's advance (the position behind it, in int16
// BYTES; EOB: past the end from any AC position), adv_b = the second symbol's advance in coefficients (0 and vb = va: one symbol).
// On failure the lane gets ia = i2 + 254 (leaves the AC loop), n = 0, values 0 and the detail code is ORed into `err` (touched on
// the exact path only: the fast path carries no instruction for it).
template <bool IS_DC>
__device__ __forceinline__ void k2_symbol(uint8_t *ring, K2Feed &f, K2Pos &p, int32_t endpos, int32_t &lim, const K2Tab &h, bool closed_by_marker,
                                          uint32_t i2, int32_t &va, int32_t &vb, uint32_t &ia, uint32_t &adv_b, uint32_t &err) {
    const uint32_t nxt = *reinterpret_cast<const uint32_t *>(ring + __builtin_amdgcn_ubfe((uint32_t)(p.pm1 + 96), 5, 4) * 4);
    const uint32_t hi = __builtin_amdgcn_alignbit(p.w0, p.w1, ~(uint32_t)p.pm1);
    // (the index as a shift by the table kind's constant and one shift-add for the address: hipcc's own form -- shift, mask, add --
    // is one instruction longer; the empty asm keeps it from folding the two shifts)
    uint32_t idx = hi >> (IS_DC ? 32u - kK2DcBits : 32u - kK2AcBits);
    asm volatile("" : "+v"(idx));
    const uint32_t e = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(h.lut) + idx * 4u);
    uint32_t n = e & 15u;
    va = (int32_t)__builtin_amdgcn_sbfe(e, 20, 6);
    vb = (int32_t)e >> 26;
    ia = IS_DC ? i2 : i2 + 2u * __builtin_amdgcn_ubfe(e, 8, 6);
    adv_b = IS_DC ? 0u : __builtin_amdgcn_ubfe(e, 14, 6);
    // slow: not a fast entry (n - 1 is negative), the step does not fit below the limit, or a pair whose first symbol ends the
    // block (ia >= 128 with a second symbol behind it: that symbol is the next block's) -- one signed test
    const int32_t room = lim - (p.pm1 + 1) - (int32_t)n;
    const uint32_t pair_end = IS_DC ? 0u : ((127u - ia) & (0u - adv_b));
    const bool slow = (int32_t)((n - 1u) | (uint32_t)room | pair_end) < 0;
    if (slow) {  // exec-masked; the wave skips it when no lane is flagged
        const uint32_t ntot = (e >> 19) & 63u;
        if (n == 0 && (int32_t)e > 0 && lim - (p.pm1 + 1) - (int32_t)ntot >= 0) {
            // medium: the code fits the index, the magnitude comes from the stream (Extend(v, nbits)); its advance is where a fast entry's is
            const uint32_t cat = (e >> 14) & 31u;
            const int32_t raw = (int32_t)__builtin_amdgcn_ubfe(hi, 32u - ntot, cat);
            va = vb = raw - ((((raw + raw) >> cat) - 1) & ((1 << cat) - 1));
            n = ntot;
            adv_b = 0;
        } else {
            uint32_t adv = 0;
            const uint32_t e1 = k2_slow_symbol(ring, f, p.pm1, endpos, h, IS_DC, closed_by_marker, n, va, adv);
            vb = va;
            ia = i2 + adv * 2u;
            adv_b = 0;
            lim = k2_limit(endpos, f.wr);
            if (e1 != 0) {
                err |= e1;
                n = 0;
                va = vb = 0;
                ia = i2 + 254u;
            }
        }
    }
    const int32_t np = p.pm1 + (int32_t)n;
    const bool step = ((uint32_t)(np ^ p.pm1) >> 5) != 0;
    p.pm1 = np;
    p.w0 = step ? p.w1 : p.w0;
    p.w1 = step ? p.w2 : p.w1;
    p.w2 = step ? nxt : p.w2;
}
// (ONE symbol, the table kind known only per lane: the K2S final pass on its way to its first MCU)
__device__ __forceinline__ uint32_t k2_symbol_any(uint8_t *ring, K2Feed &f, K2Pos &p, int32_t endpos, int32_t &lim, const K2Tab &h, bool is_dc,
                                                  bool closed_by_marker, int32_t &value, uint32_t &adv2) {
    const uint32_t nxt = *reinterpret_cast<const uint32_t *>(ring + __builtin_amdgcn_ubfe((uint32_t)(p.pm1 + 96), 5, 4) * 4);
    const uint32_t hi = __builtin_amdgcn_alignbit(p.w0, p.w1, ~(uint32_t)p.pm1);
    const uint32_t e = h.lut[hi >> h.shift];
    uint32_t n = (e & 15u) != 0 ? ((e >> 4) & 15u) : 0u;  // the entry's first symbol
    value = (int32_t)__builtin_amdgcn_sbfe(e, 20, 6);
    adv2 = is_dc ? 0u : ((e >> 7) & 0x7Eu);
    uint32_t err = 0;
    const bool slow = (int32_t)((n - 1u) | (uint32_t)(lim - (p.pm1 + 1) - (int32_t)n)) < 0;
    if (slow) {
        uint32_t adv = 0;
        err = k2_slow_symbol(ring, f, p.pm1, endpos, h, is_dc, closed_by_marker, n, value, adv);
        adv2 = is_dc ? 0u : adv * 2u;
        lim = k2_limit(endpos, f.wr);
        if (err != 0) {
            n = 0;
            value = 0;
            adv2 = 254;
        }
    }
    const int32_t np = p.pm1 + (int32_t)n;
    const bool step = ((uint32_t)(np ^ p.pm1) >> 5) != 0;
    p.pm1 = np;
    p.w0 = step ? p.w1 : p.w0;
    p.w1 = step ? p.w2 : p.w1;
    p.w2 = step ? nxt : p.w2;
    return err;
}

// The K2 family's lookups (format above) for every table of the pool, as a DC table (odd blocks) and as an AC table.
// Image (table * 2 + is_dc) * kK2TabBytes: L1 | L2 | header.
constexpr int kLutPoolBits = kK2LutBits;
__device__ __forceinline__ uint32_t k2_entry_of(const DevHuffTable &h, uint32_t code16, bool is_dc, uint32_t max_size) {
    // the reference's Lookup on these 16 bits (JpegHuffmanDecodingTable.cs:73-113): first-level table, then the maxcode walk
    const uint32_t e9 = h.lut[code16 >> (16 - kHuffLutBits)];
    uint32_t size = e9 >> 8, sym = e9 & 0xFFu;
    if (size == 0) {
        size = kHuffLutBits + 1;
        while (code16 > h.maxcode[size]) size++;  // maxcode[17] = 0xFFFF terminates
        if (size > 16) return 0;
        sym = h.values[(h.valoffset[size] + (code16 >> (16 - size))) & 0xFF];
    }
    if (size > max_size) return 0;
    const uint32_t cat = is_dc ? sym : (sym & 15u);
    if (cat > 16u) return kK2BadCat;  // (the exact path reports it)
    if (is_dc) return (size + cat) | (cat << 6);
    const uint32_t adv = (sym & 15u) ? (sym >> 4) + 1u : ((sym >> 4) ? 16u : 63u);
    return (size + cat) | (adv << 6) | (cat << 12);
}
// First-level entry `idx` of the u32 lookup (format at kK2AcBits): the reference's Lookup on the index bits with ones behind them,
// then -- AC, first symbol not EOB -- once more on what the first symbol left of the index.
__device__ __forceinline__ uint32_t k2_fast_entry(const DevHuffTable &h, uint32_t idx, bool is_dc, uint32_t lb) {
    const uint32_t ones = (1u << (16u - lb)) - 1u;
    const uint32_t a = k2_entry_of(h, (idx << (16u - lb)) | ones, is_dc, lb);
    if (a == 0) return 0;
    if (is_dc && (a & kK2BadCat) != 0) return 0x80000000u;
    const uint32_t na = a & 63u, cat_a = is_dc ? ((a >> 6) & 31u) : (a >> 12), adv_a = is_dc ? 0u : ((a >> 6) & 63u);
    if (na > lb || cat_a > 5u) return (adv_a << 8) | (cat_a << 14) | (na << 19);  // medium
    const int32_t raw_a = (int32_t)((idx >> (lb - na)) & ((1u << cat_a) - 1u));
    const int32_t va = cat_a ? raw_a - ((((raw_a + raw_a) >> cat_a) - 1) & ((1 << cat_a) - 1)) : 0;
    uint32_t n = na, adv_b = 0;
    int32_t vb = va;
    if (!is_dc && adv_a != 63u && na < lb) {
        const uint32_t rem = lb - na;
        const uint32_t idx_b = ((idx << na) | ((1u << na) - 1u)) & ((1u << lb) - 1u);
        const uint32_t b = k2_entry_of(h, (idx_b << (16u - lb)) | ones, false, rem);
        if (b != 0) {
            const uint32_t nb = b & 63u, cat_b = b >> 12;
            if (nb <= rem && cat_b <= 5u) {
                const int32_t raw_b = (int32_t)((idx_b >> (lb - nb)) & ((1u << cat_b) - 1u));
                vb = cat_b ? raw_b - ((((raw_b + raw_b) >> cat_b) - 1) & ((1 << cat_b) - 1)) : 0;
                adv_b = (b >> 6) & 63u;
                n = na + nb;
            }
        }
    }
    return n | (na << 4) | (adv_a << 8) | (adv_b << 14) | (((uint32_t)va & 63u) << 20) | (((uint32_t)vb & 63u) << 26);
}
// the scan's tables as the K2 family keeps them in LDS: the pooled u32 images (lut_pool_kernel) copied as they are, one behind the other
__device__ __forceinline__ void k2_stage_scan_tables(const DevScan &s, const uint8_t *lut_pool, uint8_t *tabs, uint32_t *blk_info, int n_slots,
                                                     uint32_t nthreads) {
    const uint32_t tid = threadIdx.x;
    uint32_t off = 0, off16[kMaxHuffSlots];
#pragma unroll
    for (int sl = 0; sl < kMaxHuffSlots; sl++) {
        off16[sl] = off >> 4;
        if (sl >= n_slots) continue;
        const uint32_t pi = s.huff_pool[sl];
        if (pi == 0xFFFF) continue;
        bool is_dc = false;
        for (int c = 0; c < s.scan_components; c++) is_dc |= s.comp[c].dc_slot == sl;
        const uint32_t bytes = is_dc ? kK2DcTabBytes : kK2AcTabBytes;
        const uint4 *src = reinterpret_cast<const uint4 *>(lut_pool + (size_t)pi * kLutPoolBytesPerTable + (is_dc ? kPoolNewDc : kPoolNewAc));
        uint4 *dst = reinterpret_cast<uint4 *>(tabs + off);
        for (uint32_t i = tid; i < bytes / 16; i += nthreads) dst[i] = src[i];
        off += bytes;
    }
    // per block-in-MCU: scan component | DC table offset << 8 | AC table offset << 20 (kept in LDS: the block loop must not touch
    // global memory for it, a vector load there would wait for the coefficient stores of the previous block)
    if (tid < kMaxBlocksPerMcu) {
        const uint32_t ci = s.blk_comp[tid];
        uint32_t dc = 0, ac = 0;
#pragma unroll
        for (int sl = 0; sl < kMaxHuffSlots; sl++) {
            dc = s.comp[ci].dc_slot == sl ? off16[sl] : dc;
            ac = s.comp[ci].ac_slot == sl ? off16[sl] : ac;
        }
        blk_info[tid] = ci | (dc << 8) | (ac << 20);
    }
}

// A lane's stream positioned at bit `bit` (0..7, MSB first) of byte u0 of the scan's unstuffed data, with n_bits of data from there
// on: K2's ring + feed + position (64 bytes staged, the next 16 prefetched).  Returns pm1 of the start; *endpos = position of the
// first bit behind the data.  (The start as byte and bit, not as one bit number: a scan of restart intervals may be longer than
// 2^32 bits; the lane's own data, n_bits, may not.)
__device__ __forceinline__ int32_t k2_open_at_bit(const uint8_t *ubase, uint32_t u0, uint32_t bit, uint32_t n_bits, uint8_t *ring, K2Feed &feed,
                                                  K2Pos &pos, int32_t *endpos) {
    const int32_t pm1_0 = (int32_t)((u0 & 3u) * 8u + bit) - 1;
    *endpos = pm1_0 + 1 + (int32_t)n_bits;
    const uint8_t *g = ubase + (u0 & ~3u);  // 4-byte aligned 16-byte loads; buffers are padded
    uint4 c0, c1, c2, c3;
    __builtin_memcpy(&c0, g, 16);
    __builtin_memcpy(&c1, g + 16, 16);
    __builtin_memcpy(&c2, g + 32, 16);
    __builtin_memcpy(&c3, g + 48, 16);
    __builtin_memcpy(&feed.nx, g + 64, 16);
    k2_ring_write(ring, 0, c0);
    k2_ring_write(ring, 1, c1);
    k2_ring_write(ring, 2, c2);
    k2_ring_write(ring, 3, c3);
    feed.wr = 4;
    feed.gp = g + 80;
    k2_pos_init(pos, ring, pm1_0);
    return pm1_0;
}

// ReadBlockBaseline (ref: ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:179-222) of one lane, in two pieces: k2_decode_dc reads the DC
// symbol and returns the coefficient, k2_decode_ac stores it (zig-zag index 0) and runs the AC loop.  my_stage = the lane's 128
// staged bytes, swz16 = the XOR swizzle of their 16-byte chunks.
//
// The DC predictor comes in BY VALUE and the new one is returned: the caller keeps its four predictors in four named registers and
// does the select and the write-back itself, BETWEEN the two calls.  Do not fold the pieces together:
//  * one helper that takes the four predictors by reference makes hipcc turn them into an indexed private array: 20 bytes of scratch
//    per lane and scratch loads and stores in the block loop of every kernel -- while the VGPR count goes DOWN by six, which looks
//    like a gain (tests/test_k2_family_isa_cpu.py pins the count from both sides for that reason);
//  * one helper that returns the DC value behind the AC loop moves the predictor's write-back behind the loop: 14 more instructions
//    per kernel.
// (The store of index 0 is the AC piece's: behind the write-back, where it always was.  In the DC piece -- in front of the
// write-back -- hipcc schedules the tail of the symbol loop differently: the same opcodes, the position words' selects later.)
__device__ __forceinline__ int32_t k2_decode_dc(uint8_t *ring, K2Feed &feed, K2Pos &pos, int32_t endpos, int32_t &lim, const K2Tab &hdc,
                                                bool closed_by_marker, int32_t pred, uint32_t &err) {
    int32_t v, vb;
    uint32_t ia = 0, adv_b = 0;
    k2_symbol<true>(ring, feed, pos, endpos, lim, hdc, closed_by_marker, 0u, v, vb, ia, adv_b, err);
    return v + pred;
}
__device__ __forceinline__ void k2_decode_ac(uint8_t *ring, K2Feed &feed, K2Pos &pos, int32_t endpos, int32_t &lim, const K2Tab &hac,
                                             bool closed_by_marker, int32_t dc, uint8_t *my_stage, uint32_t swz16, uint32_t &err) {
    int32_t v, vb;
    uint32_t ia = 0, adv_b = 0;
    *reinterpret_cast<int16_t *>(my_stage + swz16) = (int16_t)dc;  // zig-zag index 0
    uint32_t i2 = err == 0 ? 2u : 128u;  // 2 x zig-zag index of the next coefficient
    while (i2 < 128u) {
        // one step = one symbol or, where the lookup held two, both (round 6): Math.Min(i++, 63) for a coefficient; EOB /
        // ZRL store a zero at a position nothing was written to yet; a step of one symbol stores it twice
        k2_symbol<false>(ring, feed, pos, endpos, lim, hac, closed_by_marker, i2, v, vb, ia, adv_b, err);
        const uint32_t at = ia - 2u < 126u ? ia - 2u : 126u;
        *reinterpret_cast<int16_t *>(my_stage + (at ^ swz16)) = (int16_t)v;
        i2 = ia + 2u * adv_b;
        const uint32_t at_b = i2 - 2u < 126u ? i2 - 2u : 126u;
        *reinterpret_cast<int16_t *>(my_stage + (at_b ^ swz16)) = (int16_t)vb;
    }
}

// what the lanes staged is visible to the whole wave behind this, and what they read is read in front of it
__device__ __forceinline__ void k2_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Flush the wave's 64 staged blocks to the coefficient buffer as whole 128-byte lines and re-zero the staging: lane (blk, chunk) of
// pass `it` moves 16 bytes of the block staged by lane blk.  where(blk, dst): whether lane blk's block of this step exists, and if so
// dst = its first coefficient in the buffer.
template <class Where>
__device__ __forceinline__ void k2_flush_dense(uint8_t *stage, uint32_t lane, Where where) {
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const uint32_t blk = it * 8 + (lane >> 3);
        const uint32_t chunk = lane & 7;
        uint4 *src = reinterpret_cast<uint4 *>(stage + blk * 128 + ((chunk ^ ((blk >> 1) & 7)) * 16));
        const uint4 v = *src;
        const uint4 z = {0, 0, 0, 0};
        *src = z;
        int16_t *dst = nullptr;
        if (where(blk, dst)) *reinterpret_cast<uint4 *>(dst + chunk * 8) = v;
    }
}

// A workgroup's dynamic LDS: the staged tables (tab_bytes: the batch's largest set) | per wave kK2WaveBytes | blk_info[kMaxBlocksPerMcu]
struct K2Group {
    uint8_t *tabs;
    uint32_t *blk_info;
    uint8_t *stage;  // this wave's coefficient staging (8 KB), zero
    uint8_t *ring;   // this lane's ring
};
// stages scan s's tables (ref: InitDecodeComponents resolves them per scan, JpegHuffmanScanDecoder.cs:63-64), zeroes the wave's staging;
// every thread of the workgroup (nthreads of them) must come here
__device__ __forceinline__ K2Group k2_group_setup(uint8_t *smem, uint32_t tab_bytes, uint32_t nthreads, const DevScan &s, const uint8_t *lut_pool,
                                                  int n_slots) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t *wave_all = smem + tab_bytes;
    K2Group g;
    g.tabs = smem;
    g.blk_info = reinterpret_cast<uint32_t *>(wave_all + (nthreads >> 6) * kK2WaveBytes);
    k2_stage_scan_tables(s, lut_pool, g.tabs, g.blk_info, n_slots, nthreads);
    g.stage = wave_all + wave * kK2WaveBytes;
    g.ring = g.stage + 8192 + lane * kK2RingStride;
    const uint4 z = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 8; i++) reinterpret_cast<uint4 *>(g.stage)[i * 64 + lane] = z;
    __syncthreads();
    return g;
}

// A pooled wave's next chunk (wave-uniform): the counter is never cleared, `base` = the tickets drawn from it before this launch.
// A launch draws n_chunks + (waves launched) tickets, every wave exactly one beyond the end.
// (Drawing the ticket of the NEXT chunk before starting on the one in hand was measured and lost: tools/microbench/k2_ticket_ahead/.)
__device__ __forceinline__ uint32_t k2_next_ticket(uint32_t *counter, uint32_t base, uint32_t lane) {
    uint32_t c = 0;
    if (lane == 0) c = atomicAdd(counter, 1u) - base;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
}

// Per-wave cycle counters (tools/trace/k2_phases.py), in builds with -DJPGPU_K2_PROFILE only: K2_PROF_DEFINE(array, export) defines
// eight counters and the C function that reads (and clears) them; K2_PROF_ADD adds to one from lane 0 (a `lane` must be in scope).
#ifdef JPGPU_K2_PROFILE
#define K2_TICK() __builtin_readcyclecounter()
#define K2_PROF_ADD(array, i, v) do { if (lane == 0) atomicAdd(&array[i], (unsigned long long)(v)); } while (0)
#define K2_PROF_DEFINE(array, export_name)                                                                                              \
    __device__ unsigned long long array[8];                                                                                             \
    extern "C" int export_name(unsigned long long *out, int reset) {                                                                    \
        if (hipMemcpyFromSymbol(out, HIP_SYMBOL(array), sizeof(array)) != hipSuccess) return 1;                                         \
        if (reset) { unsigned long long z[8] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(array), z, sizeof z) != hipSuccess) return 1; }    \
        return 0;                                                                                                                       \
    }
#else
#define K2_TICK() 0ull
#define K2_PROF_ADD(array, i, v) do { (void)(v); } while (0)
#define K2_PROF_DEFINE(array, export_name)
#endif

}  // namespace jpgpu
