// jpeglibrary_amd/csrc/kernels_device.h -- device-side helpers shared by the kernel translation units (k1_markers.hip,
// k2_huffman.hip, k2s_subseq.hip, k2p_progressive.hip, k3_idct.hip, kt_transcode.hip): wave primitives, the unstuffed bit reader
// (UBits, LdsHuff, ub_*), the restart check and the fail-block word, the subsequence state word and table staging (sub_*), the
// dynamic-LDS allowance.  Everything here is __forceinline__.  What only K2 and the K2S final pass use -- the LDS ring, the u32
// lookups, the symbol step, the block decode, the flush -- is in k2_wave.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "common.h"
#include "kernels.h"

namespace jpgpu {

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

__device__ __forceinline__ uint32_t wave_reduce_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_reduce_max_i(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        int32_t t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return (uint32_t)v;
}
// DPP forms of the wave-wide sums (all 64 lanes must be active): data-parallel-primitive operands move values between lanes
// inside the VALU, no LDS crossbar round trip per step as with ds_bpermute (__shfl_*).  Control codes: row_shr:n = 0x110 + n,
// row_bcast:15 = 0x142, row_bcast:31 = 0x143, wave_shl:1 = 0x130, wave_shr:1 = 0x138; lanes without a source receive 0.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint32_t dpp0(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    v += dpp0<0x111>(v);       // inside each row of 16 lanes
    v += dpp0<0x112>(v);
    v += dpp0<0x114>(v);
    v += dpp0<0x118>(v);
    v += dpp0<0x142, 0xA>(v);  // rows 1 and 3 take the total of the row before them
    v += dpp0<0x143, 0xC>(v);  // rows 2 and 3 take the total of rows 0-1
    return v;
}
// sum over the wave, the same value in every lane (as a scalar)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(v), 63);
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t lane_get(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint32_t lane_put(uint32_t old, uint32_t v, uint32_t l) {
    // (no clang builtin for v_writelane in ROCm 7.2, and two scalar operands need M0 on gfx9; this runs once per long code:
    // a compare and a select instead of hand-written M0 traffic)
    return __lane_id() == l ? v : old;
}


// Bit source of one lane == a fresh JpegBitReader positioned at the start of its restart interval (ref: JpegBitReader.cs),
// reading the UNSTUFFED copy written by K1: interval bytes [ustart, uend) followed by at least 16 one-bits.
//   hi   : the next 32 bits of the stream (bit 31 first), always fully valid after ub_consume
//   lo   : the bits after them, left aligned, lcnt of them valid (low bits zero)
//   rem  : real data bits left in the interval == the reference's "bits available"; reads past them see the ones
//          padding, which is exactly PeekBits(16)'s padding (JpegBitReader.cs:163-167); once rem is 0 every peek is 0xFFFF
// Words come from a register queue of 2 x 16 bytes (qw current, nx prefetched a whole chunk ahead: memory latency is off
// the critical path).  All arithmetic is 32-bit.
struct UBits {
    const uint8_t *p;  // address of the next 16-byte chunk to prefetch
    uint4 qw, nx;
    uint32_t qn;
    uint32_t hi, lo;
    int32_t lcnt;
    int32_t rem;
};

__device__ __forceinline__ uint32_t ub_next_word(UBits &r) {
    const uint32_t w = r.qw.x;
    r.qw.x = r.qw.y;
    r.qw.y = r.qw.z;
    r.qw.z = r.qw.w;
    r.qn--;
    if (r.qn == 0) {
        r.qw = r.nx;
        __builtin_memcpy(&r.nx, r.p, 16);  // 4-byte aligned 16-byte load; buffers are padded
        r.p += 16;
        r.qn = 4;
    }
    return __builtin_bswap32(w);
}

// consume n bits, 1 <= n <= 32
__device__ __forceinline__ void ub_consume(UBits &r, uint32_t n) {
    r.hi = __builtin_amdgcn_alignbit(r.hi, r.lo, (32u - n) & 31u);  // n == 32 -> lo
    r.lo = n >= 32u ? 0u : (r.lo << n);
    r.lcnt -= (int32_t)n;
    if (r.lcnt < 0) {
        const uint32_t d = (uint32_t)(-r.lcnt);  // 1..32 low bits of hi are missing
        const uint32_t w = ub_next_word(r);
        r.hi |= w >> ((32u - d) & 31u);  // d == 32 -> w
        r.lo = d >= 32u ? 0u : (w << d);
        r.lcnt = 32 - (int32_t)d;
    }
}

__device__ __forceinline__ void ub_init(UBits &r, const uint8_t *ubase, uint32_t ustart, uint32_t uend) {
    const uint32_t a = ustart & ~3u;
    __builtin_memcpy(&r.qw, ubase + a, 16);
    __builtin_memcpy(&r.nx, ubase + a + 16, 16);
    r.p = ubase + a + 32;
    r.qn = 4;
    r.hi = ub_next_word(r);
    r.lo = ub_next_word(r);
    r.lcnt = 32;
    const uint32_t skip = (ustart & 3u) * 8;
    if (skip) ub_consume(r, skip);
    r.rem = (int32_t)((uend - ustart) * 8u);
}

// LDS image of a staged DevHuffTable
struct LdsHuff {
    const uint16_t *lut;
    const uint16_t *maxcode;
    const uint8_t *valoffset;
    const uint8_t *values;
};

__device__ __forceinline__ LdsHuff lds_huff(const uint8_t *tabs, uint32_t slot) {
    const uint8_t *t = tabs + slot * sizeof(DevHuffTable);
    LdsHuff h;
    h.lut = reinterpret_cast<const uint16_t *>(t);
    h.maxcode = reinterpret_cast<const uint16_t *>(t + offsetof(DevHuffTable, maxcode));
    h.valoffset = t + offsetof(DevHuffTable, valoffset);
    h.values = t + offsetof(DevHuffTable, values);
    return h;
}

__device__ __forceinline__ LdsHuff lds_huff16(const uint8_t *tabs, uint32_t off16) {
    const uint8_t *t = tabs + off16 * 16;
    LdsHuff h;
    h.lut = reinterpret_cast<const uint16_t *>(t);
    h.maxcode = reinterpret_cast<const uint16_t *>(t + offsetof(DevHuffTable, maxcode));
    h.valoffset = t + offsetof(DevHuffTable, valoffset);
    h.values = t + offsetof(DevHuffTable, values);
    return h;
}

// One Huffman symbol and its magnitude bits:
//   DecodeHuffmanCode (ref: ScanDecoder/JpegHuffmanScanDecoder.cs:81-88, JpegHuffmanDecodingTable.cs:73-113) followed by
//   ReceiveAndExtend (ref: ScanDecoder/JpegHuffmanScanDecoder.cs:100-115) when the category s is non-zero
//   (s = sym for a DC symbol, sym & 15 for an AC symbol).
// Returns 0, or the failure detail.  value = extended magnitude (0 when s == 0).
template <class R>
__device__ __forceinline__ uint32_t ub_symbol(R &r, const LdsHuff &h, bool is_dc, bool closed_by_marker, uint32_t &sym_out,
                                              int32_t &value) {
    const uint32_t code16 = r.rem > 0 ? (r.hi >> 16) : 0xFFFFu;
    const uint32_t e = h.lut[code16 >> (16 - kHuffLutBits)];
    uint32_t size = e >> 8, sym = e & 0xFF;
    if (size == 0) {
        size = kHuffLutBits + 1;
        while (code16 > h.maxcode[size]) size++;  // maxcode[17] = 0xFFFF terminates
        if (size > 16) return kDetailInvalidHuffmanCode;
        sym = h.values[(h.valoffset[size] + (code16 >> (16 - size))) & 0xFF];
    }
    sym_out = sym;
    const uint32_t s = is_dc ? sym : (sym & 15u);
    // advance Math.Min(entry.CodeSize, bitsRead)
    r.rem = r.rem > (int32_t)size ? r.rem - (int32_t)size : 0;
    value = 0;
    if (s != 0) {
        if (s > 16u) return kDetailInvalidHuffmanCode;  // categories above 16 are outside the verified envelope
        if ((int32_t)s > r.rem) return (r.rem == 0 && closed_by_marker) ? kDetailMarkerInData : kDetailStreamEnded;
        const int32_t v = (int32_t)__builtin_amdgcn_ubfe(r.hi, 32u - size - s, s);
        value = v - ((((v + v) >> s) - 1) & ((1 << s) - 1));  // Extend(v, nbits)
        r.rem -= (int32_t)s;
    }
    ub_consume(r, size + s);
    return 0;
}

// LDS staging of one wave: 64 blocks x 128 B, 16-byte chunks XOR-swizzled so that both the per-lane
// scattered 2-byte stores and the block-major 16-byte flush reads are (nearly) bank-conflict free.
__device__ __forceinline__ uint32_t stage_addr(uint32_t blk, uint32_t coef_index) {
    const uint32_t chunk = (coef_index >> 3) ^ ((blk >> 1) & 7);
    return blk * 128 + chunk * 16 + (coef_index & 7) * 2;
}

// DevScanStatus::pad[1] of a sequential scan that fails in block `block` (scan order); see common.h
__device__ __forceinline__ uint32_t fail_block_word(uint64_t block) { return kFailBlockBase - (uint32_t)(block < 0xFFFFFFF0ull ? block : 0xFFFFFFF0ull); }

// Restart check after an interval (ref: ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:139-163): runs after every completed
// interval except a final partial one.  AdvanceAlignByte + TryReadMarker: no whole byte may be left before the closing
// marker, and the marker must be RSTn (continue) or EOI (return early).  Returns the error code word or kNoError.
__device__ __forceinline__ uint32_t restart_check(const DevScan &s, const DevScanStatus &st, DevScanStatus *status_out, uint32_t interval,
                                                  uint32_t n_ends, uint32_t n_intervals, uint32_t dri_eff, int32_t rem, uint32_t err) {
    if (err != 0) return (interval << 8) | err;
    // bits left behind the scan's last block when the scan's terminating marker closes that interval: the host needs the
    // whole bytes among them for the reader position the reference resumes its marker walk from (:167-176)
    if (interval == n_intervals - 1) status_out->pad[2] = rem > 0 ? (uint32_t)rem : 0u;
    const bool needs_check = s.dri != 0 && (interval < n_intervals - 1 || s.restart_check_at_end);
    if (!needs_check) return kNoError;
    uint32_t closing = 0xD0;  // entries before the last indexed one are RSTn by construction
    if (interval == n_ends - 1) closing = st.terminator;
    // "Expect restart marker." is thrown behind the interval's last MCU: every block of the interval has reached the writer
    const uint32_t behind = fail_block_word((uint64_t)(interval + 1) * dri_eff * s.blocks_per_mcu);
    const bool sequential = s.kind == kScanSequential;  // (a progressive scan's pad[1] is its progress word)
    if (rem >= 8) {
        if (sequential) atomicMax(&status_out->pad[1], behind);
        return (interval << 8) | kDetailExpectRestart;
    }
    if (closing == 0xD9) {
        if (interval < n_intervals - 1) atomicMin(&status_out->decoded_mcus, (interval + 1) * dri_eff);
        return kNoError;
    }
    if ((closing & 0xF8) != 0xD0) {
        if (sequential) atomicMax(&status_out->pad[1], behind);
        return (interval << 8) | kDetailExpectRestart;
    }
    return kNoError;
}

// DecodeHuffmanCode alone (ref: ScanDecoder/JpegHuffmanScanDecoder.cs:81-88): the symbol, no magnitude bits.
template <class R>
__device__ __forceinline__ uint32_t ub_huff(R &r, const LdsHuff &h, uint32_t &sym_out) {
    const uint32_t code16 = r.rem > 0 ? (r.hi >> 16) : 0xFFFFu;
    const uint32_t e = h.lut[code16 >> (16 - kHuffLutBits)];
    uint32_t size = e >> 8, sym = e & 0xFF;
    if (size == 0) {
        size = kHuffLutBits + 1;
        while (code16 > h.maxcode[size]) size++;  // maxcode[17] = 0xFFFF terminates
        if (size > 16) return kDetailInvalidHuffmanCode;
        sym = h.values[(h.valoffset[size] + (code16 >> (16 - size))) & 0xFF];
    }
    sym_out = sym;
    r.rem = r.rem > (int32_t)size ? r.rem - (int32_t)size : 0;  // advance Math.Min(entry.CodeSize, bitsRead)
    ub_consume(r, size);
    return 0;
}

// TryReadBits(n), 1 <= n <= 16 (ref: JpegBitReader.cs:190-204): false when fewer than n bits are left
template <class R>
__device__ __forceinline__ bool ub_try_read_bits(R &r, uint32_t n, uint32_t &bits) {
    if ((int32_t)n > r.rem) return false;
    bits = r.hi >> (32u - n);
    r.rem -= (int32_t)n;
    ub_consume(r, n);
    return true;
}

// subsequence length: (1 << DevScan::sub_shift) bits -- 1024 for small batches (more lanes), up to 4096 for large ones (a
// longer subsequence re-synchronises more often inside itself: fewer rounds until the exit states stop changing)
constexpr uint32_t kSubBad = 0x80000000u;  // the lane hit an invalid code / ran out of data under its entry state

// exit state word: overshoot (bits past the nominal end, 0..63) | b << 6 | k << 11 | kSubBad
__device__ __forceinline__ uint32_t sub_pack(uint32_t overshoot, uint32_t b, uint32_t k) { return overshoot | (b << 6) | (k << 11); }

__device__ __forceinline__ void sub_stage_tables(const DevScan &s, const DevHuffTable *huff_pool, uint8_t *tabs, uint32_t *blk_info, int n_slots,
                                                 uint32_t nthreads) {
    const uint32_t tid = threadIdx.x;
    for (int slot = 0; slot < kMaxHuffSlots && slot < n_slots; slot++) {
        const uint32_t pi = s.huff_pool[slot];
        if (pi == 0xFFFF) continue;
        const uint4 *src = reinterpret_cast<const uint4 *>(&huff_pool[pi]);
        uint4 *dst = reinterpret_cast<uint4 *>(tabs + slot * sizeof(DevHuffTable));
        for (uint32_t i = tid; i < sizeof(DevHuffTable) / 16; i += nthreads) dst[i] = src[i];
    }
    if (tid < kMaxBlocksPerMcu) {
        const uint32_t ci = s.blk_comp[tid];
        const uint32_t dc_off = s.comp[ci].dc_slot * (uint32_t)(sizeof(DevHuffTable) / 16);
        const uint32_t ac_off = s.comp[ci].ac_slot * (uint32_t)(sizeof(DevHuffTable) / 16);
        blk_info[tid] = dc_off | (ac_off << 12) | (ci << 24);
    }
    __syncthreads();
}

// More than 64 KB of dynamic LDS has to be allowed per kernel -- and per DEVICE: a process that drives several devices (one
// jpgpu_ctx each) must do it on each of them.  done: one bit per device ordinal.
static inline hipError_t allow_dynamic_lds(const void *kernel, int bytes, std::atomic<uint64_t> &done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    done.fetch_or(bit, std::memory_order_release);
    return hipSuccess;
}

}  // namespace jpgpu
