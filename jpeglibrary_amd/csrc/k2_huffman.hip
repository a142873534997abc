// jpeglibrary_amd/csrc/k2_huffman.hip -- K2: Huffman MCU decode, one lane per restart interval; the pooled lookups (lut_pool_kernel)
//
// MUST be compiled with -ffp-contract=off: the reference's Vector4 arithmetic never fuses a*b+c
// (FastFloatingPointDCT.cs:79-185).  No fast-math.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "encode_kernels.h"
#include "kernels_device.h"
#include "k2_wave.h"

namespace jpgpu {

// ------------------------------------------------------------------------------------------------
// K2: Huffman MCU decode.  One lane per restart interval.
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void lut_pool_kernel(const DevHuffTable *__restrict__ pool, uint8_t *__restrict__ lut_pool) {
    const DevHuffTable &h = pool[blockIdx.x >> 1];
    const bool is_dc = (blockIdx.x & 1) != 0;
    uint8_t *tab = lut_pool + (size_t)(blockIdx.x >> 1) * kLutPoolBytesPerTable;
    uint8_t *img = tab + (is_dc ? kK2TabBytes : 0u);  // the u16 image (the K2S round kernel's source)
    uint16_t *l1 = reinterpret_cast<uint16_t *>(img);
    uint16_t *l2 = reinterpret_cast<uint16_t *>(img + kK2L1Bytes);
    // the u32 image (K2, the K2S final pass): first level with values and pairs | the same second level, header and arrays
    const uint32_t lb = is_dc ? kK2DcBits : kK2AcBits;
    uint8_t *img32 = tab + (is_dc ? kPoolNewDc : kPoolNewAc);
    uint32_t *f1 = reinterpret_cast<uint32_t *>(img32);
    uint16_t *f2 = reinterpret_cast<uint16_t *>(img32 + (4u << lb));
    __shared__ uint32_t first_miss, first_miss32;
    if (threadIdx.x == 0) first_miss = 1u << kK2LutBits, first_miss32 = 1u << lb;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (1u << kK2LutBits); i += 256) {
        // a code of at most 11 bits is decided by the prefix alone (maxcode[l] has its low 16 - l bits set): evaluate with ones behind it
        const uint32_t e = k2_entry_of(h, (i << (16 - kK2LutBits)) | ((1u << (16 - kK2LutBits)) - 1u), is_dc, kK2LutBits);
        l1[i] = (uint16_t)e;
        if (e == 0) atomicMin(&first_miss, i);  // (a bad category is an answer, not a miss)
    }
    for (uint32_t i = threadIdx.x; i < (1u << lb); i += 256) {
        const uint32_t e = k2_fast_entry(h, i, is_dc, lb);
        f1[i] = e;
        if (e == 0) atomicMin(&first_miss32, i);
    }
    __syncthreads();
    {
        const uint32_t lo = first_miss << (16 - kK2LutBits);
        const uint32_t t16 = lo > 65536u - kK2L2Entries ? lo : 65536u - kK2L2Entries;
        for (uint32_t j = threadIdx.x; j < kK2L2Entries; j += 256) l2[j] = t16 + j < 65536u ? (uint16_t)k2_entry_of(h, t16 + j, is_dc, 16) : (uint16_t)0;
        if (threadIdx.x < 4) reinterpret_cast<uint32_t *>(img + kK2L1Bytes + 2u * kK2L2Entries)[threadIdx.x] = threadIdx.x == 0 ? t16 : 0u;
        if (threadIdx.x < kK2SmallBytes / 16)
            reinterpret_cast<uint4 *>(img + kK2L1Bytes + 2u * kK2L2Entries + 16u)[threadIdx.x] =
                reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(&h) + offsetof(DevHuffTable, maxcode))[threadIdx.x];
    }
    {
        const uint32_t lo = first_miss32 << (16 - lb);
        const uint32_t t16 = lo > 65536u - kK2L2Entries ? lo : 65536u - kK2L2Entries;
        for (uint32_t j = threadIdx.x; j < kK2L2Entries; j += 256) f2[j] = t16 + j < 65536u ? (uint16_t)k2_entry_of(h, t16 + j, is_dc, 16) : (uint16_t)0;
        if (threadIdx.x < 4) reinterpret_cast<uint32_t *>(img32 + (4u << lb) + 2u * kK2L2Entries)[threadIdx.x] = threadIdx.x == 0 ? t16 : 0u;
        if (threadIdx.x < kK2SmallBytes / 16)
            reinterpret_cast<uint4 *>(img32 + (4u << lb) + 2u * kK2L2Entries + 16u)[threadIdx.x] =
                reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(&h) + offsetof(DevHuffTable, maxcode))[threadIdx.x];
    }
}

// per-wave cycle counters (tools/trace/k2_phases.py): [0] waves, [1] table staging, [2] stream init, [3] decode, [4] top-up, [5] flush, [6] total
K2_PROF_DEFINE(k2_prof, jpgpu_debug_k2_profile)

// One wave's 64 restart intervals wave_first .. wave_first + 63 of scan `scan_index` (tables staged, the wave's coefficient staging zero on
// entry and on exit).
__device__ __forceinline__ void k2_wave(const uint8_t *__restrict__ udata, const DevScan &s, uint32_t scan_index, uint32_t wave_first,
                                        const uint32_t *__restrict__ ends_u, DevScanStatus *__restrict__ status, int16_t *__restrict__ coefs,
                                        const K2Group &g, uint32_t lane, unsigned long long k2_t0) {
    const uint8_t *tabs = g.tabs;
    const uint32_t *blk_info = g.blk_info;
    uint8_t *stage = g.stage, *ring = g.ring;
    const unsigned long long k2_t1 = K2_TICK();
    const DevScanStatus st = status[scan_index];
    const uint32_t n_ends = st.n_ends;
    const uint32_t n_intervals = s.n_intervals;
    const uint32_t total_mcus = s.total_mcus;
    const uint32_t dri_eff = s.dri ? s.dri : total_mcus;
    const uint32_t bpm = s.blocks_per_mcu;
    const uint32_t interval = wave_first + lane;
    const bool active = interval < n_ends;
    const uint32_t *eu = ends_u + s.ends_off;
    const uint8_t *ubase = udata + s.data_off;

    // the lane's stream == a fresh JpegBitReader on its restart interval (ref: JpegBitReader.cs)
    uint32_t my_mcus = 0;
    bool closed_by_marker = false;
    uint32_t u0 = 0, u1 = 0;
    if (active) {
        u0 = interval == 0 ? 0u : eu[interval - 1] + 2u;
        u1 = eu[interval];
        my_mcus = (interval == n_intervals - 1) ? total_mcus - interval * dri_eff : dri_eff;
        closed_by_marker = !(interval == n_ends - 1 && st.terminator == 0);
    }
    K2Feed feed;
    K2Pos pos;
    int32_t endpos = 0;  // first bit after the interval's data
    k2_open_at_bit(ubase, u0, 0u, (u1 - u0) * 8u, ring, feed, pos, &endpos);
    // the wave iterates to the largest MCU count among its lanes (only the image's last interval is shorter)
    uint32_t wave_mcus = 0;
    if (wave_first < n_ends) {
        wave_mcus = dri_eff;
        if (wave_first == n_intervals - 1) wave_mcus = total_mcus - wave_first * dri_eff;
    }

    int32_t pred0 = 0, pred1 = 0, pred2 = 0, pred3 = 0;  // DcPredictor per scan component
    uint32_t err = 0;
    const unsigned long long k2_t2 = K2_TICK();
    unsigned long long k2_dec = 0, k2_top = 0, k2_fl = 0;
    uint8_t *my_stage = stage + lane * 128;
    const uint32_t swz16 = ((lane >> 1) & 7u) << 4;  // XOR swizzle of the 16-byte chunks of the lane's staged block

    // flush: whole 128-byte lines (k2_flush_dense) or, for a scan handed over as half-line planes (common.h: kScanSplitHandoff;
    // wave-uniform), lane (blk, chunk) of a pass stores 16 bytes of a 64-byte slot
    const uint64_t coef_off = s.coef_off;
    const bool split = (s.reserved0 & kScanSplitHandoff) != 0;
    uint8_t *split_lo = reinterpret_cast<uint8_t *>(coefs + coef_off * 64);
    const uint64_t split_hi_off = split_plane_lines(n_intervals, dri_eff, bpm) * 128;
    uint64_t *split_flags = reinterpret_cast<uint64_t *>(coefs) + (s.reserved0 >> kSplitFlagShift) + (uint64_t)(wave_first >> 6) * dri_eff * bpm;
    uint32_t split_step = 0;  // mcu * bpm + b
    uint64_t my_flags = 0;

    for (uint32_t mcu = 0; mcu < wave_mcus; mcu++) {
        for (uint32_t b = 0; b < bpm; b++) {
            const uint32_t bi = __builtin_amdgcn_readfirstlane(blk_info[b]);  // wave-uniform
            const uint32_t ci = bi & 0xFFu;
            const K2Tab hdc = k2_tab_dc(tabs, bi);
            const K2Tab hac = k2_tab_ac(tabs, bi);
            const unsigned long long k2_a = K2_TICK();
            int32_t lim = k2_limit(endpos, feed.wr);
            if (active && err == 0 && mcu < my_mcus) {
                // (the predictor's select and write-back stay HERE, between the two pieces: see k2_decode_dc)
                const int32_t pred = ci == 0 ? pred0 : (ci == 1 ? pred1 : (ci == 2 ? pred2 : pred3));
                const int32_t v = k2_decode_dc(ring, feed, pos, endpos, lim, hdc, closed_by_marker, pred, err);
                if (ci == 0) pred0 = v;
                else if (ci == 1) pred1 = v;
                else if (ci == 2) pred2 = v;
                else pred3 = v;
                k2_decode_ac(ring, feed, pos, endpos, lim, hac, closed_by_marker, v, my_stage, swz16, err);
                // the block the reference throws in: blocks in front of it have reached the writer, this one and the rest have not
                if (err != 0)
                    atomicMax(&status[scan_index].pad[1], fail_block_word(((uint64_t)interval * dri_eff + mcu) * bpm + b));
            }
            // top up the ring HERE: the wait for the prefetched chunk then only covers memory operations issued before this
            // block was decoded (the chunk itself and the previous block's coefficient stores), never fresh ones
            const unsigned long long k2_b = K2_TICK();
            k2_topup(ring, feed, pos.pm1);
            const unsigned long long k2_c = K2_TICK();
            // flush 64 blocks of this wave to the coefficient buffer as whole 128-byte lines, re-zero the staging
            k2_wave_sync();
            if (!split) {
                // lane blk staged restart interval wave_first + blk: its block exists where the interval has this MCU
                k2_flush_dense(stage, lane, [&](uint32_t blk, int16_t *&dst) {
                    const uint32_t owner = wave_first + blk;
                    if (owner >= n_ends) return false;
                    const uint32_t owner_mcus = (owner == n_intervals - 1) ? total_mcus - owner * dri_eff : dri_eff;
                    if (mcu >= owner_mcus) return false;
                    dst = coefs + (coef_off + ((uint64_t)owner * dri_eff + mcu) * bpm + b) * 64;
                    return true;
                });
            } else {
                // half-line planes: lanes 8j .. 8j + 7 of a pass hold blocks 2p, 2p + 1 = restart intervals 2p, 2p + 1: one whole line of the
                // lo plane, and -- when either block has a non-zero coefficient in 32..63 -- the same line of the hi plane
                // The step's flag word is bit j = lane j's block: every lane looks at the hi half of the block it staged itself (its own
                // swizzle, conflict-free like the decode's writes), one ballot per block step.
#ifndef JPGPU_K2_PRICE_FLUSH
                uint4 own = *reinterpret_cast<const uint4 *>(my_stage + (64u ^ swz16));
#pragma unroll
                for (uint32_t c = 80; c < 128; c += 16) {
                    const uint4 o = *reinterpret_cast<const uint4 *>(my_stage + (c ^ swz16));
                    own.x |= o.x, own.y |= o.y, own.z |= o.z, own.w |= o.w;
                }
                const uint64_t step_flags = __ballot((own.x | own.y | own.z | own.w) != 0);
#else
                const uint64_t step_flags = 0;  // (priced by omission: no hi half is looked at, read or stored; wrong for flagged blocks)
#endif
#pragma unroll
                for (int it = 0; it < 4; it++) {
                    const uint32_t blk = it * 16 + (lane >> 2);
                    const uint32_t chunk = lane & 3;
                    const uint32_t swz = (blk >> 1) & 7;
                    uint4 *src_lo = reinterpret_cast<uint4 *>(stage + blk * 128 + ((chunk ^ swz) * 16));
                    const uint4 v = *src_lo;
                    const uint4 z = {0, 0, 0, 0};
                    *src_lo = z;
                    // a line is written where its even interval has this MCU (the odd one is its equal or the scan's short last one)
                    const uint32_t even = wave_first + (blk & ~1u);
                    const bool have = even < n_ends && mcu < ((even == n_intervals - 1) ? total_mcus - even * dri_eff : dri_eff);
                    const uint64_t off = split_slot(wave_first + blk, mcu, b, dri_eff, bpm) * 64 + chunk * 16;
                    if (have) *reinterpret_cast<uint4 *>(split_lo + off) = v;
                    // The hi side of a pass whose sixteen blocks are all unflagged is skipped (wave-uniform).  The staging is zero on entry,
                    // a lane writes only its own block, and the hi half of an unflagged block was never written or written with zeros
                    // (the look-up above has just read it as zeros): leaving its re-zero out still leaves the staging zero on exit,
                    // which the next block step and -- in a pooled wave -- the next ticket's chunk rely on.
                    const uint32_t pass_flags = (uint32_t)(step_flags >> (16 * it)) & 0xFFFFu;
                    if (pass_flags != 0) {
                        uint4 *src_hi = reinterpret_cast<uint4 *>(stage + blk * 128 + (((chunk + 4) ^ swz) * 16));
                        const uint4 w = *src_hi;
                        *src_hi = z;
                        // the line goes out when either block of the pair is flagged; the unflagged one's slot is zeros from the staging
                        if (have && ((pass_flags >> ((lane >> 2) & ~1u)) & 3u) != 0) *reinterpret_cast<uint4 *>(split_lo + split_hi_off + off) = w;
                    }
                }
                // the step's flag word stays in the lane whose index is the step's; 64 of them (or the chunk's last ones) go out in one store
                if (lane == (split_step & 63u)) my_flags = step_flags;
                if ((split_step & 63u) == 63u || split_step + 1 == wave_mcus * bpm) {
                    if (lane <= (split_step & 63u)) split_flags[(split_step & ~63u) + lane] = my_flags;
                }
                split_step++;
            }
            k2_wave_sync();
            const unsigned long long k2_d = K2_TICK();
            k2_dec += k2_b - k2_a;
            k2_top += k2_c - k2_b;
            k2_fl += k2_d - k2_c;
        }
    }
    K2_PROF_ADD(k2_prof, 0, 1);
    K2_PROF_ADD(k2_prof, 1, k2_t1 - k2_t0);
    K2_PROF_ADD(k2_prof, 2, k2_t2 - k2_t1);
    K2_PROF_ADD(k2_prof, 3, k2_dec);
    K2_PROF_ADD(k2_prof, 4, k2_top);
    K2_PROF_ADD(k2_prof, 5, k2_fl);
    K2_PROF_ADD(k2_prof, 6, K2_TICK() - k2_t0);

    if (active) {
        int32_t rem = endpos - (pos.pm1 + 1);
        if (rem < 0) rem = 0;
        const uint32_t code = restart_check(s, st, &status[scan_index], interval, n_ends, n_intervals, dri_eff, rem, err);
        if (code != kNoError) atomicMin(&status[scan_index].first_error, code);
    }
}

// K2 proper: a workgroup per WAVES * 64 consecutive restart intervals of one scan.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void huffman_decode_kernel(const uint8_t *__restrict__ udata,
                                                                    const DevScan *__restrict__ scans,
                                                                    const HuffWork *__restrict__ work,
                                                                    const uint32_t *__restrict__ ends_u,
                                                                    DevScanStatus *__restrict__ status,
                                                                    const DevHuffTable *__restrict__ huff_pool,
                                                                    int16_t *__restrict__ coefs, int n_slots,
                                                                    const uint8_t *__restrict__ lut_pool, uint32_t tab_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const HuffWork wk = work[blockIdx.x];
    const DevScan &s = scans[wk.scan];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long k2_t0 = K2_TICK();
    const K2Group g = k2_group_setup(smem, tab_bytes, 64 * WAVES, s, lut_pool, n_slots);
    k2_wave(udata, s, wk.scan, wk.first_interval + wave * 64, ends_u, status, coefs, g, lane, k2_t0);
}

// POOL (round 6; the K2S final pass has had it since round 5).  Runs of consecutive scans that stage the same tables in the same slots
// -- every batch of files from one encoder -- need no workgroup per WAVES * 64 intervals of ONE scan: one workgroup per CU stages the
// tables once and every WAVE takes the next 64 intervals of the run from a counter until there are none.  No wave waits for a slower one
// of its workgroup before the CU gets new work, nothing is restaged (a workgroup of the plain form lives for 24 block steps), and the
// last workgroup of a scan is no longer half empty (8 100 intervals = 11.5 workgroups of 704).  The counter is never cleared: a launch
// draws n_chunks + (waves launched) tickets -- every wave exactly one beyond the end -- and the host passes the sum of the launches before.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void huffman_pool_kernel(const uint8_t *__restrict__ udata, const DevScan *__restrict__ scans,
                                                                  const HuffWork *__restrict__ work, uint32_t n_chunks,
                                                                  uint32_t *__restrict__ counter, uint32_t ticket_base,
                                                                  const uint32_t *__restrict__ ends_u, DevScanStatus *__restrict__ status,
                                                                  int16_t *__restrict__ coefs, int n_slots, const uint8_t *__restrict__ lut_pool,
                                                                  uint32_t tab_bytes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long k2_t0 = K2_TICK();
    const K2Group g = k2_group_setup(smem, tab_bytes, 64 * WAVES, scans[work[0].scan], lut_pool, n_slots);  // (every entry of `work` stages the same)
    for (uint32_t c; (c = k2_next_ticket(counter, ticket_base, lane)) < n_chunks;) {
        const HuffWork wk = work[c];
        k2_wave(udata, scans[wk.scan], wk.scan, wk.first_interval, ends_u, status, coefs, g, lane, c == 0 ? k2_t0 : K2_TICK());
    }
}

static size_t k2_lds_bytes(uint32_t tab_bytes, int waves) { return (size_t)tab_bytes + (size_t)waves * kK2WaveBytes + kMaxBlocksPerMcu * sizeof(uint32_t); }

// f(std::integral_constant<int, W>) for W = huffman_waves(tab_bytes): the kernels exist for 7 (eight AC tables) .. 11 waves
template <class F>
static hipError_t k2_with_waves(uint32_t tab_bytes, F f) {
    switch (huffman_waves(tab_bytes)) {
    case 11: return f(std::integral_constant<int, 11>{});
    case 10: return f(std::integral_constant<int, 10>{});
    case 9: return f(std::integral_constant<int, 9>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 7>{});
    }
}

template <int WAVES>
static hipError_t launch_huffman_w(hipStream_t stream, const uint8_t *data, const DevScan *scans, const HuffWork *work, int n_work,
                                   const uint32_t *ends, DevScanStatus *status, const DevHuffTable *huff_pool, int16_t *coefs,
                                   int n_slots, const uint8_t *lut_pool, uint32_t tab_bytes) {
    const size_t lds = k2_lds_bytes(tab_bytes, WAVES);
    static std::atomic<uint64_t> configured{0};
    const hipError_t ea = allow_dynamic_lds(reinterpret_cast<const void *>(&huffman_decode_kernel<WAVES>), 160 * 1024, configured);
    if (ea != hipSuccess) return ea;
    hipLaunchKernelGGL((huffman_decode_kernel<WAVES>), dim3(n_work), dim3(64 * WAVES), lds, stream, data, scans, work, ends, status, huff_pool, coefs,
                       n_slots, lut_pool, tab_bytes);
    return hipGetLastError();
}

// `work` holds one entry per huffman_waves(tab_bytes) * 64 restart intervals (DeviceBatch builds it with the same function);
// tab_bytes = the largest k2_scan_tab_bytes() among the batch's scans
hipError_t launch_huffman(hipStream_t stream, const uint8_t *data, const DevScan *scans, const HuffWork *work, int n_work,
                          const uint32_t *ends, DevScanStatus *status, const DevHuffTable *huff_pool, int16_t *coefs,
                          int n_slots, const uint8_t *lut_pool, uint32_t tab_bytes) {
    if (n_work <= 0) return hipSuccess;
    return k2_with_waves(tab_bytes, [&](auto w) {
        return launch_huffman_w<decltype(w)::value>(stream, data, scans, work, n_work, ends, status, huff_pool, coefs, n_slots, lut_pool, tab_bytes);
    });
}

template <int WAVES>
static hipError_t launch_huffman_pool_w(hipStream_t stream, const uint8_t *data, const DevScan *scans, const HuffWork *work, int n_chunks, uint32_t *counter,
                                        uint32_t ticket_base, int groups, const uint32_t *ends, DevScanStatus *status, int16_t *coefs, int n_slots,
                                        const uint8_t *lut_pool, uint32_t tab_bytes) {
    const size_t lds = k2_lds_bytes(tab_bytes, WAVES);
    static std::atomic<uint64_t> configured{0};
    const hipError_t ea = allow_dynamic_lds(reinterpret_cast<const void *>(&huffman_pool_kernel<WAVES>), 160 * 1024, configured);
    if (ea != hipSuccess) return ea;
    hipLaunchKernelGGL((huffman_pool_kernel<WAVES>), dim3(groups), dim3(64 * WAVES), lds, stream, data, scans, work, (uint32_t)n_chunks, counter, ticket_base,
                       ends, status, coefs, n_slots, lut_pool, tab_bytes);
    return hipGetLastError();
}
// One pooled run: `work` = its n_chunks entries (scan, first interval) of 64 intervals each, all staging the same tables; `groups`
// workgroups of huffman_waves(tab_bytes) waves; draws n_chunks + groups * waves tickets from *counter, the first of them ticket_base.
hipError_t launch_huffman_pool(hipStream_t stream, const uint8_t *data, const DevScan *scans, const HuffWork *work, int n_chunks, uint32_t *counter,
                               uint32_t ticket_base, int groups, const uint32_t *ends, DevScanStatus *status, int16_t *coefs, int n_slots,
                               const uint8_t *lut_pool, uint32_t tab_bytes) {
    if (n_chunks <= 0 || groups <= 0) return hipSuccess;
    return k2_with_waves(tab_bytes, [&](auto w) {
        return launch_huffman_pool_w<decltype(w)::value>(stream, data, scans, work, n_chunks, counter, ticket_base, groups, ends, status, coefs, n_slots,
                                                         lut_pool, tab_bytes);
    });
}

// Lookups of every table of the pool (once per upload: the tables of a batch do not change between decodes).
hipError_t launch_lut_pool(hipStream_t stream, const DevHuffTable *huff_pool, int n_tables, uint8_t *lut_pool) {
    if (n_tables <= 0) return hipSuccess;
    hipLaunchKernelGGL(lut_pool_kernel, dim3(2 * n_tables), dim3(256), 0, stream, huff_pool, lut_pool);
    return hipGetLastError();
}

}  // namespace jpgpu
