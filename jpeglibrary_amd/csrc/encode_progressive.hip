// jpeglibrary_amd/csrc/encode_progressive.hip -- the progressive entropy coder of the libjpeg arithmetic (include/jpgpu.h, 4e): jcphuff.c
// over quantised blocks, the unit of work one scan of one image, one lane per block of the scan in scan order.
//
// What a block writes does not depend on the blocks in front of it, except for the EOB run: a block that codes no coefficient behind
// some point extends the run (EOBRUN++), a block that codes one first flushes the run of the blocks in front of it -- the EOBn symbol,
// the run's low bits, then the correction bits those blocks deferred (refinement scans).  Seen from the stream that is: the run's
// symbol stands in front of the deferred bits of its FIRST block, and every later block of the run adds its deferred bits and nothing
// else.  So EP2 resolves the runs forward, from the block that starts one, into "heads": the length coded at that block.  The limits --
// 32767 blocks, more than 937 deferred bits -- split a run into pieces, each with a head of its own; only the lane of the run's first
// block walks it, over one byte per block (EP1), sixteen at a time where nothing is deferred.  A flat image is ONE run through the
// whole scan: one lane walks it, nothing waits for another workgroup.
//   With the heads known a block's symbols and bits are its own: EP3 counts them, EP4 measures them with the built tables, EP5 writes.
#include <hip/hip_runtime.h>

#include "encode_progressive.h"

namespace jpgpu {
namespace {

__device__ __forceinline__ uint32_t ep_bit_count(uint32_t a) { return a ? 32u - (uint32_t)__builtin_clz(a) : 0u; }
__device__ __forceinline__ uint32_t ep_abs(int32_t c) { return (uint32_t)(c < 0 ? -c : c); }

// the block of the coefficient buffer that block b of the scan is
__device__ __forceinline__ uint32_t ep_source_block(const DevProgScan &sc, uint32_t b) {
    if (sc.ss == 0) return b;
    const uint32_t by = b / sc.grid_w, bx = b - by * sc.grid_w;
    const uint32_t mcu = (by / sc.comp_v) * sc.mcus_per_line + bx / sc.comp_h;
    return mcu * sc.bpm + sc.first_blk + (by % sc.comp_v) * sc.comp_h + bx % sc.comp_h;
}

// f(k, coefficient) for k = ss .. se in order: eight coefficients per 16-byte load, taken from registers named at compile time
template <typename F>
__device__ __forceinline__ void ep_for_band(const int16_t *blk, uint32_t ss, uint32_t se, F f) {
    const uint4 *src = reinterpret_cast<const uint4 *>(blk);
    for (uint32_t g = ss >> 3; g <= (se >> 3); g++) {
        const uint4 v = src[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t k = g * 8u + j;
            const int32_t c = (j & 1u) ? ((int32_t)w[j >> 1] >> 16) : (int32_t)(int16_t)(w[j >> 1] & 0xFFFFu);
            if (k >= ss && k <= se) f(k, c);
        }
    }
}

// EP1's byte of an AC block.  `last` is the last coefficient of the band the block codes a symbol for: |coef| >> Al != 0 in a first
// scan, == 1 in a refinement scan.  Whatever lies behind it -- zeros, or values the scans before made non-zero -- goes into the run.
__device__ __forceinline__ uint32_t ep_classify(const DevProgScan &sc, const int16_t *blk) {
    uint32_t last = 0, deferred = 0;
    const uint32_t al = sc.al;
    if (sc.ah == 0) {
        ep_for_band(blk, sc.ss, sc.se, [&](uint32_t k, int32_t c) {
            if ((ep_abs(c) >> al) != 0) last = k;
        });
    } else {
        ep_for_band(blk, sc.ss, sc.se, [&](uint32_t k, int32_t c) {
            const uint32_t t = ep_abs(c) >> al;
            if (t == 1) {
                last = k;
                deferred = 0;
            } else if (t > 1) {
                deferred++;
            }
        });
    }
    return (last != 0 ? 0x80u : 0u) | (last != sc.se ? 0x40u : 0u) | deferred;
}

// One block of a scan in jcphuff.c's order: sym(table of the scan, symbol) for every Huffman symbol, bits(value, n <= 32) for everything
// else.  head = the run piece coded at this block (EP2).
template <typename Sym, typename Bits>
__device__ __forceinline__ void ep_block(const DevProgScan &sc, const int16_t *img, uint32_t b, uint32_t head, Sym sym, Bits bits) {
    const uint32_t src = ep_source_block(sc, b), al = sc.al;
    const int16_t *blk = img + (size_t)src * 64;
    if (sc.ss == 0) {
        const int32_t v = (int32_t)blk[0] >> al;  // (an arithmetic shift)
        if (sc.ah != 0) {
            bits((uint32_t)v & 1u, 1u);
            return;
        }
        // the previous block of the same component in MCU order
        const uint32_t mcu = src / sc.bpm, k = src - mcu * sc.bpm, comp = k < sc.ny ? 0u : k - sc.ny + 1u;
        int32_t pred = 0;
        if (comp == 0 && k > 0) pred = (int32_t)img[(size_t)(src - 1u) * 64] >> al;
        else if (mcu > 0) pred = (int32_t)img[(size_t)((mcu - 1u) * sc.bpm + (comp == 0 ? sc.ny - 1u : k)) * 64] >> al;
        const int32_t d = v - pred;
        const uint32_t n = ep_bit_count(ep_abs(d));
        sym(comp ? 1u : 0u, n);
        bits((uint32_t)(d < 0 ? d - 1 : d) & ((1u << n) - 1u), n);
        return;
    }
    uint32_t r = 0, br = 0;
    unsigned long long defer = 0;  // the br correction bits buffered in this block, the first one highest
    auto put_deferred = [&]() {
        if (br > 32u) {
            bits((uint32_t)(defer >> 32), br - 32u);
            bits((uint32_t)defer, 32u);
        } else if (br != 0) {
            bits((uint32_t)defer, br);
        }
        defer = 0;
        br = 0;
    };
    if (sc.ah == 0) {
        ep_for_band(blk, sc.ss, sc.se, [&](uint32_t, int32_t c) {
            const uint32_t t = ep_abs(c) >> al;
            if (t == 0) {
                r++;
                return;
            }
            while (r > 15u) {
                sym(0u, 0xF0u);
                r -= 16u;
            }
            const uint32_t n = ep_bit_count(t);
            sym(0u, (r << 4) + n);
            bits((c < 0 ? ~t : t) & ((1u << n) - 1u), n);
            r = 0;
        });
    } else {
        uint32_t eob = 0;
        ep_for_band(blk, sc.ss, sc.se, [&](uint32_t k, int32_t c) {
            if ((ep_abs(c) >> al) == 1u) eob = k;
        });
        ep_for_band(blk, sc.ss, sc.se, [&](uint32_t k, int32_t c) {
            const uint32_t t = ep_abs(c) >> al;
            if (t == 0) {
                r++;
                return;
            }
            while (r > 15u && k <= eob) {
                sym(0u, 0xF0u);
                r -= 16u;
                put_deferred();
            }
            if (t > 1u) {
                defer = (defer << 1) | (t & 1u);
                br++;
                return;
            }
            sym(0u, (r << 4) + 1u);
            bits(c < 0 ? 0u : 1u, 1u);
            put_deferred();
            r = 0;
        });
    }
    if (head != 0) {
        const uint32_t n = 31u - (uint32_t)__builtin_clz(head);
        sym(0u, n << 4);
        bits(head & ((1u << n) - 1u), n);
    }
    put_deferred();
}

__global__ __launch_bounds__(256) void prog_classify_kernel(const DevProgScan *__restrict__ scans, const EncWork *__restrict__ work,
                                                            const int16_t *__restrict__ coefs, uint8_t *__restrict__ info) {
    const EncWork wk = work[blockIdx.x];
    const DevProgScan &sc = scans[wk.image];
    const uint32_t b = wk.first + threadIdx.x;
    if (sc.ss == 0 || b >= sc.n_blocks) return;
    const int16_t *img = coefs + sc.coef_off * 64;
    info[sc.blk_off + b] = (uint8_t)ep_classify(sc, img + (size_t)ep_source_block(sc, b) * 64);
}

__global__ __launch_bounds__(256) void prog_runs_kernel(const DevProgScan *__restrict__ scans, const EncWork *__restrict__ work,
                                                        const uint8_t *__restrict__ info, uint16_t *__restrict__ heads) {
    const EncWork wk = work[blockIdx.x];
    const DevProgScan &sc = scans[wk.image];
    const uint32_t b = wk.first + threadIdx.x, n = sc.n_blocks;
    if (sc.ss == 0 || b >= n) return;
    const uint8_t *in = info + sc.blk_off;  // (blk_off is a multiple of 16)
    uint16_t *hd = heads + sc.blk_off;
    const uint32_t me = in[b];
    if ((me & 0x40u) == 0) return;                                        // nothing of this block goes into a run
    if (b != 0 && (me & 0x80u) == 0 && (in[b - 1] & 0x40u) != 0) return;  // it goes into the run of the block in front
    uint32_t count = 0, deferred = 0, start = b;
    auto member = [&](uint32_t j, uint32_t d) {  // block j joins; the piece is coded (at `start`) when a limit is reached
        count++;
        deferred += d;
        if (count == kProgMaxRun || deferred > kProgMaxDeferred) {
            hd[start] = (uint16_t)count;
            start = j + 1u;
            count = 0;
            deferred = 0;
        }
    };
    member(b, me & 63u);
    uint32_t j = b + 1u;
    bool open = true;  // the run goes on until a block codes a coefficient
    auto one = [&]() {
        const uint32_t v = in[j];
        if (v & 0x80u) {
            open = false;
        } else {
            member(j, v & 63u);
            j++;
        }
    };
    while (open && j < n && (j & 15u) != 0) one();
    while (open && j + 16u <= n) {
        const uint4 q = *reinterpret_cast<const uint4 *>(in + j);
        // sixteen blocks that code nothing and defer nothing, and no limit among them: the run grows by sixteen
        if (((q.x | q.y | q.z | q.w) & 0xBFBFBFBFu) == 0 && count + 16u < kProgMaxRun) {
            count += 16u;
            j += 16u;
            continue;
        }
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            if (open) {
                const uint32_t v = (w[i >> 2] >> ((i & 3u) * 8u)) & 0xFFu;
                if (v & 0x80u) {
                    open = false;
                } else {
                    member(j, v & 63u);
                    j++;
                }
            }
        }
    }
    while (open && j < n) one();
    if (count != 0) hd[start] = (uint16_t)count;  // (closed by the block at j, or by the scan's end)
}

__global__ __launch_bounds__(256) void prog_stats_kernel(const DevProgScan *__restrict__ scans, const EncWork *__restrict__ work,
                                                         const int16_t *__restrict__ coefs, const uint16_t *__restrict__ heads,
                                                         uint32_t *__restrict__ stats) {
    __shared__ uint32_t lh[2 * 256];
    const EncWork wk = work[blockIdx.x];
    const DevProgScan &sc = scans[wk.image];
    lh[threadIdx.x] = 0;
    lh[256 + threadIdx.x] = 0;
    __syncthreads();
    const uint32_t b = wk.first + threadIdx.x;
    uint32_t other = 0;  // bits that are no Huffman code
    if (b < sc.n_blocks) {
        const uint32_t head = sc.ss != 0 ? heads[sc.blk_off + b] : 0u;
        ep_block(sc, coefs + sc.coef_off * 64, b, head, [&](uint32_t t, uint32_t s) { atomicAdd(&lh[t * 256u + s], 1u); },
                 [&](uint32_t, uint32_t n) { other += n; });
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) other += __shfl_xor(other, o, 64);
    uint32_t *mine = stats + (size_t)wk.image * kProgStatWords;
    if ((threadIdx.x & 63u) == 0 && other != 0) atomicAdd(reinterpret_cast<unsigned long long *>(mine + 512), (unsigned long long)other);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 512u; i += 256u)
        if (lh[i] != 0) atomicAdd(&mine[i], lh[i]);
}

// the scan's two table slots staged in LDS (an AC scan reads the first)
__device__ __forceinline__ void ep_stage_tables(const EncHuffTable *__restrict__ tables, uint32_t first, EncHuffTable *sh_tab) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tables + first);
    uint32_t *dst = reinterpret_cast<uint32_t *>(sh_tab);
    for (uint32_t i = threadIdx.x; i < 2u * (uint32_t)sizeof(EncHuffTable) / 4u; i += 256u) dst[i] = src[i];
    __syncthreads();
}

__global__ __launch_bounds__(256) void prog_bits_kernel(const DevProgScan *__restrict__ scans, const EncWork *__restrict__ work,
                                                        const EncHuffTable *__restrict__ tables, const int16_t *__restrict__ coefs,
                                                        const uint16_t *__restrict__ heads, uint32_t *__restrict__ bits,
                                                        uint32_t *__restrict__ wg_bits) {
    __shared__ EncHuffTable sh_tab[2];
    __shared__ uint32_t sh_wave[4];
    const EncWork wk = work[blockIdx.x];
    const DevProgScan &sc = scans[wk.image];
    ep_stage_tables(tables, sc.table, sh_tab);
    const uint32_t b = wk.first + threadIdx.x;
    uint32_t n = 0;
    if (b < sc.n_blocks) {
        const uint32_t head = sc.ss != 0 ? heads[sc.blk_off + b] : 0u;
        ep_block(sc, coefs + sc.coef_off * 64, b, head, [&](uint32_t t, uint32_t s) { n += sh_tab[t].len[s]; }, [&](uint32_t, uint32_t len) { n += len; });
    }
    uint32_t incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if ((threadIdx.x & 63u) >= (uint32_t)o) incl += t;
    }
    if ((threadIdx.x & 63u) == 63u) sh_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (k < (threadIdx.x >> 6)) before += sh_wave[k];
        total += sh_wave[k];
    }
    if (b < sc.n_blocks) bits[sc.blk_off + b] = before + incl - n;
    if (threadIdx.x == 0) wg_bits[blockIdx.x] = total;
}

// exclusive prefix sums of a scan's workgroup totals (one workgroup per scan)
__global__ __launch_bounds__(256) void prog_offsets_kernel(const DevProgScan *__restrict__ scans, const uint32_t *__restrict__ wg_bits,
                                                           uint64_t *__restrict__ wg_base) {
    const DevProgScan &sc = scans[blockIdx.x];
    __shared__ uint64_t sh[256];
    const uint32_t tid = threadIdx.x, n = sc.n_wg;
    const uint32_t per = (n + 255u) / 256u;
    const uint32_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    const uint32_t *src = wg_bits + sc.work_first;
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += src[i];
    sh[tid] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint64_t v = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    uint64_t run = sh[tid] - sum;
    for (uint32_t i = lo; i < hi; i++) {
        wg_base[sc.work_first + i] = run;
        run += src[i];
    }
}

// The stream is kept as big-endian 32-bit words (every word stored byte-swapped), ORed into a zeroed buffer: a word can hold the bits of
// several lanes.  Nothing is written at or beyond the scan's last word, whatever the offsets say.
__global__ __launch_bounds__(256) void prog_emit_kernel(const DevProgScan *__restrict__ scans, const EncWork *__restrict__ work,
                                                        const EncHuffTable *__restrict__ tables, const int16_t *__restrict__ coefs,
                                                        const uint16_t *__restrict__ heads, const uint32_t *__restrict__ bits,
                                                        const uint64_t *__restrict__ wg_base, uint8_t *__restrict__ raw) {
    __shared__ EncHuffTable sh_tab[2];
    const EncWork wk = work[blockIdx.x];
    const DevProgScan &sc = scans[wk.image];
    ep_stage_tables(tables, sc.table, sh_tab);
    const uint32_t b = wk.first + threadIdx.x;
    if (b >= sc.n_blocks) return;
    uint32_t *words = reinterpret_cast<uint32_t *>(raw + sc.raw_off);
    const uint64_t n_words = (sc.raw_bits + 31ull) >> 5;
    const uint64_t start = wg_base[blockIdx.x] + bits[sc.blk_off + b];
    uint64_t wi = start >> 5;
    uint32_t fill = (uint32_t)(start & 31u), cur = 0;
    auto flush = [&]() {
        if (cur != 0 && wi < n_words) atomicOr(&words[wi], __builtin_bswap32(cur));
    };
    auto put = [&](uint32_t code, uint32_t len) {  // len <= 32, code < 2^len
        if (len == 0) return;
        const uint32_t left = code << (32u - len);
        cur |= left >> fill;
        const uint32_t before = fill;
        fill += len;
        if (fill >= 32u) {
            flush();
            wi++;
            cur = __builtin_amdgcn_alignbit(left, 0u, before);  // what did not fit: left << (32 - before), 0 when before == 0
            fill -= 32u;
        }
    };
    const uint32_t head = sc.ss != 0 ? heads[sc.blk_off + b] : 0u;
    ep_block(sc, coefs + sc.coef_off * 64, b, head, [&](uint32_t t, uint32_t s) { put(sh_tab[t].code[s], sh_tab[t].len[s]); }, put);
    if (b + 1u == sc.n_blocks) {  // the scan ends padded with one-bits to a byte
        const uint32_t rem = (uint32_t)((8u - (sc.raw_bits & 7u)) & 7u);
        if (rem) put((1u << rem) - 1u, rem);
    }
    if (fill) flush();
}

__global__ __launch_bounds__(256) void prog_assemble_kernel(const DevProgFile *__restrict__ files, const DevEncImage *__restrict__ scan_streams,
                                                            const uint64_t *__restrict__ scan_len, const uint8_t *__restrict__ headers,
                                                            const uint8_t *__restrict__ staged, uint8_t *__restrict__ out,
                                                            uint64_t *__restrict__ file_len) {
    const DevProgFile &f = files[blockIdx.y];
    uint8_t *dst = out + f.dst_off;
    if (blockIdx.x == 0) {
        for (uint32_t j = threadIdx.x; j < f.hdr_len; j += 256u) dst[j] = headers[f.hdr_off + j];
        return;
    }
    const uint32_t s = blockIdx.x - 1u;
    if (s >= f.n_scans) return;
    uint64_t at = f.hdr_len;
    for (uint32_t k = 0; k < s; k++) at += scan_len[f.first_scan + k] - 2u;
    const uint64_t len = scan_len[f.first_scan + s] - 2u;  // (the stuffing stage closes every stream with EOI)
    const uint8_t *src = staged + scan_streams[f.first_scan + s].out_off;
    for (uint64_t j = threadIdx.x; j < len; j += 256u) dst[at + j] = src[j];
    if (s + 1u == f.n_scans && threadIdx.x == 0) {
        dst[at + len] = 0xFF;
        dst[at + len + 1u] = 0xD9;
        file_len[blockIdx.y] = at + len + 2u;
    }
}

}  // namespace

hipError_t launch_prog_classify(hipStream_t stream, const DevProgScan *scans, const EncWork *work, int n_work, const int16_t *coefs, uint8_t *info) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(prog_classify_kernel, dim3(n_work), dim3(256), 0, stream, scans, work, coefs, info);
    return hipGetLastError();
}
hipError_t launch_prog_runs(hipStream_t stream, const DevProgScan *scans, const EncWork *work, int n_work, const uint8_t *info, uint16_t *heads) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(prog_runs_kernel, dim3(n_work), dim3(256), 0, stream, scans, work, info, heads);
    return hipGetLastError();
}
hipError_t launch_prog_stats(hipStream_t stream, const DevProgScan *scans, const EncWork *work, int n_work, const int16_t *coefs, const uint16_t *heads,
                             uint32_t *stats) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(prog_stats_kernel, dim3(n_work), dim3(256), 0, stream, scans, work, coefs, heads, stats);
    return hipGetLastError();
}
hipError_t launch_prog_bits(hipStream_t stream, const DevProgScan *scans, int n_scans, const EncWork *work, int n_work, const EncHuffTable *tables,
                            const int16_t *coefs, const uint16_t *heads, uint32_t *bits, uint32_t *wg_bits, uint64_t *wg_base) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(prog_bits_kernel, dim3(n_work), dim3(256), 0, stream, scans, work, tables, coefs, heads, bits, wg_bits);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(prog_offsets_kernel, dim3(n_scans), dim3(256), 0, stream, scans, wg_bits, wg_base);
    return hipGetLastError();
}
hipError_t launch_prog_emit(hipStream_t stream, const DevProgScan *scans, const EncWork *work, int n_work, const EncHuffTable *tables, const int16_t *coefs,
                            const uint16_t *heads, const uint32_t *bits, const uint64_t *wg_base, uint8_t *raw) {
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(prog_emit_kernel, dim3(n_work), dim3(256), 0, stream, scans, work, tables, coefs, heads, bits, wg_base, raw);
    return hipGetLastError();
}
hipError_t launch_prog_assemble(hipStream_t stream, const DevProgFile *files, int n_files, int max_scans, const DevEncImage *scan_streams,
                                const uint64_t *scan_len, const uint8_t *headers, const uint8_t *staged, uint8_t *out, uint64_t *file_len) {
    if (n_files <= 0) return hipSuccess;
    hipLaunchKernelGGL(prog_assemble_kernel, dim3(max_scans + 1, n_files), dim3(256), 0, stream, files, scan_streams, scan_len, headers, staged, out, file_len);
    return hipGetLastError();
}

}  // namespace jpgpu
