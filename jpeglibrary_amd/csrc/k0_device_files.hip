// jpeglibrary_amd/csrc/k0_device_files.hip -- ingest of files that lie in device memory already (jpgpu_batch_upload_device):
// gather into the input buffer, the heads the host parser needs, the two bytes at each ingest verdict.
//
// Everything here runs on the upload stream as a fixed number of launches per upload; nothing is issued per file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpgpu.h"
#include "common.h"
#include "kernels.h"

namespace jpgpu {

// Gather: every piece is up to kGatherPieceBytes of one file, copied from wherever the caller's bytes lie to a 16-byte aligned
// place in the input buffer, plus `pad` zero bytes behind it (the slack up to the file's 256-byte slot boundary; the two
// pieces with len = 0 are the slack in front of the first file and behind the last).  len + pad is a multiple of 16.
//
// The write side decides the form: a wave stores 64 x 16 contiguous, aligned bytes per instruction (1 KiB, whole 128-byte
// lines), so every line of the buffer is written once and never read-modified.  The read side takes the caller's address as
// it comes: lane i loads the 16 bytes its store needs from src + 16 i, whatever src mod 16 is -- a wave-load of a misaligned
// source touches nine lines instead of eight and the ninth is the next wave-load's first (a hit in the CU's cache), so HBM
// still delivers every line once.  No load reaches outside [src, src + len): the last, partial 16 bytes are read byte by byte
// (the caller's allocation may end there).  Four loads are issued per lane before the first store; a workgroup moves 64 KiB,
// i.e. four such rounds: the ~100 KiB files of a typical batch give a few thousand workgroups, several per CU.
__global__ __launch_bounds__(256) void gather_device_kernel(const GatherPiece *__restrict__ pieces, uint8_t *__restrict__ dst) {
    const GatherPiece pc = pieces[blockIdx.x];
    typedef const __attribute__((address_space(1))) uint8_t *GlobalBytes;  // (an address out of a list: say that it is global memory, or the loads are flat)
    GlobalBytes src = (GlobalBytes)pc.src;
    uint4 *d = reinterpret_cast<uint4 *>(dst + pc.dst_off);
    const uint32_t n_full = pc.len >> 4, rem = pc.len & 15u;
    const uint32_t n_all = (pc.len + pc.pad) >> 4;
    for (uint32_t base = threadIdx.x; base < n_all; base += 4u * 256u) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t c = base + (uint32_t)k * 256u;
            v[k] = make_uint4(0u, 0u, 0u, 0u);
            if (c < n_full) {
                __builtin_memcpy(&v[k], src + (size_t)c * 16u, 16);  // (unaligned global loads are fine on gfx9+)
            } else if (c == n_full && rem != 0) {
                GlobalBytes t = src + (size_t)n_full * 16u;
                uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
                for (uint32_t j = 0; j < 15; j++) {
                    if (j < rem) {
                        const uint32_t b = (uint32_t)t[j] << (8u * (j & 3u));
                        if (j < 4) w0 |= b;
                        else if (j < 8) w1 |= b;
                        else if (j < 12) w2 |= b;
                        else w3 |= b;
                    }
                }
                v[k] = make_uint4(w0, w1, w2, w3);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t c = base + (uint32_t)k * 256u;
            if (c < n_all) d[c] = v[k];
        }
    }
}

// Heads: how many bytes of file i must the host see to plan it from its headers?  One lane per file walks the marker
// segments from the file's first byte (its copy in the input buffer): SOI, then FF xx, a length, a skip, ... up to the first
// SOS header, never past the file or kDeviceHeadMax.  head_len[i] = min(len, kDeviceHeadMax, end of that SOS header +
// JPGPU_DEVICE_HEAD_PAD); anything unexpected (no FF where a marker must be, a fill byte, a marker without a length, a length
// that runs off the file or the 64 KiB, no SOS) gives min(len, kDeviceHeadMax) with kHeadGaveUp set.  This is a hint about how
// many bytes to fetch and nothing else: the host parses what it gets (plan_file_headers) and fetches the whole file when
// that does not end in a header-only plan.
__global__ __launch_bounds__(64) void head_walk_kernel(const uint8_t *__restrict__ data, const DeviceFile *__restrict__ files, int n,
                                                       uint32_t *__restrict__ head_len) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const DeviceFile f = files[i];
    const uint8_t *p = data + f.off;
    const uint32_t limit = f.len < kDeviceHeadMax ? f.len : kDeviceHeadMax;
    uint32_t result = limit | kHeadGaveUp;
    if (f.len == 0) {
        head_len[i] = 0;  // (the empty file: nothing to walk, nothing to fetch)
        return;
    }
    if (limit >= 4 && p[0] == 0xFF && p[1] == 0xD8) {
        uint32_t pos = 2;
        while (pos + 4 <= limit) {
            const uint32_t m = p[pos + 1];
            if (p[pos] != 0xFF || m == 0xFF || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) break;
            const uint32_t seg = ((uint32_t)p[pos + 2] << 8) | p[pos + 3];
            const uint32_t end = pos + 2 + seg;
            if (seg < 2 || end > limit) break;
            if (m == 0xDA) {
                const uint32_t want = end + (uint32_t)JPGPU_DEVICE_HEAD_PAD;
                result = want < limit ? want : limit;
                break;
            }
            pos = end;
        }
    }
    head_len[i] = result;
}

// Where head i goes in the packed buffer: head_off[i] = sum of the heads in front of it, each rounded up to 16 bytes; head_off[n] =
// the total.  One workgroup: lane t adds up its run of ceil(n / 256) files, lane 0 turns the 256 sums into bases, every lane writes
// its run's offsets.  n is a batch's files -- thousands: not worth more than this.
__global__ __launch_bounds__(256) void head_scan_kernel(const uint32_t *__restrict__ head_len, int n, uint64_t *__restrict__ head_off) {
    __shared__ uint64_t sh[256];
    const int per = (n + 255) / 256;
    const int lo = (int)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    uint64_t sum = 0;
    for (int i = lo; i < hi; i++) sum += ((head_len[i] & ~kHeadGaveUp) + 15u) & ~15u;
    sh[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int t = 0; t < 256; t++) {
            const uint64_t s = sh[t];
            sh[t] = run;
            run += s;
        }
        head_off[n] = run;
    }
    __syncthreads();
    uint64_t at = sh[threadIdx.x];
    for (int i = lo; i < hi; i++) {
        head_off[i] = at;
        at += ((head_len[i] & ~kHeadGaveUp) + 15u) & ~15u;
    }
}

// The heads packed into one buffer (head i at head_off[i], a multiple of 16), for one D2H copy.  One workgroup per file; the
// file's slot starts at a multiple of 256 and is padded to one, so whole aligned 16-byte pieces are moved.
__global__ __launch_bounds__(256) void head_pack_kernel(const uint8_t *__restrict__ data, const DeviceFile *__restrict__ files,
                                                        const uint32_t *__restrict__ head_len, const uint64_t *__restrict__ head_off,
                                                        uint8_t *__restrict__ heads) {
    const DeviceFile f = files[blockIdx.x];
    const uint32_t n16 = ((head_len[blockIdx.x] & ~kHeadGaveUp) + 15u) >> 4;
    const uint4 *s = reinterpret_cast<const uint4 *>(data + f.off);
    uint4 *d = reinterpret_cast<uint4 *>(heads + head_off[blockIdx.x]);
    for (uint32_t c = threadIdx.x; c < n16; c += 256u) d[c] = s[c];
}

// The two bytes at each verdict of first_marker_kernel (the host checks them for FF D9 and has no copy of a device file):
// bytes[k] = data[pos] | data[pos + 1] << 8 where first[k] = pos is a position with pos + 1 inside the segment, else 0.
__global__ __launch_bounds__(256) void verdict_bytes_kernel(const uint8_t *__restrict__ data, const uint2 *__restrict__ segs,
                                                            const uint32_t *__restrict__ seg_hi, const uint32_t *__restrict__ first, int n,
                                                            uint32_t *__restrict__ bytes) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= n) return;
    const uint64_t off = (uint64_t)segs[k].x | ((uint64_t)seg_hi[k] << 32);
    const uint32_t len = segs[k].y, pos = first[k];
    uint32_t b = 0;
    if (pos != 0xFFFFFFFFu && (uint64_t)pos + 1 < len) b = (uint32_t)data[off + pos] | ((uint32_t)data[off + pos + 1] << 8);
    bytes[k] = b;
}

hipError_t launch_gather_device(hipStream_t stream, const GatherPiece *pieces, int n_pieces, uint8_t *dst) {
    if (n_pieces <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_device_kernel, dim3((uint32_t)n_pieces), dim3(256), 0, stream, pieces, dst);
    return hipGetLastError();
}

hipError_t launch_head_walk(hipStream_t stream, const uint8_t *data, const DeviceFile *files, int n, uint32_t *head_len) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(head_walk_kernel, dim3((uint32_t)(n + 63) / 64u), dim3(64), 0, stream, data, files, n, head_len);
    return hipGetLastError();
}

hipError_t launch_head_scan(hipStream_t stream, const uint32_t *head_len, int n, uint64_t *head_off) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(head_scan_kernel, dim3(1), dim3(256), 0, stream, head_len, n, head_off);
    return hipGetLastError();
}

hipError_t launch_head_pack(hipStream_t stream, const uint8_t *data, const DeviceFile *files, int n, const uint32_t *head_len,
                            const uint64_t *head_off, uint8_t *heads) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(head_pack_kernel, dim3((uint32_t)n), dim3(256), 0, stream, data, files, head_len, head_off, heads);
    return hipGetLastError();
}

hipError_t launch_verdict_bytes(hipStream_t stream, const uint8_t *data, const void *segs, const uint32_t *seg_hi, const uint32_t *first,
                                int n, uint32_t *bytes) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(verdict_bytes_kernel, dim3((uint32_t)(n + 255) / 256u), dim3(256), 0, stream, data, (const uint2 *)segs, seg_hi, first, n,
                       bytes);
    return hipGetLastError();
}

}  // namespace jpgpu
