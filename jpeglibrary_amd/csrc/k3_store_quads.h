// jpeglibrary_amd/csrc/k3_store_quads.h -- K3's interleaved rows stored as whole 64-byte blocks per lane quad (host + device:
// tests/test_k3_store_quads_cpu.py enumerates every claim below on the CPU)
//
// In the 4:2:0 / 4:2:2 fast layouts a task is one pixel row of one MCU: 48 bytes, held by its lane as three 16-byte registers o0, o1, o2.
// Stored by their owner, one store instruction writes 64 pieces of 16 bytes, 48 bytes apart.  When the four lanes of a quad hold four
// consecutive MCUs of one pixel row -- 192 contiguous bytes, twelve pieces c = 3 * lane + register -- the lanes exchange pieces first, so that
// store s writes pieces 4s .. 4s + 3: one aligned 64-byte block per quad and instruction.  Inside a block the pieces are dealt so that two
// lanes of every store keep a register of their own under the same name: an output dword costs two selected quad_perm moves, not three.
#pragma once
#include <stdint.h>

#ifndef JPGPU_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPGPU_HD __host__ __device__
#else
#define JPGPU_HD
#endif
#endif

namespace jpgpu {

constexpr uint32_t kK3QuadStores = 3, kK3QuadLanes = 4, kK3QuadPieceBytes = 16;

// what lane `lane` of a quad writes in store `store`: register src_reg (o0 / o1 / o2) of lane src_lane, which is piece `piece` of the quad
struct K3QuadMove {
    uint8_t src_lane, src_reg, piece;
};
JPGPU_HD constexpr K3QuadMove k3_quad_move(uint32_t store, uint32_t lane) {
    constexpr K3QuadMove table[kK3QuadStores][kK3QuadLanes] = {
        {{0, 0, 0}, {1, 0, 3}, {0, 1, 1}, {0, 2, 2}},
        {{1, 2, 5}, {1, 1, 4}, {2, 1, 7}, {2, 0, 6}},
        {{3, 0, 9}, {3, 1, 10}, {2, 2, 8}, {3, 2, 11}},
    };
    return table[store][lane];
}

// The lane's address in store `store`, as bytes from the start of ITS OWN 48 bytes (dst_px): dst_px - 48 * lane + 16 * piece.
// Sixteenths of it for the four lanes, one signed byte each (-7 .. 10), so that a lane takes its own with a shift and a sign extension.
JPGPU_HD constexpr uint32_t k3_quad_offsets_packed(uint32_t store) {
    uint32_t packed = 0;
    for (uint32_t lane = 0; lane < kK3QuadLanes; lane++) {
        const int32_t sixteenths = (int32_t)k3_quad_move(store, lane).piece - 3 * (int32_t)lane;
        packed |= ((uint32_t)sixteenths & 0xFFu) << (8 * lane);
    }
    return packed;
}
JPGPU_HD inline uint32_t k3_quad_lane_offset(uint32_t packed, uint32_t lane) {  // (two's complement: added to a 32-bit offset that is at least 48 * lane)
    return (uint32_t)((int32_t)(int8_t)(packed >> (8 * (lane & 3u))) * (int32_t)kK3QuadPieceBytes);
}

// A tile of n_mcu MCUs whose first MCU is column gx0 of a line of mpl MCUs: tasks t .. t + 3 (t a multiple of 4: the workgroup's size is
// one) are MCUs m .. m + 3 of one pixel row of the tile, in one MCU line of the image and side by side there.  Wave-uniform.
JPGPU_HD inline bool k3_quad_eligible(uint32_t n_mcu, uint32_t mpl, uint32_t gx0) { return ((n_mcu | mpl | gx0) & 3u) == 0; }

}  // namespace jpgpu
