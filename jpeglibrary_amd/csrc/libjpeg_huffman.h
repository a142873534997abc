// jpeglibrary_amd/csrc/libjpeg_huffman.h -- libjpeg's optimal Huffman tables on the host (jchuff.c: jpeg_gen_optimal_table), what
// coding "optimized" and "progressive" of the libjpeg arithmetic build from a scan's statistics (include/jpgpu.h, 4e)
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "encode_kernels.h"

namespace jpgpu {

// freq[256] -> the DHT lists: bits16[l - 1] codes of length l, values[0 .. *n_values) by code length, then by symbol.
//   A pseudo-symbol 256 of frequency 1 keeps the all-ones code free.  Repeatedly the two least non-zero frequencies -- among equals the
// LARGEST index -- are merged, one bit added to the code size of every symbol on both chains; sizes up to 32 are then limited to 16
// (for i = 32 .. 17: while bits[i] > 0, j = i - 2 stepping down to a non-empty length; bits[i] -= 2, bits[i - 1]++, bits[j + 1] += 2,
// bits[j]--) and the pseudo-symbol leaves the longest non-empty length.  A histogram without any symbol gives the empty table: sixteen zero
// counts, no values (libjpeg never builds one; the pseudo-symbol alone has no code to leave).
inline void libjpeg_optimal_table(const uint32_t freq_in[256], uint8_t bits16[16], uint8_t values[256], int *n_values) {
    int64_t freq[257];
    int codesize[257], others[257], bits[33];
    bool any = false;
    for (int i = 0; i < 256; i++) {
        freq[i] = freq_in[i];
        any = any || freq_in[i] != 0;
    }
    if (!any) {
        memset(bits16, 0, 16);
        *n_values = 0;
        return;
    }
    freq[256] = 1;
    memset(codesize, 0, sizeof codesize);
    memset(bits, 0, sizeof bits);
    for (int i = 0; i < 257; i++) others[i] = -1;
    for (;;) {
        int c1 = -1, c2 = -1;
        int64_t v = INT64_MAX;
        for (int i = 0; i <= 256; i++)
            if (freq[i] && freq[i] <= v) v = freq[i], c1 = i;
        v = INT64_MAX;
        for (int i = 0; i <= 256; i++)
            if (freq[i] && freq[i] <= v && i != c1) v = freq[i], c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        for (codesize[c1]++; others[c1] >= 0;) {
            c1 = others[c1];
            codesize[c1]++;
        }
        others[c1] = c2;
        for (codesize[c2]++; others[c2] >= 0;) {
            c2 = others[c2];
            codesize[c2]++;
        }
    }
    for (int i = 0; i <= 256; i++)
        if (codesize[i]) bits[codesize[i] > 32 ? 32 : codesize[i]]++;  // (256 symbols of 32-bit counts stay below 32 by far)
    for (int i = 32; i > 16; i--)
        while (bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && bits[j] == 0) j--;
            if (j == 0) break;  // (no shorter code to split: cannot happen for a code tree, whose lengths satisfy Kraft's equality)
            bits[i] -= 2;
            bits[i - 1]++;
            bits[j + 1] += 2;
            bits[j]--;
        }
    int longest = 16;
    while (longest > 0 && bits[longest] == 0) longest--;
    if (longest > 0) bits[longest]--;
    for (int l = 1; l <= 16; l++) bits16[l - 1] = (uint8_t)bits[l];
    int n = 0;
    for (int size = 1; size <= 32; size++)
        for (int s = 0; s < 256; s++)
            if (codesize[s] == size) values[n++] = (uint8_t)s;
    *n_values = n;
}

// The table built from `freq` in both its forms: by symbol for the kernels, and as a DHT segment's body (Tc/Th, 16 counts, the values)
inline void libjpeg_build_table(const uint32_t freq[256], uint8_t tc_th, EncHuffTable *table, std::vector<uint8_t> *dht_body) {
    uint8_t bits[16], values[256];
    int n = 0;
    libjpeg_optimal_table(freq, bits, values, &n);
    memset(table, 0, sizeof *table);
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; l++) {  // T.81 Annex C
        for (int c = 0; c < bits[l - 1]; c++, k++, code++) {
            table->code[values[k]] = (uint16_t)code;
            table->len[values[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
    dht_body->assign(1, tc_th);
    dht_body->insert(dht_body->end(), bits, bits + 16);
    dht_body->insert(dht_body->end(), values, values + n);
}

}  // namespace jpgpu
