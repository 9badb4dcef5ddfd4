// rs_crc16_device.hpp -- CRC-16 device pieces shared by the fused encode + CRC-16 kernel's
// in-kernel combine (rs_coding_kernels.hpp) and the stand-alone CRC-16 passes
// (rs_crc16_kernels.hip); crc16.hpp has the algebra.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_crc_rows.hpp"
#include "rs_device.hpp"
#include "rs_plan.hpp"

namespace rsmi {

// A^(2^i)(s) through the nibble-sliced tables P4[i][4][16]
__device__ __forceinline__ uint32_t crc_pow4(const uint16_t* sQ, int i, uint32_t s) {
    const uint16_t* t = sQ + i * 64;
    return xor3(uint32_t(t[s & 15]), uint32_t(t[16 + ((s >> 4) & 15)]), uint32_t(t[32 + ((s >> 8) & 15)])) ^
           uint32_t(t[48 + ((s >> 12) & 15)]);
}

// Classes -> their end: class m (lane & 15) holds the value of chunks m, m + 16, m + 32, m + 48,
// relative to the end of chunk 48 + m; a 4-level scan over the 16 lanes (A^(16 * 2^j)) leaves
// sum_m A^(16 (15 - m)) (class m), the value relative to the end of chunk 63, in lane 15 of the row.
__device__ __forceinline__ uint32_t crc_class_scan(const uint16_t* sQ, uint32_t acc, uint32_t m) {
    return rows_scan<4>(acc, m, [&](int j, uint32_t a) { return crc_pow4(sQ, 4 + j, a); });  // 16 * 2^j bytes
}

// R(row) of rows 4 p + g (lane l = 16 g + m: class m) of one block from its unit records
// (rs_fused_mfma_kernel): for each unit h a lane gathers its class's 16-bit value from the
// class's four record bytes (one dword load; the loads of 8 units are issued before their power
// steps) and steps its running value by one unit (A^4096 for 4-tile units) before adding it; a
// 4-level scan over the 16 classes (A^(16 * 2^j)) then leaves the row's value relative to the end
// of the last unit in lane 15 of the group, and A^e, e = (S - that end) mod 32767 (column form),
// moves it to the row's end.  out[r] is written once (host memory allowed).
__device__ __forceinline__ void crc16_combine_rows(const uint16_t* sQ, const uint8_t* rec, uint32_t upb, uint32_t nacc,
                                                   uint32_t nsh, const Crc16Shift& sh, uint32_t* out, uint32_t p,
                                                   uint32_t lane) {
    const uint32_t m = lane & 15u, g = lane >> 4;
    const uint32_t r = g + 4u * p, rr = r < nsh ? r : nsh - 1;  // idle lanes repeat a row, store nothing
    const uint32_t sp = 4u * (rr & 1u);
    // the class's four bytes (j = 0..3) of accumulator rr / 2 in unit h
    const uint8_t* rb = rec + (rr >> 1) * kWave + m * 4u;
    uint32_t acc = 0;
    for (uint32_t h0 = 0; h0 < upb; h0 += 8) {
        uint32_t x[8];
#pragma unroll
        for (int hh = 0; hh < 8; hh++) {
            const uint32_t h = h0 + hh < upb ? h0 + hh : upb - 1;
            x[hh] = *reinterpret_cast<const uint32_t*>(rb + uint64_t(h) * nacc * kWave);
        }
#pragma unroll
        for (int hh = 0; hh < 8; hh++) {
            if (h0 + hh >= upb) break;
            const uint32_t y = x[hh] >> sp;
            const uint32_t v = (y & 15u) | ((y >> 4) & 0xF0u) | ((y >> 8) & 0xF00u) | ((y >> 12) & 0xF000u);
            acc = crc_pow4(sQ, 10 + kFusedUnitLog, acc) ^ v;  // earlier units move one unit further
        }
    }
    acc = crc_class_scan(sQ, acc, m);
    uint32_t y = 0;  // A^e(acc), column form
#pragma unroll
    for (int bit = 0; bit < 16; bit++) y ^= ((acc >> bit) & 1u) ? sh.col[bit] : 0u;
    if (m == 15 && r < nsh) out[r] = y;
}

}  // namespace rsmi
