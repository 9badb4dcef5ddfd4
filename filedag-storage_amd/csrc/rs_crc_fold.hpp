// rs_crc_fold.hpp -- the CRC-16 fold on the matrix cores that rs_fused_mfma_kernel
// (rs_coding_kernels.hpp), rs_scrub_mfma_kernel (rs_scrub_kernels.hip) and rs_mixed_fused_kernel
// (rs_mixed_fused_kernels.hip) share: R(row), the raw CRC-16 (crc16.hpp), of every row a kernel
// reads or writes, folded while it streams the stripe.  The kernels keep what is theirs (how a
// tile's rows are loaded, coded, compared and stored) and call the fold where its instructions are
// to stand: form w's MFMA between the GF work of dword w and w + 1 of an input row, the pass over
// the output rows before the stores, the input rows' correction after them.
//
// R(chunk) is GF(2)-linear in the chunk's 128 bits, so a tile's fold is a GF(2) matrix product
// evaluated as exact fp4 counts (v_mfma_scale_f32_16x16x128_f8f6f4, as in
// rs_crc16_rows_mfma_kernel): B = one data bit per nibble (forms x & 0x11111111, & 0x22..,
// & 0x44.. and (x >> 3) & 0x11111111 -- the GF tables want x >> 3 anyway), A = the weights of the
// tile's position in its unit (crc16.hpp FW, loaded once per tile and shared by every row).  Per
// row and tile: 4 bitwise ops per dword and 4 MFMAs, against 15 VALU and 8 LDS lookups per dword
// for the nibble fold.
//
// A unit is kFusedUnitTiles = 4 consecutive tiles of one block, taken by the 4 waves of one
// workgroup (one tile each), and the counts of a row accumulate over the unit's tiles, so the
// parity is read once per unit.  Two rows (slots 2 a and 2 a + 1) share one f32 accumulator: the
// odd slot's MFMAs run with B scale 2^12, and a unit's counts stay below 2^11 (4 tiles x 4 MFMAs x
// 128 products), so count0 + 2^12 count1 < 2^24 is exact in f32 and the parities are bits 0 and 12
// of the integer.  Record of a unit: per accumulator and lane l = 16 j + m, a byte whose bits 0-3 /
// 4-7 = parity of element i of the even / odd slot (CRC bit 4 j + i of class m: chunks m, m + 16,
// m + 32, m + 48 of the unit's tiles, relative to the end of chunk 48 + m of its last tile); four
// accumulators per dword, dword d of the unit at lane slot 4 m + j, so a class's four dwords are
// contiguous for rs_crc16_combine_mfma_kernel, which turns the records into R(row).
//
// Bytes at or past S count as zero: in a row's last tile the lane's chunk is masked to the bytes
// before S, and lanes past the row's last chunk (which loaded a clamped chunk) count nothing.
//
// UA: rows at any alignment and pitch (S >= 16; the Split layout), loaded as unaligned windows.
// The fold needs every lane's bytes at their chunk position: only the lane holding a row's last,
// overlapping window (it starts at S - 16, not at 16 ch) differs: its window must move right by
// dsh = 16 ch - (S - 16) bytes.  The rows go into the fold unshifted, and the row's last tile then
// adds (window XOR shifted window) of that lane alone (the counts only matter mod 2): for the rows
// a kernel holds in registers from those, and for its K input rows from a reload, so the common
// tiles carry none of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_crc_rows.hpp"
#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"

namespace rsmi {

// The unit a workgroup takes; UA: each XCD takes one contiguous eighth of the units (their rows
// share boundary lines, as the UA coding kernels' tiles do).  A launch's grid may run past its
// last unit: the kernel returns (u >= nunits) before it asks for the unit's tiles.
template <bool UA>
__device__ __forceinline__ uint32_t fold_unit() {
    return UA ? tile_group(blockIdx.x, gridDim.x, (gridDim.x & 7u) ? 0u : gridDim.x) : uint32_t(blockIdx.x);
}
// Unit u of a launch whose blocks (or list entries) have upb units of tpb tiles in all: its block,
// its first tile and its tiles (wave w takes tile t0 + w; a block's last unit may leave waves idle).
struct FoldUnit {
    uint32_t blk, t0, nt;
};
__device__ __forceinline__ FoldUnit fold_unit_tiles(uint32_t u, uint32_t upb, uint32_t tpb) {
    FoldUnit x;
    x.blk = u / upb;
    x.t0 = (u - x.blk * upb) * kFusedUnitTiles;
    x.nt = tpb - x.t0 < uint32_t(kFusedUnitTiles) ? tpb - x.t0 : uint32_t(kFusedUnitTiles);
    return x;
}

// a row of a tile as the kernels hold it: four dwords or one u32x4
__device__ __forceinline__ u32x4 fold_row(const uint32_t (&x)[4]) { return u32x4{x[0], x[1], x[2], x[3]}; }
__device__ __forceinline__ const u32x4& fold_row(const u32x4& x) { return x; }

// A wave's fold of NACC accumulators (slots 2 a and 2 a + 1 in accumulator a) over its tile of
// the unit.
template <int NACC>
struct CrcFold {
    mfma_v4f cacc[NACC];
    uint32_t mk[4];  // bytes of the lane's chunk that count
    u32x4 W[4];      // the tile position's weights, one operand per bit form
    uint32_t dsh;    // UA: the last window's shift to its chunk position (0 when S is a multiple of 16)
    bool fix, mine;  // fix, wave-uniform: this tile's last window moves; mine: this lane holds it

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int a = 0; a < NACC; a++) cacc[a] = mfma_v4f{0.f, 0.f, 0.f, 0.f};
    }

    // Tile `tile` of a row of cpb chunks, S bytes, at position pos of its unit.  The weights come
    // from global memory: the 16 KiB table stays in the L2, and a workgroup that staged it in LDS
    // first would hold its waves' HBM loads back by the staging's latency.
    template <bool UA>
    __device__ __forceinline__ void tile_setup(uint32_t tile, uint32_t pos, uint32_t lane, uint32_t cpb, uint32_t S,
                                               const uint32_t* crc_tbl) {
        const uint32_t ch = lane_chunk<UA>(tile, lane, cpb, S).ch;
        const bool last_tile = (tile + 1) * uint32_t(kWave * 16) > S;  // wave-uniform
        dsh = UA ? 16u * (cpb - 1u) - (S - 16u) : 0u;
        fix = UA && last_tile && dsh != 0u;
        mine = ch == cpb - 1u;
        // all-ones except in a row's last tile
#pragma unroll
        for (int w = 0; w < 4; w++) mk[w] = ~0u;
        if (last_tile) {
            const int valid = int(S) - int(ch * 16u);
#pragma unroll
            for (int w = 0; w < 4; w++) mk[w] = bytes_mask(valid - 4 * w);
        }
        const u32x4* wt = reinterpret_cast<const u32x4*>(crc_tbl + kCrcFWOff) + (4 - kFusedUnitTiles + pos) * 4 * kWave + lane;
#pragma unroll
        for (int q = 0; q < 4; q++) W[q] = wt[q * kWave];
    }

    // the window's 16 bytes shifted right by dsh bytes (1..15, zero fill): two u64 halves
    __device__ __forceinline__ u32x4 shifted(const u32x4& x) const {
        const uint64_t lo = uint64_t(x[0]) | (uint64_t(x[1]) << 32), hi = uint64_t(x[2]) | (uint64_t(x[3]) << 32);
        const uint32_t sb = 8u * dsh;
        const uint64_t nlo = sb == 0u ? lo : sb < 64u ? (lo >> sb) | (hi << ((64u - sb) & 63u)) : hi >> ((sb - 64u) & 63u);
        const uint64_t nhi = sb < 64u ? hi >> sb : 0u;
        return u32x4{uint32_t(nlo), uint32_t(nlo >> 32), uint32_t(nhi), uint32_t(nhi >> 32)};
    }
    // the correction that moves the window's bytes to their chunk position: the counts only matter
    // mod 2, so adding (window XOR shifted window), its lane alone, does it
    __device__ __forceinline__ u32x4 correction(const u32x4& x) const {
        const u32x4 y = shifted(x);
        return u32x4{mine ? x[0] ^ y[0] : 0u, mine ? x[1] ^ y[1] : 0u, mine ? x[2] ^ y[2] : 0u, mine ? x[3] ^ y[3] : 0u};
    }

    // one MFMA: bit form q of slot r's chunk x into the slot's accumulator (the odd slot of a pair
    // at B scale 2^12)
    __device__ __forceinline__ void mfma(const u32x4& x, int r, int q) {
        mfma_v4f& acc = cacc[r / 2];
        const uint32_t msk = q == 1 ? 0x22222222u : q == 2 ? 0x44444444u : 0x11111111u;
        mfma_v8i bd;
#pragma unroll
        for (int w = 0; w < 4; w++)
            bd[w] = int(__builtin_amdgcn_bitop3_b32(q < 3 ? x[w] : x[w] >> 3, mk[w], msk, 0x80));  // a & b & c
        bd[4] = bd[5] = bd[6] = bd[7] = 0;
        const u32x4 Wq = W[q];
        const mfma_v8i aw = {int(Wq[0]), int(Wq[1]), int(Wq[2]), int(Wq[3]), 0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aw, bd, acc, 4, 4, 0, 127, 0, (r & 1) ? 127 + 12 : 127);
    }
    // keep the MFMAs where they are issued: the accumulators are only read at the unit's end, so
    // without an anchor the MFMAs sink there and every row's bit forms stay live
    __device__ __forceinline__ void anchor(int r) { asm volatile("" : "+v"(cacc[r / 2])); }

    // The MT rows of slots K.. that the kernel holds in registers (uint32_t[MT][4] or u32x4[MT]):
    // bit form by bit form, even rows before odd ones, so consecutive MFMAs go to different
    // accumulators wherever two rows do not share one.
    template <int K, int MT, class Rows>
    __device__ __forceinline__ void rows(const Rows& x) {
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int j = h; j < MT; j += 2) mfma(fold_row(x[j]), K + j, q);
#pragma unroll
        for (int j = 0; j < MT; j++) anchor(K + j);
    }
    // Where fix is set (a UA row's last tile: every row's last window went in unshifted), those
    // rows' counts corrected from the registers
    template <int K, int MT, class Rows>
    __device__ __forceinline__ void fix_rows(const Rows& x) {
#pragma unroll
        for (int j = 0; j < MT; j++) {
            const u32x4 d = correction(fold_row(x[j]));
#pragma unroll
            for (int q = 0; q < 4; q++) mfma(d, K + j, q);
            anchor(K + j);
        }
    }
    // and the K input rows' (slots 0..K-1, row c at ib + in_off[c]) from a reload of the lane's
    // window at byte win: a shifted copy of every row in flight would not fit the registers.
    // NTL: the reload is nontemporal.
    template <int K, bool NTL>
    __device__ __forceinline__ void fix_reload(const uint8_t* ib, const uint64_t (&in_off)[K], uint32_t win) {
        // an opaque base: the reloads must not be merged with the row loop's loads (that would
        // keep every row's window live through the tile)
        const uint8_t* rb = ib;
        uint32_t rw = win;
        asm volatile("" : "+s"(rb), "+v"(rw));
#pragma unroll
        for (int c = 0; c < K; c++) {
            u32x4 x = {0u, 0u, 0u, 0u};
            if (mine) x = ld16u<NTL>(rb + in_off[c] + rw);  // that lane's 16 bytes only
            const u32x4 d = correction(x);
#pragma unroll
            for (int q = 0; q < 4; q++) mfma(d, c, q);
            anchor(c);  // one reload at a time
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // The end of unit u, every wave of the workgroup: the unit's four tiles meet in LDS (count sums
    // stay below 2^24: exact), and wave w reads out accumulators w, w + 4, ..., so no wave is left
    // with the whole unit's tail.  Parities -> the unit's record: byte (accumulator a, lane slot),
    // bits i / 4 + i = element i's parity of slot 2 a / 2 a + 1 (bits 0 and 12 of the exact count).
    __device__ __forceinline__ void finish(uint32_t u, uint32_t wid, uint32_t lane, uint8_t* crc_rec) {
        __shared__ mfma_v4f s_red[kWG / kWave][NACC][kWave];
#pragma unroll
        for (int a = 0; a < NACC; a++) s_red[wid][a][lane] = cacc[a];
        __syncthreads();
        for (int a = int(wid); a < NACC; a += kWG / kWave) {
            const mfma_v4f c = s_red[0][a][lane] + s_red[1][a][lane] + s_red[2][a][lane] + s_red[3][a][lane];
            uint32_t y = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) y |= (uint32_t(c[e]) & 0x1001u) << e;
            crc_rec[(uint64_t(u) * NACC + a) * kWave + (lane & 15u) * 4u + (lane >> 4)] = uint8_t(y | (y >> 8));
        }
    }
};

}  // namespace rsmi
