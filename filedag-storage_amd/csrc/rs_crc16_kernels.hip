// rs_crc16_kernels.hip -- the stand-alone CRC-16 passes over shard rows and the combines of the
// coding kernels' CRC records (rs_coding_kernels.hpp: rs_fast_kernel CRC, rs_fused_mfma_kernel).
//
// R(row) of the datanode entry checksum (crc16.hpp has the algebra).  A wave owns one item: a
// super-segment of up to kCrcSupGroups groups of kCrcSegTiles = 8 consecutive 1 KiB tiles of
// one row.  Each lane folds its 16-byte chunk of every tile with positional LDS lookups -- 32
// nibble lookups in 16-entry tables (every wave-wide lookup reads 8 distinct dwords in 8
// distinct banks, so it never conflicts).  Tile k of a group uses its own table set G[k]
// (relative to the group's end), so the folds of a group are independent and combine by XOR,
// and a running register carries the groups (A^8192 between them): no dependent power step per
// tile.  A Hillis-Steele scan over the 64 lanes (A^(16*2^j) per level) leaves the item's
// value, relative to the item's end, in lane 63; shifting it by (S - item end) mod 32767 bytes
// places it relative to the row's end, and one atomic XOR adds it into the row's word.  The
// scan and the shift cost about as much as 8 tiles of folding, so items span 32 tiles
// (8-tile items spent 30 % of the pass there).  Powers use nibble-sliced tables
// (P4, conflict-free, 1.9 KiB), so a workgroup stages 12 KiB of LDS.  Bytes at or past S read
// as zero (zero bytes contribute nothing to R, they only move the reference point, which the
// final shift accounts for).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc16.hpp"
#include "rs_crc16_device.hpp"
#include "rs_device.hpp"
#include "rs_plan.hpp"

namespace rsmi {

__device__ __forceinline__ uint32_t crc_nib_chunk(const uint8_t* nb, const u32x4& v) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        uint32_t lo = (v[w] << 1) & 0x1E1E1E1Eu, hi = (v[w] >> 3) & 0x1E1E1E1Eu;
        asm volatile("" : "+v"(lo), "+v"(hi));
        uint32_t l[8];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int p = 4 * w + q;
            l[2 * q] = *reinterpret_cast<const uint16_t*>(nb + 64 * p + ((lo >> (8 * q)) & 0xFF));
            l[2 * q + 1] = *reinterpret_cast<const uint16_t*>(nb + 64 * p + 32 + ((hi >> (8 * q)) & 0xFF));
        }
        c = xor3(c, xor3(l[0], l[1], l[2]), xor3(l[3], l[4], l[5])) ^ (l[6] ^ l[7]);
    }
    return c;
}

// M(s) for a 16x16 matrix held lane-distributed (lane l < 16 of every 16-lane row holds M's
// image of 1 << l) and a wave-uniform s: each lane keeps its column if bit l of s is set, and an
// XOR scan over the 16-lane row (DPP row_shr 1, 2, 4, 8) leaves the image in lane 15.  No LDS.
__device__ __forceinline__ uint32_t crc_apply_cols(uint32_t col, uint32_t s, uint32_t l16) {
    uint32_t x = ((s >> l16) & 1u) ? col : 0u;
    x ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(x), 0x111, 0xF, 0xF, false));  // row_shr:1
    x ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(x), 0x112, 0xF, 0xF, false));  // row_shr:2
    x ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(x), 0x114, 0xF, 0xF, false));  // row_shr:4
    x ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(x), 0x118, 0xF, 0xF, false));  // row_shr:8
    return uint32_t(__builtin_amdgcn_readlane(int(x), 15));
}

// An item's wave-uniform value -> row word: the shift to the row's end, one atomic XOR (lane 63).
// The shift is A^d (d = the bytes between the item's end and the last item's end, mod 32767:
// a few power steps, none for the row's last item) and then the launch's A^E (E = S - the last
// item's end) in column form.
__device__ __forceinline__ void crc_item_add(const uint16_t* sQ, uint32_t lane, uint32_t val, uint32_t d,
                                             uint32_t col_e, uint32_t* word) {
#pragma unroll
    for (int i = 0; i < kCrcPowers; i++)
        if ((d >> i) & 1) val = crc_pow4(sQ, i, val);
    val = crc_apply_cols(col_e, val, lane & 15u);
    if (lane == kWave - 1) atomicXor(word, val);
}

// The item's value -> row word: lane scan, then crc_item_add.
__device__ __forceinline__ void crc_item_out(const uint16_t* sQ, uint32_t lane, uint32_t acc, uint64_t item_end,
                                             uint64_t last_end, uint32_t col_e, uint32_t* word) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const uint32_t w = crc_pow4(sQ, 4 + j, acc);  // 16 * 2^j bytes
        const uint32_t t = __shfl_up(w, 1u << j);
        if (lane >= (1u << j)) acc ^= t;
    }
    const uint32_t val = uint32_t(__builtin_amdgcn_readlane(int(acc), kWave - 1));  // wave-uniform from here
    crc_item_add(sQ, lane, val, uint32_t((last_end - item_end) % kCrcOrder), col_e, word);
}

// Position of item `it` (nsup items per row): its row and first tile.
struct CrcItem {
    uint64_t b;
    uint32_t r, t0, nt;  // block, row in block, first tile, tiles in the item
};
__device__ __forceinline__ CrcItem crc_item(uint64_t it, uint32_t nsup, uint32_t nrows, uint32_t tpb) {
    constexpr uint32_t kSup = kCrcSupGroups * kCrcSegTiles;
    CrcItem x;
    uint32_t sup;
    if (it < (uint64_t(1) << 32)) {  // 32-bit divisions (scalar), the common case
        const uint32_t i32 = uint32_t(it), rid = i32 / nsup;
        sup = i32 - rid * nsup;
        const uint32_t b = rid / nrows;
        x.b = b;
        x.r = rid - b * nrows;
    } else {
        sup = uint32_t(it % nsup);
        const uint64_t rid = it / nsup;
        x.b = rid / nrows;
        x.r = uint32_t(rid - x.b * nrows);
    }
    x.t0 = sup * kSup;
    x.nt = tpb - x.t0 < kSup ? tpb - x.t0 : kSup;
    return x;
}
// the byte the item's value is relative to: the end of its last group, counted as 8 tiles
__device__ __forceinline__ uint64_t crc_item_end(const CrcItem& x) {
    return (uint64_t(x.t0) + (x.nt + kCrcSegTiles - 1) / kCrcSegTiles * kCrcSegTiles) * (kWave * 16);
}

// LDS staging shared by the rows passes: P4, then G
#define RSMI_CRC_ROWS_STAGE()                                                                             \
    __shared__ uint32_t s_tbl[kCrcP4Words + kCrcGWords];                                                  \
    for (int i = threadIdx.x; i < kCrcP4Words; i += kWG) s_tbl[i] = tbl[kCrcP4Off + i];                   \
    for (int i = threadIdx.x; i < kCrcGWords; i += kWG) s_tbl[kCrcP4Words + i] = tbl[kCrcGOff + i];       \
    __syncthreads();                                                                                      \
    const uint16_t* sQ = reinterpret_cast<const uint16_t*>(s_tbl);                                        \
    const uint8_t* nb = reinterpret_cast<const uint8_t*>(s_tbl + kCrcP4Words); /* G[8][32][16] */  \
    uint32_t col_e = 0; /* A^E, lane-distributed */                                                    \
    _Pragma("unroll") for (int b_ = 0; b_ < 16; b_++) col_e = (threadIdx.x & 15u) == uint32_t(b_) ? sh.col[b_] : col_e; \
    const uint64_t last_end = (uint64_t(tpb) + kCrcSegTiles - 1) / kCrcSegTiles * kCrcSegTiles * (kWave * 16);

template <bool ALIGNED>
__global__ __launch_bounds__(kWG) void rs_crc16_rows_kernel(const uint32_t* __restrict__ tbl,
                                                            const uint8_t* __restrict__ base, uint64_t bstride,
                                                            uint64_t rpitch, uint32_t nrows, uint64_t S, uint32_t tpb,
                                                            uint32_t nsup, uint64_t nitems, uint32_t* __restrict__ out,
                                                            uint64_t out_bs, Crc16Shift sh) {
    RSMI_CRC_ROWS_STAGE()
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t nw = uint64_t(gridDim.x) * (kWG / kWave);
    for (uint64_t it = uint64_t(blockIdx.x) * (kWG / kWave) + wid; it < nitems; it += nw) {
        const CrcItem x = crc_item(it, nsup, nrows, tpb);
        const uint8_t* row = base + x.b * bstride + uint64_t(x.r) * rpitch;
        uint32_t acc = 0;
        for (uint32_t g0 = 0; g0 < x.nt; g0 += kCrcSegTiles) {
            const uint32_t t0 = x.t0 + g0;
            const uint32_t nt = x.nt - g0 < uint32_t(kCrcSegTiles) ? x.nt - g0 : uint32_t(kCrcSegTiles);
            u32x4 v[kCrcSegTiles];
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++)
                if (uint32_t(i) < nt) {
                    const uint64_t off = (uint64_t(t0 + i) * kWave + lane) * 16;
                    // wave-uniform: only a row's last tile needs the per-lane bounds and masks
                    if (ALIGNED && (uint64_t(t0 + i) + 1) * (kWave * 16) <= S)
                        v[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row + off));
                    else
                        v[i] = crc_chunk_load<ALIGNED>(row, off, S);
                }
            uint32_t gs = 0;  // the group's value, relative to the end of its 8th tile
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++)
                if (uint32_t(i) < nt) gs ^= crc_nib_chunk(nb + 1024 * i, v[i]);
            acc = crc_pow4(sQ, 13, acc) ^ gs;  // earlier groups move 8 KiB further from the end
        }
        crc_item_out(sQ, lane, acc, crc_item_end(x), last_end, col_e, out + x.b * out_bs + x.r);
    }
}

// The nibble rows pass, software-pipelined, for 16-byte-aligned rows (the default).  A wave
// works in units of half a group (4 tiles) and issues the loads of its next unit (of this item
// or its next one) before it folds the current one (two register sets of 16 VGPRs, the loop
// unrolled by two), so its own fold covers the next unit's memory latency instead of only the
// other waves on the SIMD; half-group units keep the kernel under 64 VGPRs (8 waves per SIMD,
// with 12 KiB of LDS per workgroup).  Loads are unconditional -- chunks past the row's end read
// the row's last chunk and are masked to zero in the fold, and the prefetch past the wave's
// last unit re-reads that unit -- so no load sits behind a branch and the compiler's vmcnt
// waits count only the older set.
__global__ __launch_bounds__(kWG) void rs_crc16_rows_pipe_kernel(const uint32_t* __restrict__ tbl,
                                                                 const uint8_t* __restrict__ base, uint64_t bstride,
                                                                 uint64_t rpitch, uint32_t nrows, uint64_t S,
                                                                 uint32_t tpb, uint32_t nsup, uint64_t nitems,
                                                                 uint32_t* __restrict__ out, uint64_t out_bs,
                                                                 Crc16Shift sh) {
    RSMI_CRC_ROWS_STAGE()
    constexpr int kU = kCrcSegTiles / 2;  // tiles per unit
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t nw = uint64_t(gridDim.x) * (kWG / kWave);
    const uint64_t last = (S - 1) / 16 * 16;  // the row's last chunk (S > 0)
    // a unit of work: tiles t0 + 4 h .. t0 + 4 h + 3 of item it (its position computed once per item)
    struct Unit {
        uint64_t it;
        CrcItem x;
        uint32_t h;
    };
    auto at = [&](uint64_t it) -> Unit { return Unit{it, crc_item(it, nsup, nrows, tpb), 0}; };
    auto next = [&](const Unit& u) -> Unit {
        if ((u.h + 1) * kU < u.x.nt) return Unit{u.it, u.x, u.h + 1};
        return at(u.it + nw);
    };
    auto issue = [&](const Unit& u, u32x4(&v)[kU]) {
        const uint8_t* row = base + u.x.b * bstride + uint64_t(u.x.r) * rpitch;
#pragma unroll
        for (int i = 0; i < kU; i++) {
            const uint64_t off = (uint64_t(u.x.t0 + u.h * kU + i) * kWave + lane) * 16;
            v[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row + (off < last ? off : last)));
        }
    };
    uint32_t acc = 0, gs = 0;
    auto finish = [&](const Unit& u, u32x4(&v)[kU]) {
        const CrcItem& x = u.x;
        const uint32_t u0 = u.h * kU, t0 = x.t0 + u0;
        const uint32_t nt = x.nt - u0 < uint32_t(kU) ? x.nt - u0 : uint32_t(kU);
        const uint8_t* gt = nb + 1024 * kU * (u.h & 1);  // table sets of this half of the group
#pragma unroll
        for (int i = 0; i < kU; i++) {
            if (uint32_t(i) < nt) {
                if ((uint64_t(t0 + i) + 1) * (kWave * 16) > S) {  // wave-uniform: the row's last tile
                    const int64_t valid = int64_t(S) - int64_t((uint64_t(t0 + i) * kWave + lane) * 16);
#pragma unroll
                    for (int w = 0; w < 4; w++) v[i][w] &= bytes_mask(valid - 4 * w);
                }
                gs ^= crc_nib_chunk(gt + 1024 * i, v[i]);
            }
        }
        const bool item_end = u0 + kU >= x.nt;
        if ((u.h & 1) || item_end) {  // the group is complete
            acc = crc_pow4(sQ, 13, acc) ^ gs;  // earlier groups move 8 KiB further from the end
            gs = 0;
        }
        if (item_end) {
            crc_item_out(sQ, lane, acc, crc_item_end(x), last_end, col_e, out + x.b * out_bs + x.r);
            acc = 0;
        }
    };
    const uint64_t it0 = uint64_t(blockIdx.x) * (kWG / kWave) + wid;
    if (it0 >= nitems) return;
    Unit cur = at(it0);
    u32x4 va[kU], vb[kU];
    issue(cur, va);
    for (;;) {
        Unit nx = next(cur);
        bool more = nx.it < nitems;
        issue(more ? nx : cur, vb);
        finish(cur, va);
        if (!more) break;
        cur = nx;
        nx = next(cur);
        more = nx.it < nitems;
        issue(more ? nx : cur, va);
        finish(cur, vb);
        if (!more) break;
        cur = nx;
    }
}

// The rows pass with the fold on the matrix cores, aligned rows.  R(chunk) is
// GF(2)-linear in the chunk's 128 bits, so a tile's fold is a GF(2) matrix product; the fp4
// MFMA v_mfma_scale_f32_16x16x128_f8f6f4 sums integer products exactly, and bit 0 of each count
// is the product's bit.  B = the tile's data, one data bit per fp4 nibble (v & 0x11111111,
// 0x22.., 0x44.., (v >> 1) & 0x44..; bit 3 is the e2m1 sign), column m = lane & 15, k block
// j = lane >> 4 (chunk 16 j + m); A = the weights of tile t of an 8-tile group (MW, in LDS,
// one ds_read_b128 per MFMA), row n = CRC bit; every product of a set data bit and a set weight
// is 1.0.  The counts of a whole group accumulate in one f32 quad (at most 4096 per count), so
// the parity is read once per group: four ballots, and lane m (< 16) gathers class m's value
// (chunks m, m + 16, m + 32, m + 48 of the group's tiles, relative to the end of chunk 48 + m
// of tile 7).  Groups step by A^8192 as in the nibble pass; at the item's end a 4-level scan
// over lanes 0..15 (A^(16 * 2^j)) leaves the value relative to the group's end in lane 15, and
// the shift to the row's end is the nibble pass's.  4 MFMAs and 20 VALU per tile fold what the
// nibble tables fold with 32 lookups and ~70 VALU.
//
// UA: rows at any byte alignment (the Split layout: rows back to back at pitch S).  The fold runs
// on the memory's 16-byte grid instead of the row's: the row's bytes are folded where they lie,
// from the aligned chunk at or below the row's first byte (its mis = row & 15 leading bytes, the
// previous row's tail, masked to zero) to the aligned chunk holding its last byte (bytes past it
// masked), so every load is the aligned pass's and no data moves between lanes.  Only the reference
// point changes: an item's value is relative to its end on that grid, mis bytes before its end on
// the row's grid, so the shift to the row's end takes mis bytes more (the launch's tiles per row
// count mis + S bytes, S + 15 at most).
template <bool UA>
__global__ __launch_bounds__(kWG) void rs_crc16_rows_mfma_kernel(const uint32_t* __restrict__ tbl,
                                                                 const uint8_t* __restrict__ base, uint64_t bstride,
                                                                 uint64_t rpitch, uint32_t nrows, uint64_t S,
                                                                 uint32_t tpb, uint32_t nsup, uint64_t nitems,
                                                                 uint32_t* __restrict__ out, uint64_t out_bs,
                                                                 Crc16Shift sh) {
    __shared__ uint32_t s_p4[kCrcP4Words];
    __shared__ u32x4 s_w[kCrcMWWords / 4];
    for (int i = threadIdx.x; i < kCrcP4Words; i += kWG) s_p4[i] = tbl[kCrcP4Off + i];
    for (int i = threadIdx.x; i < kCrcMWWords / 4; i += kWG)
        s_w[i] = reinterpret_cast<const u32x4*>(tbl + kCrcMWOff)[i];
    __syncthreads();
    const uint16_t* sQ = reinterpret_cast<const uint16_t*>(s_p4);
    uint32_t col_e = 0;  // A^E, lane-distributed
#pragma unroll
    for (int b = 0; b < 16; b++) col_e = (threadIdx.x & 15u) == uint32_t(b) ? sh.col[b] : col_e;
    const uint64_t last_end = (uint64_t(tpb) + kCrcSegTiles - 1) / kCrcSegTiles * kCrcSegTiles * (kWave * 16);
    const uint32_t lane = threadIdx.x & (kWave - 1), m = lane & 15u;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t nw = uint64_t(gridDim.x) * (kWG / kWave);
    for (uint64_t it = uint64_t(blockIdx.x) * (kWG / kWave) + wid; it < nitems; it += nw) {
        const CrcItem x = crc_item(it, nsup, nrows, tpb);
        const uint8_t* row = base + x.b * bstride + uint64_t(x.r) * rpitch;
        // UA: the row's misalignment (wave-uniform), its aligned base and the aligned chunk that
        // holds its last byte
        const uint32_t mis = UA ? uint32_t(__builtin_amdgcn_readfirstlane(int(reinterpret_cast<uintptr_t>(row) & 15u))) : 0u;
        const uint8_t* rowa = row - mis;
        const uint64_t Sm = mis + S;  // the row's end on the memory grid
        const uint64_t lasta = (Sm - 1) / 16 * 16;
        uint32_t acc = 0;  // lanes 0..15: class m's running value
        for (uint32_t g0 = 0; g0 < x.nt; g0 += kCrcSegTiles) {
            const uint32_t t0 = x.t0 + g0;
            const uint32_t nt = x.nt - g0 < uint32_t(kCrcSegTiles) ? x.nt - g0 : uint32_t(kCrcSegTiles);
            u32x4 v[kCrcSegTiles];
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++) {
                const uint64_t off = (uint64_t(t0 + i) * kWave + lane) * 16;  // unconditional, clamped
                v[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rowa + (off < lasta ? off : lasta)));
            }
            mfma_v4f c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++) {
                if (uint32_t(i) < nt) {
                    u32x4 d = v[i];
                    if ((uint64_t(t0 + i) + 1) * (kWave * 16) > Sm) {  // wave-uniform: the row's last tile
                        const int64_t valid = int64_t(Sm) - int64_t((uint64_t(t0 + i) * kWave + lane) * 16);
#pragma unroll
                        for (int w = 0; w < 4; w++) d[w] &= bytes_mask(valid - 4 * w);
                    }
                    if (UA && t0 + i == 0 && mis != 0u && lane == 0) {  // UA: the bytes before the row
#pragma unroll
                        for (int w = 0; w < 4; w++) d[w] &= ~bytes_mask(int(mis) - 4 * w);  // dword w's leading bytes dropped
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        mfma_v8i bd;
#pragma unroll
                        for (int w = 0; w < 4; w++)
                            bd[w] = int(q < 3 ? d[w] & (0x11111111u << q) : (d[w] >> 1) & 0x44444444u);
                        bd[4] = bd[5] = bd[6] = bd[7] = 0;
                        const u32x4 wt = s_w[(i * 4 + q) * kWave + lane];
                        const mfma_v8i aw = {int(wt[0]), int(wt[1]), int(wt[2]), int(wt[3]), 0, 0, 0, 0};
                        c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aw, bd, c, 4, 4, 0, 127, 0, 127);
                    }
                }
            }
            // parity bits -> class m's 16-bit value: bit n of class m is bit 16 (n >> 2) + m of
            // ballot n & 3
            uint32_t Y = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint64_t bl = __builtin_amdgcn_ballot_w64((int(c[i]) & 1) != 0);
                const uint32_t lo = uint32_t(bl) >> m, hi = uint32_t(bl >> 32) >> m;
                Y |= ((lo & 0x10001u) | ((hi & 0x10001u) << 8)) << i;  // n = i, 4 + i (bit 16), 8 + i, 12 + i (bit 24)
            }
            const uint32_t val = (Y & 0x0F0Fu) | ((Y >> 12) & 0xF0F0u);
            acc = crc_pow4(sQ, 13, acc) ^ val;  // earlier groups move 8 KiB further from the end
        }
        // classes -> the group's end, in lane 15 (wave-uniform from here)
        const uint32_t val = uint32_t(__builtin_amdgcn_readlane(int(crc_class_scan(sQ, acc, m)), 15));
        // UA: the item's end lies mis bytes before its end on the row's grid
        crc_item_add(sQ, lane, val, uint32_t((last_end - crc_item_end(x) + mis) % kCrcOrder), col_e,
                     out + x.b * out_bs + x.r);
    }
}

void* crc16_rows_mfma_kernel(bool aligned) {
    return aligned ? reinterpret_cast<void*>(&rs_crc16_rows_mfma_kernel<false>)
                   : reinterpret_cast<void*>(&rs_crc16_rows_mfma_kernel<true>);
}

// R(row) from rs_fused_mfma_kernel's unit records (crc16_combine_rows, rs_crc16_device.hpp): a
// persistent grid whose waves take items (block b, row group p) in turn, lane l = 16 g + m class m
// of row 4 p + g (the workgroup stages the power tables once).  out[block * nsh + r] is written
// once (host memory allowed).
__global__ __launch_bounds__(kWG) void rs_crc16_combine_mfma_kernel(const uint32_t* __restrict__ tbl,
                                                                    const uint8_t* __restrict__ rec, uint32_t upb,
                                                                    uint32_t nacc, uint32_t nsh, Crc16Shift sh,
                                                                    uint64_t nblocks, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_p4[kCrcP4Words];
    for (int i = threadIdx.x; i < kCrcP4Words; i += kWG) s_p4[i] = tbl[kCrcP4Off + i];
    __syncthreads();
    const uint16_t* sQ = reinterpret_cast<const uint16_t*>(s_p4);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t npass = (nsh + 3) / 4;  // wave-uniform
    const uint64_t nitems = nblocks * npass, nw = uint64_t(gridDim.x) * (kWG / kWave);
    for (uint64_t it = uint64_t(blockIdx.x) * (kWG / kWave) + wid; it < nitems; it += nw) {
        const uint64_t b = it / npass;
        const uint32_t p = uint32_t(it - b * npass);
        crc16_combine_rows(sQ, rec + b * upb * nacc * kWave, upb, nacc, nsh, sh, out + b * nsh, p, lane);
    }
}

void* crc16_combine_mfma_kernel() { return reinterpret_cast<void*>(&rs_crc16_combine_mfma_kernel); }

// R(row) from the fused encode's tile records (rs_fast_kernel CRC): one wave per block (a
// persistent grid strides over blocks).  Lane l takes quads i = 64 j + l of the block (quad i =
// chunks 4i..4i+3, tile i / 16, record lane 4 (i % 16) + q), loads the quad values of every
// row (two rows per dword, ns2 * 16 bytes), and keeps one running register per row that steps
// by A^4096 (64 quads) between its quads; a lane scan (A^(64 * 2^j)) leaves the sums, relative
// to the end of the last step E = 4096 J bytes, in lane 63.  Lane r then takes row r's sum,
// moves it to the row's end (A^(S - E), mod 32767) and adds the row's tail (UA records: the
// last chunk, folded with its quad position's tables, so moved back by 16 (3 - q) to S).  out[block * nsh + r] is written once (host memory allowed).
template <int NS2>
__global__ __launch_bounds__(kWG) void rs_crc16_combine_kernel(const uint32_t* __restrict__ tbl,
                                                               const uint32_t* __restrict__ rec,
                                                               const uint32_t* __restrict__ tail, uint32_t tpb,
                                                               uint32_t nsh, uint64_t S, uint64_t nblocks,
                                                               uint32_t* __restrict__ out) {
    constexpr int R = 8 * NS2;  // rows carried per lane (padding rows stay zero)
    // nibble-sliced powers (P4, 1.9 KiB, 16-entry tables: conflict-free), 4 lookups per power
    __shared__ uint32_t s_tbl[kCrcP4Words];
    for (int i = threadIdx.x; i < kCrcP4Words; i += kWG) s_tbl[i] = tbl[kCrcP4Off + i];
    __syncthreads();
    auto pw = [&](int i, uint32_t x) { return crc_pow4(reinterpret_cast<const uint16_t*>(s_tbl), i, x); };
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t nw = uint64_t(gridDim.x) * (kWG / kWave);
    const uint32_t nq = 16 * tpb, J = (nq + kWave - 1) / kWave;
    int64_t e = (int64_t(S) - int64_t(J) * 4096) % int64_t(kCrcOrder);
    if (e < 0) e += kCrcOrder;
    const uint32_t qt = uint32_t((S + 15) / 16 - 1) & 3u;            // the tail chunk's lane in its quad
    const uint32_t et = (kCrcOrder - 16 * (3 - qt)) % kCrcOrder;      // A^-(16 (3 - q))
    for (uint64_t b = uint64_t(blockIdx.x) * (kWG / kWave) + wid; b < nblocks; b += nw) {
        uint32_t acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = 0;
        const uint32_t* rb = rec + uint64_t(b) * tpb * (NS2 * kWave);
        for (uint32_t j = 0; j < J; j++) {
            const uint32_t i = j * kWave + lane;
            u32x4 v[NS2];
#pragma unroll
            for (int s = 0; s < NS2; s++) {
                v[s] = u32x4{0, 0, 0, 0};
                if (i < nq) v[s] = *reinterpret_cast<const u32x4*>(rb + (i >> 4) * (NS2 * kWave) + s * kWave + (i & 15) * 4);
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                // row r = 8 s + 4 h + q: dword q of record s, half h
                const uint32_t x = (v[r / 8][r % 4] >> (16 * ((r / 4) & 1))) & 0xFFFFu;
                acc[r] = j ? pw(12, acc[r]) ^ x : x;  // earlier quads of this lane move 4 KiB
            }
        }
#pragma unroll
        for (int l = 0; l < 6; l++) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t w = pw(6 + l, acc[r]);  // 64 * 2^l bytes
                const uint32_t t = __shfl_up(w, 1u << l);
                if (lane >= (1u << l)) acc[r] ^= t;
            }
        }
        uint32_t x = 0;  // lane r: row r's sum
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t s = uint32_t(__builtin_amdgcn_readlane(int(acc[r]), kWave - 1));
            x = lane == uint32_t(r) ? s : x;
        }
        for (int k = 0; k < kCrcPowers; k++)
            if ((e >> k) & 1) x = pw(k, x);
        if (lane < nsh) {
            if (tail) {
                // the tail lane folded with its quad position's tables (relative to S + 16 (3 - q))
                uint32_t y = tail[b * nsh + lane];
                for (int k = 0; k < kCrcPowers; k++)
                    if ((et >> k) & 1) y = pw(k, y);
                x ^= y;
            }
            out[b * nsh + lane] = x;
        }
    }
}

void* crc16_combine_kernel(int ns2) {
    switch (ns2) {
        case 1: return reinterpret_cast<void*>(&rs_crc16_combine_kernel<1>);
        case 2: return reinterpret_cast<void*>(&rs_crc16_combine_kernel<2>);
        case 3: return reinterpret_cast<void*>(&rs_crc16_combine_kernel<3>);
        default: return nullptr;
    }
}

// aligned rows: the pipelined pass; any other layout: the plain nibble pass
void* crc16_rows_kernel(bool aligned) {
    return aligned ? reinterpret_cast<void*>(&rs_crc16_rows_pipe_kernel)
                   : reinterpret_cast<void*>(&rs_crc16_rows_kernel<false>);
}

}  // namespace rsmi
