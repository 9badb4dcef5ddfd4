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
#include "rs_crc_rows.hpp"
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
    acc = rows_scan<6>(acc, lane, [&](int j, uint32_t a) { return crc_pow4(sQ, 4 + j, a); });  // 16 * 2^j bytes
    const uint32_t val = uint32_t(__builtin_amdgcn_readlane(int(acc), kWave - 1));  // wave-uniform from here
    crc_item_add(sQ, lane, val, uint32_t((last_end - item_end) % kCrcOrder), col_e, word);
}

// the byte an item's value is relative to: the end of its last group, counted as 8 tiles; and the
// row's last item's (the launch's A^E starts there)
__device__ __forceinline__ uint64_t crc_item_end(const RowsItem& x) {
    return (uint64_t(x.t0) + (x.nt + kCrcSegTiles - 1) / kCrcSegTiles * kCrcSegTiles) * (kWave * 16);
}
__device__ __forceinline__ uint64_t crc_last_end(uint32_t tpb) {
    return (uint64_t(tpb) + kCrcSegTiles - 1) / kCrcSegTiles * kCrcSegTiles * (kWave * 16);
}

// LDS staging of the nibble passes: P4, then G[8][32][16]
struct CrcNibTables {
    const uint16_t* sQ;
    const uint8_t* nb;
};
__device__ __forceinline__ CrcNibTables crc_stage_nib(uint32_t (&s_tbl)[kCrcP4Words + kCrcGWords], const uint32_t* tbl) {
    for (int i = threadIdx.x; i < kCrcP4Words; i += kWG) s_tbl[i] = tbl[kCrcP4Off + i];
    for (int i = threadIdx.x; i < kCrcGWords; i += kWG) s_tbl[kCrcP4Words + i] = tbl[kCrcGOff + i];
    __syncthreads();
    return CrcNibTables{reinterpret_cast<const uint16_t*>(s_tbl), reinterpret_cast<const uint8_t*>(s_tbl + kCrcP4Words)};
}

// The nibble pass for rows at any byte alignment: byte-aligned loads on the row's own grid
// (crc_chunk_load), a group's loads issued before its folds.
__global__ __launch_bounds__(kWG) void rs_crc16_rows_kernel(const uint32_t* __restrict__ tbl,
                                                            const uint8_t* __restrict__ base, uint64_t bstride,
                                                            uint64_t rpitch, uint32_t nrows, uint64_t S, uint32_t tpb,
                                                            uint32_t nsup, uint64_t nitems, uint32_t* __restrict__ out,
                                                            uint64_t out_bs, Crc16Shift sh) {
    __shared__ uint32_t s_tbl[kCrcP4Words + kCrcGWords];
    const CrcNibTables T = crc_stage_nib(s_tbl, tbl);
    const uint32_t col_e = lane_column(sh.col);  // A^E, lane-distributed
    const uint64_t last_end = crc_last_end(tpb);
    const RowsWave wv = rows_wave<kWG>();
    const uint32_t lane = wv.lane;
    for (uint64_t it = wv.it0; it < nitems; it += wv.nw) {
        const RowsItem x = rows_item(it, nsup, nrows, tpb);
        const uint8_t* row = base + x.b * bstride + uint64_t(x.r) * rpitch;
        uint32_t acc = 0;
        for (uint32_t g0 = 0; g0 < x.nt; g0 += kCrcSegTiles) {
            const uint32_t t0 = x.t0 + g0;
            const uint32_t nt = x.nt - g0 < uint32_t(kCrcSegTiles) ? x.nt - g0 : uint32_t(kCrcSegTiles);
            u32x4 v[kCrcSegTiles];
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++)
                if (uint32_t(i) < nt) v[i] = crc_chunk_load(row, (uint64_t(t0 + i) * kWave + lane) * 16, S);
            uint32_t gs = 0;  // the group's value, relative to the end of its 8th tile
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++)
                if (uint32_t(i) < nt) gs ^= crc_nib_chunk(T.nb + 1024 * i, v[i]);
            acc = crc_pow4(T.sQ, 13, acc) ^ gs;  // earlier groups move 8 KiB further from the end
        }
        crc_item_out(T.sQ, lane, acc, crc_item_end(x), last_end, col_e, out + x.b * out_bs + x.r);
    }
}

// The nibble pass for 16-byte-aligned rows (the default): rows_pipe (rs_crc_rows.hpp) with the
// tile-set tables G, A^8192 from P4 and crc_item_out; 12 KiB of LDS per workgroup.
__global__ __launch_bounds__(kWG) void rs_crc16_rows_pipe_kernel(const uint32_t* __restrict__ tbl,
                                                                 const uint8_t* __restrict__ base, uint64_t bstride,
                                                                 uint64_t rpitch, uint32_t nrows, uint64_t S,
                                                                 uint32_t tpb, uint32_t nsup, uint64_t nitems,
                                                                 uint32_t* __restrict__ out, uint64_t out_bs,
                                                                 Crc16Shift sh) {
    __shared__ uint32_t s_tbl[kCrcP4Words + kCrcGWords];
    const CrcNibTables T = crc_stage_nib(s_tbl, tbl);
    const uint32_t col_e = lane_column(sh.col);  // A^E, lane-distributed
    const uint64_t last_end = crc_last_end(tpb);
    const RowsWave wv = rows_wave<kWG>();
    const uint32_t lane = wv.lane;
    rows_pipe<false>(
        wv, base, bstride, rpitch, nrows, S, tpb, nsup, nitems,
        [&](uint32_t i, const u32x4& v) { return crc_nib_chunk(T.nb + 1024 * i, v); },
        [&](uint32_t acc) { return crc_pow4(T.sQ, 13, acc); },
        [&](uint32_t acc, const RowsItem& x, uint32_t) {
            crc_item_out(T.sQ, lane, acc, crc_item_end(x), last_end, col_e, out + x.b * out_bs + x.r);
        });
}

// The rows pass with the fold on the matrix cores.  R(chunk) is
// GF(2)-linear in the chunk's 128 bits, so a tile's fold is a GF(2) matrix product; the fp4
// MFMA v_mfma_scale_f32_16x16x128_f8f6f4 sums integer products exactly, and bit 0 of each count
// is the product's bit.  B = the tile's data, one data bit per fp4 nibble (fp4_bit_plane),
// column m = lane & 15, k block j = lane >> 4 (chunk 16 j + m); A = the weights of tile t of an
// 8-tile group (MW, in LDS, one ds_read_b128 per MFMA), row n = CRC bit; every product of a set
// data bit and a set weight is 1.0.  The counts of a whole group accumulate in one f32 quad (at
// most 4096 per count), so the parity is read once per group (ballot_class_value): lane m (< 16)
// gathers class m's value (chunks m, m + 16, m + 32, m + 48 of the group's tiles, relative to the
// end of chunk 48 + m of tile 7).  Groups step by A^8192 as in the nibble pass; at the item's end a
// 4-level scan over lanes 0..15 (A^(16 * 2^j)) leaves the value relative to the group's end in
// lane 15, and the shift to the row's end is the nibble pass's.  4 MFMAs and 20 VALU per tile fold
// what the nibble tables fold with 32 lookups and ~70 VALU.
//
// UA: rows at any byte alignment (the Split layout: rows back to back at pitch S) fold on the
// memory's 16-byte grid (RowSpan, rs_crc_rows.hpp), so every load is the aligned pass's; the shift
// to the row's end takes mis bytes more.
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
    const uint32_t col_e = lane_column(sh.col);  // A^E, lane-distributed
    const uint64_t last_end = crc_last_end(tpb);
    const RowsWave wv = rows_wave<kWG>();
    const uint32_t lane = wv.lane, m = lane & 15u;
    for (uint64_t it = wv.it0; it < nitems; it += wv.nw) {
        const RowsItem x = rows_item(it, nsup, nrows, tpb);
        const RowSpan<UA> sp = row_span<UA>(base + x.b * bstride + uint64_t(x.r) * rpitch, S);
        uint32_t acc = 0;  // lanes 0..15: class m's running value
        for (uint32_t g0 = 0; g0 < x.nt; g0 += kCrcSegTiles) {
            const uint32_t t0 = x.t0 + g0;
            const uint32_t nt = x.nt - g0 < uint32_t(kCrcSegTiles) ? x.nt - g0 : uint32_t(kCrcSegTiles);
            u32x4 v[kCrcSegTiles];
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++) v[i] = sp.load(t0 + i, lane);
            mfma_v4f c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++) {
                if (uint32_t(i) < nt) {
                    u32x4 d = v[i];
                    mask_row_ends<UA>(d, t0 + i, lane, sp);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const mfma_v8i bd = fp4_bit_plane(d, q);
                        const u32x4 wt = s_w[(i * 4 + q) * kWave + lane];
                        const mfma_v8i aw = {int(wt[0]), int(wt[1]), int(wt[2]), int(wt[3]), 0, 0, 0, 0};
                        c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aw, bd, c, 4, 4, 0, 127, 0, 127);
                    }
                }
            }
            // earlier groups move 8 KiB further from the end
            acc = crc_pow4(sQ, 13, acc) ^ ballot_class_value(c, m);
        }
        // classes -> the group's end, in lane 15 (wave-uniform from here)
        const uint32_t val = uint32_t(__builtin_amdgcn_readlane(int(crc_class_scan(sQ, acc, m)), 15));
        // UA: the item's end lies mis bytes before its end on the row's grid
        crc_item_add(sQ, lane, val, uint32_t((last_end - crc_item_end(x) + sp.mis) % kCrcOrder), col_e,
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
                   : reinterpret_cast<void*>(&rs_crc16_rows_kernel);
}

// The named forms of the rows passes (NamedRows, rs_crc_rows.hpp): R(row) of the rows a device array
// names, per block, in a stripe's two halves.  Tables, folds, scans and end shifts are the regular
// passes'; only the item source differs.  UA (either half off the 16-byte grid): the memory-grid
// fold (RowSpan), an item's end mis bytes before its end on the row's grid, for both folds.

// the nibble fold: rows_pipe_named with the tile-set tables G, A^8192 from P4 and crc_item_out
template <bool UA>
__global__ __launch_bounds__(kWG) void rs_crc16_named_kernel(const uint32_t* __restrict__ tbl, NamedRowsArgs a,
                                                             uint64_t S, uint32_t tpb, uint32_t nsup, uint64_t nitems,
                                                             uint32_t* __restrict__ out, Crc16Shift sh) {
    __shared__ uint32_t s_tbl[kCrcP4Words + kCrcGWords];
    const CrcNibTables T = crc_stage_nib(s_tbl, tbl);
    const uint32_t col_e = lane_column(sh.col);  // A^E, lane-distributed
    const uint64_t last_end = crc_last_end(tpb);
    const RowsWave wv = rows_wave<kWG>();
    const uint32_t lane = wv.lane;
    const NamedRows src{a, tpb, nsup, out};
    rows_pipe_named<UA>(
        wv, src, S, nitems, [&](uint32_t i, const u32x4& v) { return crc_nib_chunk(T.nb + 1024 * i, v); },
        [&](uint32_t acc) { return crc_pow4(T.sQ, 13, acc); },
        [&](uint32_t acc, const NamedRows::Item& x, uint32_t mis) {
            crc_item_out(T.sQ, lane, acc, crc_item_end(RowsItem{x.b, x.r, x.t0, x.nt}) - mis, last_end, col_e,
                         src.word(x));
        });
}

// the fold on the matrix cores: rs_crc16_rows_mfma_kernel's item, for the items that name a row
template <bool UA>
__global__ __launch_bounds__(kWG) void rs_crc16_named_mfma_kernel(const uint32_t* __restrict__ tbl, NamedRowsArgs a,
                                                                  uint64_t S, uint32_t tpb, uint32_t nsup,
                                                                  uint64_t nitems, uint32_t* __restrict__ out,
                                                                  Crc16Shift sh) {
    __shared__ uint32_t s_p4[kCrcP4Words];
    __shared__ u32x4 s_w[kCrcMWWords / 4];
    for (int i = threadIdx.x; i < kCrcP4Words; i += kWG) s_p4[i] = tbl[kCrcP4Off + i];
    for (int i = threadIdx.x; i < kCrcMWWords / 4; i += kWG)
        s_w[i] = reinterpret_cast<const u32x4*>(tbl + kCrcMWOff)[i];
    __syncthreads();
    const uint16_t* sQ = reinterpret_cast<const uint16_t*>(s_p4);
    const uint32_t col_e = lane_column(sh.col);  // A^E, lane-distributed
    const uint64_t last_end = crc_last_end(tpb);
    const RowsWave wv = rows_wave<kWG>();
    const uint32_t lane = wv.lane, m = lane & 15u;
    const NamedRows src{a, tpb, nsup, out};
    for (uint64_t it = wv.it0; it < nitems; it += wv.nw) {
        NamedRows::Item x;
        if (!src.item(it, x)) continue;  // the entry names nothing
        const RowSpan<UA> sp = row_span<UA>(src.row(x), S);
        uint32_t acc = 0;  // lanes 0..15: class m's running value
        for (uint32_t g0 = 0; g0 < x.nt; g0 += kCrcSegTiles) {
            const uint32_t t0 = x.t0 + g0;
            const uint32_t nt = x.nt - g0 < uint32_t(kCrcSegTiles) ? x.nt - g0 : uint32_t(kCrcSegTiles);
            u32x4 v[kCrcSegTiles];
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++) v[i] = sp.load(t0 + i, lane);
            mfma_v4f c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < kCrcSegTiles; i++) {
                if (uint32_t(i) < nt) {
                    u32x4 d = v[i];
                    mask_row_ends<UA>(d, t0 + i, lane, sp);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const mfma_v8i bd = fp4_bit_plane(d, q);
                        const u32x4 wt = s_w[(i * 4 + q) * kWave + lane];
                        const mfma_v8i aw = {int(wt[0]), int(wt[1]), int(wt[2]), int(wt[3]), 0, 0, 0, 0};
                        c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aw, bd, c, 4, 4, 0, 127, 0, 127);
                    }
                }
            }
            acc = crc_pow4(sQ, 13, acc) ^ ballot_class_value(c, m);  // earlier groups move 8 KiB further
        }
        const uint32_t val = uint32_t(__builtin_amdgcn_readlane(int(crc_class_scan(sQ, acc, m)), 15));
        crc_item_add(sQ, lane, val,
                     uint32_t((last_end - crc_item_end(RowsItem{x.b, x.r, x.t0, x.nt}) + sp.mis) % kCrcOrder), col_e,
                     src.word(x));
    }
}

void* crc16_named_kernel(bool mfma, bool aligned) {
    if (mfma)
        return aligned ? reinterpret_cast<void*>(&rs_crc16_named_mfma_kernel<false>)
                       : reinterpret_cast<void*>(&rs_crc16_named_mfma_kernel<true>);
    return aligned ? reinterpret_cast<void*>(&rs_crc16_named_kernel<false>)
                   : reinterpret_cast<void*>(&rs_crc16_named_kernel<true>);
}

}  // namespace rsmi
