// rs_gf_tile.hpp -- the GF(2^8) tile pipeline of the coding kernels (rs_coding_kernels.hpp) and the
// verify kernel (rs_verify_kernels.hip): the tile walk, the lane's chunk, the aligned row store, and
// the column loop gf_tile_columns, which rs_fused_mfma_kernel and rs_verify_kernel call and
// rs_fast_kernel writes out (its register budget: see there).
//
// GF multiply without MFMA: a product a*x is linear in the bits of x, so it is the XOR of three
// table lookups on bit fields of x (bits 0-2, 3-5, 6-7).  Each lookup is a single v_perm_b32 that
// selects 4 bytes at once from an 8-byte pool of products, with the field values as per-byte
// selectors.  Per input dword: 5 VALU ops build the three selector words (shared by all MT
// outputs); per (output, input) dword: 3 v_perm_b32 and 1.5 v_bitop3_b32 (3-input XOR).  Tables
// for the current column come from LDS by broadcast ds_read_b128 (same address in every lane).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_device.hpp"
#include "rs_plan.hpp"

namespace rsmi {

// Rows in flight per lane for the software pipeline: narrow outputs (MT <= 2) keep every
// input row in flight (registers are cheap there, measured +2.6% on RS(10,4) 1-row
// reconstruct); wide outputs keep a ring of 6.
template <int K, int MT>
constexpr int rows_in_flight() {
    constexpr int cap = MT <= 2 ? 16 : 6;
    return K < cap ? K : cap;
}

// A wave's walk over its tiles t, t + nw, ...: (block, tile in block) kept incrementally.
struct TileWalk {
    uint32_t blk, tib, step_b, step_t;
    __device__ __forceinline__ TileWalk(uint32_t t, uint32_t nw, uint32_t tpb)
        : blk(t / tpb), tib(t - blk * tpb), step_b(nw / tpb), step_t(nw - step_b * tpb) {}
    __device__ __forceinline__ void next(uint32_t tpb) {
        blk += step_b;
        tib += step_t;
        if (tib >= tpb) {
            tib -= tpb;
            blk++;
        }
    }
};

// A lane's 16-byte chunk of a row of cpb chunks: ch, its chunk of tile `tile` (lanes past the row's
// last chunk skip their stores); chl, the chunk it loads, clamped so loads stay unconditional; UA:
// win, the byte offset of its window, min(16 chl, S - 16) (the row's last window overlaps the one
// before it instead of running past S).
struct LaneChunk {
    uint32_t ch, chl, win;
};
template <bool UA>
__device__ __forceinline__ LaneChunk lane_chunk(uint32_t tile, uint32_t lane, uint32_t cpb, uint32_t S) {
    LaneChunk x;
    x.ch = tile * kWave + lane;
    x.chl = x.ch < cpb ? x.ch : cpb - 1;
    x.win = UA ? (x.chl * 16u < S - 16u ? x.chl * 16u : S - 16u) : 0u;
    return x;
}

// a callable of gf_tile_columns that a kernel has no use for
struct GfNone {
    template <class... A>
    __device__ __forceinline__ void operator()(A&&...) const {}
};

// acc[j] = XOR_c coef[j][c] * row c over a lane's chunk: the software pipeline over the K input
// rows.  v is a ring of P rows in flight, rows 0..P-1 already issued by the caller; there is one
// scheduling region per column (sched_barrier) so the compiler cannot hoist every load and table
// read to the top and blow the register budget.  s_tbl: the plan's tables in LDS, staged (and
// the workgroup's barrier passed) by the caller.  The callables are what differs between the
// kernels; c and w are constants once the loops are unrolled:
//   before_col(c, x)       before column c's GF work on x = v[c % P] (may rewrite x)
//   after_dword(c, w, x)   after the GF work of x's dword w
//   after_col(c, x)        after column c's GF work, before its slot is refilled
//   refill(c, x)           x's slot is free: issue the load that takes it (row c + P, if any)
template <int K, int MT, int P, class BeforeCol, class AfterDword, class AfterCol, class Refill>
__device__ __forceinline__ void gf_tile_columns(const u32x4* s_tbl, u32x4 (&v)[P], uint32_t (&acc)[MT][4],
                                                BeforeCol&& before_col, AfterDword&& after_dword,
                                                AfterCol&& after_col, Refill&& refill) {
    // acc ^= p1^p2^p3 per column, folded two columns at a time with 3-input XORs:
    // even columns leave p3 pending, odd columns retire it (1.5 VALU per column).
    uint32_t pend[MT][4];

    // Opaque per-tile table base: stops LICM from hoisting all K*20 table words out
    // of the tile loop (which would pin ~200 VGPRs and drop occupancy to 1 wave).
    uint32_t tb = 0;
    asm volatile("" : "+v"(tb));
    const u32x4* tbl = s_tbl + tb;
    u32x4 Tn[5];
#pragma unroll
    for (int f = 0; f < 5; f++) Tn[f] = tbl[f];

#pragma unroll
    for (int c = 0; c < K; c++) {
        const int slot = c % P;
        u32x4 T[5];
#pragma unroll
        for (int f = 0; f < 5; f++) T[f] = Tn[f];
        before_col(c, v[slot]);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t x = u4get(v[slot], w);
            const uint32_t s1 = x & 0x07070707u;
            const uint32_t s2 = (x >> 3) & 0x07070707u;
            const uint32_t s3 = (x >> 6) & 0x03030303u;
#pragma unroll
            for (int j = 0; j < MT; j++) {
                const uint32_t p1 = __builtin_amdgcn_perm(u4get(T[1], j), u4get(T[0], j), s1);
                const uint32_t p2 = __builtin_amdgcn_perm(u4get(T[3], j), u4get(T[2], j), s2);
                const uint32_t p3 = __builtin_amdgcn_perm(u4get(T[4], j), u4get(T[4], j), s3);
                uint32_t& a = acc[j][w];
                uint32_t& q = pend[j][w];
                if (c == 0 && K == 1) {
                    a = xor3(p1, p2, p3);
                } else if (c == 0) {
                    a = p1 ^ p2;
                    q = p3;
                } else if (c & 1) {
                    a = xor3(a, p1, p2);
                    a = xor3(a, p3, q);
                } else if (c == K - 1) {
                    a = xor3(a, p1, p2);
                    a ^= p3;
                } else {
                    a = xor3(a, p1, p2);
                    q = p3;
                }
            }
            after_dword(c, w, v[slot]);
        }
        after_col(c, v[slot]);
        refill(c, v[slot]);
        if (c + 1 < K) {
#pragma unroll
            for (int f = 0; f < 5; f++) Tn[f] = tbl[(c + 1) * 5 + f];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // Anchor the results outside the store predicate; otherwise the compiler sinks the
    // whole column pipeline into the `ch < cpb` branch and hoists every table read.
#pragma unroll
    for (int j = 0; j < MT; j++)
#pragma unroll
        for (int w = 0; w < 4; w++) asm volatile("" : "+v"(acc[j][w]));
}

// The output rows' chunk ch (< cpb) on an aligned layout: row j at ob + out_off[j].  A whole chunk
// is stored under the store policy ST (store_policy, rs_plan.hpp: 0 plain, 1 nontemporal, n >= 2
// nontemporal but the last n - 1 rows plain, -1 write-through); the row's last, partial chunk
// (1..15 bytes) is stored as whole dwords, then bytes, so no byte at or past S is ever written.
template <int ST, int MT>
__device__ __forceinline__ void store_rows_aligned(uint8_t* ob, const uint64_t (&out_off)[MT], uint32_t ch,
                                                   uint32_t S, const uint32_t (&acc)[MT][4]) {
    const uint32_t boff = ch * 16u;
    if (boff + 16u <= S) {
#pragma unroll
        for (int j = 0; j < MT; j++) {
            const u32x4 o = u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
            if constexpr (ST == kStoreWriteThrough)
                // buffer_store_dwordx4 sc0 sc1 (cache policy 17) through a raw descriptor of the
                // row's S bytes (gfx9 word 3: 32-bit data format), the chunk at byte boff
                __builtin_amdgcn_raw_buffer_store_b128(
                    o, __builtin_amdgcn_make_buffer_rsrc(ob + out_off[j], 0, int(S), 0x00020000), int(boff), 0, 17);
            else if constexpr (ST == 1)
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(ob + out_off[j]) + ch);
            else if (ST >= 2 && j + (ST - 1) < MT)  // a constant once the row loop is unrolled
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(ob + out_off[j]) + ch);
            else
                *(reinterpret_cast<u32x4*>(ob + out_off[j]) + ch) = o;
        }
    } else {
#pragma unroll
        for (int j = 0; j < MT; j++) {
            uint8_t* p = ob + out_off[j] + boff;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const uint32_t val = acc[j][w];
                const uint32_t o = boff + 4u * w;
                if (o + 4u <= S) {
                    *reinterpret_cast<uint32_t*>(p + 4 * w) = val;
                } else if (o < S) {
                    p[4 * w] = uint8_t(val);
                    if (o + 1u < S) p[4 * w + 1] = uint8_t(val >> 8);
                    if (o + 2u < S) p[4 * w + 2] = uint8_t(val >> 16);
                }
            }
        }
    }
}

}  // namespace rsmi
