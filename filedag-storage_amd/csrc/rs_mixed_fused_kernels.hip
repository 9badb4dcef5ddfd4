// rs_mixed_fused_kernels.hip -- rsmi_reconstruct_mixed_batch_*_verify on the GPU: the in-place
// reconstruct of a batch in which every block has its own erasure pattern, and R(row) of the
// datanode entry checksum for every row the call reads (the pattern's K survivors) and writes (its
// MT rebuilt rows), from the one read of the survivors.
//
// rs_mixed_fused_kernel is rs_mixed_kernel's lookup (rs_mixed_kernels.hip: a class's list names the
// block and the pattern, the pattern names the one-tile plan; the entry, the plan pointer and the
// plan's rows are scalar loads through the constant address space) in rs_fused_mfma_kernel's
// geometry and with its fold (rs_coding_kernels.hpp): a workgroup takes a unit of kFusedUnitTiles =
// 4 consecutive tiles of one block, wave w tile w.  Unit u of a launch is unit u % upb of list entry
// u / upb, so the four waves share one block and one plan and the v_perm tables are staged once per
// workgroup behind one barrier.  Every survivor chunk as loaded and every output chunk as computed
// goes through four fp4 MFMAs with the weights of the tile's position in its unit (crc16.hpp FW),
// two shards to an f32 accumulator.  The four waves' counts meet in LDS and the unit's record goes
// out, by list position, in the layout rs_crc16_combine_mfma_kernel (rs_crc16_kernels.hip) turns
// into R(row): slot c for survivor c, slot K + j for output j.  The launcher runs that kernel with
// the class's entries as its blocks, then rs_mixed_scatter_kernel, which moves the entry's K + MT
// values to the rows of the block they belong to.
//
// The fold (crc_mfma, shifted / correction, record, the LDS meet) is a copy of the fused encode's,
// as the scrub's is: sharing it would have to leave every existing kernel's code unchanged.
// Unaligned-window layouts (UA) mask as the fused encode does: the lane that holds a row's last
// window folds the window's bytes before S at the chunk position, and the row's last tile then adds
// (window XOR shifted window) for that lane alone, the outputs from registers, the survivors from a
// reload of that lane's 16 bytes.  Lanes past the row's last chunk fold nothing and store nothing;
// padding never reaches a checksum and is never written.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc16.hpp"
#include "rs_crc_rows.hpp"
#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"

namespace rsmi {

// Memory no kernel of the launch writes (the list, the plan pointers, the plans), read at
// workgroup-uniform addresses: the constant address space makes every such read a scalar load.
template <class T>
using ConstPtr = const T __attribute__((address_space(4)))*;
template <class T>
__device__ __forceinline__ ConstPtr<T> const_ptr(const T* p) {
    return (ConstPtr<T>)(reinterpret_cast<uintptr_t>(p));
}

// list: the class's entries; plans[entry.pat]: the entry's plan; base, bs, rs: the segment's first
// block, block stride and row stride (in place: the plan's input and output rows are rows of one
// block).  nunits = entries * upb, one workgroup each.  crc_rec: the launch's first unit's record,
// NACC * 64 bytes per unit.
template <int K, int MT, int WPS, bool UA>
__global__ __launch_bounds__(kWG, WPS) void rs_mixed_fused_kernel(
    const MixedEntry* __restrict__ list, const RsPlanDev* const* __restrict__ plans, uint8_t* base, uint64_t bs,
    uint64_t rs, uint32_t S, uint32_t cpb, uint32_t tpb, uint32_t upb, uint32_t nunits,
    const uint32_t* __restrict__ crc_tbl, uint8_t* __restrict__ crc_rec) {
    static_assert(kFusedUnitTiles == kWG / kWave && kFastWG == kWG, "one tile per wave of the unit's workgroup");
    constexpr int NSH = K + MT;
    constexpr int NACC = (NSH + 1) / 2;  // two shards per accumulator
    constexpr int P = rows_in_flight<K, MT>();
    __shared__ u32x4 s_tbl[K * kColDwords / 4];

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    // UA: each XCD takes one contiguous eighth of the units (their rows share boundary lines)
    const uint32_t u =
        UA ? tile_group(blockIdx.x, gridDim.x, (gridDim.x & 7u) ? 0u : gridDim.x) : uint32_t(blockIdx.x);
    if (u >= nunits) return;  // the whole workgroup, before its barrier
    const uint32_t ent = u / upb;
    const uint32_t t0 = (u - ent * upb) * kFusedUnitTiles;
    const uint32_t nt = tpb - t0 < uint32_t(kFusedUnitTiles) ? tpb - t0 : uint32_t(kFusedUnitTiles);

    const ConstPtr<MixedEntry> lst = const_ptr(list);
    const uint32_t blk = lst[ent].blk, pat = lst[ent].pat;
    const RsPlanDev* pg = const_ptr(plans)[pat];
    const ConstPtr<RsPlanDev> plan = const_ptr(pg);
    {
        // the unit's four waves share the plan: its tables once per workgroup
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_tbl);
        for (int i = threadIdx.x; i < K * kColDwords; i += kWG) dst[i] = pg->tbl[i];
        __syncthreads();
    }
    uint8_t* ib = base + uint64_t(blk) * bs;

    mfma_v4f cacc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; a++) cacc[a] = mfma_v4f{0.f, 0.f, 0.f, 0.f};

    // wave w takes tile w; a block's last unit may leave waves idle
    if (wid < nt) {
        uint64_t in_off[K], out_off[MT];
#pragma unroll
        for (int c = 0; c < K; c++) in_off[c] = uint64_t(plan->in_row[c]) * rs;
#pragma unroll
        for (int j = 0; j < MT; j++) out_off[j] = uint64_t(plan->out_row[j]) * rs;

        const LaneChunk lc = lane_chunk<UA>(t0 + wid, lane, cpb, S);
        const bool last_tile = (t0 + wid + 1) * uint32_t(kWave * 16) > S;  // wave-uniform
        // UA: the last window's shift to its chunk position (0 when S is a multiple of 16)
        const uint32_t dsh = UA ? 16u * (cpb - 1u) - (S - 16u) : 0u;
        const bool fix = UA && last_tile && dsh != 0u;  // wave-uniform: this tile's last window moves
        const bool mine = lc.ch == cpb - 1u;
        // the window's 16 bytes shifted right by dsh bytes (1..15, zero fill): two u64 halves
        auto shifted = [&](const u32x4& x) -> u32x4 {
            const uint64_t lo = uint64_t(x[0]) | (uint64_t(x[1]) << 32), hi = uint64_t(x[2]) | (uint64_t(x[3]) << 32);
            const uint32_t sb = 8u * dsh;
            const uint64_t nlo = sb == 0u ? lo : sb < 64u ? (lo >> sb) | (hi << ((64u - sb) & 63u)) : hi >> ((sb - 64u) & 63u);
            const uint64_t nhi = sb < 64u ? hi >> sb : 0u;
            return u32x4{uint32_t(nlo), uint32_t(nlo >> 32), uint32_t(nhi), uint32_t(nhi >> 32)};
        };
        // the counts only matter mod 2, so adding (window XOR shifted window), its lane alone, moves
        // the window's bytes to their chunk position
        auto correction = [&](const u32x4& x) -> u32x4 {
            const u32x4 y = shifted(x);
            return u32x4{mine ? x[0] ^ y[0] : 0u, mine ? x[1] ^ y[1] : 0u, mine ? x[2] ^ y[2] : 0u, mine ? x[3] ^ y[3] : 0u};
        };
        // the fold's mask: the bytes of the lane's chunk position before S (lanes past the row's
        // last chunk, which loaded a clamped chunk, count nothing); all-ones except in a row's last tile
        uint32_t mk[4] = {~0u, ~0u, ~0u, ~0u};
        if (last_tile) {
            const int valid = int(S) - int(lc.ch * 16u);
#pragma unroll
            for (int w = 0; w < 4; w++) mk[w] = bytes_mask(valid - 4 * w);
        }
        // this tile position's weights, one operand per bit form, shared by every row (from global
        // memory: the 16 KiB table stays in the L2)
        const u32x4* wt = reinterpret_cast<const u32x4*>(crc_tbl + kCrcFWOff) + (4 - kFusedUnitTiles + wid) * 4 * kWave + lane;
        u32x4 W[4];
#pragma unroll
        for (int q = 0; q < 4; q++) W[q] = wt[q * kWave];
        // one MFMA: bit form q of shard slot r's chunk x into the slot's accumulator (the odd slot
        // of a pair at B scale 2^12)
        auto crc_mfma = [&](const u32x4& x, int r, int q) {
            mfma_v4f& acc = cacc[r / 2];
            const uint32_t msk = q == 1 ? 0x22222222u : q == 2 ? 0x44444444u : 0x11111111u;
            mfma_v8i bd;
#pragma unroll
            for (int w = 0; w < 4; w++)
                bd[w] = int(__builtin_amdgcn_bitop3_b32(q < 3 ? x[w] : x[w] >> 3, mk[w], msk, 0x80));  // a & b & c
            bd[4] = bd[5] = bd[6] = bd[7] = 0;
            const u32x4 Wq = W[q];
            const mfma_v8i aw = {int(Wq[0]), int(Wq[1]), int(Wq[2]), int(Wq[3]), 0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(aw, bd, acc, 4, 4, 0, 127, 0,
                                                                   (r & 1) ? 127 + 12 : 127);
        };
        // keep the MFMAs where they are issued: the accumulators are only read at the unit's end
        auto anchor = [&](int r) { asm volatile("" : "+v"(cacc[r / 2])); };
        auto load_col = [&](int c) {
            if constexpr (UA)
                return ld16u<true>(ib + in_off[c] + lc.win);
            else
                return ld16<true>(reinterpret_cast<const u32x4*>(ib + in_off[c]) + lc.chl);
        };

        u32x4 v[P];
#pragma unroll
        for (int c = 0; c < P; c++) v[c] = load_col(c);
        uint32_t acc[MT][4];
        gf_tile_columns<K, MT, P>(
            s_tbl, v, acc, GfNone{},
            // form w's MFMA between the GF work of dword w and w + 1, under the wave's own VALU stream
            [&](int c, int w, const u32x4& x) {
                crc_mfma(x, c, w);
                __builtin_amdgcn_sched_barrier(0);
            },
            [&](int c, const u32x4&) { anchor(c); },
            [&](int c, u32x4& x) {
                if (c + P < K) x = load_col(c + P);
            });
        // the output rows: bit form by bit form, even rows before odd ones, so consecutive MFMAs go
        // to different accumulators wherever two output rows do not share one
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int j = h; j < MT; j += 2) crc_mfma(u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]}, K + j, q);
#pragma unroll
        for (int j = 0; j < MT; j++) anchor(K + j);
        // UA: every row's last window went in unshifted; the output rows' counts are corrected from
        // registers here, the survivors' after the stores from a reload (a copy of every row would
        // not fit)
        if (UA && fix) {
#pragma unroll
            for (int j = 0; j < MT; j++) {
                const u32x4 d = correction(u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]});
#pragma unroll
                for (int q = 0; q < 4; q++) crc_mfma(d, K + j, q);
                anchor(K + j);
            }
        }
        if (lc.ch < cpb) {
            if constexpr (UA) {
#pragma unroll
                for (int j = 0; j < MT; j++)
                    st16u<false>(ib + out_off[j] + lc.win, u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]});
            } else {
                store_rows_aligned<0, MT>(ib, out_off, lc.ch, S, acc);
            }
        }
        if (UA && fix) {
            // an opaque base: the reloads must not be merged with the row loop's loads
            const uint8_t* rb = ib;
            uint32_t rw = lc.win;
            asm volatile("" : "+s"(rb), "+v"(rw));
#pragma unroll
            for (int c = 0; c < K; c++) {
                u32x4 x = {0u, 0u, 0u, 0u};
                if (mine) x = ld16u<true>(rb + in_off[c] + rw);  // that lane's 16 bytes only
                const u32x4 d = correction(x);
#pragma unroll
                for (int q = 0; q < 4; q++) crc_mfma(d, c, q);
                anchor(c);  // one reload at a time
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // parities -> the unit's record: byte (accumulator a, lane slot), bits i / 4 + i = element i's
    // parity of slot 2 a / 2 a + 1 (bits 0 and 12 of the exact count)
    auto record = [&](int a, const mfma_v4f& c) {
        uint32_t y = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) y |= (uint32_t(c[e]) & 0x1001u) << e;
        crc_rec[(uint64_t(u) * NACC + a) * kWave + (lane & 15u) * 4u + (lane >> 4)] = uint8_t(y | (y >> 8));
    };
    // the unit's four tiles meet in LDS (count sums stay below 2^24: exact), and wave w reads out
    // accumulators w, w + 4, ...
    __shared__ mfma_v4f s_red[kWG / kWave][NACC][kWave];
#pragma unroll
    for (int a = 0; a < NACC; a++) s_red[wid][a][lane] = cacc[a];
    __syncthreads();
    for (int a = int(wid); a < NACC; a += kWG / kWave)
        record(a, s_red[0][a][lane] + s_red[1][a][lane] + s_red[2][a][lane] + s_red[3][a][lane]);
}

// comb[e * nsh + s]: R of slot s (survivor s < K, output s - K) of the class's entry e, as the
// records' combine left it.  One thread per (entry, slot) moves it to the row of the block it is
// the checksum of: out[blk * n + row], out being the segment's first block's n words.
__global__ __launch_bounds__(kWG) void rs_mixed_scatter_kernel(const MixedEntry* __restrict__ list,
                                                               const RsPlanDev* const* __restrict__ plans,
                                                               const uint32_t* __restrict__ comb, uint32_t nsh,
                                                               uint32_t K, uint32_t n, uint32_t nitems,
                                                               uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * uint32_t(kWG) + threadIdx.x;
    if (i >= nitems) return;
    const uint32_t e = i / nsh, s = i - e * nsh;
    const MixedEntry x = list[e];
    const RsPlanDev* plan = plans[x.pat];
    const uint32_t row = s < K ? plan->in_row[s] : plan->out_row[s - K];
    if (row < n) out[uint64_t(x.blk) * n + row] = comb[i];
}

void* mixed_scatter_kernel() { return reinterpret_cast<void*>(&rs_mixed_scatter_kernel); }

template <int K, int MT>
static void fill_mixed_fused_km(MixedFusedKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_mixed_fused_kernel<K, MT, kFusedWavesPerSimd, false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_mixed_fused_kernel<K, MT, kFusedWavesPerSimd, true>);
}

template <int K>
static void fill_mixed_fused_k(MixedFusedKernelTable& t) {
    fill_mixed_fused_km<K, 1>(t);
    fill_mixed_fused_km<K, 2>(t);
    fill_mixed_fused_km<K, 3>(t);
    fill_mixed_fused_km<K, 4>(t);
}

// the shapes of rs_mixed_kernel, both layouts
const MixedFusedKernelTable& mixed_fused_kernels() {
    static const MixedFusedKernelTable t = [] {
        MixedFusedKernelTable x{};
        fill_mixed_fused_k<1>(x);
        fill_mixed_fused_k<2>(x);
        fill_mixed_fused_k<3>(x);
        fill_mixed_fused_k<4>(x);
        fill_mixed_fused_k<5>(x);
        fill_mixed_fused_k<6>(x);
        fill_mixed_fused_k<8>(x);
        fill_mixed_fused_k<10>(x);
        fill_mixed_fused_k<12>(x);
        fill_mixed_fused_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
