// rs_mixed_fused_kernels.hip -- rsmi_reconstruct_mixed_batch_*_verify on the GPU: the in-place
// reconstruct of a batch in which every block has its own erasure pattern, and R(row) of the
// datanode entry checksum for every row the call reads (the pattern's K survivors) and writes (its
// MT rebuilt rows), from the one read of the survivors.
//
// rs_mixed_fused_kernel is rs_mixed_kernel's lookup (rs_mixed_kernels.hip: a class's list names the
// block and the pattern, the pattern names the one-tile plan; the entry, the plan pointer and the
// plan's rows are scalar loads through the constant address space) in rs_fused_mfma_kernel's
// geometry and with the fold of rs_crc_fold.hpp: a workgroup takes a unit of kFusedUnitTiles =
// 4 consecutive tiles of one block, wave w tile w.  Unit u of a launch is unit u % upb of list entry
// u / upb, so the four waves share one block and one plan and the v_perm tables are staged once per
// workgroup behind one barrier.  Every survivor chunk as loaded and every output chunk as computed
// goes into the fold, and the unit's record goes out, by list position, in the layout
// rs_crc16_combine_mfma_kernel (rs_crc16_kernels.hip) turns into R(row): slot c for survivor c,
// slot K + j for output j.  The launcher runs that kernel with the class's entries as its blocks,
// then rs_mixed_scatter_kernel, which moves the entry's K + MT values to the rows of the block they
// belong to.
//
// Unaligned-window layouts (UA): the outputs' last window is corrected from registers before the
// stores, the survivors' after them from a reload.  Lanes past the row's last chunk fold nothing
// and store nothing; padding never reaches a checksum and is never written.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc16.hpp"
#include "rs_crc_fold.hpp"
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
    const uint32_t u = fold_unit<UA>();
    if (u >= nunits) return;  // the whole workgroup, before its barrier
    const FoldUnit un = fold_unit_tiles(u, upb, tpb);  // the unit's block is its list entry
    const uint32_t ent = un.blk, t0 = un.t0, nt = un.nt;

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

    CrcFold<NACC> fold;
    fold.clear();

    // wave w takes tile w; a block's last unit may leave waves idle
    if (wid < nt) {
        uint64_t in_off[K], out_off[MT];
#pragma unroll
        for (int c = 0; c < K; c++) in_off[c] = uint64_t(plan->in_row[c]) * rs;
#pragma unroll
        for (int j = 0; j < MT; j++) out_off[j] = uint64_t(plan->out_row[j]) * rs;

        const LaneChunk lc = lane_chunk<UA>(t0 + wid, lane, cpb, S);
        fold.template tile_setup<UA>(t0 + wid, wid, lane, cpb, S, crc_tbl);
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
                fold.mfma(x, c, w);
                __builtin_amdgcn_sched_barrier(0);
            },
            [&](int c, const u32x4&) { fold.anchor(c); },
            [&](int c, u32x4& x) {
                if (c + P < K) x = load_col(c + P);
            });
        // the output rows' pass before the stores; UA: every row's last window went in unshifted:
        // the output rows' counts are corrected here, the survivors' after the stores
        fold.template rows<K, MT>(acc);
        if (UA && fold.fix) fold.template fix_rows<K, MT>(acc);
        if (lc.ch < cpb) {
            if constexpr (UA) {
#pragma unroll
                for (int j = 0; j < MT; j++)
                    st16u<false>(ib + out_off[j] + lc.win, u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]});
            } else {
                store_rows_aligned<0, MT>(ib, out_off, lc.ch, S, acc);
            }
        }
        if (UA && fold.fix) fold.template fix_reload<K, true>(ib, in_off, lc.win);
    }

    fold.finish(u, wid, lane, crc_rec);
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
