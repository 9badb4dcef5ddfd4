// rs_mixed_kernels.hip -- rsmi_reconstruct_mixed_batch_* on the GPU: the in-place reconstruct of a
// batch in which every block has its own erasure pattern.
//
// The host sorts the blocks by the number of rows their pattern rebuilds (rsmi_mixed.cpp) and
// launches rs_mixed_kernel<K, MT, UA> once per class MT over that class's tiles only.  Tile t of a
// launch is tile t % tpb of list entry t / tpb; the entry names the block and the pattern, the
// pattern names the one-tile plan the uniform call uses for it (reconstruct_plan).  What a uniform
// launch takes once, a wave here takes per tile, all of it through scalar loads: the entry, the
// plan pointer, the plan's K input and MT output rows.  The v_perm tables are per wave as well: a
// workgroup's four waves may hold tiles of four blocks with four plans, so each wave stages its
// own LDS slice (K x 80 bytes) and waits on its own LDS counter.  There is no workgroup barrier in
// this kernel: its waves start and leave on their own.  The GF(2^8) work is gf_tile_columns, the
// loads are nontemporal as in stripe_tile, the stores are the coding kernels': whole windows inside
// [0, S) on unaligned-window layouts, store_rows_aligned (the row's last, partial chunk as dwords,
// then bytes) on aligned ones; lanes past the row's last chunk store nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"
#include "rs_verify_tile.hpp"

namespace rsmi {

// Memory no kernel of the launch writes (the list, the plan pointers, the plans), read at
// wave-uniform addresses: the constant address space makes every such read a scalar load, also
// behind the row stores of an earlier tile of the wave's walk.
template <class T>
using ConstPtr = const T __attribute__((address_space(4)))*;
template <class T>
__device__ __forceinline__ ConstPtr<T> const_ptr(const T* p) {
    return (ConstPtr<T>)(reinterpret_cast<uintptr_t>(p));
}

// list: the class's entries; plans[entry.pat]: the entry's plan; base, bs, rs: the batch's first
// block, block stride and row stride (in place: the plan's input and output rows are rows of one
// block).  ntiles = entries * tpb.
template <int K, int MT, bool UA>
__global__ __launch_bounds__(kFastWG, kMinWavesPerSimd) void rs_mixed_kernel(
    const MixedEntry* __restrict__ list, const RsPlanDev* const* __restrict__ plans, uint8_t* base, uint64_t bs,
    uint64_t rs, uint32_t S, uint32_t cpb, uint32_t tpb, uint32_t ntiles) {
    constexpr int kSlice = K * kColDwords / 4;  // a wave's tables, in 16-byte words
    __shared__ u32x4 s_tbl[(kFastWG / kWave) * kSlice];
    constexpr int P = rows_in_flight<K, MT>();

    const WaveTiles wt = wave_tiles<UA>();
    const uint32_t lane = wt.lane, nw = wt.nw;
    uint32_t t = wt.t;
    if (t >= ntiles) return;
    u32x4* tbl = s_tbl + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave) * kSlice;

    const ConstPtr<MixedEntry> lst = const_ptr(list);
    const ConstPtr<const RsPlanDev*> pls = const_ptr(plans);
    uint64_t in_off[K], out_off[MT];
    uint32_t staged = ~0u;  // the pattern whose tables and rows the wave holds

    for (TileWalk tw(t, nw, tpb); t < ntiles; t += nw, tw.next(tpb)) {
        const uint32_t blk = lst[tw.blk].blk, pat = lst[tw.blk].pat;
        if (pat != staged) {
            const RsPlanDev* pg = pls[pat];
            const ConstPtr<RsPlanDev> plan = const_ptr(pg);
#pragma unroll
            for (int c = 0; c < K; c++) in_off[c] = uint64_t(plan->in_row[c]) * rs;
#pragma unroll
            for (int j = 0; j < MT; j++) out_off[j] = uint64_t(plan->out_row[j]) * rs;
            // the wave's own slice: LDS serves a wave's accesses in order, so the reads of the tile
            // before are served before these writes, and the wait below is for the writes of this
            // wave alone
            const u32x4* src = reinterpret_cast<const u32x4*>(pg->tbl);
            for (int i = int(lane); i < kSlice; i += kWave) tbl[i] = src[i];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            staged = pat;
        }
        uint8_t* ib = base + uint64_t(blk) * bs;
        const LaneChunk lc = lane_chunk<UA>(tw.tib, lane, cpb, S);
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
        gf_tile_columns<K, MT, P>(tbl, v, acc, GfNone{}, GfNone{}, GfNone{}, [&](int c, u32x4& x) {
            if (c + P < K) x = load_col(c + P);
        });
        if (lc.ch < cpb) {
            if constexpr (UA) {
#pragma unroll
                for (int j = 0; j < MT; j++)
                    st16u<false>(ib + out_off[j] + lc.win, u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]});
            } else {
                store_rows_aligned<0, MT>(ib, out_off, lc.ch, S, acc);
            }
        }
    }
}

template <int K, int MT>
static void fill_mixed_km(MixedKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_mixed_kernel<K, MT, false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_mixed_kernel<K, MT, true>);
}

template <int K>
static void fill_mixed_k(MixedKernelTable& t) {
    fill_mixed_km<K, 1>(t);
    fill_mixed_km<K, 2>(t);
    fill_mixed_km<K, 3>(t);
    fill_mixed_km<K, 4>(t);
}

// the K of the coding and verify kernels: a pattern of such a shape that rebuilds at most 4 rows
// has a class here, every other block takes the uniform call's launch
const MixedKernelTable& mixed_kernels() {
    static const MixedKernelTable t = [] {
        MixedKernelTable x{};
        fill_mixed_k<1>(x);
        fill_mixed_k<2>(x);
        fill_mixed_k<3>(x);
        fill_mixed_k<4>(x);
        fill_mixed_k<5>(x);
        fill_mixed_k<6>(x);
        fill_mixed_k<8>(x);
        fill_mixed_k<10>(x);
        fill_mixed_k<12>(x);
        fill_mixed_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
