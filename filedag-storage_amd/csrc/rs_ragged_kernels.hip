// rs_ragged_kernels.hip -- rsmi_encode_ragged_batch_* on the GPU: the encode of a batch in which
// every block has its own shard size and its own rows.
//
// The host sorts the blocks into the aligned and the unaligned-window class (rsmi_ragged.cpp) and
// launches rs_ragged_kernel<K, MT, UA> once per class and tile of the encode plan over that
// class's units.  A unit is (block, first tile): up to kRaggedUnitTiles consecutive tiles of one
// block.  Workgroup e takes unit e, its wave w tile first + w, and a wave whose tile lies past
// its block's last leaves at once: no search, and no division by a per-block tile count.  What a
// uniform launch takes as kernel arguments a wave here reads per tile through scalar loads: the
// unit (8 bytes) and its block's descriptor (RaggedBlockDev: the block's rows, their strides, S
// and its chunks).  Every block of an encode shares the one plan, so the v_perm tables are staged
// once per workgroup behind the barrier, as in rs_fast_kernel.  The GF(2^8) work is
// gf_tile_columns with nontemporal loads; the stores are the coding kernels': whole windows
// inside [0, S) on unaligned-window blocks, store_rows_aligned (the row's last, partial chunk as
// dwords, then bytes) on aligned ones; lanes past the row's last chunk store nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"

namespace rsmi {

// Memory no kernel of the launch writes (the units, the descriptors, the plan), read at
// wave-uniform addresses: the constant address space makes every such read a scalar load, also
// behind the row stores of an earlier unit of the workgroup's walk.
template <class T>
using ConstPtr = const T __attribute__((address_space(4)))*;
template <class T>
__device__ __forceinline__ ConstPtr<T> const_ptr(const T* p) {
    return (ConstPtr<T>)(reinterpret_cast<uintptr_t>(p));
}

// A row address read from a descriptor: named global memory (the rows are device memory or
// page-locked host memory, never LDS or scratch), so the row loads and stores are global_load /
// global_store as in the kernels whose rows are kernel arguments, not flat ones.
__device__ __forceinline__ uint8_t* global_ptr(uint64_t addr) {
    return (uint8_t*)((uint8_t __attribute__((address_space(1)))*)(uintptr_t(addr)));
}

// plan: the encode plan's tile (K data rows in, MT parity rows out); units: the class's units;
// blocks: the descriptors they name.  The grid is nunits workgroups unless waves_per_cu caps it;
// the workgroups then stride over the units.
template <int K, int MT, bool UA>
__global__ __launch_bounds__(kFastWG, kMinWavesPerSimd) void rs_ragged_kernel(
    const RsPlanDev* __restrict__ plan, const RaggedUnit* __restrict__ units,
    const RaggedBlockDev* __restrict__ blocks, uint32_t nunits) {
    static_assert(kRaggedUnitTiles == kFastWG / kWave, "one tile per wave of the unit's workgroup");
    __shared__ u32x4 s_tbl[K * kColDwords / 4];
    {
        const uint32_t* src = plan->tbl;
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_tbl);
        for (int i = threadIdx.x; i < K * kColDwords; i += kFastWG) dst[i] = src[i];
    }
    __syncthreads();  // the kernel's only barrier: every wave passes it before any leaves

    constexpr int P = rows_in_flight<K, MT>();
    // write-heavy tiles store nontemporally, as the coding kernels' cache policy 1
    constexpr bool NTS = K < 4 * MT;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const ConstPtr<RsPlanDev> pl = const_ptr(plan);
    const ConstPtr<RaggedUnit> un = const_ptr(units);
    const ConstPtr<RaggedBlockDev> bd = const_ptr(blocks);

    for (uint32_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const uint32_t blk = un[u].blk, tile = un[u].tile + wid;
        const uint32_t S = bd[blk].S, cpb = bd[blk].cpb;
        if (tile * uint32_t(kWave) >= cpb) continue;  // past the block's last tile
        const uint8_t* ib = global_ptr(bd[blk].data);
        uint8_t* ob = global_ptr(bd[blk].parity);
        const uint64_t in_rs = bd[blk].data_rs, out_rs = bd[blk].parity_rs;
        uint64_t in_off[K], out_off[MT];
#pragma unroll
        for (int c = 0; c < K; c++) in_off[c] = uint64_t(pl->in_row[c]) * in_rs;
#pragma unroll
        for (int j = 0; j < MT; j++) out_off[j] = uint64_t(pl->out_row[j]) * out_rs;

        const LaneChunk lc = lane_chunk<UA>(tile, lane, cpb, S);
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
        gf_tile_columns<K, MT, P>(s_tbl, v, acc, GfNone{}, GfNone{}, GfNone{}, [&](int c, u32x4& x) {
            if (c + P < K) x = load_col(c + P);
        });
        if (lc.ch < cpb) {
            if constexpr (UA) {
#pragma unroll
                for (int j = 0; j < MT; j++)
                    st16u<NTS>(ob + out_off[j] + lc.win, u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]});
            } else {
                store_rows_aligned<NTS ? 1 : 0, MT>(ob, out_off, lc.ch, S, acc);
            }
        }
    }
}

template <int K, int MT>
static void fill_ragged_km(RaggedKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_ragged_kernel<K, MT, false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_ragged_kernel<K, MT, true>);
}

template <int K>
static void fill_ragged_k(RaggedKernelTable& t) {
    static_assert(ragged_shape(K), "the host classes blocks by ragged_shape");
    fill_ragged_km<K, 1>(t);
    fill_ragged_km<K, 2>(t);
    fill_ragged_km<K, 3>(t);
    fill_ragged_km<K, 4>(t);
}

// the K of the coding kernels: a block of such a shape has a class here, every other block takes
// the uniform call's launch
const RaggedKernelTable& ragged_kernels() {
    static const RaggedKernelTable t = [] {
        RaggedKernelTable x{};
        fill_ragged_k<1>(x);
        fill_ragged_k<2>(x);
        fill_ragged_k<3>(x);
        fill_ragged_k<4>(x);
        fill_ragged_k<5>(x);
        fill_ragged_k<6>(x);
        fill_ragged_k<8>(x);
        fill_ragged_k<10>(x);
        fill_ragged_k<12>(x);
        fill_ragged_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
