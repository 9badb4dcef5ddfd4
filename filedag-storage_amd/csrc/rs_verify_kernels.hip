// rs_verify_kernels.hip -- Encoder.Verify on the GPU: is every stored parity row what the encode
// of the block's data rows would produce?
//
// rs_verify_kernel runs the coding kernels' GF(2^8) pipeline (rs_gf_tile.hpp: v_perm tables in LDS,
// a ring of rows in flight, one scheduling region per column) over the tiles of the context's
// encode plan, but where the encode stores its MT output chunks the verify loads the MT *stored*
// parity chunks and compares.  It reads k + m rows and writes nothing: the same HBM bytes as the
// encode of the shape, all of them loads.  A mismatch raises bad[block * m + parity row] with one
// vector atomic OR from one lane of the wave that saw it, so a clean stripe issues no store and
// no atomic at all.
//
// Bytes that are not part of a row never count: lanes past the row's last chunk (their loads are
// clamped to a valid chunk) and, on aligned layouts, the bytes at or past S of the row's last,
// partial chunk -- the layout contract lets padding be read, so it may hold anything, in data
// rows and in parity rows alike.  On unaligned-window layouts (UA) the row's last window ends at
// S and overlaps the one before it; the overlapped bytes are compared twice, which is harmless.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"
#include "rs_verify_tile.hpp"

namespace rsmi {

// The tile loop is verify_tiles (rs_verify_tile.hpp), shared with rs_locate_kernel.
template <int K, int MT, bool UA>
__global__ __launch_bounds__(kFastWG, kMinWavesPerSimd) void rs_verify_kernel(
    const RsPlanDev* __restrict__ plan, const uint8_t* __restrict__ in, const uint8_t* __restrict__ par,
    uint64_t in_bs, uint64_t in_rs, uint64_t par_bs, uint64_t par_rs, uint32_t S, uint32_t cpb, uint32_t tpb,
    uint32_t ntiles, uint32_t* __restrict__ bad, uint32_t m) {
    __shared__ u32x4 s_tbl[K * kColDwords / 4];
    stage_tables<K>(s_tbl, plan, nullptr);
    verify_tiles<K, MT, UA, false>(s_tbl, plan, in, par, in_bs, in_rs, par_bs, par_rs, S, cpb, tpb, ntiles, bad, m,
                                   nullptr);
}

// Fallback compare for shapes rs_verify_kernel is not built for: rows a (the encode of the data
// rows, in context scratch) against the stored parity rows b over bytes [0, S), any alignment,
// bytewise.  nrows rows per block; raises bad[block * nrows + row] like rs_verify_kernel.
__global__ __launch_bounds__(kWG) void rs_compare_rows_kernel(const uint8_t* __restrict__ a, uint64_t a_rs,
                                                              uint64_t a_bs, const uint8_t* __restrict__ b,
                                                              uint64_t b_rs, uint64_t b_bs, uint64_t S, uint32_t nrows,
                                                              uint64_t nblocks, uint32_t* __restrict__ bad) {
    const uint64_t groups = (S + 3) / 4;
    for (uint64_t blk = blockIdx.y; blk < nblocks; blk += gridDim.y) {
        for (uint32_t j = 0; j < nrows; j++) {
            const uint8_t* pa = a + blk * a_bs + uint64_t(j) * a_rs;
            const uint8_t* pb = b + blk * b_bs + uint64_t(j) * b_rs;
            uint32_t d = 0;
            for (uint64_t g = uint64_t(blockIdx.x) * kWG + threadIdx.x; g < groups; g += uint64_t(gridDim.x) * kWG) {
                const uint64_t x0 = g * 4;
                const int nb = int(S - x0 < 4 ? S - x0 : 4);
                for (int i = 0; i < nb; i++) d |= uint32_t(pa[x0 + i] ^ pb[x0 + i]);
            }
            // every lane of the wave is here again: blk and j are uniform over the workgroup
            if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull && (threadIdx.x & (kWave - 1)) == 0u)
                __hip_atomic_fetch_or(bad + blk * nrows + j, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

void* compare_rows_kernel() { return reinterpret_cast<void*>(&rs_compare_rows_kernel); }

template <int K, int MT>
static void fill_verify_km(VerifyKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_verify_kernel<K, MT, false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_verify_kernel<K, MT, true>);
}

template <int K>
static void fill_verify_k(VerifyKernelTable& t) {
    fill_verify_km<K, 1>(t);
    fill_verify_km<K, 2>(t);
    fill_verify_km<K, 3>(t);
    fill_verify_km<K, 4>(t);
}

// the K of the coding kernels (rs_kernels.hip fast_kernels), every MT, both layouts
const VerifyKernelTable& verify_kernels() {
    static const VerifyKernelTable t = [] {
        VerifyKernelTable x{};
        fill_verify_k<1>(x);
        fill_verify_k<2>(x);
        fill_verify_k<3>(x);
        fill_verify_k<4>(x);
        fill_verify_k<5>(x);
        fill_verify_k<6>(x);
        fill_verify_k<8>(x);
        fill_verify_k<10>(x);
        fill_verify_k<12>(x);
        fill_verify_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
