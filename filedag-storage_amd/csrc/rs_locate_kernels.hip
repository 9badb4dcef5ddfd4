// rs_locate_kernels.hip -- rsmi_locate on the GPU: which shard breaks a stripe?
//
// rs_locate_kernel is rs_verify_kernel up to the compare (verify_tiles, rs_verify_tile.hpp: one
// pass over the k + m rows, the same flags raised the same way), and on a tile with a non-zero
// syndrome it goes on to AND the set of shards that explain the tile into the block's candidate
// word (locate_tile).  A clean tile costs one more branch on the ballot the flags already take.
// rs_locate_verdict_kernel then turns a block's flags and candidates into its verdict.
// rs_locate_rows_kernel is the byte-granular form for the shapes rs_locate_kernel is not built
// for: it reads the encode of the data rows (context scratch) and the stored parity rows of the
// blocks whose flags are set.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rsmi.h"
#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"
#include "rs_verify_tile.hpp"

namespace rsmi {

// rplan: the plan of the ratio matrix R (rows 1..MT-1 are used), its tables staged in LDS behind
// the encode plan's.  cand: the launch's first block's candidate word, all-ones before the launch.
template <int K, int MT, bool UA>
__global__ __launch_bounds__(kFastWG, kMinWavesPerSimd) void rs_locate_kernel(
    const RsPlanDev* __restrict__ plan, const uint8_t* __restrict__ in, const uint8_t* __restrict__ par,
    uint64_t in_bs, uint64_t in_rs, uint64_t par_bs, uint64_t par_rs, uint32_t S, uint32_t cpb, uint32_t tpb,
    uint32_t ntiles, uint32_t* __restrict__ bad, uint32_t m, const RsPlanDev* __restrict__ rplan,
    uint32_t* __restrict__ cand) {
    __shared__ u32x4 s_tbl[2 * K * kColDwords / 4];
    stage_tables<K>(s_tbl, plan, rplan);
    verify_tiles<K, MT, UA, true>(s_tbl, plan, in, par, in_bs, in_rs, par_bs, par_rs, S, cpb, tpb, ntiles, bad, m,
                                  cand);
}

// One thread per block: culprit[b] from the block's m flags and its candidate words (words per
// block; null: none were formed, m = 1, where every shard explains any damage).
//   no flag set                         RSMI_LOCATE_CLEAN
//   exactly one candidate among 0..n-1  that shard
//   none, or more than one              RSMI_LOCATE_UNKNOWN
__global__ __launch_bounds__(kWG) void rs_locate_verdict_kernel(const uint32_t* __restrict__ bad,
                                                                const uint32_t* __restrict__ cand, uint32_t m,
                                                                uint32_t n, uint32_t words, uint64_t nblocks,
                                                                int32_t* __restrict__ culprit) {
    const uint64_t b = uint64_t(blockIdx.x) * kWG + threadIdx.x;
    if (b >= nblocks) return;
    uint32_t dirty = 0;
    for (uint32_t j = 0; j < m; j++) dirty |= bad[b * m + j];
    int32_t v = RSMI_LOCATE_CLEAN;
    if (dirty) {
        v = RSMI_LOCATE_UNKNOWN;
        int found = 0;
        for (uint32_t w = 0; cand && w < words; w++) {
            const uint32_t left = n - 32u * w;
            const uint32_t x = cand[b * words + w] & (left >= 32u ? ~0u : (1u << left) - 1u);
            if (x) {
                found += __popc(x);
                v = int32_t(32u * w) + (__ffs(x) - 1);
            }
        }
        if (found != 1) v = RSMI_LOCATE_UNKNOWN;
    }
    culprit[b] = v;
}

// Byte-granular locate of the blocks whose flags are set, any shape and alignment.  a: the encode
// of the data rows; b: the stored parity rows (m rows per block each), so syn_j = a_j ^ b_j.
// tbl: GF(2^8) log[256] | exp[512] | R[m][k] bytes (rsmi_locate_matrix), staged in LDS (R in the
// launch's dynamic LDS, m * k bytes).  A thread walks byte columns and keeps the candidates of
// its columns in registers; they are ANDed into the workgroup's words in LDS and from there into
// cand[block * words ..] (all-ones before the launch), with atomics that return nothing.
__global__ __launch_bounds__(kWG) void rs_locate_rows_kernel(const uint8_t* __restrict__ a, uint64_t a_rs,
                                                             uint64_t a_bs, const uint8_t* __restrict__ b,
                                                             uint64_t b_rs, uint64_t b_bs, uint64_t S, uint32_t k,
                                                             uint32_t m, uint64_t nblocks,
                                                             const uint32_t* __restrict__ bad,
                                                             const uint8_t* __restrict__ tbl,
                                                             uint32_t* __restrict__ cand) {
    constexpr int kWords = kMaxK / 32;
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_exp[512];
    __shared__ uint32_t s_cand[kWords];
    extern __shared__ uint8_t s_R[];
    for (uint32_t i = threadIdx.x; i < 256u; i += kWG) s_log[i] = tbl[i];
    for (uint32_t i = threadIdx.x; i < 512u; i += kWG) s_exp[i] = tbl[256u + i];
    for (uint32_t i = threadIdx.x; i < m * k; i += kWG) s_R[i] = tbl[768u + i];
    const uint32_t n = k + m, words = (n + 31u) / 32u;
    auto mul = [&](uint32_t x, uint32_t y) -> uint32_t {
        return x && y ? uint32_t(s_exp[uint32_t(s_log[x]) + uint32_t(s_log[y])]) : 0u;
    };

    for (uint64_t blk = blockIdx.y; blk < nblocks; blk += gridDim.y) {
        uint32_t flags = 0;  // uniform over the workgroup, as blk is
        for (uint32_t j = 0; j < m; j++) flags |= bad[blk * m + j];
        if (!flags) continue;
        __syncthreads();  // the tables are staged; the last block's words are read
        if (threadIdx.x < uint32_t(kWords)) s_cand[threadIdx.x] = ~0u;
        __syncthreads();
        const uint8_t* pa = a + blk * a_bs;
        const uint8_t* pb = b + blk * b_bs;
        auto syn = [&](uint32_t j, uint64_t x) -> uint32_t {
            return uint32_t(pa[uint64_t(j) * a_rs + x] ^ pb[uint64_t(j) * b_rs + x]);
        };
        uint32_t mine[kWords];
#pragma unroll
        for (int w = 0; w < kWords; w++) mine[w] = ~0u;
        for (uint64_t x = uint64_t(blockIdx.x) * kWG + threadIdx.x; x < S; x += uint64_t(gridDim.x) * kWG) {
            const uint32_t s0 = syn(0, x);
            uint32_t nz = 0, last = 0;  // the non-zero syndromes of the column, and the last of them
            for (uint32_t j = 0; j < m; j++)
                if (syn(j, x)) {
                    nz++;
                    last = j;
                }
            if (!nz) continue;
#pragma unroll
            for (int w = 0; w < kWords; w++) {
                if (uint32_t(w) >= words) break;
                uint32_t pass = 0;
                for (uint32_t bit = 0; bit < 32u && 32u * w + bit < n; bit++) {
                    const uint32_t sh = 32u * w + bit;
                    bool ok;
                    if (sh < k) {  // a data shard: syn_j == R[j][sh] * syn_0 for every j >= 1
                        ok = true;
                        for (uint32_t j = 1; ok && j < m; j++) ok = syn(j, x) == mul(s_R[j * k + sh], s0);
                    } else {  // a parity shard: it holds the column's only non-zero syndrome
                        ok = nz == 1u && last == sh - k;
                    }
                    pass |= uint32_t(ok) << bit;
                }
                mine[w] &= pass;
            }
        }
#pragma unroll
        for (int w = 0; w < kWords; w++)
            if (uint32_t(w) < words && mine[w] != ~0u)
                (void)__hip_atomic_fetch_and(&s_cand[w], mine[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        if (threadIdx.x < words && s_cand[threadIdx.x] != ~0u)
            (void)__hip_atomic_fetch_and(cand + blk * words + threadIdx.x, s_cand[threadIdx.x], __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    }
}

void* locate_verdict_kernel() { return reinterpret_cast<void*>(&rs_locate_verdict_kernel); }
void* locate_rows_kernel() { return reinterpret_cast<void*>(&rs_locate_rows_kernel); }

template <int K, int MT>
static void fill_locate_km(LocateKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_locate_kernel<K, MT, false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_locate_kernel<K, MT, true>);
}

template <int K>
static void fill_locate_k(LocateKernelTable& t) {
    fill_locate_km<K, 2>(t);
    fill_locate_km<K, 3>(t);
    fill_locate_km<K, 4>(t);
}

// the K of the verify kernels, m = 2..4 (m = 1 names nothing: the verify launch serves it)
const LocateKernelTable& locate_kernels() {
    static const LocateKernelTable t = [] {
        LocateKernelTable x{};
        fill_locate_k<1>(x);
        fill_locate_k<2>(x);
        fill_locate_k<3>(x);
        fill_locate_k<4>(x);
        fill_locate_k<5>(x);
        fill_locate_k<6>(x);
        fill_locate_k<8>(x);
        fill_locate_k<10>(x);
        fill_locate_k<12>(x);
        fill_locate_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
