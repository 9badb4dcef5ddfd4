// rs_heal_kernels.hip -- rsmi_heal on the GPU: rewrite the shard that breaks a stripe.
//
// rs_heal_kernel follows rs_locate_verdict_kernel on the stream and reads its verdicts.  A tile of
// a block whose verdict names no shard (clean, or unknown) costs its wave one scalar load; a tile
// of a block with a culprit x runs Verify's pipeline once more (heal_tiles, rs_verify_tile.hpp:
// the same ring, loads, masks and lane chunks) and stores row x's chunk XOR the delta its
// syndromes give, from the same load the syndromes were formed from.  Only row x is written, only
// bytes [0, S).  rs_heal_rows_kernel is the byte-granular form for the shapes rs_heal_kernel is
// not built for, over the rows the fallback encodes into scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"
#include "rs_verify_tile.hpp"

namespace rsmi {

// rs_locate_kernel's parameter list (launch_stripe_tiles serves both): rplan, the ratio plan with
// inv(M[0][c]) in output slot 0; verdict, the launch's first block's verdict.  bad and m are not
// used.
template <int K, int MT, bool UA>
__global__ __launch_bounds__(kFastWG, kMinWavesPerSimd) void rs_heal_kernel(
    const RsPlanDev* __restrict__ plan, uint8_t* in, uint8_t* par, uint64_t in_bs, uint64_t in_rs, uint64_t par_bs,
    uint64_t par_rs, uint32_t S, uint32_t cpb, uint32_t tpb, uint32_t ntiles, uint32_t* __restrict__ bad, uint32_t m,
    const RsPlanDev* __restrict__ rplan, const int32_t* __restrict__ verdict) {
    __shared__ u32x4 s_tbl[2 * K * kColDwords / 4];
    (void)bad;
    (void)m;
    heal_tiles<K, MT, UA>(s_tbl, plan, rplan, in, par, in_bs, in_rs, par_bs, par_rs, S, cpb, tpb, ntiles, verdict);
}

// Byte-granular heal of the blocks whose verdict names a shard, any shape and alignment.  enc: the
// encode of the data rows as they are stored (context scratch, m rows per block); par: the stored
// parity rows; data: the stored data rows.  tbl: GF(2^8) log[256] | exp[512] | R[m][k] |
// inv(M[0][c])[k] (rsmi_locate.cpp).
//   parity culprit j  par_j[x] = enc_j[x]
//   data culprit c    data_c[x] ^= inv(M[0][c]) * (enc_0[x] ^ par_0[x])
// over x in [0, S); a byte that is right already is not written.
__global__ __launch_bounds__(kWG) void rs_heal_rows_kernel(const uint8_t* __restrict__ enc, uint64_t enc_rs,
                                                           uint64_t enc_bs, uint8_t* data, uint64_t data_rs,
                                                           uint64_t data_bs, uint8_t* par, uint64_t par_rs,
                                                           uint64_t par_bs, uint64_t S, uint32_t k, uint32_t m,
                                                           uint64_t nblocks, const int32_t* __restrict__ verdict,
                                                           const uint8_t* __restrict__ tbl) {
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_exp[512];
    for (uint32_t i = threadIdx.x; i < 256u; i += kWG) s_log[i] = tbl[i];
    for (uint32_t i = threadIdx.x; i < 512u; i += kWG) s_exp[i] = tbl[256u + i];
    __syncthreads();
    for (uint64_t blk = blockIdx.y; blk < nblocks; blk += gridDim.y) {
        const int32_t vd = verdict[blk];  // uniform over the workgroup, as blk is
        if (vd < 0 || uint32_t(vd) >= k + m) continue;
        const uint32_t xr = uint32_t(vd);
        const uint8_t* pe = enc + blk * enc_bs;
        if (xr >= k) {
            const uint8_t* src = pe + uint64_t(xr - k) * enc_rs;
            uint8_t* dst = par + blk * par_bs + uint64_t(xr - k) * par_rs;
            for (uint64_t x = uint64_t(blockIdx.x) * kWG + threadIdx.x; x < S; x += uint64_t(gridDim.x) * kWG)
                if (dst[x] != src[x]) dst[x] = src[x];
        } else {
            const uint8_t* p0 = par + blk * par_bs;
            uint8_t* dst = data + blk * data_bs + uint64_t(xr) * data_rs;
            const uint32_t li = s_log[tbl[768u + m * k + xr]];
            for (uint64_t x = uint64_t(blockIdx.x) * kWG + threadIdx.x; x < S; x += uint64_t(gridDim.x) * kWG) {
                const uint32_t s0 = uint32_t(pe[x] ^ p0[x]);
                if (s0) dst[x] ^= s_exp[li + uint32_t(s_log[s0])];
            }
        }
    }
}

void* heal_rows_kernel() { return reinterpret_cast<void*>(&rs_heal_rows_kernel); }

template <int K, int MT>
static void fill_heal_km(HealKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_heal_kernel<K, MT, false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_heal_kernel<K, MT, true>);
}

template <int K>
static void fill_heal_k(HealKernelTable& t) {
    fill_heal_km<K, 2>(t);
    fill_heal_km<K, 3>(t);
    fill_heal_km<K, 4>(t);
}

// the K and m of the locate kernels: every verdict they can give has a kernel to act on it
const HealKernelTable& heal_kernels() {
    static const HealKernelTable t = [] {
        HealKernelTable x{};
        fill_heal_k<1>(x);
        fill_heal_k<2>(x);
        fill_heal_k<3>(x);
        fill_heal_k<4>(x);
        fill_heal_k<5>(x);
        fill_heal_k<6>(x);
        fill_heal_k<8>(x);
        fill_heal_k<10>(x);
        fill_heal_k<12>(x);
        fill_heal_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
