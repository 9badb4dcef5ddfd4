// rs_pair_kernels.hip -- rsmi_locate_pair on the GPU: which two shards break a stripe?
//
// rs_locate_pair_kernel follows rs_locate_verdict_kernel on the stream and reads its verdicts, as
// rs_heal_kernel does.  A tile of a block that is clean or has a single culprit costs its wave one
// scalar load; a tile of an UNKNOWN block runs Verify's pipeline once more (pair_tiles,
// rs_pair_tile.hpp) and ANDs the pairs that explain it into the block's pair words.
// rs_locate_pair_verdict_kernel then widens rsmi_locate's verdicts to two words and decodes the
// pair words of the UNKNOWN blocks.  rs_locate_pair_rows_kernel is the byte-granular form for the
// shapes rs_locate_pair_kernel is not built for, over the rows the fallback encodes into scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rsmi.h"
#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_pair_tile.hpp"
#include "rs_plan.hpp"
#include "rs_verify_tile.hpp"

namespace rsmi {

// rs_locate_kernel's parameter list (launch_stripe_tiles serves it): pairw in the flags' place, the
// launch's first block's pair words; pplan, plan "P"; verdict, the launch's first block's verdict
// from rsmi_locate.  m is not used.
template <int K, int MT, bool UA>
__global__ __launch_bounds__(kFastWG, kMinWavesPerSimd) void rs_locate_pair_kernel(
    const RsPlanDev* __restrict__ plan, const uint8_t* __restrict__ in, const uint8_t* __restrict__ par,
    uint64_t in_bs, uint64_t in_rs, uint64_t par_bs, uint64_t par_rs, uint32_t S, uint32_t cpb, uint32_t tpb,
    uint32_t ntiles, uint32_t* __restrict__ pairw, uint32_t m, const RsPlanDev* __restrict__ pplan,
    const int32_t* __restrict__ verdict) {
    __shared__ u32x4 s_tbl[(2 * K + pair_blocks(K, MT)) * kColDwords / 4];
    (void)m;
    pair_tiles<K, MT, UA>(s_tbl, plan, pplan, in, par, in_bs, in_rs, par_bs, par_rs, S, cpb, tpb, ntiles, verdict,
                          pairw);
}

// One thread per block: out[2b], out[2b+1] from rsmi_locate's verdict and the block's pair words
// (words per block, bit pair_bit(n, x, y); null: none were formed).
//   verdict >= -1 (clean, or a single shard)    (verdict, -1)
//   UNKNOWN, exactly one pair among the C(n,2)  (x, y)
//   UNKNOWN otherwise                           (-2, -2)
__global__ __launch_bounds__(kWG) void rs_locate_pair_verdict_kernel(const int32_t* __restrict__ culprit,
                                                                     const uint32_t* __restrict__ pairw, uint32_t n,
                                                                     uint32_t words, uint64_t nblocks,
                                                                     int32_t* __restrict__ out) {
    const uint64_t b = uint64_t(blockIdx.x) * kWG + threadIdx.x;
    if (b >= nblocks) return;
    const int32_t v = culprit[b];
    int32_t x = v, y = RSMI_LOCATE_CLEAN;
    if (v < RSMI_LOCATE_CLEAN) {
        x = y = RSMI_LOCATE_UNKNOWN;
        const uint32_t pairs = n * (n - 1u) / 2u;
        uint32_t found = 0, p = 0;
        for (uint32_t w = 0; pairw && w < words; w++) {
            const uint32_t left = pairs - 32u * w;
            const uint32_t bits = pairw[b * words + w] & (left >= 32u ? ~0u : (1u << left) - 1u);
            if (bits) {
                found += uint32_t(__popc(bits));
                p = 32u * w + uint32_t(__ffs(bits) - 1);
            }
        }
        if (found == 1u) {
            uint32_t r = 0;  // rows of the lexicographic order: row r holds n - 1 - r pairs
            while (p >= n - 1u - r) {
                p -= n - 1u - r;
                r++;
            }
            x = int32_t(r);
            y = int32_t(r + 1u + p);
        }
    }
    out[2 * b] = x;
    out[2 * b + 1] = y;
}

// Byte-granular pair test of the UNKNOWN blocks, any shape with m >= 3 and any alignment, n up to
// 256.  a: the encode of the data rows (context scratch); b: the stored parity rows (m rows per
// block each), so syn_l = a_l ^ b_l.  tbl: GF(2^8) log[256] | exp[512] | R[m][k] (rsmi_locate_matrix;
// R in the launch's dynamic LDS).  Column z of the check matrix is, up to a factor that does not
// change a span, R[.][z] for a data shard and the unit vector of row z - k for a parity shard.
// One workgroup per block, its threads striding over the pairs: per pair two pivot rows are
// chosen once (a non-singular 2 x 2 minor of the two columns), the byte columns are solved on
// them and checked on the other rows, and the scan stops at the first column the pair fails.  The
// workgroup counts the pairs that explain every column and, when there is exactly one, writes it
// over the block's (-2, -2) in out (two words per block, widened before the launch).
__global__ __launch_bounds__(kWG) void rs_locate_pair_rows_kernel(const uint8_t* __restrict__ a, uint64_t a_rs,
                                                                  uint64_t a_bs, const uint8_t* __restrict__ b,
                                                                  uint64_t b_rs, uint64_t b_bs, uint64_t S, uint32_t k,
                                                                  uint32_t m, uint64_t nblocks,
                                                                  const int32_t* __restrict__ culprit,
                                                                  const uint8_t* __restrict__ tbl,
                                                                  int32_t* __restrict__ out) {
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_exp[512];
    __shared__ uint32_t s_count, s_found;
    extern __shared__ uint8_t s_R[];
    for (uint32_t i = threadIdx.x; i < 256u; i += kWG) s_log[i] = tbl[i];
    for (uint32_t i = threadIdx.x; i < 512u; i += kWG) s_exp[i] = tbl[256u + i];
    for (uint32_t i = threadIdx.x; i < m * k; i += kWG) s_R[i] = tbl[768u + i];
    const uint32_t n = k + m, pairs = n * (n - 1u) / 2u;
    auto mul = [&](uint32_t x, uint32_t y) -> uint32_t {
        return x && y ? uint32_t(s_exp[uint32_t(s_log[x]) + uint32_t(s_log[y])]) : 0u;
    };
    // entry l of check column z
    auto col = [&](uint32_t z, uint32_t l) -> uint32_t { return z < k ? uint32_t(s_R[l * k + z]) : uint32_t(l == z - k); };

    for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        if (culprit[blk] != RSMI_LOCATE_UNKNOWN) continue;  // uniform over the workgroup, as blk is
        __syncthreads();  // the tables are staged; the last block's result is read
        if (threadIdx.x == 0) s_count = s_found = 0u;
        __syncthreads();
        const uint8_t* pa = a + blk * a_bs;
        const uint8_t* pb = b + blk * b_bs;
        auto syn = [&](uint32_t l, uint64_t x) -> uint32_t {
            return uint32_t(pa[uint64_t(l) * a_rs + x] ^ pb[uint64_t(l) * b_rs + x]);
        };
        for (uint32_t p = threadIdx.x; p < pairs; p += kWG) {
            uint32_t x = 0, q = p;
            while (q >= n - 1u - x) {
                q -= n - 1u - x;
                x++;
            }
            const uint32_t y = x + 1u + q;
            // the pivot rows: two data shards differ in their ratios of rows 0 and 1; a parity
            // shard's own row and any other row; two parity shards' own rows
            uint32_t ra, rb;
            if (y < k) {
                ra = 0u;
                rb = 1u;
            } else if (x < k) {
                ra = y - k;
                rb = ra == 0u ? 1u : 0u;
            } else {
                ra = x - k;
                rb = y - k;
            }
            const uint32_t ua = col(x, ra), va = col(y, ra), ub = col(x, rb), vb = col(y, rb);
            const uint32_t det = mul(ua, vb) ^ mul(ub, va);
            if (!det) continue;  // no MDS matrix has a singular minor here
            const uint32_t idet = uint32_t(s_exp[255u - uint32_t(s_log[det])]);
            const uint32_t ia = mul(vb, idet), ib = mul(va, idet), ic = mul(ub, idet), id = mul(ua, idet);
            bool ok = true;
            for (uint64_t i = 0; ok && i < S; i++) {
                const uint32_t sa = syn(ra, i), sb = syn(rb, i);
                const uint32_t al = mul(ia, sa) ^ mul(ib, sb), be = mul(ic, sa) ^ mul(id, sb);
                for (uint32_t l = 0; ok && l < m; l++)
                    if (l != ra && l != rb) ok = syn(l, i) == (mul(al, col(x, l)) ^ mul(be, col(y, l)));
            }
            if (ok) {
                atomicAdd(&s_count, 1u);
                atomicExch(&s_found, (x << 16) | y);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_count == 1u) {
            out[2 * blk] = int32_t(s_found >> 16);
            out[2 * blk + 1] = int32_t(s_found & 0xFFFFu);
        }
    }
}

void* pair_verdict_kernel() { return reinterpret_cast<void*>(&rs_locate_pair_verdict_kernel); }
void* pair_rows_kernel() { return reinterpret_cast<void*>(&rs_locate_pair_rows_kernel); }

template <int K, int MT>
static void fill_pair_km(PairKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_locate_pair_kernel<K, MT, false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_locate_pair_kernel<K, MT, true>);
}

template <int K>
static void fill_pair_k(PairKernelTable& t) {
    fill_pair_km<K, 3>(t);
    fill_pair_km<K, 4>(t);
}

// the K of the locate kernels, m = 3..4 (m <= 2: every pair explains everything, none is named)
const PairKernelTable& pair_kernels() {
    static const PairKernelTable t = [] {
        PairKernelTable x{};
        fill_pair_k<1>(x);
        fill_pair_k<2>(x);
        fill_pair_k<3>(x);
        fill_pair_k<4>(x);
        fill_pair_k<5>(x);
        fill_pair_k<6>(x);
        fill_pair_k<8>(x);
        fill_pair_k<10>(x);
        fill_pair_k<12>(x);
        fill_pair_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
