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

namespace rsmi {

// K data rows in, MT (<= 4) stored parity rows compared, one 16-byte chunk per lane per row.
// plan: a tile of the encode plan (in_row = 0..K-1, out_row = the tile's parity rows relative to
// the parity base).  bad: the launch's first block's flags, m words per block.
// UA: rows at any byte alignment and pitch (S >= 16), a lane's window at min(16 ch, S - 16).
// The stored parity chunks are members of the row ring: parity row j takes the slot that input
// row K - P + j leaves (its load is issued P columns before the GF work ends), and with fewer
// slots than parity rows (K < MT) the rest are loaded ahead of the column loop, so no load waits
// behind the GF work.  Every load is nontemporal: nothing is read twice.
// Launch geometry: one tile per wave; the loop strides over further tiles only when the caller
// caps the grid (option waves_per_cu).
template <int K, int MT, bool UA>
__global__ __launch_bounds__(kFastWG, kMinWavesPerSimd) void rs_verify_kernel(
    const RsPlanDev* __restrict__ plan, const uint8_t* __restrict__ in, const uint8_t* __restrict__ par,
    uint64_t in_bs, uint64_t in_rs, uint64_t par_bs, uint64_t par_rs, uint32_t S, uint32_t cpb, uint32_t tpb,
    uint32_t ntiles, uint32_t* __restrict__ bad, uint32_t m) {
    __shared__ u32x4 s_tbl[K * kColDwords / 4];
    {
        const uint32_t* src = plan->tbl;
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_tbl);
        for (int i = threadIdx.x; i < K * kColDwords; i += kFastWG) dst[i] = src[i];
    }
    __syncthreads();

    constexpr uint32_t kWavesPerWG = kFastWG / kWave;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t nw = gridDim.x * kWavesPerWG;
    // UA: each XCD takes one contiguous eighth of the tiles, as in rs_fast_kernel (a tile at an
    // odd address shares its first and last lines with its neighbours)
    const uint32_t wg =
        UA ? tile_group(blockIdx.x, gridDim.x, (gridDim.x & 7u) ? 0u : gridDim.x) : uint32_t(blockIdx.x);
    uint32_t t = wg * kWavesPerWG + wid;
    if (t >= ntiles) return;

    constexpr int P = rows_in_flight<K, MT>();
    constexpr int PR = MT < P ? MT : P;  // parity rows that go through the ring
    uint64_t in_off[K], par_off[MT];
    uint32_t flag[MT];
#pragma unroll
    for (int c = 0; c < K; c++) in_off[c] = uint64_t(plan->in_row[c]) * in_rs;
#pragma unroll
    for (int j = 0; j < MT; j++) {
        flag[j] = plan->out_row[j];
        par_off[j] = uint64_t(flag[j]) * par_rs;
    }

    for (TileWalk tw(t, nw, tpb); t < ntiles; t += nw, tw.next(tpb)) {
        const uint32_t blk = tw.blk;
        const uint8_t* ib = in + uint64_t(blk) * in_bs;
        const uint8_t* pb = par + uint64_t(blk) * par_bs;
        const LaneChunk lc = lane_chunk<UA>(tw.tib, lane, cpb, S);
        const uint32_t ch = lc.ch, chl = lc.chl, win = lc.win;
        // the bytes of the lane's chunk that count: none for a lane past the row's last chunk; UA:
        // every byte of a window (it lies in [0, S)); aligned: the bytes before S
        uint32_t mk[4];
        {
            const int valid = ch < cpb ? (UA ? 16 : int(S) - int(ch * 16u)) : 0;
#pragma unroll
            for (int w = 0; w < 4; w++) mk[w] = bytes_mask(valid - 4 * w);
        }
        auto load_col = [&](int c) {
            if constexpr (UA)
                return ld16u<true>(ib + in_off[c] + win);
            else
                return ld16<true>(reinterpret_cast<const u32x4*>(ib + in_off[c]) + chl);
        };
        auto load_par = [&](int j) {
            if constexpr (UA)
                return ld16u<true>(pb + par_off[j] + win);
            else
                return ld16<true>(reinterpret_cast<const u32x4*>(pb + par_off[j]) + chl);
        };

        u32x4 v[P];
        u32x4 xs[MT > PR ? MT - PR : 1];  // K < MT: the parity rows the ring has no slot for
#pragma unroll
        for (int c = 0; c < P; c++) v[c] = load_col(c);
#pragma unroll
        for (int j = PR; j < MT; j++) xs[j - PR] = load_par(j);

        uint32_t acc[MT][4];
        // the freed slot takes the next input row, or, once those are all issued, a stored
        // parity row: parity row j rides in slot (K - P + j) % P
        gf_tile_columns<K, MT, P>(s_tbl, v, acc, GfNone{}, GfNone{}, GfNone{}, [&](int c, u32x4& x) {
            if (c + P < K)
                x = load_col(c + P);
            else if (c + P - K < PR)
                x = load_par(c + P - K);
        });

#pragma unroll
        for (int j = 0; j < MT; j++) {
            const u32x4 sp = j < PR ? v[(K - P + j) % P] : xs[j < PR ? 0 : j - PR];
            uint32_t d = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) d |= (acc[j][w] ^ u4get(sp, w)) & mk[w];
            // one relaxed agent-scope OR from one lane, and only when some lane of the wave saw a
            // difference: a vector atomic (no return value), never issued on a clean tile
            if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull && lane == 0u)
                __hip_atomic_fetch_or(bad + uint64_t(blk) * m + flag[j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
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
