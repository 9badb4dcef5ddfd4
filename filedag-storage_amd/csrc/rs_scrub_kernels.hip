// rs_scrub_kernels.hip -- the first pass of a scrub over stored stripes: Encoder.Verify's flags and
// R(shard) of the datanode entry checksum for every one of the k + m rows, from one read of them.
//
// rs_scrub_mfma_kernel is rs_verify_kernel's tile (stripe_tile, rs_verify_tile.hpp: v_perm tables in
// LDS, the ring of rows in flight with the stored parity rows riding in the slots the input rows
// free, every load nontemporal, nothing stored) in rs_fused_mfma_kernel's geometry and with the fold
// of rs_crc_fold.hpp: a workgroup takes a unit of kFusedUnitTiles = 4 consecutive tiles of one
// block, wave w tile w, and every data chunk and every stored parity chunk, as loaded, goes into the
// fold.  Where the fused encode folds the parity chunk it computed, the scrub folds the one it
// loaded: R(shard) is the checksum of the bytes as stored, damaged or not.  The unit's record goes
// out in the layout rs_crc16_combine_mfma_kernel (rs_crc16_kernels.hip) turns into R(row); the
// launcher runs that kernel behind this one.
//
// The two consumers mask differently on unaligned-window layouts (UA).  The syndrome counts all 16
// bytes of every window (the row's last window overlaps the one before it and is compared twice,
// as in rs_verify_kernel); the fold counts every byte before S once, at its chunk position (the
// parity rows' last window corrected from registers, the data rows' from a reload).  On aligned
// layouts both take the bytes before S.  Lanes past the row's last chunk count nothing, and padding
// never reaches a flag or a checksum.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc16.hpp"
#include "rs_crc_fold.hpp"
#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"
#include "rs_verify_tile.hpp"

namespace rsmi {

// plan: the encode plan's one tile (in_row = 0..K-1; out_row: the parity rows relative to the parity
// base, which are also the flag indices).  bad: the launch's first block's flags, m words per block,
// zeroed by the launcher.  crc_rec: the launch's first unit's record, NACC * 64 bytes per unit.
template <int K, int MT, int WPS, bool UA>
__global__ __launch_bounds__(kWG, WPS) void rs_scrub_mfma_kernel(
    const RsPlanDev* __restrict__ plan, const uint8_t* __restrict__ in, const uint8_t* __restrict__ par,
    uint64_t in_bs, uint64_t in_rs, uint64_t par_bs, uint64_t par_rs, uint32_t S, uint32_t cpb, uint32_t tpb,
    uint32_t upb, uint32_t nunits, uint32_t* __restrict__ bad, uint32_t m, const uint32_t* __restrict__ crc_tbl,
    uint8_t* __restrict__ crc_rec) {
    static_assert(kFusedUnitTiles == kWG / kWave && kFastWG == kWG, "one tile per wave of the unit's workgroup");
    constexpr int NSH = K + MT;
    constexpr int NACC = (NSH + 1) / 2;  // two shards per accumulator
    __shared__ u32x4 s_tbl[K * kColDwords / 4];
    stage_tables<K>(s_tbl, plan, nullptr);

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t u = fold_unit<UA>();
    if (u >= nunits) return;
    const FoldUnit un = fold_unit_tiles(u, upb, tpb);
    const uint32_t blk = un.blk, t0 = un.t0, nt = un.nt;
    const uint8_t* ib = in + uint64_t(blk) * in_bs;
    const uint8_t* pb = par + uint64_t(blk) * par_bs;

    CrcFold<NACC> fold;
    fold.clear();

    // wave w takes tile w; a block's last unit may leave waves idle
    if (wid < nt) {
        uint64_t in_off[K], par_off[MT];
        row_offsets<K, MT>(plan, in_rs, par_rs, in_off, par_off);
        uint32_t flag[MT];  // the flag index is the parity row
#pragma unroll
        for (int j = 0; j < MT; j++) flag[j] = plan->out_row[j];

        const LaneChunk lc = lane_chunk<UA>(t0 + wid, lane, cpb, S);
        fold.template tile_setup<UA>(t0 + wid, wid, lane, cpb, S, crc_tbl);

        u32x4 sps[MT];  // the stored parity chunks as loaded
        stripe_tile<K, MT, UA>(
            s_tbl, ib, pb, in_off, par_off, lc, cpb, S, GfNone{},
            // form w's MFMA between the GF work of dword w and w + 1, under the wave's own VALU stream
            [&](int c, int w, const u32x4& x) {
                fold.mfma(x, c, w);
                __builtin_amdgcn_sched_barrier(0);
            },
            [&](int c, const u32x4&) { fold.anchor(c); },
            [&](int j, const uint32_t(&s)[4], const u32x4& sp) {
                // one relaxed agent-scope OR from one lane, and only when some lane of the wave saw
                // a difference: never issued on a clean tile
                const uint32_t d = s[0] | s[1] | s[2] | s[3];
                if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull && lane == 0u)
                    __hip_atomic_fetch_or(bad + uint64_t(blk) * m + flag[j], 1u, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
                sps[j] = sp;
            });
        // the stored parity rows; UA: every row's last window went in unshifted
        fold.template rows<K, MT>(sps);
        if (UA && fold.fix) {
            fold.template fix_rows<K, MT>(sps);
            fold.template fix_reload<K, true>(ib, in_off, lc.win);
        }
    }

    fold.finish(u, wid, lane, crc_rec);
}

// Waves per SIMD the register allocation must allow, per shape, so that no kernel uses scratch
// memory: the ring of rows in flight, the GF accumulators and (K + MT + 1) / 2 f32 quads of counts
// are live together (profiles/scrub/isa.txt).
constexpr int scrub_wps(int K, int MT) { return kFusedWavesPerSimd; }

template <int K, int MT>
static void fill_scrub_km(ScrubKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_scrub_mfma_kernel<K, MT, scrub_wps(K, MT), false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_scrub_mfma_kernel<K, MT, scrub_wps(K, MT), true>);
}

template <int K>
static void fill_scrub_k(ScrubKernelTable& t) {
    fill_scrub_km<K, 1>(t);
    fill_scrub_km<K, 2>(t);
    fill_scrub_km<K, 3>(t);
    fill_scrub_km<K, 4>(t);
}

// the shapes of rs_verify_kernel (rs_verify_kernels.hip), both layouts
const ScrubKernelTable& scrub_kernels() {
    static const ScrubKernelTable t = [] {
        ScrubKernelTable x{};
        fill_scrub_k<1>(x);
        fill_scrub_k<2>(x);
        fill_scrub_k<3>(x);
        fill_scrub_k<4>(x);
        fill_scrub_k<5>(x);
        fill_scrub_k<6>(x);
        fill_scrub_k<8>(x);
        fill_scrub_k<10>(x);
        fill_scrub_k<12>(x);
        fill_scrub_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
