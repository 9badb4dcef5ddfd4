// rs_scrub_kernels.hip -- the first pass of a scrub over stored stripes: Encoder.Verify's flags and
// R(shard) of the datanode entry checksum for every one of the k + m rows, from one read of them.
//
// rs_scrub_mfma_kernel is rs_verify_kernel's tile (stripe_tile, rs_verify_tile.hpp: v_perm tables in
// LDS, the ring of rows in flight with the stored parity rows riding in the slots the input rows
// free, every load nontemporal, nothing stored) in rs_fused_mfma_kernel's geometry and with its fold
// (rs_coding_kernels.hpp): a workgroup takes a unit of kFusedUnitTiles = 4 consecutive tiles of one
// block, wave w tile w, and every data chunk and every stored parity chunk, as loaded, goes through
// four fp4 MFMAs with the weights of the tile's position in its unit (crc16.hpp FW), two shards to
// an f32 accumulator.  Where the fused encode folds the parity chunk it computed, the scrub folds the
// one it loaded: R(shard) is the checksum of the bytes as stored, damaged or not.  The four waves'
// counts meet in LDS and the unit's record goes out in the layout rs_crc16_combine_mfma_kernel
// (rs_crc16_kernels.hip) turns into R(row); the launcher runs that kernel behind this one.
//
// The two consumers mask differently on unaligned-window layouts (UA).  The syndrome counts all 16
// bytes of every window (the row's last window overlaps the one before it and is compared twice,
// as in rs_verify_kernel).  The fold needs every lane's bytes at their chunk position, so the lane
// that holds the row's last window folds the window's bytes before S at the chunk position, and
// the row's last tile then adds (window XOR shifted window) for that lane alone: the parity rows
// from registers, the data rows from a reload of that lane's 16 bytes.  On aligned layouts both
// take the bytes before S.  Lanes past the row's last chunk count nothing, and padding never
// reaches a flag or a checksum.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc16.hpp"
#include "rs_crc_rows.hpp"
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
    // UA: each XCD takes one contiguous eighth of the units (their rows share boundary lines)
    const uint32_t u =
        UA ? tile_group(blockIdx.x, gridDim.x, (gridDim.x & 7u) ? 0u : gridDim.x) : uint32_t(blockIdx.x);
    if (u >= nunits) return;
    const uint32_t blk = u / upb;
    const uint32_t t0 = (u - blk * upb) * kFusedUnitTiles;
    const uint32_t nt = tpb - t0 < uint32_t(kFusedUnitTiles) ? tpb - t0 : uint32_t(kFusedUnitTiles);
    const uint8_t* ib = in + uint64_t(blk) * in_bs;
    const uint8_t* pb = par + uint64_t(blk) * par_bs;

    mfma_v4f cacc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; a++) cacc[a] = mfma_v4f{0.f, 0.f, 0.f, 0.f};

    // wave w takes tile w; a block's last unit may leave waves idle
    if (wid < nt) {
        uint64_t in_off[K], par_off[MT];
        row_offsets<K, MT>(plan, in_rs, par_rs, in_off, par_off);
        uint32_t flag[MT];  // the flag index is the parity row
#pragma unroll
        for (int j = 0; j < MT; j++) flag[j] = plan->out_row[j];

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
        // one MFMA: bit form q of shard r's chunk x into the shard's accumulator (the odd shard of
        // a pair at B scale 2^12)
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

        u32x4 sps[MT];  // the stored parity chunks as loaded
        stripe_tile<K, MT, UA>(
            s_tbl, ib, pb, in_off, par_off, lc, cpb, S, GfNone{},
            // form w's MFMA between the GF work of dword w and w + 1, under the wave's own VALU stream
            [&](int c, int w, const u32x4& x) {
                crc_mfma(x, c, w);
                __builtin_amdgcn_sched_barrier(0);
            },
            [&](int c, const u32x4&) { anchor(c); },
            [&](int j, const uint32_t(&s)[4], const u32x4& sp) {
                // one relaxed agent-scope OR from one lane, and only when some lane of the wave saw
                // a difference: never issued on a clean tile
                const uint32_t d = s[0] | s[1] | s[2] | s[3];
                if (__builtin_amdgcn_ballot_w64(d != 0u) != 0ull && lane == 0u)
                    __hip_atomic_fetch_or(bad + uint64_t(blk) * m + flag[j], 1u, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
                sps[j] = sp;
            });
        // the stored parity rows: bit form by bit form, even rows before odd ones, so consecutive
        // MFMAs go to different accumulators wherever two parity rows do not share one
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int j = h; j < MT; j += 2) crc_mfma(sps[j], K + j, q);
#pragma unroll
        for (int j = 0; j < MT; j++) anchor(K + j);
        // UA: every row's last window went in unshifted; the parity rows' counts are corrected
        // from registers, the data rows' from a reload (a copy of every row would not fit)
        if (UA && fix) {
#pragma unroll
            for (int j = 0; j < MT; j++) {
                const u32x4 d = correction(sps[j]);
#pragma unroll
                for (int q = 0; q < 4; q++) crc_mfma(d, K + j, q);
                anchor(K + j);
            }
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
    // parity of shard 2 a / 2 a + 1 (bits 0 and 12 of the exact count)
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
