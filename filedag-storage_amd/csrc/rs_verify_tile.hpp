// rs_verify_tile.hpp -- the stripe checks' tile pipeline: one step, stripe_tile, and its two
// consumers here (a third, rs_scrub_mfma_kernel, rs_scrub_kernels.hip, also folds every chunk the
// step loads into CRC-16 counts through the step's per-dword and per-column hooks).  stripe_tile
// runs the coding kernels' GF(2^8) pipeline over one tile of the encode plan, loads the stored
// parity chunks where the encode would store, and hands its caller, per parity row j, the lane's
// masked syndrome
//   syn_j = encode(data)_j ^ stored parity_j
// and the stored chunk as loaded.  verify_tiles (rs_verify_kernel, rs_verify_kernels.hip;
// rs_locate_kernel, rs_locate_kernels.hip) raises bad[block * m + parity row] where a syndrome is
// non-zero and, LOC, goes on to name the shards that explain a dirty tile (locate_tile).
// heal_tiles (rs_heal_kernel, rs_heal_kernels.hip) forms the syndromes of the blocks a verdict
// names a shard in and rewrites that shard's row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"

namespace rsmi {

// The selector words of a dword's bytes (bits 0-2, 3-5, 6-7: rs_gf_tile.hpp), and the dword times
// the coefficient in output slot j of a column's tables T.
struct GfSel {
    uint32_t s1, s2, s3;
};
__device__ __forceinline__ GfSel gf_selectors(uint32_t x) {
    return GfSel{x & 0x07070707u, (x >> 3) & 0x07070707u, (x >> 6) & 0x03030303u};
}
__device__ __forceinline__ uint32_t gf_mul_dword(const u32x4 (&T)[5], int j, const GfSel& s) {
    const uint32_t p1 = __builtin_amdgcn_perm(u4get(T[1], j), u4get(T[0], j), s.s1);
    const uint32_t p2 = __builtin_amdgcn_perm(u4get(T[3], j), u4get(T[2], j), s.s2);
    const uint32_t p3 = __builtin_amdgcn_perm(u4get(T[4], j), u4get(T[4], j), s.s3);
    return xor3(p1, p2, p3);
}

// A wave's lane index, the launch's wave count and the wave's first tile: one tile per wave, further
// tiles (t += nw) only when the caller caps the grid (option waves_per_cu).  UA: each XCD takes
// one contiguous eighth of the tiles, as in rs_fast_kernel (a tile at an odd address shares its
// first and last lines with its neighbours).
struct WaveTiles {
    uint32_t lane, nw, t;
};
template <bool UA>
__device__ __forceinline__ WaveTiles wave_tiles() {
    constexpr uint32_t kWavesPerWG = kFastWG / kWave;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t wg =
        UA ? tile_group(blockIdx.x, gridDim.x, (gridDim.x & 7u) ? 0u : gridDim.x) : uint32_t(blockIdx.x);
    return WaveTiles{threadIdx.x & (kWave - 1), gridDim.x * kWavesPerWG, wg * kWavesPerWG + wid};
}

// the byte offsets of the plan's K input rows and MT stored parity rows within a block
template <int K, int MT>
__device__ __forceinline__ void row_offsets(const RsPlanDev* plan, uint64_t in_rs, uint64_t par_rs,
                                            uint64_t (&in_off)[K], uint64_t (&par_off)[MT]) {
#pragma unroll
    for (int c = 0; c < K; c++) in_off[c] = uint64_t(plan->in_row[c]) * in_rs;
#pragma unroll
    for (int j = 0; j < MT; j++) par_off[j] = uint64_t(plan->out_row[j]) * par_rs;
}

// One tile of a stripe check: K data rows in, MT (<= 4) stored parity rows against them, one
// 16-byte chunk per lane per row.  ib, pb: the block's data and parity rows; lc: the lane's chunk
// (UA: rows at any byte alignment and pitch, S >= 16, the window at min(16 ch, S - 16)).  s_tbl:
// the plan's tables in LDS, staged and the barrier passed by the caller.
// The stored parity chunks are members of the row ring: parity row j takes the slot that input
// row K - P + j leaves (its load is issued P columns before the GF work ends), and with fewer
// slots than parity rows (K < MT) the rest are loaded ahead of the column loop, so no load waits
// behind the GF work.  Every load is nontemporal: nothing is read twice.
//   before_col(c, x)       gf_tile_columns': data row c's chunk x as loaded, before its GF work
//   after_dword(c, w, x)   gf_tile_columns': after the GF work of x's dword w
//   after_col(c, x)        gf_tile_columns': after column c's GF work, before its slot is refilled
//   on_row(j, syn, sp)     parity row j (a constant once unrolled): the syndrome's four dwords,
//                          masked to the bytes of the lane's chunk that count, and the stored chunk
template <int K, int MT, bool UA, class BeforeCol, class AfterDword, class AfterCol, class OnRow>
__device__ __forceinline__ void stripe_tile(const u32x4* s_tbl, const uint8_t* ib, const uint8_t* pb,
                                            const uint64_t (&in_off)[K], const uint64_t (&par_off)[MT],
                                            const LaneChunk& lc, uint32_t cpb, uint32_t S, BeforeCol&& before_col,
                                            AfterDword&& after_dword, AfterCol&& after_col, OnRow&& on_row) {
    constexpr int P = rows_in_flight<K, MT>();
    constexpr int PR = MT < P ? MT : P;  // parity rows that go through the ring
    // the bytes of the lane's chunk that count: none for a lane past the row's last chunk; UA:
    // every byte of a window (it lies in [0, S)); aligned: the bytes before S
    uint32_t mk[4];
    {
        const int valid = lc.ch < cpb ? (UA ? 16 : int(S) - int(lc.ch * 16u)) : 0;
#pragma unroll
        for (int w = 0; w < 4; w++) mk[w] = bytes_mask(valid - 4 * w);
    }
    auto load_row = [&](const uint8_t* row) {
        if constexpr (UA)
            return ld16u<true>(row + lc.win);
        else
            return ld16<true>(reinterpret_cast<const u32x4*>(row) + lc.chl);
    };
    auto load_col = [&](int c) { return load_row(ib + in_off[c]); };
    auto load_par = [&](int j) { return load_row(pb + par_off[j]); };

    u32x4 v[P];
    u32x4 xs[MT > PR ? MT - PR : 1];  // K < MT: the parity rows the ring has no slot for
#pragma unroll
    for (int c = 0; c < P; c++) v[c] = load_col(c);
#pragma unroll
    for (int j = PR; j < MT; j++) xs[j - PR] = load_par(j);

    uint32_t acc[MT][4];
    // the freed slot takes the next input row or, once those are issued, parity row c + P - K
    gf_tile_columns<K, MT, P>(s_tbl, v, acc, before_col, after_dword, after_col, [&](int c, u32x4& x) {
        if (c + P < K)
            x = load_col(c + P);
        else if (c + P - K < PR)
            x = load_par(c + P - K);
    });

#pragma unroll
    for (int j = 0; j < MT; j++) {
        const u32x4 sp = j < PR ? v[(K - P + j) % P] : xs[j < PR ? 0 : j - PR];
        uint32_t syn[4];
#pragma unroll
        for (int w = 0; w < 4; w++) syn[w] = (acc[j][w] ^ u4get(sp, w)) & mk[w];
        on_row(j, syn, sp);
    }
}

// The shards that explain a dirty tile, ANDed into the block's candidate word *cand (bit x: shard
// x; the caller set the word to all-ones before the launch).  syn: the lane's masked syndromes;
// rtbl: the v_perm tables of the ratio matrix R[j][c] = M[j][c] / M[0][c] (rsmi_locate_matrix)
// in LDS, laid out as a plan's tables.  Over the bytes where some syn_j != 0,
//   data shard c explains    iff  syn_j == R[j][c] * syn_0 for every j >= 1,
//   parity shard j explains  iff  syn_i == 0 for every i != j;
// a byte whose syndromes are all zero passes every test (R * 0 = 0), so the tests run over all 16
// bytes of every lane unconditionally and a clean lane (or one past the row's end) votes for every
// shard.  Each test is one ballot over the wave, so the wave's AND is built in scalar registers;
// one lane then issues one relaxed agent-scope atomic AND with no return value.  Rows that
// overlap (UA windows) are tested twice, which an AND does not see.
template <int K, int MT>
__device__ __forceinline__ void locate_tile(const u32x4* rtbl, const uint32_t (&syn)[MT][4], uint32_t lane,
                                            uint32_t* cand) {
    uint32_t wm = 0;
#pragma unroll
    for (int j = 0; j < MT; j++) {
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < MT; i++)
            if (i != j) o |= syn[i][0] | syn[i][1] | syn[i][2] | syn[i][3];
        if (__builtin_amdgcn_ballot_w64(o != 0u) == 0ull) wm |= 1u << (K + j);
    }
    // the selector words of syn_0, shared by every column
    GfSel s0[4];
#pragma unroll
    for (int w = 0; w < 4; w++) s0[w] = gf_selectors(syn[0][w]);
    // rolled: a dirty tile is the rare case, the code stays small
#pragma unroll 1
    for (int c = 0; c < K; c++) {
        u32x4 T[5];
#pragma unroll
        for (int f = 0; f < 5; f++) T[f] = rtbl[c * 5 + f];
        uint32_t diff = 0;
#pragma unroll
        for (int j = 1; j < MT; j++)
#pragma unroll
            for (int w = 0; w < 4; w++) diff |= gf_mul_dword(T, j, s0[w]) ^ syn[j][w];
        if (__builtin_amdgcn_ballot_w64(diff != 0u) == 0ull) wm |= 1u << c;
    }
    if (lane == 0u) (void)__hip_atomic_fetch_and(cand, wm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The tile loop of rs_verify_kernel and rs_locate_kernel.  plan: a tile of the encode plan
// (in_row = 0..K-1, out_row = the tile's parity rows relative to the parity base).  bad: the
// launch's first block's flags, m words per block.  s_tbl: the plan's tables in LDS (LOC: followed
// by the ratio tables).  LOC (the encode plan is this one tile, MT = m >= 2): cand, the launch's
// first block's candidate word, one per block.
template <int K, int MT, bool UA, bool LOC>
__device__ __forceinline__ void verify_tiles(const u32x4* s_tbl, const RsPlanDev* __restrict__ plan,
                                             const uint8_t* __restrict__ in, const uint8_t* __restrict__ par,
                                             uint64_t in_bs, uint64_t in_rs, uint64_t par_bs, uint64_t par_rs,
                                             uint32_t S, uint32_t cpb, uint32_t tpb, uint32_t ntiles,
                                             uint32_t* __restrict__ bad, uint32_t m, uint32_t* __restrict__ cand) {
    const WaveTiles wt = wave_tiles<UA>();
    const uint32_t lane = wt.lane, nw = wt.nw;
    uint32_t t = wt.t;
    if (t >= ntiles) return;

    uint64_t in_off[K], par_off[MT];
    row_offsets<K, MT>(plan, in_rs, par_rs, in_off, par_off);
    uint32_t flag[MT];  // the flag index is the parity row
#pragma unroll
    for (int j = 0; j < MT; j++) flag[j] = plan->out_row[j];

    for (TileWalk tw(t, nw, tpb); t < ntiles; t += nw, tw.next(tpb)) {
        const uint32_t blk = tw.blk;
        uint32_t syn[MT][4];
        uint64_t dirty = 0;  // the lanes that saw a non-zero syndrome (wave-uniform)
        stripe_tile<K, MT, UA>(
            s_tbl, in + uint64_t(blk) * in_bs, par + uint64_t(blk) * par_bs, in_off, par_off,
            lane_chunk<UA>(tw.tib, lane, cpb, S), cpb, S, GfNone{}, GfNone{}, GfNone{},
            [&](int j, const uint32_t(&s)[4], const u32x4&) {
                uint32_t d = 0;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    syn[j][w] = s[w];
                    d |= s[w];
                }
                // one relaxed agent-scope OR from one lane, and only when some lane of the wave saw a
                // difference: a vector atomic (no return value), never issued on a clean tile
                const uint64_t dj = __builtin_amdgcn_ballot_w64(d != 0u);
                if (dj != 0ull && lane == 0u)
                    __hip_atomic_fetch_or(bad + uint64_t(blk) * m + flag[j], 1u, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
                if constexpr (LOC) dirty |= dj;
            });
        if constexpr (LOC) {
            // a clean tile does nothing more: no store, no atomic
            if (dirty != 0ull) locate_tile<K, MT>(s_tbl + K * (kColDwords / 4), syn, lane, cand + blk);
        }
    }
}

// the plan's tables (and, when given, the ratio plan's behind them) into LDS, by the workgroup
template <int K>
__device__ __forceinline__ void stage_tables(u32x4* s_tbl, const RsPlanDev* plan, const RsPlanDev* rplan) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_tbl);
    for (int i = threadIdx.x; i < K * kColDwords; i += kFastWG) dst[i] = plan->tbl[i];
    if (rplan)
        for (int i = threadIdx.x; i < K * kColDwords; i += kFastWG) dst[K * kColDwords + i] = rplan->tbl[i];
    __syncthreads();
}

// The tile loop of rs_heal_kernel: stripe_tile over the blocks whose verdict names a shard x
// (verdict[block] >= 0, rsmi_locate's), and one row store that makes the stripe clean:
//   parity shard x = K + j   row ^= syn_j                  (= encode(data)_j)
//   data shard x             row ^= inv(M[0][x]) * syn_0   (syn_0 = M[0][x] * the row's error)
// (inv(M[0][c]): output slot 0 of the ratio plan's tables).  A tile of a block with a negative
// verdict loads nothing, and s_tbl is staged here, only by a workgroup with a tile to heal.
// old, the row's bytes before the heal, are those of the load the syndromes came from: a parity
// chunk is handed over by stripe_tile, a data chunk is kept as it passes through the column loop
// (before_col), decided there column by column and pinned with an empty asm volatile: left to the
// compiler the K selects sink below the loop and every row stays live.  No byte is loaded twice,
// so on UA layouts, where the row's last window overlaps the one before it and the two may belong
// to different waves, the update is idempotent per byte: a byte another wave has healed already
// gives a zero syndrome and stays, an unhealed one gives the same delta in both waves.
// A lane past the row's last chunk, a lane whose delta is zero and a tile where every delta is
// zero store nothing; an aligned row's last, partial chunk is stored as dwords, then bytes
// (store_rows_aligned), so no byte at or past S is written.
template <int K, int MT, bool UA>
__device__ __forceinline__ void heal_tiles(u32x4* s_tbl, const RsPlanDev* __restrict__ plan,
                                           const RsPlanDev* __restrict__ rplan, uint8_t* in, uint8_t* par,
                                           uint64_t in_bs, uint64_t in_rs, uint64_t par_bs, uint64_t par_rs,
                                           uint32_t S, uint32_t cpb, uint32_t tpb, uint32_t ntiles,
                                           const int32_t* __restrict__ verdict) {
    const WaveTiles wt = wave_tiles<UA>();
    const uint32_t lane = wt.lane, nw = wt.nw;
    uint32_t t = wt.t;

    // one scalar load per tile of the wave (one tile, unless waves_per_cu caps the grid): a
    // workgroup with nothing to heal ends here, before the tables and before any row load
    int work = 0;
    for (uint32_t u = t; u < ntiles; u += nw) work |= int(verdict[u / tpb] >= 0);
    if (!__syncthreads_or(work)) return;
    stage_tables<K>(s_tbl, plan, rplan);
    if (!work) return;

    uint64_t in_off[K], par_off[MT];
    row_offsets<K, MT>(plan, in_rs, par_rs, in_off, par_off);

    for (TileWalk tw(t, nw, tpb); t < ntiles; t += nw, tw.next(tpb)) {
        const uint32_t blk = tw.blk;
        const int32_t vd = __builtin_amdgcn_readfirstlane(verdict[blk]);
        if (vd < 0 || vd >= K + MT) continue;
        const uint32_t xr = uint32_t(vd);  // the culprit row, wave-uniform
        uint8_t* ib = in + uint64_t(blk) * in_bs;
        uint8_t* pb = par + uint64_t(blk) * par_bs;
        const LaneChunk lc = lane_chunk<UA>(tw.tib, lane, cpb, S);

        u32x4 old = {0u, 0u, 0u, 0u};  // the culprit row's chunk as loaded
        uint32_t syn0[4], delta[4] = {0u, 0u, 0u, 0u};
        stripe_tile<K, MT, UA>(
            s_tbl, ib, pb, in_off, par_off, lc, cpb, S,
            [&](int c, u32x4& x) {
                if (uint32_t(c) == xr) old = x;
                asm volatile("" : "+v"(old));
            },
            GfNone{}, GfNone{},
            [&](int j, const uint32_t(&s)[4], const u32x4& sp) {
                if (j == 0) {
#pragma unroll
                    for (int w = 0; w < 4; w++) syn0[w] = s[w];
                }
                if (xr == uint32_t(K + j)) {
                    old = sp;
#pragma unroll
                    for (int w = 0; w < 4; w++) delta[w] = s[w];
                }
            });
        uint8_t* row;
        if (xr < uint32_t(K)) {
            // inv(M[0][x]) * syn_0, the column's tables from LDS
            const u32x4* rt = s_tbl + K * (kColDwords / 4) + xr * 5u;
            u32x4 T[5];
#pragma unroll
            for (int f = 0; f < 5; f++) T[f] = rt[f];
#pragma unroll
            for (int w = 0; w < 4; w++) delta[w] = gf_mul_dword(T, 0, gf_selectors(syn0[w]));
            row = ib + uint64_t(plan->in_row[xr]) * in_rs;
        } else {
            row = pb + uint64_t(plan->out_row[xr - uint32_t(K)]) * par_rs;
        }
        const bool mine = (delta[0] | delta[1] | delta[2] | delta[3]) != 0u;
        if (__builtin_amdgcn_ballot_w64(mine) == 0ull) continue;
        if (mine && lc.ch < cpb) {
            const uint32_t fix[1][4] = {
                {u4get(old, 0) ^ delta[0], u4get(old, 1) ^ delta[1], u4get(old, 2) ^ delta[2], u4get(old, 3) ^ delta[3]}};
            if constexpr (UA) {
                st16u<false>(row + lc.win, u32x4{fix[0][0], fix[0][1], fix[0][2], fix[0][3]});
            } else {
                const uint64_t off[1] = {0};
                store_rows_aligned<0, 1>(row, off, lc.ch, S, fix);
            }
        }
    }
}

}  // namespace rsmi
