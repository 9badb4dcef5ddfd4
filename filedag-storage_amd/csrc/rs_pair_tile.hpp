// rs_pair_tile.hpp -- the pair tests of rs_locate_pair_kernel (rs_pair_kernels.hip): which pairs
// of shards {x, y} explain a dirty tile?  With H = [M | I] the code's check matrix, a pair explains
// a byte column iff its syndrome vector lies in span{h_x, h_y}; rsmi_locate_pair_checks
// (rsmi_pair.cpp) states that as m - 2 check rows per pair, and plan "P" carries the coefficients
// of those rows that are not 0, 1 or a ratio of plan "L".  pair_tiles is heal_tiles' loop
// (rs_verify_tile.hpp) with the pair tests in the place of the row store.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rsmi.h"
#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"
#include "rs_verify_tile.hpp"

namespace rsmi {

// a dword times the coefficient whose five table words are U
__device__ __forceinline__ uint32_t gf_mul_words(const uint32_t (&U)[5], const GfSel& s) {
    const uint32_t p1 = __builtin_amdgcn_perm(U[1], U[0], s.s1);
    const uint32_t p2 = __builtin_amdgcn_perm(U[3], U[2], s.s2);
    const uint32_t p3 = __builtin_amdgcn_perm(U[4], U[4], s.s3);
    return xor3(p1, p2, p3);
}

// One pair test: v[l] == coef_l * x for l = 2 .. MT-1 over the lane's 16 bytes, x given by its
// selector words sx.  ptbl: plan "P"'s pair columns in LDS; tau: the test's index, so coefficient
// l - 2 of the test is number e = tau * (MT - 2) + l - 2, output slot e % 4 of column block e / 4.
// True when no lane of the wave sees a difference.  One ballot per check row: nearly every pair
// fails, and most of them on their first row, so the second row's multiplies are rarely run.
template <int MT>
__device__ __forceinline__ bool pair_test(const uint32_t* ptbl, uint32_t tau, const GfSel (&sx)[4],
                                          const uint32_t (&v)[MT][4]) {
#pragma unroll
    for (int l = 2; l < MT; l++) {
        const uint32_t e = tau * uint32_t(MT - 2) + uint32_t(l - 2);
        const uint32_t* p = ptbl + (e >> 2) * uint32_t(kColDwords) + (e & 3u);
        uint32_t U[5];
#pragma unroll
        for (int f = 0; f < 5; f++) U[f] = p[f * 4];
        uint32_t diff = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) diff |= gf_mul_words(U, sx[w]) ^ v[l][w];
        if (__builtin_amdgcn_ballot_w64(diff != 0u) != 0ull) return false;
    }
    return true;
}

// The pairs that explain a dirty tile, ANDed into the block's pair words (bit pair_bit(n, x, y);
// all-ones before the launch).  syn: the lane's masked syndromes; rtbl: plan "L"'s columns (the
// ratios R[l][c] = M[l][c] / M[0][c]); ptbl: plan "P"'s pair columns.  With
// t_l = syn_l ^ R[l][c] * syn_0, over every byte of the tile
//   {K+i, K+j}       syn_l == 0 for every l other than i, j
//   {c, K+j}, j >= 1 t_l == 0 for every l >= 1 other than j
//   {c, K+0}         syn_l == (R[l][c] / R[1][c]) * syn_1 for l >= 2
//   {c, d}, c < d    t_l == (q_l / q_1) * t_1 for l >= 2, q_l = M[l][d] ^ R[l][c] * M[0][d]
// A byte column whose syndromes are all zero passes every test, so the tests run over all 16
// bytes of every lane and a clean lane (or one past the row's end) votes for every pair, as in
// locate_tile.  Each check row is one ballot; the wave's words are built in scalar registers (the
// pairs of one data shard c are consecutive bits, folded in with constant word indices) and one
// lane ANDs in the words that lost a bit.  Rolled: a dirty tile of an UNKNOWN block is the rare
// case, the code stays small.  Rows that overlap (UA windows) are tested twice; an AND does not
// see it.
template <int K, int MT>
__device__ __forceinline__ void pair_tile(const u32x4* rtbl, const uint32_t* ptbl, const uint32_t (&syn)[MT][4],
                                          uint32_t lane, uint32_t* words) {
    constexpr int N = K + MT, W = pair_words(N);
    uint32_t wm[W];
#pragma unroll
    for (int w = 0; w < W; w++) wm[w] = ~0u;

    // parity rows whose syndrome is zero over the whole tile
    bool sz[MT];
#pragma unroll
    for (int j = 0; j < MT; j++)
        sz[j] = __builtin_amdgcn_ballot_w64((syn[j][0] | syn[j][1] | syn[j][2] | syn[j][3]) != 0u) == 0ull;
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = i + 1; j < MT; j++) {
            bool ok = true;
#pragma unroll
            for (int l = 0; l < MT; l++)
                if (l != i && l != j) ok = ok && sz[l];
            const int p = pair_bit(N, K + i, K + j);
            if (!ok) wm[p >> 5] &= ~(1u << (p & 31));
        }

    // the selector words of syn_0 (the ratios' factor) and of syn_1 ({c, K+0}), shared by every c
    GfSel s0[4], s1[4];
#pragma unroll
    for (int w = 0; w < 4; w++) {
        s0[w] = gf_selectors(syn[0][w]);
        s1[w] = gf_selectors(syn[1][w]);
    }
    uint32_t tau = 0;
#pragma unroll 1
    for (int c = 0; c < K; c++) {
        u32x4 T[5];
#pragma unroll
        for (int f = 0; f < 5; f++) T[f] = rtbl[c * 5 + f];
        uint32_t t[MT][4];
        bool tz[MT];
#pragma unroll
        for (int l = 1; l < MT; l++) {
#pragma unroll
            for (int w = 0; w < 4; w++) t[l][w] = gf_mul_dword(T, l, s0[w]) ^ syn[l][w];
            tz[l] = __builtin_amdgcn_ballot_w64((t[l][0] | t[l][1] | t[l][2] | t[l][3]) != 0u) == 0ull;
        }
        // row c of the pair order: bit y - c - 1 is pair {c, y}; fail collects the pairs that lost
        uint32_t fail = 0;
#pragma unroll
        for (int j = 1; j < MT; j++) {
            bool ok = true;
#pragma unroll
            for (int l = 1; l < MT; l++)
                if (l != j) ok = ok && tz[l];
            if (!ok) fail |= 1u << uint32_t(K + j - c - 1);
        }
        if (!pair_test<MT>(ptbl, tau, s1, syn)) fail |= 1u << uint32_t(K - c - 1);
        tau++;
        GfSel st[4];  // the selector words of t_1, shared by every d
#pragma unroll
        for (int w = 0; w < 4; w++) st[w] = gf_selectors(t[1][w]);
#pragma unroll 1
        for (int d = c + 1; d < K; d++) {
            if (!pair_test<MT>(ptbl, tau, st, t)) fail |= 1u << uint32_t(d - c - 1);
            tau++;
        }
        // at most N - 1 <= 19 bits from bit pair_bit(N, c, c + 1) on: two words at the most
        const uint32_t base = uint32_t(c * N - c * (c + 1) / 2);
        const uint64_t f64 = uint64_t(fail) << (base & 31u);
        const uint32_t lo = ~uint32_t(f64), hi = ~uint32_t(f64 >> 32), wi = base >> 5;
#pragma unroll
        for (int w = 0; w < W; w++) wm[w] &= uint32_t(w) == wi ? lo : uint32_t(w) == wi + 1u ? hi : ~0u;
    }
    if (lane == 0u) {
#pragma unroll
        for (int w = 0; w < W; w++)
            if (wm[w] != ~0u) (void)__hip_atomic_fetch_and(words + w, wm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The tile loop of rs_locate_pair_kernel, heal_tiles' shape: one scalar load per tile of the wave
// reads the block's verdict (rsmi_locate's), and a workgroup with no UNKNOWN block ends before
// the tables are staged and before any row load.  A tile of an UNKNOWN block runs stripe_tile once
// more and, when some lane saw a non-zero syndrome, the pair tests.  s_tbl: the encode plan's K
// columns, then plan "P"'s: the K ratio columns of plan "L" and the pair columns.  pairw: the
// launch's first block's pair words, pair_words(K + MT) per block.
template <int K, int MT, bool UA>
__device__ __forceinline__ void pair_tiles(u32x4* s_tbl, const RsPlanDev* __restrict__ plan,
                                           const RsPlanDev* __restrict__ pplan, const uint8_t* __restrict__ in,
                                           const uint8_t* __restrict__ par, uint64_t in_bs, uint64_t in_rs,
                                           uint64_t par_bs, uint64_t par_rs, uint32_t S, uint32_t cpb, uint32_t tpb,
                                           uint32_t ntiles, const int32_t* __restrict__ verdict,
                                           uint32_t* __restrict__ pairw) {
    constexpr int NP = pair_blocks(K, MT), W = pair_words(K + MT);
    const WaveTiles wt = wave_tiles<UA>();
    const uint32_t lane = wt.lane, nw = wt.nw;
    uint32_t t = wt.t;

    int work = 0;
    for (uint32_t u = t; u < ntiles; u += nw) work |= int(verdict[u / tpb] == RSMI_LOCATE_UNKNOWN);
    if (!__syncthreads_or(work)) return;
    {
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_tbl);
        for (int i = threadIdx.x; i < K * kColDwords; i += kFastWG) dst[i] = plan->tbl[i];
        for (int i = threadIdx.x; i < (K + NP) * kColDwords; i += kFastWG) dst[K * kColDwords + i] = pplan->tbl[i];
        __syncthreads();
    }
    if (!work) return;

    uint64_t in_off[K], par_off[MT];
    row_offsets<K, MT>(plan, in_rs, par_rs, in_off, par_off);

    for (TileWalk tw(t, nw, tpb); t < ntiles; t += nw, tw.next(tpb)) {
        const uint32_t blk = tw.blk;
        if (__builtin_amdgcn_readfirstlane(verdict[blk]) != RSMI_LOCATE_UNKNOWN) continue;
        uint32_t syn[MT][4];
        uint64_t dirty = 0;  // the lanes that saw a non-zero syndrome (wave-uniform)
        stripe_tile<K, MT, UA>(s_tbl, in + uint64_t(blk) * in_bs, par + uint64_t(blk) * par_bs, in_off, par_off,
                               lane_chunk<UA>(tw.tib, lane, cpb, S), cpb, S, GfNone{}, GfNone{}, GfNone{},
                               [&](int j, const uint32_t(&s)[4], const u32x4&) {
                                   uint32_t d = 0;
#pragma unroll
                                   for (int w = 0; w < 4; w++) {
                                       syn[j][w] = s[w];
                                       d |= s[w];
                                   }
                                   dirty |= __builtin_amdgcn_ballot_w64(d != 0u);
                               });
        if (dirty == 0ull) continue;
        pair_tile<K, MT>(s_tbl + K * (kColDwords / 4),
                         reinterpret_cast<const uint32_t*>(s_tbl + 2 * K * (kColDwords / 4)), syn, lane,
                         pairw + uint64_t(blk) * W);
    }
}

}  // namespace rsmi
