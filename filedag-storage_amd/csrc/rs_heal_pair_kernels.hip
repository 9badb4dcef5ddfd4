// rs_heal_pair_kernels.hip -- rsmi_heal_pair on the GPU: rewrite the one or two shards that break a
// stripe.
//
// rs_heal_pair_kernel follows rs_locate_pair_verdict_kernel on the stream and reads its verdicts,
// two words per block.  A tile of a block whose verdict names no shard ((-1, -1) or (-2, -2)) costs
// its wave one scalar load; a tile of a block with (x, y) or (x, -1) runs Verify's pipeline once
// more (stripe_tile, rs_verify_tile.hpp: the same ring, loads, masks and lane chunks), keeps the
// chunks of rows x and y as loaded and the two syndromes the block's explanation reads, and stores
//   row x ^= D[0][l0] * syn_l0 ^ D[0][l1] * syn_l1
//   row y ^= D[1][l0] * syn_l0 ^ D[1][l1] * syn_l1
// with D = rsmi_heal_pair_matrix(x, y), from the same loads the syndromes were formed from.  Only
// rows x and y are written, only bytes [0, S).  rs_heal_pair_rows_kernel is the byte-granular form
// for the shapes rs_heal_pair_kernel is not built for, over the rows the fallback encodes into
// scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"
#include "rs_verify_tile.hpp"

namespace rsmi {

// The tile loop of rs_heal_pair_kernel, heal_tiles' shape (rs_verify_tile.hpp).  verdict: two
// words per block, rsmi_locate_pair's; hplan: plan "H" (rs_plan.hpp), one column per explanation.
// s_tbl: the encode plan's K columns, staged only by a workgroup with a tile to heal.
//
// The coefficients are the block's own and wave-uniform.  l0 and l1 are read with one scalar load
// ahead of the tile; they are not needed before the first parity row arrives, so the load hides
// behind the column loop.  The column's 80 bytes of v_perm tables are fetched after the tile, when
// the ring's registers are free, by five 16-byte vector loads at one address for the whole wave
// (the address is made opaque so that it stays a vector one): a broadcast read of one or two L2
// lines.  Scalar loads would put the 20 words into SGPRs, and v_perm_b32 takes both halves of its
// byte pool from the tables: a VOP3 instruction reads one SGPR at the most on gfx9 (the constant
// bus), so every second word would be copied into a VGPR first.  The whole plan in LDS (RS(16,4):
// 210 columns, 16.4 KiB beside the encode tables) fits a CU's 160 KiB at 4-5 workgroups, but every
// workgroup with a tile to heal would stage all of it to read at most four columns.
//
// old_x, old_y, the rows' bytes before the heal, are those of the loads the syndromes came from:
// a parity chunk is handed over by stripe_tile, a data chunk is kept as it passes through the
// column loop, pinned column by column as heal_tiles pins its one.  No byte is loaded twice, and
// D [h_x h_y] = I_2: a byte column in which rows x and y were loaded with the errors (a, b), each
// either the row's error or zero, has syn = h_x a ^ h_y b and gets the deltas (a, b).  So on UA
// layouts, where a row's last window overlaps the one before it and the two may belong to
// different waves, the update is idempotent per byte, whichever of the two rows another wave has
// healed already.
// A lane past the row's last chunk, a lane whose delta in a row is zero and a tile where every
// delta is zero store nothing; an aligned row's last, partial chunk is stored as dwords, then
// bytes (store_rows_aligned), so no byte at or past S is written.
template <int K, int MT, bool UA>
__device__ __forceinline__ void heal_pair_tiles(u32x4* s_tbl, const RsPlanDev* __restrict__ plan,
                                                const RsPlanDev* __restrict__ hplan, uint8_t* in, uint8_t* par,
                                                uint64_t in_bs, uint64_t in_rs, uint64_t par_bs, uint64_t par_rs,
                                                uint32_t S, uint32_t cpb, uint32_t tpb, uint32_t ntiles,
                                                const int32_t* __restrict__ verdict) {
    constexpr int N = K + MT;
    const WaveTiles wt = wave_tiles<UA>();
    const uint32_t lane = wt.lane, nw = wt.nw;
    uint32_t t = wt.t;

    // scalar loads of the verdicts of the wave's tiles (one tile, unless waves_per_cu caps the
    // grid): a workgroup with nothing to heal ends here, before the tables and before any row load.
    // The first word says it all: it is negative exactly when no shard is named.
    int work = 0;
    for (uint32_t u = t; u < ntiles; u += nw) work |= int(verdict[2u * (u / tpb)] >= 0);
    if (!__syncthreads_or(work)) return;
    stage_tables<K>(s_tbl, plan, nullptr);
    if (!work) return;

    uint64_t in_off[K], par_off[MT];
    row_offsets<K, MT>(plan, in_rs, par_rs, in_off, par_off);

    for (TileWalk tw(t, nw, tpb); t < ntiles; t += nw, tw.next(tpb)) {
        const uint32_t blk = tw.blk;
        const int32_t vx = __builtin_amdgcn_readfirstlane(verdict[2u * blk]);
        const int32_t vy = __builtin_amdgcn_readfirstlane(verdict[2u * blk + 1u]);
        // (x, -1) or (x, y) with x < y < n; anything else names nothing
        if (vx < 0 || vx >= N || vy >= N || (vy >= 0 && vy <= vx)) continue;
        const uint32_t xr = uint32_t(vx), yr = uint32_t(vy);  // the rows, wave-uniform; yr = ~0: none
        const uint32_t e = uint32_t(vy < 0 ? N * (N - 1) / 2 + vx : vx * N - vx * (vx + 1) / 2 + (vy - vx - 1));
        const uint32_t ll = hplan->in_row[e];
        const uint32_t l0 = ll & 0xFFu, l1 = ll >> 8;
        uint8_t* ib = in + uint64_t(blk) * in_bs;
        uint8_t* pb = par + uint64_t(blk) * par_bs;
        const LaneChunk lc = lane_chunk<UA>(tw.tib, lane, cpb, S);

        u32x4 oldx = {0u, 0u, 0u, 0u}, oldy = {0u, 0u, 0u, 0u};  // the rows' chunks as loaded
        uint32_t s0[4] = {0u, 0u, 0u, 0u}, s1[4] = {0u, 0u, 0u, 0u};  // syn_l0, syn_l1
        stripe_tile<K, MT, UA>(
            s_tbl, ib, pb, in_off, par_off, lc, cpb, S,
            [&](int c, u32x4& x) {
                if (uint32_t(c) == xr) oldx = x;
                if (uint32_t(c) == yr) oldy = x;
                asm volatile("" : "+v"(oldx), "+v"(oldy));
            },
            GfNone{}, GfNone{},
            [&](int j, const uint32_t(&s)[4], const u32x4& sp) {
                if (xr == uint32_t(K + j)) oldx = sp;
                if (yr == uint32_t(K + j)) oldy = sp;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    if (l0 == uint32_t(j)) s0[w] = s[w];
                    if (l1 == uint32_t(j)) s1[w] = s[w];
                }
            });
        // both syndromes zero in every lane: every delta is zero, the tables are not fetched
        if (__builtin_amdgcn_ballot_w64((s0[0] | s0[1] | s0[2] | s0[3] | s1[0] | s1[1] | s1[2] | s1[3]) != 0u) == 0ull)
            continue;

        uint32_t eo = e * uint32_t(kColDwords / 4);
        asm volatile("" : "+v"(eo));
        const u32x4* ht = reinterpret_cast<const u32x4*>(hplan->tbl) + eo;
        u32x4 T[5];
#pragma unroll
        for (int f = 0; f < 5; f++) T[f] = ht[f];
        uint32_t dx[1][4], dy[1][4];
        uint32_t ox = 0, oy = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const GfSel a = gf_selectors(s0[w]), b = gf_selectors(s1[w]);
            dx[0][w] = gf_mul_dword(T, 0, a) ^ gf_mul_dword(T, 1, b);
            dy[0][w] = gf_mul_dword(T, 2, a) ^ gf_mul_dword(T, 3, b);
            ox |= dx[0][w];
            oy |= dy[0][w];
        }
        if (__builtin_amdgcn_ballot_w64((ox | oy) != 0u) == 0ull) continue;
        // a row's delta is zero wherever its syndromes are masked out: in a lane past the row's
        // last chunk, and in the bytes at or past S
        auto store = [&](uint32_t r, const u32x4& old, uint32_t (&d)[1][4]) {
            uint8_t* row = r < uint32_t(K) ? ib + uint64_t(plan->in_row[r]) * in_rs
                                           : pb + uint64_t(plan->out_row[r - uint32_t(K)]) * par_rs;
#pragma unroll
            for (int w = 0; w < 4; w++) d[0][w] ^= u4get(old, w);
            if constexpr (UA) {
                st16u<false>(row + lc.win, u32x4{d[0][0], d[0][1], d[0][2], d[0][3]});
            } else {
                const uint64_t off[1] = {0};
                store_rows_aligned<0, 1>(row, off, lc.ch, S, d);
            }
        };
        if (ox && lc.ch < cpb) store(xr, oldx, dx);
        if (oy && vy >= 0 && lc.ch < cpb) store(yr, oldy, dy);
    }
}

// rs_locate_kernel's parameter list (launch_stripe_tiles serves it): hplan, plan "H"; verdict, the
// launch's first block's two verdict words.  bad and m are not used.
template <int K, int MT, bool UA>
__global__ __launch_bounds__(kFastWG, kMinWavesPerSimd) void rs_heal_pair_kernel(
    const RsPlanDev* __restrict__ plan, uint8_t* in, uint8_t* par, uint64_t in_bs, uint64_t in_rs, uint64_t par_bs,
    uint64_t par_rs, uint32_t S, uint32_t cpb, uint32_t tpb, uint32_t ntiles, uint32_t* __restrict__ bad, uint32_t m,
    const RsPlanDev* __restrict__ hplan, const int32_t* __restrict__ verdict) {
    __shared__ u32x4 s_tbl[K * kColDwords / 4];
    (void)bad;
    (void)m;
    heal_pair_tiles<K, MT, UA>(s_tbl, plan, hplan, in, par, in_bs, in_rs, par_bs, par_rs, S, cpb, tpb, ntiles, verdict);
}

// Byte-granular heal of the blocks whose verdict names one or two shards, any shape with m >= 3
// and any alignment, n up to 256.  enc: the encode of the data rows as they are stored (context
// scratch, m rows per block); par: the stored parity rows; data: the stored data rows; verdict:
// two words per block.  tbl: GF(2^8) log[256] | exp[512] | R[m][k] | inv(M[0][c])[k]
// (rsmi_locate.cpp), so M[l][c] = R[l][c] / inv(M[0][c]).  Per block the workgroup forms
// rsmi_heal_pair_matrix(x, y)'s two columns l0, l1 and four coefficients (a single shard x: the
// first row alone), then over x in [0, S)
//   row_x[i] ^= D00 * syn_l0[i] ^ D01 * syn_l1[i]     row_y[i] ^= D10 * syn_l0[i] ^ D11 * syn_l1[i]
// with syn_l = enc_l ^ par_l; a byte that is right already is not written.
__global__ __launch_bounds__(kWG) void rs_heal_pair_rows_kernel(const uint8_t* __restrict__ enc, uint64_t enc_rs,
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
    auto mul = [&](uint32_t x, uint32_t y) -> uint32_t {
        return x && y ? uint32_t(s_exp[uint32_t(s_log[x]) + uint32_t(s_log[y])]) : 0u;
    };
    auto inv = [&](uint32_t x) -> uint32_t { return uint32_t(s_exp[255u - uint32_t(s_log[x])]); };
    const uint32_t n = k + m;
    // M[l][c] of the encode matrix's parity part (no MDS matrix has a zero there)
    auto M = [&](uint32_t l, uint32_t c) -> uint32_t {
        return mul(uint32_t(tbl[768u + l * k + c]), inv(uint32_t(tbl[768u + m * k + c])));
    };
    for (uint64_t blk = blockIdx.y; blk < nblocks; blk += gridDim.y) {
        const int32_t vx = verdict[2 * blk], vy = verdict[2 * blk + 1];  // uniform over the workgroup, as blk is
        if (vx < 0 || uint32_t(vx) >= n || vy >= int32_t(n) || (vy >= 0 && vy <= vx)) continue;
        const uint32_t x = uint32_t(vx), y = uint32_t(vy);
        uint32_t l0 = 0, l1 = 1, d00 = 0, d01 = 0, d10 = 0, d11 = 0;
        if (vy < 0) {
            // rsmi_heal's update: a parity row from its own syndrome, a data row from syn_0
            l0 = x >= k ? x - k : 0u;
            l1 = l0;
            d00 = x >= k ? 1u : uint32_t(tbl[768u + m * k + x]);
        } else if (x >= k) {
            l0 = x - k;
            l1 = y - k;
            d00 = d11 = 1u;
        } else if (y >= k) {
            l1 = y - k;
            l0 = l1 == 0u ? 1u : 0u;
            d00 = inv(M(l0, x));
            d10 = mul(M(l1, x), d00);
            d11 = 1u;
        } else {
            const uint32_t a = M(0, x), b = M(0, y), cc = M(1, x), dd = M(1, y);
            const uint32_t det = mul(a, dd) ^ mul(b, cc);
            if (!det) continue;  // no MDS matrix has a singular minor
            const uint32_t idet = inv(det);
            d00 = mul(dd, idet);
            d01 = mul(b, idet);
            d10 = mul(cc, idet);
            d11 = mul(a, idet);
        }
        const uint8_t* e0 = enc + blk * enc_bs + uint64_t(l0) * enc_rs;
        const uint8_t* e1 = enc + blk * enc_bs + uint64_t(l1) * enc_rs;
        uint8_t* p0 = par + blk * par_bs + uint64_t(l0) * par_rs;
        uint8_t* p1 = par + blk * par_bs + uint64_t(l1) * par_rs;
        auto row = [&](uint32_t r) -> uint8_t* {
            return r < k ? data + blk * data_bs + uint64_t(r) * data_rs : par + blk * par_bs + uint64_t(r - k) * par_rs;
        };
        uint8_t* rx = row(x);
        uint8_t* ry = vy >= 0 ? row(y) : rx;
        for (uint64_t i = uint64_t(blockIdx.x) * kWG + threadIdx.x; i < S; i += uint64_t(gridDim.x) * kWG) {
            const uint32_t s0 = uint32_t(e0[i] ^ p0[i]), s1 = uint32_t(e1[i] ^ p1[i]);
            if (!(s0 | s1)) continue;
            const uint32_t dx = mul(d00, s0) ^ mul(d01, s1), dy = mul(d10, s0) ^ mul(d11, s1);
            if (dx) rx[i] ^= uint8_t(dx);
            if (dy) ry[i] ^= uint8_t(dy);
        }
    }
}

void* heal_pair_rows_kernel() { return reinterpret_cast<void*>(&rs_heal_pair_rows_kernel); }

template <int K, int MT>
static void fill_heal_pair_km(HealPairKernelTable& t) {
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_heal_pair_kernel<K, MT, false>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_heal_pair_kernel<K, MT, true>);
}

template <int K>
static void fill_heal_pair_k(HealPairKernelTable& t) {
    fill_heal_pair_km<K, 3>(t);
    fill_heal_pair_km<K, 4>(t);
}

// the K and m of the pair kernels: every verdict they can give has a kernel to act on it
const HealPairKernelTable& heal_pair_kernels() {
    static const HealPairKernelTable t = [] {
        HealPairKernelTable x{};
        fill_heal_pair_k<1>(x);
        fill_heal_pair_k<2>(x);
        fill_heal_pair_k<3>(x);
        fill_heal_pair_k<4>(x);
        fill_heal_pair_k<5>(x);
        fill_heal_pair_k<6>(x);
        fill_heal_pair_k<8>(x);
        fill_heal_pair_k<10>(x);
        fill_heal_pair_k<12>(x);
        fill_heal_pair_k<16>(x);
        return x;
    }();
    return t;
}

}  // namespace rsmi
