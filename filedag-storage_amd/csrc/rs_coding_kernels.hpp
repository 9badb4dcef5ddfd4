// rs_coding_kernels.hpp -- CDNA4 (gfx950) Reed-Solomon coding kernel templates, instantiated by
// rs_kernels.hip (the table-less forms) and rs_kernels_tb.hip (the table-of-bases forms).
//
// One kernel family computes every RS operation the Dag Node needs:
//   out_row[j][x] = XOR_c coef[j][c] * in_row[c][x]      (GF(2^8), poly 0x11D)
// Encode (erasure.go:60, upstream Encode) uses the parity rows of the systematic matrix
// over the k data rows; reconstruct (erasure.go:82/88, ReconstructData/Reconstruct) uses
// the decode rows over the first k present rows.  Positions x are independent, so the
// kernel is a pure HBM stream: read K rows, write MT rows, no reuse across workgroups.
// The GF(2^8) arithmetic is rs_gf_tile.hpp's pipeline.
//
// Layout contract (fast path): row r of block b lives at base + b*bstride + r*rstride,
// every base/stride 16-byte aligned, rstride >= roundup(S,16).  A wave owns a "tile" of
// 64*D consecutive 16-byte chunks of one block; lanes past the block's last chunk clamp
// their loads to a valid chunk and skip their stores, and the one partial chunk at the
// end of a row is stored bytewise so no byte at or past S is ever written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "crc16.hpp"
#include "rs_crc16_device.hpp"
#include "rs_crc_fold.hpp"
#include "rs_device.hpp"
#include "rs_gf_tile.hpp"
#include "rs_plan.hpp"

namespace rsmi {

// A table copied into LDS in two steps: its words are loaded into registers at the kernel's
// start and written to LDS (then one barrier) once the wave's first rows are in flight, so the
// table's latency and the rows' overlap instead of adding up (a per-block call over PCIe is
// latency-bound, tools/latency.cpp).  Every thread of the workgroup takes part.
template <int N>
struct LdsTable {
    static constexpr int kPer = (N + kWG - 1) / kWG;
    uint32_t r[kPer];
    __device__ __forceinline__ void load(const uint32_t* __restrict__ src) {
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const int x = int(threadIdx.x) + i * kWG;
            r[i] = x < N ? src[x] : 0u;
        }
    }
    __device__ __forceinline__ void store(uint32_t* dst) const {
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const int x = int(threadIdx.x) + i * kWG;
            if (x < N) dst[x] = r[i];
        }
    }
};

// Block blk's rows: at p + blk * bs, or, over a table of block bases (TB, BlockBases), at the
// table's entry for blk plus the offset p (one scalar load from the kernel arguments per wave).
// The diagnostic build RSMI_DIAG_CACHED (tools/Makefile diag-cached) wraps the tiles onto the
// first 16 blocks (~7 MB, cache-resident), so the kernel's own issue rate (VALU, LDS, waits) is
// what the launch time shows.
template <bool TB, class T>
__device__ __forceinline__ T* block_rows(const BasesArg<TB>& bases, T* p, uint32_t blk, uint64_t bs) {
#ifdef RSMI_DIAG_CACHED
    return p + uint64_t(blk & 15) * bs;
#else
    if constexpr (TB)
        return reinterpret_cast<T*>(uintptr_t(bases.b[blk]) + reinterpret_cast<uintptr_t>(p));
    else
        return p + uint64_t(blk) * bs;
#endif
}

// A table launch's completion release (BlockBases::done_flag; every workgroup calls it once, as
// its last act, with all its waves).  Every thread first releases its own stores at system scope
// (buffer_wbl2 + s_waitcnt vmcnt(0) in every wave): the barrier alone does not wait for other
// waves' stores on gfx950 (back-off barrier, and a workgroup-scope release emits no vmcnt wait in
// non-tgsplit mode), so without the per-wave fence waves 1..3 could still have parity or R(shard)
// stores in flight to page-locked host memory when wave 0 counts.  After the barrier, one
// system-scope fetch-add counts the workgroup, and the launch's last workgroup resets the counter
// for the next launch and releases the flag.  A table without a flag (and every table-less
// instantiation) skips all of it.  ISA check: DESIGN.md §4.3.
template <bool TB>
__device__ __forceinline__ void launch_done(const BasesArg<TB>& bases) {
    if constexpr (TB) {
        if (!bases.done_flag) return;  // kernel argument: uniform over the launch
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope, every thread
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t old = __hip_atomic_fetch_add(bases.done_ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM);
            if (old + 1u == gridDim.x) {
                __hip_atomic_store(bases.done_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(bases.done_flag, bases.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// K inputs, MT (<= 4) outputs, one 16-byte chunk per lane per row.
// NT: cache policy, 1 = nontemporal loads and stores (write-heavy tiles), 2 = nontemporal
// loads, default stores (tiles that read at least 4 rows per row written); DESIGN.md §4.1.
// WPS: waves per SIMD the register allocation must allow.
// UA: rows at any byte alignment and pitch (S >= 16).  A lane's 16-byte window starts at
// min(16*ch, S - 16): the row's last window overlaps the one before it instead of running
// past S, so loads never leave [0, S) and every store is a whole 16-byte window (the
// overlapped bytes get the same value from both lanes).  This serves the Split layout itself
// (rows back to back at pitch S, odd for RS(10,4)) and page-locked host memory read and
// written in place over PCIe.
// CRC (encode plans only: input row c is shard c, output row j shard K + j): also fold every
// row the tile reads or writes into CRC-16 values (crc16.hpp).  Lane q of each 4-lane quad
// folds its 16-byte chunk with the quad-relative nibble tables Q (relative to the end of the
// quad), two DPP XORs sum the quad, and lane q keeps rows r = q mod 4: one dword store per two
// such rows leaves the tile's record rec[(block * tpb + tile) * ns2 * 64 + s2 * 64 + lane]
// (rows 8 s2 + q and 8 s2 + 4 + q of quad lane / 4, u16 each).  Bytes at or past S count as
// zero (aligned layouts: the row's last chunk is masked).  UA: the row's last window ends at S,
// not on the 16-byte grid, so its chunk stays out of the quad sums and its value (relative to S)
// goes to tail[block * (K + MT) + r].  rs_crc16_combine_kernel turns records and tails into
// R(row).
// Launch geometry: one tile per wave; the loop strides over further tiles only
// when the caller caps the grid (option waves_per_cu).
// TB: the blocks lie where a table of block bases says (BlockBases: a coalesced group of callers'
// own page-locked buffers, one launch for the group); in / out are offsets from each base.
// ST: how the aligned form stores its output rows (store_policy, rs_plan.hpp): 0 plain, 1
// nontemporal, n >= 2 nontemporal but the last n - 1 rows plain, -1 write-through.  The default is
// what NT says, and the launch label prints NT alone.
// WMAX: at most this many waves per SIMD (waves_cap, rs_plan.hpp; 0: no cap).  The attribute stands
// before the launch bounds, which would override it.
template <int K, int MT, int NT, int WPS = kMinWavesPerSimd, bool UA = false, bool CRC = false, bool TB = false,
          int ST = (NT == 1 ? 1 : 0), int WMAX = 0>
__global__ __attribute__((amdgpu_waves_per_eu(WPS, WMAX)))
__launch_bounds__(kFastWG, WPS) void rs_fast_kernel(const RsPlanDev* __restrict__ plan,
                                                       const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                       uint64_t in_bs, uint64_t in_rs, uint64_t out_bs,
                                                       uint64_t out_rs, uint32_t S, uint32_t cpb, uint32_t tpb,
                                                       uint32_t ntiles, uint32_t head,
                                                       const uint32_t* __restrict__ crc_tbl,
                                                       uint32_t* __restrict__ crc_rec, uint32_t* __restrict__ crc_tail,
                                                       BasesArg<TB> bases) {
    static_assert(NT == 1 || NT == 2, "cache policy 1 or 2");
    static_assert(ST >= kStoreWriteThrough && ST <= MT, "store policy -1, 0, 1, or 2..MT: the last ST - 1 rows plain");
    static_assert(WMAX == 0 || WMAX >= WPS, "the occupancy cap is at least the floor");
    constexpr int NSH = K + MT;            // CRC: shards of the block (encode plans)
    constexpr int NSL = (NSH + 3) / 4;     // CRC: rows each lane keeps (r = q mod 4)
    __shared__ u32x4 s_tbl[K * kColDwords / 4];
    __shared__ uint32_t s_crc[CRC ? kCrcQWords : 1];
    {
        const uint32_t* src = plan->tbl;
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_tbl);
        for (int i = threadIdx.x; i < K * kColDwords; i += kFastWG) dst[i] = src[i];
        if constexpr (CRC)
            for (int i = threadIdx.x; i < kCrcQWords; i += kFastWG) s_crc[i] = crc_tbl[kCrcQOff + i];
    }
    __syncthreads();

    constexpr uint32_t kWavesPerWG = kFastWG / kWave;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t nw = gridDim.x * kWavesPerWG;
    // The first head workgroups are renumbered so each XCD (the dispatcher deals workgroups
    // round-robin over the 8 XCDs) sweeps one contiguous range of tiles; the rest keep the plain
    // order (tile_group, rs_plan.hpp; head chosen by launch_head).  UA: a row's 1 KiB tile at an
    // odd address shares its first and last 64-byte lines with the neighbouring tiles; with the
    // neighbours on the same XCD those lines come from one L2 (Split layout: encode +4-5%,
    // DESIGN.md §3), so head is the whole grid.  Aligned layouts share no lines: only the shapes
    // of tile_group_shape are ever passed a head, the others keep blockIdx.x.
    const uint32_t wg =
        (UA || tile_group_shape(K, MT)) ? tile_group(blockIdx.x, gridDim.x, head) : uint32_t(blockIdx.x);
    uint32_t t = wg * kWavesPerWG + wid;
    if constexpr (TB) {
        // a table launch may release a completion flag (launch_done, as every workgroup's last
        // act): its workgroups leave together, waves past the last tile skip the tile loop
        if (wg * kWavesPerWG >= ntiles) {
            launch_done<TB>(bases);
            return;
        }
    } else {
        if (t >= ntiles) return;
    }

    constexpr int P = rows_in_flight<K, MT>();
    uint64_t in_off[K], out_off[MT];
#pragma unroll
    for (int c = 0; c < K; c++) in_off[c] = uint64_t(plan->in_row[c]) * in_rs;
#pragma unroll
    for (int j = 0; j < MT; j++) out_off[j] = uint64_t(plan->out_row[j]) * out_rs;

    for (TileWalk tw(t, nw, tpb); t < ntiles; t += nw, tw.next(tpb)) {
        const uint32_t blk = tw.blk, tib = tw.tib;
        const uint8_t* ib = block_rows<TB>(bases, in, blk, in_bs);
        uint8_t* ob = block_rows<TB>(bases, out, blk, out_bs);
        const LaneChunk lc = lane_chunk<UA>(tib, lane, cpb, S);
        const uint32_t ch = lc.ch, chl = lc.chl, win = lc.win;
        // CRC: bytes of the lane's 16-byte chunk that are not part of the row's chunk ch count as
        // zero -- UA: the leading bytes of the row's overlapping last window; aligned: the bytes
        // at or past S of the row's last chunk.  The mask lives in the nibble-offset masks (a
        // zero nibble looks up a zero entry: the tables are linear), so it costs nothing per
        // row, and it is branch-free, so the folds stay in straight code (a branch inside the
        // column loop lets the compiler sink every column's GF math past it).
        uint32_t nm[4];  // per dword: 0x1E in every byte lane that counts
        uint32_t slot[NSL], tl[(NSH + 1) / 2];  // rows kept by this lane; UA: the last chunk's values
        bool in_quad = true;
        if constexpr (CRC) {
            const int lead = UA ? int(chl * 16u - win) : 0;          // UA: bytes before the chunk
            const int valid = UA ? 16 : int(S) - int(chl * 16u);     // aligned: bytes before S
#pragma unroll
            for (int w = 0; w < 4; w++) {
                uint32_t m = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int pos = 4 * w + b;
                    if (pos >= lead && pos < valid) m |= 0x1Eu << (8 * b);
                }
                nm[w] = m;
            }
            in_quad = UA ? ch + 1 < cpb : ch < cpb;  // UA: the last chunk is a tail; lanes past it add nothing
#pragma unroll
            for (int i = 0; i < NSL; i++) slot[i] = 0;
        }
        const uint32_t qq = (lane & 3u) * 0x20202020u;  // byte offset of this lane's table set
        // fold shard r's chunk x into this lane's slot for r (compile-time r after unrolling)
        auto crc_row = [&](const u32x4& x, int r) {
            if constexpr (CRC) {
                const uint8_t* qt = reinterpret_cast<const uint8_t*>(s_crc);
                uint32_t cr = 0;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    uint32_t lo = ((x[w] << 1) & nm[w]) | qq, hi = ((x[w] >> 3) & nm[w]) | qq;
                    asm volatile("" : "+v"(lo), "+v"(hi));  // one byte extract per offset
                    uint32_t l[8];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int p = 4 * w + q;
                        l[2 * q] = *reinterpret_cast<const uint16_t*>(qt + 256 * p + ((lo >> (8 * q)) & 0xFF));
                        l[2 * q + 1] = *reinterpret_cast<const uint16_t*>(qt + 256 * p + 128 + ((hi >> (8 * q)) & 0xFF));
                    }
                    // 8 lookups and the running value: four 3-input XORs
                    cr = xor3(xor3(l[0], l[1], l[2]), xor3(l[3], l[4], l[5]), xor3(l[6], l[7], cr));
                }
                if constexpr (UA) tl[r / 2] = (r & 1) ? (tl[r / 2] | (cr << 16)) : cr;
                cr = in_quad ? cr : 0u;
                cr ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(cr), 0xB1, 0xF, 0xF, false));  // quad_perm 1,0,3,2
                cr ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(cr), 0x4E, 0xF, 0xF, false));  // quad_perm 2,3,0,1
                slot[r / 4] = (lane & 3u) == uint32_t(r & 3) ? cr : slot[r / 4];
            }
        };
        // UA4 (read-heavy unaligned tiles): the lane's 16-byte window is loaded from the dword
        // boundary at or below it (a 4-byte-aligned dwordx4 plus the dword after it) and
        // funnel-shifted by the window's byte offset in that dword (v_alignbyte_b32), instead of
        // one byte-aligned 16-byte load: +7% on the Split layout's RS(10,4) 1-row reconstruct
        // (4.78 -> 5.11 TB/s, profiles/r03/ua/ua4_ab.txt).  Every dword loaded holds a byte of the
        // row: the dwordx4 holds the window's first byte, and the extra dword is the one holding its
        // last byte, (p + 15) & ~3.  That is the dword after the dwordx4 when the window is not
        // 4-aligned; when it is (r == 0: a row's last window at S - 16 with S a multiple of 4, as in
        // a page-exact buffer), it is the dwordx4's own last dword again, never the dword at S, and
        // alignbyte with r == 0 ignores it.
        constexpr bool UA4 = UA && (RSMI_UA_DWORD_LOADS == 2 || (NT == 2 && RSMI_UA_DWORD_LOADS == 1));
        uint32_t vx[UA4 ? P : 1];  // UA4: the dword holding each row's window's last byte
        auto load_col = [&](int c) {
            if constexpr (UA4) {
                const uintptr_t p = reinterpret_cast<uintptr_t>(ib + in_off[c] + win);
                const uintptr_t a = p & ~uintptr_t(3);
                vx[c % P] = *reinterpret_cast<const uint32_t*>((p + 15) & ~uintptr_t(3));
                return u32x4(*reinterpret_cast<const u32x4a4*>(a));
            } else if constexpr (UA) {
                // nontemporal loads for write-heavy tiles; read-heavy UA tiles keep the lines
                // they share with their neighbours in the L2
                return ld16u<NT == 1 && RSMI_UA_NT_LOADS>(ib + in_off[c] + win);
            } else {
                return ld16<true>(reinterpret_cast<const u32x4*>(ib + in_off[c]) + chl);
            }
        };
        // UA4: row c's window from its two loads
        auto window = [&](int c, u32x4& d) {
            if constexpr (UA4) {
                const uint32_t r = uint32_t(reinterpret_cast<uintptr_t>(ib + in_off[c] + win)) & 3u;
                const uint32_t e = vx[c % P];
                d = u32x4{__builtin_amdgcn_alignbyte(d[1], d[0], r), __builtin_amdgcn_alignbyte(d[2], d[1], r),
                          __builtin_amdgcn_alignbyte(d[3], d[2], r), __builtin_amdgcn_alignbyte(e, d[3], r)};
            }
        };

        u32x4 v[P];
#pragma unroll
        for (int c = 0; c < P; c++) v[c] = load_col(c);

        // gf_tile_columns (rs_gf_tile.hpp), written out: through the function the ,CRC forms of
        // (10, 4) and (16, 4), at 125 and 127 VGPRs here, spill, and the form that does not spill
        // lifts the (10, 4) encode to 5 waves per SIMD, which costs the 1 MiB blocks 5 %
        // (profiles/shared_pipeline/ab.txt).  Keep the two in step.
        uint32_t acc[MT][4], pend[MT][4];
        uint32_t tb = 0;
        asm volatile("" : "+v"(tb));
        const u32x4* tbl = s_tbl + tb;
        u32x4 Tn[5];
#pragma unroll
        for (int f = 0; f < 5; f++) Tn[f] = tbl[f];

#pragma unroll
        for (int c = 0; c < K; c++) {
            const int slot = c % P;
            u32x4 T[5];
#pragma unroll
            for (int f = 0; f < 5; f++) T[f] = Tn[f];
            window(c, v[slot]);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const uint32_t x = u4get(v[slot], w);
                const uint32_t s1 = x & 0x07070707u;
                const uint32_t s2 = (x >> 3) & 0x07070707u;
                const uint32_t s3 = (x >> 6) & 0x03030303u;
#pragma unroll
                for (int j = 0; j < MT; j++) {
                    const uint32_t p1 = __builtin_amdgcn_perm(u4get(T[1], j), u4get(T[0], j), s1);
                    const uint32_t p2 = __builtin_amdgcn_perm(u4get(T[3], j), u4get(T[2], j), s2);
                    const uint32_t p3 = __builtin_amdgcn_perm(u4get(T[4], j), u4get(T[4], j), s3);
                    uint32_t& a = acc[j][w];
                    uint32_t& q = pend[j][w];
                    if (c == 0 && K == 1) {
                        a = xor3(p1, p2, p3);
                    } else if (c == 0) {
                        a = p1 ^ p2;
                        q = p3;
                    } else if (c & 1) {
                        a = xor3(a, p1, p2);
                        a = xor3(a, p3, q);
                    } else if (c == K - 1) {
                        a = xor3(a, p1, p2);
                        a ^= p3;
                    } else {
                        a = xor3(a, p1, p2);
                        q = p3;
                    }
                }
            }
            crc_row(v[slot], c);
            if (c + P < K) v[slot] = load_col(c + P);
            if (c + 1 < K) {
#pragma unroll
                for (int f = 0; f < 5; f++) Tn[f] = tbl[(c + 1) * 5 + f];
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < MT; j++)
#pragma unroll
            for (int w = 0; w < 4; w++) asm volatile("" : "+v"(acc[j][w]));

        if constexpr (CRC) {
#pragma unroll
            for (int j = 0; j < MT; j++) crc_row(u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]}, K + j);
            uint32_t* rec = crc_rec + (uint64_t(blk) * tpb + tib) * ((NSL + 1) / 2) * kWave + lane;
#pragma unroll
            for (int i = 0; i < NSL; i += 2) rec[i / 2 * kWave] = slot[i] | (i + 1 < NSL ? slot[i + 1] << 16 : 0u);
            if constexpr (UA) {
                if (ch + 1 == cpb) {
                    uint32_t* tp = crc_tail + uint64_t(blk) * NSH;
#pragma unroll
                    for (int r = 0; r < NSH; r++) tp[r] = (tl[r / 2] >> (16 * (r & 1))) & 0xFFFFu;
                }
            }
        }
        if (UA && ch < cpb) {
#pragma unroll
            for (int j = 0; j < MT; j++) {
                const u32x4 o = u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
                st16u<NT == 1 && RSMI_UA_NT_STORES>(ob + out_off[j] + win, o);
            }
        } else if (!UA && ch < cpb) {
            store_rows_aligned<ST>(ob, out_off, ch, S, acc);
        }
    }
    launch_done<TB>(bases);
}

// ------------------------------------------------------------------ fused encode + CRC-16, matrix-core fold
// DagNode.Put's device form (node.go:358-408 with server.go:57-80's checksum of every shard):
// the encode of rs_fast_kernel (aligned layouts, encode plans: input row c is shard c, output row
// j shard K + j) with R(shard) of every row it reads and writes folded on the matrix cores
// instead of the nibble tables of the CRC variants above.  The fold is rs_crc_fold.hpp's (the fp4
// forms, the two shards to an accumulator, the unit's record and the UA correction are told
// there): a unit is kFusedUnitTiles = 4 consecutive tiles of one block, coded by the 4 waves of
// one workgroup (one tile each), and the waves' counts meet in LDS at the unit's end.
//
// UA: rows at any alignment and pitch (S >= 16; the Split layout), with the unaligned-window
// loads and stores of rs_fast_kernel's UA form.  Workgroups take XCD-contiguous units, as the UA
// coding kernels do.
// INL (small launches, a block of a few units): the block's last unit to finish combines its
// records into R(row) itself, so the call needs no second launch (below).
// TB: over a table of block bases, as rs_fast_kernel TB (a coalesced group of DagNode.Put
// callers' own page-locked buffers in one launch).
template <int K, int MT, int NT, int WPS, bool UA = false, bool INL = false, bool TB = false>
__global__ __launch_bounds__(kWG, WPS) void rs_fused_mfma_kernel(const RsPlanDev* __restrict__ plan,
                                                              const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                              uint64_t in_bs, uint64_t in_rs, uint64_t out_bs,
                                                              uint64_t out_rs, uint32_t S, uint32_t cpb, uint32_t tpb,
                                                              uint32_t upb, uint32_t nunits,
                                                              const uint32_t* __restrict__ crc_tbl,
                                                              uint8_t* __restrict__ crc_rec, uint32_t* __restrict__ ctr,
                                                              uint32_t* __restrict__ raw, Crc16Shift sh,
                                                              BasesArg<TB> bases) {
    static_assert(NT == 1 || NT == 2, "cache policy 1 or 2");
    static_assert(kFusedUnitTiles == kWG / kWave, "one tile per wave of the unit's workgroup");
    constexpr int NSH = K + MT;
    constexpr int NACC = (NSH + 1) / 2;  // two shards per accumulator
    __shared__ u32x4 s_tbl[K * kColDwords / 4];
    // INL: the combine's power tables, staged with the coding tables (off the combine's path)
    __shared__ uint32_t s_p4[INL ? kCrcP4Words : 1];
    // the tables; INL (latency-bound launches): written to LDS once the wave's first rows are in
    // flight (stage, below), else at once
    LdsTable<K * kColDwords> lt;
    lt.load(plan->tbl);
    LdsTable<INL ? kCrcP4Words : 1> lp;
    if constexpr (INL) lp.load(crc_tbl + kCrcP4Off);
    __builtin_amdgcn_sched_barrier(0);
    bool staged = false;  // wave-uniform: every wave passes the staging barrier exactly once
    auto stage = [&]() {
        if (staged) return;
        lt.store(reinterpret_cast<uint32_t*>(s_tbl));
        if constexpr (INL) lp.store(s_p4);
        __syncthreads();
        staged = true;
    };
    if constexpr (!INL) stage();

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    // a workgroup codes a unit, wave w its tile w: every wave codes one tile, as in the plain
    // encode, and the waves' counts meet in LDS at the end (below)
    const uint32_t u = fold_unit<UA>();
    if (u >= nunits) {
        stage();
        launch_done<TB>(bases);
        return;
    }
    const FoldUnit un = fold_unit_tiles(u, upb, tpb);
    const uint32_t blk = un.blk, t0 = un.t0, nt = un.nt;
    const uint8_t* ib = block_rows<TB>(bases, in, blk, in_bs);
    uint8_t* ob = block_rows<TB>(bases, out, blk, out_bs);

    constexpr int P = rows_in_flight<K, MT>();
    uint64_t in_off[K], out_off[MT];
#pragma unroll
    for (int c = 0; c < K; c++) in_off[c] = uint64_t(plan->in_row[c]) * in_rs;
#pragma unroll
    for (int j = 0; j < MT; j++) out_off[j] = uint64_t(plan->out_row[j]) * out_rs;

    CrcFold<NACC> fold;
    fold.clear();

    // the output rows of one tile: the lane's chunk ch (UA: its window at byte win)
    auto store_out = [&](uint32_t ch, uint32_t win, const uint32_t (&acc)[MT][4]) {
        if (UA && ch < cpb) {
#pragma unroll
            for (int j = 0; j < MT; j++) st16u<NT == 1>(ob + out_off[j] + win, u32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]});
        } else if (!UA && ch < cpb) {
            store_rows_aligned<NT == 1 ? 1 : 0>(ob, out_off, ch, S, acc);
        }
    };
    // INL: the output rows are stored after the unit's record is published, so the publish's
    // release waits for the record alone, not for the rows' writes (over PCIe when the call
    // codes page-locked host memory in place); one tile per wave keeps them in registers
    uint32_t dacc[INL ? MT : 1][4];
    uint32_t dch = ~0u, dwin = 0u;

    for (uint32_t i = wid; i < nt; i += kWG / kWave) {
        const LaneChunk lc = lane_chunk<UA>(t0 + i, lane, cpb, S);
        const uint32_t ch = lc.ch, chl = lc.chl, win = lc.win;
        fold.template tile_setup<UA>(t0 + i, i, lane, cpb, S, crc_tbl);
        auto load_col = [&](int c) {
            if constexpr (UA)
                return ld16u<NT == 1>(ib + in_off[c] + win);
            else
                return ld16<true>(reinterpret_cast<const u32x4*>(ib + in_off[c]) + chl);
        };

        u32x4 v[P];
#pragma unroll
        for (int c = 0; c < P; c++) v[c] = load_col(c);
        stage();
        uint32_t acc[MT][4];
        gf_tile_columns<K, MT, P>(
            s_tbl, v, acc, GfNone{},
            // form w's MFMA between the GF work of dword w and w + 1: its latency (and the
            // chain of the row's four MFMAs) hides under this wave's own VALU stream
            [&](int c, int w, const u32x4& x) {
                fold.mfma(x, c, w);
                __builtin_amdgcn_sched_barrier(0);
            },
            [&](int c, const u32x4&) { fold.anchor(c); },
            [&](int c, u32x4& x) {
                if (c + P < K) x = load_col(c + P);
            });
        // the output rows' pass before the stores; UA: every row's last window went in unshifted:
        // the output rows' counts are corrected here, the input rows' after the stores
        fold.template rows<K, MT>(acc);
        if (UA && fold.fix) fold.template fix_rows<K, MT>(acc);

        if constexpr (INL) {
#pragma unroll
            for (int j = 0; j < MT; j++)
#pragma unroll
                for (int w = 0; w < 4; w++) dacc[j][w] = acc[j][w];
            dch = ch;
            dwin = win;
        } else {
            store_out(ch, win, acc);
        }
        if (UA && fold.fix) fold.template fix_reload<K, NT == 1>(ib, in_off, win);
    }
    stage();  // waves without a tile (the unit's last tiles past the row's end)

    fold.finish(u, wid, lane, crc_rec);
    if constexpr (INL) {
        // The block's last unit to finish combines its records into R(row) (no second launch).
        // Each workgroup publishes its record (fence, then one atomic increment of the block's
        // counter); atomicInc wraps the counter back to 0 at the block's last unit, so the
        // counters are ready for the next launch without a memset.  The agent-scope release writes
        // back the XCD's L2 (the 8 XCDs' L2s are not coherent with each other): per unit of a
        // 4096-block launch that cost 25x the separate combine (8.2 ms against 0.33), so only
        // launches of a few units take this form (rsmi_crc.cpp, kFusedInlineUnits).
        // A block of one unit needs none of it: its own workgroup wrote every record.
        if (upb > 1u) {
            __threadfence();
            __syncthreads();
            __shared__ uint32_t s_last;
            if (threadIdx.x == 0) s_last = atomicInc(ctr + blk, upb - 1) == upb - 1 ? 1u : 0u;
            __syncthreads();
            if (!s_last) {
                if (dch != ~0u) store_out(dch, dwin, dacc);
                launch_done<TB>(bases);
                return;
            }
            __threadfence();
        }
        if (dch != ~0u) store_out(dch, dwin, dacc);
        __syncthreads();
        const uint8_t* rb = crc_rec + uint64_t(blk) * upb * NACC * kWave;
        for (uint32_t p = wid; p < uint32_t(NSH + 3) / 4; p += kWG / kWave)
            crc16_combine_rows(reinterpret_cast<const uint16_t*>(s_p4), rb, upb, NACC, NSH, sh,
                               raw + uint64_t(blk) * NSH, p, lane);
    }
    launch_done<TB>(bases);
}

// One kernel per (K, MT) and layout, with the cache policy of the shape (auto_cache_policy in
// rsmi_core.cpp): nontemporal stores unless the tile reads at least 4 rows per row it writes
// (the rows of the grouped tile order: store_policy, rs_plan.hpp).
constexpr int auto_nt(int K, int MT) { return K >= 4 * MT ? 2 : 1; }
constexpr int ua_nt(int K, int MT) { return RSMI_UA_NT ? RSMI_UA_NT : auto_nt(K, MT); }

}  // namespace rsmi
