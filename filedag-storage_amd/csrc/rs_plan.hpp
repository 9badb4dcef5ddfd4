// rs_plan.hpp -- device-side coding plan shared by the host launcher and the kernels.
#pragma once
#include <cstdint>
#include <type_traits>

namespace rsmi {

constexpr int kWave = 64;       // CDNA wavefront
constexpr int kWG = 256;        // threads per workgroup (4 waves)
constexpr int kFastWG = kWG;    // ... of the coding and verify kernels (one tile per wave)
constexpr int kMaxK = 256;      // k + m <= 256 (erasure.go:22)
constexpr int kMaxMT = 4;       // outputs per launch tile
constexpr int kColDwords = 20;  // per input column: 5 table fields x 4 outputs
// The fast kernels' register budget: at least this many waves fit a SIMD (128 VGPRs).  A floor, not
// a cap: a kernel that needs fewer registers runs at more waves (up to 8; DESIGN.md §4.1 lists the
// aligned kernels) unless its shape has a cap of its own (waves_cap).
constexpr int kMinWavesPerSimd = 4;
// unaligned-window tiles: dword-aligned loads funnel-shifted for read-heavy tiles (1, the
// default), for every UA tile (2), or byte-aligned 16-byte loads (0)
#ifndef RSMI_UA_DWORD_LOADS
#define RSMI_UA_DWORD_LOADS 1
#endif
// A/B knobs for the unaligned-window coding kernels (tools/ua_ab.sh, Split layout): the cache
// policy of their instantiations (0: the shape's own, auto_nt; 1 or 2: that one for every UA
// shape), and whether a write-heavy UA tile's stores are nontemporal (1) or default (0)
#ifndef RSMI_UA_NT
#define RSMI_UA_NT 0
#endif
#ifndef RSMI_UA_NT_STORES
#define RSMI_UA_NT_STORES 1
#endif
// ... and whether its loads are nontemporal (1) or default (0)
#ifndef RSMI_UA_NT_LOADS
#define RSMI_UA_NT_LOADS 1
#endif

#if defined(__HIPCC__)
#define RSMI_HOST_DEVICE __host__ __device__
#else
#define RSMI_HOST_DEVICE
#endif
// Workgroup -> tile group of the coding kernels (launch geometry).  The dispatcher
// deals workgroups round-robin over the 8 XCDs, so workgroup wg lands on XCD wg & 7 (observed,
// not promised: the mapping is for speed only and a bijection of [0, grid) whatever the placement).
// The first head workgroups (head a multiple of 8, head <= grid) are renumbered so that each XCD
// sweeps one contiguous range of head / 8 tile groups; the rest keep the plain order, which leaves
// the launch's tail to the dispatcher's balancing.  head = 0: the plain order.
RSMI_HOST_DEVICE inline uint32_t tile_group(uint32_t wg, uint32_t grid, uint32_t head) {
    (void)grid;
    return wg < head ? (wg & 7u) * (head >> 3) + (wg >> 3) : wg;
}
// The share of an aligned launch's workgroups that is grouped: num / den of the grid for the
// shapes of the table below, none for every other.  Of 1, 15/16, 7/8 and 3/4 the whole grid was
// best on the one shape that gains (profiles/xcd_tail/ab.txt).
struct TileGroupShare {
    uint32_t num, den;
};
constexpr TileGroupShare kTileGroupShare = {1, 1};
// Per tile shape (K, MT) and row size S, beside auto_cache_policy (rsmi_core.cpp): measured on the
// BASELINE shapes.  RS(10,4) rows of 256 KiB blocks (S = 26 215, 26 tiles a row) gain about 1.2 %,
// encode (MT = 4) and one-row reconstruct (MT = 1) alike; the same K with 1 MiB blocks
// (S = 104 858) loses 1.3 %, RS(4,2), RS(16,4) and RS(2,1) lose 0.4-3.5 % at every share.  Shapes
// that were not measured keep the plain order.
// The aligned kernels of the other (K, MT) leave the mapping out at compile time (rs_fast_kernel),
// so their code stays what it was.
constexpr bool tile_group_shape(int K, int MT) { return K == 10 && (MT == 4 || MT == 1); }
constexpr uint32_t kGroupedRowMax = 32768u;  // ... with rows of at most this many bytes
inline TileGroupShare tile_group_share(int K, int MT, uint32_t S) {
    if (tile_group_shape(K, MT) && S <= kGroupedRowMax) return kTileGroupShare;
    return {0, 1};
}
// How the plain aligned coding kernel (rs_fast_kernel without UA, CRC or TB) stores its output
// rows on the rows that take the grouped order, beside the cache policy NT (auto_cache_policy,
// rsmi_core.cpp), which keeps naming the loads and the launch label:
//   0  plain stores            1  nontemporal stores
//   n >= 2  nontemporal stores, but the last n - 1 output rows plain
//   -1  write-through stores (sc0 sc1: the line leaves the L2 with the store)
// Measured under the grouped order on the two shapes that take it: the RS(10,4)
// encode with its last parity row stored plain is 3.9 % faster than with all four nontemporal (all
// plain -4.6 %, two plain rows slow the launch that follows; profiles/store_path/ab.txt); the
// one-row reconstruct stores its row write-through, which takes 9 us off its 193 (nontemporal
// -5.8 %; write-through for the last 512 / 1024 / 2048 / 3072 workgroups of each XCD's range of
// 3328 gains the less the shorter the tail, and the encode's plain row written through gains
// nothing; profiles/rec_inflight/ab.txt).  Every other shape, and longer rows of these, keep what
// the cache policy says and the kernel they had (FastKernelTable::fn).
constexpr int kStoreWriteThrough = -1;
constexpr int store_policy(int K, int MT, int NT) {
    if (K == 10 && MT == 4) return 2;
    if (K == 10 && MT == 1) return kStoreWriteThrough;
    return NT == 1 ? 1 : 0;
}
// The most waves per SIMD that kernel runs at on those rows (0: whatever its registers allow,
// kMinWavesPerSimd being the floor).  The one-row reconstruct needs 64 VGPRs, which alone would
// put 8 waves on a SIMD, each with all 10 rows in flight: 320 KiB requested per CU.  Capped at 4
// (160 KiB) the headline step gains 0.7 % (caps 6 / 5 / 3 / 2: 0.0 / +0.4 / +0.5 / -2.9 %; 8 or
// 6 rows in flight instead of 10 lose 0.3-0.6 % uncapped and 0.3-0.5 % under the cap with a
// write-through tail; profiles/rec_inflight/ab.txt).
constexpr int waves_cap(int K, int MT) { return K == 10 && MT == 1 ? 4 : 0; }
// a shape whose kernel on those rows differs from its cache policy's has one more instantiation
// for them (FastKernelTable::fn_sp)
constexpr bool grouped_kernel_shape(int K, int MT, int NT) {
    return tile_group_shape(K, MT) && (store_policy(K, MT, NT) != (NT == 1 ? 1 : 0) || waves_cap(K, MT) != 0);
}
// head of a coding launch (launch_plan) of grid workgroups.  Unaligned-window layouts (ua): the
// whole grid when it is a multiple of 8, else none (neighbouring tiles share cache lines there,
// DESIGN.md §3).  A grid capped by waves_per_cu (strided: each wave loops over further tiles)
// keeps the plain order.
inline uint32_t launch_head(uint32_t grid, int K, int MT, uint32_t S, bool ua, bool strided) {
    if (ua) return (grid & 7u) == 0u ? grid : 0u;
    if (strided) return 0u;
    const TileGroupShare s = tile_group_share(K, MT, S);
    return uint32_t(uint64_t(grid) * s.num / s.den) & ~7u;
}

// One launch tile: MT (<= 4) output rows computed from K input rows.
// tbl[c*20 + f*4 + j] = field-f product word for coefficient coef[j][c] (gf256.hpp
// perm_tables); padded outputs (j >= MT) have all-zero tables.
struct RsPlanDev {
    uint32_t k, mt, pad0[14];
    uint32_t in_row[kMaxK];
    uint32_t out_row[kMaxMT], pad1[12];
    uint32_t tbl[kMaxK * kColDwords];
};

// A coalesced group of blocks that each lie in their own caller's page-locked buffer (concurrent
// DagNode.Put / Get callers, rsmi_coalesce.cpp), coded by one launch: block b's rows start at
// b[b], and the launch's in / out pointers are offsets from there.  Passed by value, so the
// table travels in the kernel arguments (one scalar load per wave, no copy to the device); a
// group of more blocks takes several launches.  The kernels' table-less instantiations take
// NoBases in its place, an unused empty argument that leaves their code unchanged.
// done_flag (the fused encode + CRC-16 with its combine inside, rs_fused_mfma_kernel TB INL): the
// launch's workgroups count themselves in done_ctr as they finish, and the last one releases
// done_seq into the page-locked done_flag, so the caller sees the group's end by polling it
// instead of synchronising the stream (rsmi_coalesce.cpp)
constexpr int kTableBlocks = 64;
struct BlockBases {
    uint64_t b[kTableBlocks];
    uint32_t* done_ctr = nullptr;
    uint32_t* done_flag = nullptr;
    uint32_t done_seq = 0, done_pad = 0;
};
struct NoBases {};
template <bool TB>
using BasesArg = std::conditional_t<TB, BlockBases, NoBases>;

// Instantiated fast kernels, one per (K, MT) with the shape's cache policy (null when K has no
// instantiation): aligned layouts, unaligned-window layouts, and both with the datanode CRC-16
// of every row fused in (encode plans).
struct FastKernelTable {
    void* fn[17][kMaxMT + 1];
    void* fn_sp[17][kMaxMT + 1];  // aligned rows up to kGroupedRowMax of a grouped_kernel_shape (null: fn)
    void* ua[17][kMaxMT + 1];
    void* crc[17][kMaxMT + 1];
    void* ua_crc[17][kMaxMT + 1];
    void* fused[17][kMaxMT + 1];     // aligned, the CRC-16 folded on the matrix cores (rs_fused_mfma_kernel)
    void* fused_ua[17][kMaxMT + 1];  // the same on unaligned-window layouts (S >= 16)
    void* fused_inl[17][kMaxMT + 1];     // fused with the combine in the kernel (small launches;
    void* fused_ua_inl[17][kMaxMT + 1];  // null: the two-launch form)
    // the same over a table of block bases (BlockBases; rs_kernels_tb.hip, for the shapes of the
    // BASELINE configs; null: one launch per block)
    void* fn_tb[17][kMaxMT + 1];
    void* ua_tb[17][kMaxMT + 1];
    void* fused_tb[17][kMaxMT + 1];
    void* fused_ua_tb[17][kMaxMT + 1];
    void* fused_inl_tb[17][kMaxMT + 1];
    void* fused_ua_inl_tb[17][kMaxMT + 1];
};
void fill_table_kernels(FastKernelTable& t);  // rs_kernels_tb.hip

const FastKernelTable& fast_kernels();
void* generic_kernel();
void* repitch_kernel();

// The tile kernels of the calls over stored stripes, one table per call: a kernel per (K, MT), on
// aligned and on unaligned-window layouts (null where the shape has none).  The calls' own names
// for it follow.
struct StripeKernelTable {
    void* fn[17][kMaxMT + 1];
    void* ua[17][kMaxMT + 1];
};

// Encoder.Verify (rs_verify_kernels.hip): rs_verify_kernel per (K, MT), aligned and
// unaligned-window layouts (null when K has no instantiation), and the compare of the fallback
// (encode into scratch, then rs_compare_rows_kernel)
using VerifyKernelTable = StripeKernelTable;
const VerifyKernelTable& verify_kernels();
void* compare_rows_kernel();

// rsmi_scrub (rs_scrub_kernels.hip): rs_scrub_mfma_kernel per (K, MT), the shapes of
// rs_verify_kernel, aligned and unaligned-window layouts (null: Verify and the CRC-16 rows pass,
// one after the other)
using ScrubKernelTable = StripeKernelTable;
const ScrubKernelTable& scrub_kernels();

// rsmi_locate (rs_locate_kernels.hip): rs_locate_kernel per (K, MT = m), m = 2..4, aligned and
// unaligned-window layouts (null when the shape has none), the verdict kernel that follows every
// locate launch, and the byte-granular kernel of the fallback
using LocateKernelTable = StripeKernelTable;
const LocateKernelTable& locate_kernels();
void* locate_verdict_kernel();
void* locate_rows_kernel();

// rsmi_heal (rs_heal_kernels.hip): rs_heal_kernel per (K, MT = m), the shapes of rs_locate_kernel,
// and the byte-granular kernel of the fallback
using HealKernelTable = StripeKernelTable;
const HealKernelTable& heal_kernels();
void* heal_rows_kernel();

// rsmi_locate_pair (rs_pair_kernels.hip): rs_locate_pair_kernel per (K, MT = m), the K of
// rs_locate_kernel with m = 3..4 (m <= 2 names no pair), aligned and unaligned-window layouts; the
// verdict kernel that ends every pair call, and the byte-granular kernel of the fallback
using PairKernelTable = StripeKernelTable;
const PairKernelTable& pair_kernels();
void* pair_verdict_kernel();
void* pair_rows_kernel();
// The pair tests of a tile kernel (rs_pair_tile.hpp), in the order of plan "P" (rsmi_pair.cpp):
// per data shard c the test of {c, parity 0}, then of {c, d} for d = c + 1 .. K - 1; each takes
// m - 2 coefficients, four to a column block of the plan.
constexpr int pair_tests(int K) { return K + K * (K - 1) / 2; }
constexpr int pair_blocks(int K, int MT) { return (pair_tests(K) * (MT - 2) + 3) / 4; }
// bit p of a block's pair words: the lexicographic index of (x, y), x < y < n
constexpr int pair_bit(int n, int x, int y) { return x * n - x * (x + 1) / 2 + (y - x - 1); }
constexpr int pair_words(int n) { return (n * (n - 1) / 2 + 31) / 32; }

// rsmi_heal_pair (rs_heal_pair_kernels.hip): rs_heal_pair_kernel per (K, MT = m), the shapes of
// rs_locate_pair_kernel, and the byte-granular kernel of the fallback.  Plan "H" (rsmi_heal_pair.cpp)
// has one column per explanation of a block: the C(n, 2) pairs {x, y} at pair_bit(n, x, y), then the n
// single shards.  Column e carries D's four coefficients in its output slots (D[0][l0], D[0][l1],
// D[1][l0], D[1][l1]) and l0 | l1 << 8 in in_row[e].
using HealPairKernelTable = StripeKernelTable;
const HealPairKernelTable& heal_pair_kernels();
void* heal_pair_rows_kernel();
constexpr int heal_pair_entries(int n) { return n * (n - 1) / 2 + n; }
constexpr int heal_pair_entry(int n, int x, int y) { return y < 0 ? n * (n - 1) / 2 + x : pair_bit(n, x, y); }

// rsmi_reconstruct_mixed_batch_* (rs_mixed_kernels.hip): rs_mixed_kernel per (K, MT), the K of
// the verify kernels, aligned and unaligned-window layouts (null when the shape has none).  A
// launch codes the tiles of one class of blocks: entry e of its list names the block and, through
// the launch's array of plan pointers, the one-tile plan (MT output rows) of that block's pattern.
struct MixedEntry {
    uint32_t blk, pat;
};
struct MixedKernelTable {
    void* fn[17][kMaxMT + 1];
    void* ua[17][kMaxMT + 1];
};
const MixedKernelTable& mixed_kernels();
// rsmi_reconstruct_mixed_batch_*_verify (rs_mixed_fused_kernels.hip): rs_mixed_fused_kernel per
// (K, MT), the shapes of rs_mixed_kernel, aligned and unaligned-window layouts (null: the class
// takes rs_mixed_kernel and the named rows pass), and the kernel that moves a class's combined
// checksums from (entry, slot) to (block, row)
struct MixedFusedKernelTable {
    void* fn[17][kMaxMT + 1];
    void* ua[17][kMaxMT + 1];
};
const MixedFusedKernelTable& mixed_fused_kernels();
void* mixed_scatter_kernel();

// rsmi_encode_ragged_batch_* (rs_ragged_kernels.hip): rs_ragged_kernel per (K, MT), the K of the
// coding kernels, aligned and unaligned-window blocks.  A launch codes the blocks of one class with
// one tile of the encode plan; every block has its own shard size and its own rows.  Workgroup e
// takes unit e: up to kRaggedUnitTiles consecutive 1 KiB-per-row tiles of one block, a tile per
// wave.  The unit names its block's descriptor, which holds what a uniform launch takes as kernel
// arguments: the block's first data and parity row, their row strides, S and its 16-byte chunks.
constexpr int kRaggedUnitTiles = kFastWG / kWave;
struct RaggedUnit {
    uint32_t blk, tile;  // index into the launch's descriptors; the unit's first tile
};
struct alignas(16) RaggedBlockDev {
    uint64_t data, parity;        // device addresses of data row 0 and parity row 0
    uint64_t data_rs, parity_rs;  // row strides in bytes
    uint32_t S, cpb;
    uint32_t pad[6];
};
static_assert(sizeof(RaggedUnit) == 8 && sizeof(RaggedBlockDev) == 64, "what the kernels' scalar loads read");
// the K with an rs_ragged_kernel (blocks of any other shape take launch_plan, one by one)
constexpr bool ragged_shape(int K) { return K >= 1 && (K <= 6 || K == 8 || K == 10 || K == 12 || K == 16); }
using RaggedKernelTable = StripeKernelTable;
const RaggedKernelTable& ragged_kernels();

// CRC-16 of shard rows (crc16.hpp): the device table buffer holds P[15][2][256] (the powers
// A^(2^i), byte-sliced) and N[32][16] (u16); a wave folds kCrcSegTiles 1 KiB tiles of one row
// with one N lookup per nibble (16-entry tables: each wave-wide lookup touches 8 distinct
// banks, so it never conflicts).
constexpr int kCrcSegTiles = 8;   // tiles a wave loads at once (one group)
constexpr int kCrcSupGroups = 4;  // groups per item: the scan and the end shift run once per 32 tiles
constexpr int kCrcPWords = 15 * 2 * 256 / 2;
constexpr int kCrcNWords = 32 * 16 / 2;
constexpr int kCrcQWords = 16 * 2 * 4 * 16 / 2;  // quad-relative nibble tables (fused kernels)
constexpr int kCrcQOff = kCrcPWords + kCrcNWords;
constexpr int kCrcGWords = 8 * 32 * 16 / 2;     // tile-set nibble tables (rows pass)
constexpr int kCrcGOff = kCrcQOff + kCrcQWords;
constexpr int kCrcP4Words = 15 * 4 * 16 / 2;     // nibble-sliced powers (rows pass)
constexpr int kCrcP4Off = kCrcGOff + kCrcGWords;
constexpr int kCrcMWWords = 8 * 4 * 64 * 4;       // fp4 weight operands (matrix-core rows pass)
constexpr int kCrcMWOff = kCrcP4Off + kCrcP4Words;
constexpr int kCrcFWWords = 4 * 4 * 64 * 4;       // fp4 weights of the fused encode + CRC kernel
constexpr int kCrcFWOff = kCrcMWOff + kCrcMWWords;
constexpr int kCrcTableWords = kCrcFWOff + kCrcFWWords;
// launches of at most this many units combine their records in the fused kernel (one launch
// instead of two; larger ones keep the separate combine, see rs_fused_mfma_kernel INL)
#ifndef RSMI_FUSED_INLINE_UNITS
#define RSMI_FUSED_INLINE_UNITS 64
#endif
constexpr uint32_t kFusedInlineUnits = RSMI_FUSED_INLINE_UNITS;
// fused encode + CRC on the matrix cores: a unit is 4 tiles, one per wave of its workgroup (the
// two-shard accumulators stay exact up to 4 tiles)
constexpr int kFusedUnitTiles = kWG / kWave;
constexpr int kFusedUnitLog = 2;
static_assert(kFusedUnitTiles == 1 << kFusedUnitLog, "a unit of 4 tiles");
#ifndef RSMI_FUSED_WPS
#define RSMI_FUSED_WPS 3
#endif
constexpr int kFusedWavesPerSimd = RSMI_FUSED_WPS;  // its register budget: 168 VGPRs (the row accumulators)
// CRC-32 (crc32.hpp) device tables, u32 words: NT[8][32][16] | SN[6][8][16] (both staged in
// LDS, 19 KiB) | SC[24][32] (column form, read with scalar loads)
constexpr int kCrc32FoldWords = 8 * 32 * 16;
constexpr int kCrc32PowWords = 8 * 16;  // one nibble-sliced power
constexpr int kCrc32LdsWords = kCrc32FoldWords + 7 * kCrc32PowWords;  // NT | SN[6] | SG
#ifndef RSMI_CRC32_FOLD_DEFAULT
#define RSMI_CRC32_FOLD_DEFAULT 1
#endif
constexpr int kCrc32MWOff = kCrc32LdsWords + 24 * 32;       // MW[8][4][2][64][4] (matrix-core pass)
constexpr int kCrc32MWWords = 8 * 4 * 2 * 64 * 4;
// RSMI_CRC32_MFMA_HALF 1: the matrix-core CRC-32 pass reads the parity per half group (4 tiles,
// weights MW[4..7], 32 KiB, the halves joined by A^4096), so 4-wave workgroups stage half the
// weights; 0: per 8-tile group, all 64 KiB staged by 8-wave workgroups
#ifndef RSMI_CRC32_MFMA_HALF
#define RSMI_CRC32_MFMA_HALF 0
#endif
constexpr bool kCrc32MfmaHalf = RSMI_CRC32_MFMA_HALF;
constexpr int kCrc32MfmaWG = kCrc32MfmaHalf ? 256 : 512;
constexpr int kCrc32MfmaTiles = kCrc32MfmaHalf ? 4 : 8;  // tiles per parity read-out
constexpr int kCrc32SG4Off = kCrc32MWOff + kCrc32MWWords;  // SG4[8][16]: A^4096, nibble-sliced
constexpr int kCrc32TableWords = kCrc32SG4Off + 8 * 16;
// per-launch shift to the row's end, column form (crc32.hpp), passed by value: A^(S mod 8192),
// the end of an inner segment moved over whatever of the row follows whole segments
struct Crc32Shift {
    uint32_t col[32];
};
// the CRC-16 rows pass's per-launch shift, column form: A^E with E = (S - end of the row's last
// item) mod 32767, col[b] = A^E(1 << b)
struct Crc16Shift {
    uint32_t col[16];
};
void* crc16_rows_kernel(bool aligned);
void* crc16_rows_mfma_kernel(bool aligned);  // the fold on the matrix cores (unaligned rows: folded on the memory's 16-byte grid)
void* crc16_combine_kernel(int ns2);  // ns2 = record dwords per lane (rows / 8, rounded up)
void* crc16_combine_mfma_kernel();    // records of rs_fused_mfma_kernel
void* crc32_rows_kernel(bool aligned);
void* crc32_rows_mfma_kernel(bool aligned);  // the fold on the matrix cores (512-thread workgroups)
// The named rows passes (rs_crc_rows.hpp NamedRows): the rows of a stripe's two halves that a
// device array names.  rows[b*slots + s] in [0, n) names row r of block b (r < k at data + b*data_bs
// + r*data_rs, else parity + b*parity_bs + (r-k)*parity_rs); out_n == 0: the entry's checksum goes
// to out[b*slots + s], otherwise to out[b*out_n + r].
struct NamedRowsArgs {
    const int32_t* rows;
    const uint8_t* data;
    uint64_t data_bs, data_rs;
    const uint8_t* parity;
    uint64_t parity_bs, parity_rs;
    uint32_t k, n, slots, out_n;
};
void* crc16_named_kernel(bool mfma, bool aligned);
void* crc32_named_kernel(bool mfma, bool aligned);  // mfma: 512-thread workgroups

}  // namespace rsmi
