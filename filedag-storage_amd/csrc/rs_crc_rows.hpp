// rs_crc_rows.hpp -- what the stand-alone CRC rows passes share (rs_crc16_kernels.hip,
// rs_crc32_kernels.hip): the work items of a launch, a row's span on the memory's 16-byte grid, the
// software-pipelined nibble pass, the matrix-core passes' operand and read-out, and the scans.  The
// CRC-specific parts (the nibble fold, the power lookups, the end shift, the staged tables) come in
// as lambdas; DESIGN.md §4.2.  The named forms of the passes (NamedRows, rows_pipe_named: the rows a
// device array names) share everything but the item loop.
//
// A launch's work item is a super-segment of one row: up to kRowsSupGroups groups of kRowsSegTiles
// consecutive 1 KiB tiles, a lane folding its 16-byte chunk of every tile.  A group's tiles fold
// relative to the group's end, a running register carries the groups (A^8192 between them), and the
// scan and the end shift run once per item.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_device.hpp"
#include "rs_plan.hpp"

namespace rsmi {

typedef int mfma_v8i __attribute__((ext_vector_type(8)));
typedef float mfma_v4f __attribute__((ext_vector_type(4)));

// one item shape for both CRCs (rs_crc32_kernels.hip asserts crc32.hpp's constants against these)
constexpr int kRowsSegTiles = kCrcSegTiles;
constexpr int kRowsSupGroups = kCrcSupGroups;

// Position of item `it` (nsup items per row): its row and its tiles.
struct RowsItem {
    uint64_t b;
    uint32_t r, t0, nt;  // block, row in block, first tile, tiles in the item
};
__device__ __forceinline__ RowsItem rows_item(uint64_t it, uint32_t nsup, uint32_t nrows, uint32_t tpb) {
    constexpr uint32_t kSup = kRowsSupGroups * kRowsSegTiles;
    RowsItem x;
    uint32_t sup;
    if (it < (uint64_t(1) << 32)) {  // 32-bit divisions (scalar), the common case
        const uint32_t i32 = uint32_t(it), rid = i32 / nsup;
        sup = i32 - rid * nsup;
        const uint32_t b = rid / nrows;
        x.b = b;
        x.r = rid - b * nrows;
    } else {
        sup = uint32_t(it % nsup);
        const uint64_t rid = it / nsup;
        x.b = rid / nrows;
        x.r = uint32_t(rid - x.b * nrows);
    }
    x.t0 = sup * kSup;
    x.nt = tpb - x.t0 < kSup ? tpb - x.t0 : kSup;
    return x;
}

// The named item source (rsmi_crc_named_rows_dev): the rows a device array names.  Item `it` is
// super-segment it % nsup of entry it / nsup, entry e block e / slots, slot e % slots.  The entry
// word is device data the host never saw: it is loaded once per item (wave-uniform, a scalar load)
// and range-checked before anything is formed from it, so an entry outside [0, n) costs that load
// and nothing else -- no address, no row load, no table lookup, no output access.  Row r < k lies in
// the data half, row k + j in the parity half; the output word is the entry's (out_n == 0:
// out[b*slots + s]) or the row's (out[b*out_n + r], what the mixed reconstruct returns).
struct NamedRows {
    struct Item {
        uint64_t b, e;
        uint32_t r, t0, nt;  // block, entry, row in block, first tile, tiles in the item
    };
    NamedRowsArgs a;
    uint32_t tpb, nsup;
    uint32_t* out;
    // item `it` (< the launch's items) -> x; false where its entry names no row
    __device__ __forceinline__ bool item(uint64_t it, Item& x) const {
        constexpr uint32_t kSup = kRowsSupGroups * kRowsSegTiles;
        uint32_t sup;
        if (it < (uint64_t(1) << 32)) {  // 32-bit divisions (scalar), the common case
            const uint32_t i32 = uint32_t(it), e = i32 / nsup;
            sup = i32 - e * nsup;
            x.e = e;
            x.b = e / a.slots;
        } else {
            sup = uint32_t(it % nsup);
            x.e = it / nsup;
            x.b = x.e / a.slots;
        }
        x.r = uint32_t(__builtin_amdgcn_readfirstlane(a.rows[x.e]));
        if (x.r >= a.n) return false;  // unsigned: the negative verdicts and anything past the last row
        x.t0 = sup * kSup;
        x.nt = tpb - x.t0 < kSup ? tpb - x.t0 : kSup;
        return true;
    }
    __device__ __forceinline__ const uint8_t* row(const Item& x) const {
        const bool d = x.r < a.k;
        return (d ? a.data : a.parity) + x.b * (d ? a.data_bs : a.parity_bs) +
               uint64_t(d ? x.r : x.r - a.k) * (d ? a.data_rs : a.parity_rs);
    }
    __device__ __forceinline__ uint32_t* word(const Item& x) const {
        return a.out_n ? out + x.b * a.out_n + x.r : out + x.e;
    }
};

// The persistent grid: a wave takes items it0, it0 + nw, ... (WG threads per workgroup).
struct RowsWave {
    uint32_t lane;
    uint64_t it0, nw;
};
template <int WG>
__device__ __forceinline__ RowsWave rows_wave() {
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    return RowsWave{threadIdx.x & (kWave - 1), uint64_t(blockIdx.x) * (WG / kWave) + wid,
                    uint64_t(gridDim.x) * (WG / kWave)};
}

// A launch's by-value shift matrix (column form, N columns), lane-distributed: lane l takes column
// l mod N.
template <int N>
__device__ __forceinline__ uint32_t lane_column(const uint32_t (&col)[N]) {
    uint32_t c = 0;
#pragma unroll
    for (int b = 0; b < N; b++) c = (threadIdx.x & uint32_t(N - 1)) == uint32_t(b) ? col[b] : c;
    return c;
}

// A row's span on the memory's 16-byte grid.  UA (rows at any byte alignment): the row is folded
// where its bytes lie, from the aligned chunk at or below its first byte (rowa = row - mis, mis =
// row & 15, wave-uniform) to the aligned chunk holding its last byte, so every load is aligned and
// no data moves between lanes; an item's value then ends mis bytes before its end on the row's own
// grid, which the caller's end shift adds (the launch's tiles per row count mis + S <= S + 15
// bytes).  Aligned rows: mis = 0 at compile time.
template <bool UA>
struct RowSpan {
    const uint8_t* rowa;
    uint32_t mis;
    uint64_t Sm, last;  // the row's end on that grid; its last chunk (S > 0)
    // the lane's chunk of tile t: unconditional, a chunk past the row's end re-reads the last one
    __device__ __forceinline__ u32x4 load(uint32_t t, uint32_t lane) const {
        const uint64_t off = (uint64_t(t) * kWave + lane) * 16;
        return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rowa + (off < last ? off : last)));
    }
};
template <bool UA>
__device__ __forceinline__ RowSpan<UA> row_span(const uint8_t* row, uint64_t S) {
    const uint32_t mis = UA ? uint32_t(__builtin_amdgcn_readfirstlane(int(reinterpret_cast<uintptr_t>(row) & 15u))) : 0u;
    return RowSpan<UA>{row - mis, mis, mis + S, (mis + S - 1) / 16 * 16};
}

// The lane's chunk of `tile` as loaded -> the row's bytes only: the bytes at or past the row's end
// (wave-uniform test: only a row's last tile) and, UA, the bytes before the row (lane 0 of tile 0)
// read as zero.  Zero bytes add nothing to R; they only move the reference point.  The empty asm
// statements keep both masks behind their branches, as they were when each kernel had them inline:
// without them the compiler (ROCm 7's clang, -O3) turns the masks of this shared function into
// selects that every tile pays for -- rs_crc32_rows_pipe_kernel<true> then has 178 v_cndmask_b32
// and 7 s_and_saveexec_b64 against 146 and 15 with them (and in the parent).  To see whether they
// are still needed, compile rs_crc32_kernels.hip without them and count those two opcodes
// (profiles/crc_rows/README.md).
template <bool UA>
__device__ __forceinline__ void mask_row_ends(u32x4& v, uint32_t tile, uint32_t lane, const RowSpan<UA>& span) {
    if ((uint64_t(tile) + 1) * (kWave * 16) > span.Sm) {
        asm volatile("");
        const int64_t valid = int64_t(span.Sm) - int64_t((uint64_t(tile) * kWave + lane) * 16);
#pragma unroll
        for (int w = 0; w < 4; w++) v[w] &= bytes_mask(valid - 4 * w);
    }
    if (UA && tile == 0 && span.mis != 0u && lane == 0) {
        asm volatile("");
#pragma unroll
        for (int w = 0; w < 4; w++) v[w] &= ~bytes_mask(int(span.mis) - 4 * w);  // dword w's leading bytes dropped
    }
}

// The nibble rows pass, software-pipelined.  A wave works in units of half a group (4 tiles) and
// issues the loads of its next unit (of this item or its next one) before it folds the current one
// (two register sets of 16 VGPRs, the loop unrolled by two), so its own fold covers the next unit's
// memory latency instead of only the other waves on the SIMD; half-group units keep the kernels
// under 64 VGPRs (8 waves per SIMD).  Loads are unconditional -- chunks past the row's end read the
// row's last chunk and are masked to zero in the fold, and the prefetch past the wave's last unit
// re-reads that unit -- so no load sits behind a branch and the compiler's vmcnt waits count only
// the older set.
//   fold(i, v)            R(chunk v) by tile i's tables of the group, relative to the group's end
//   step_group(acc)       A^8192(acc): earlier groups move 8 KiB further from the end
//   item_out(acc, x, mis) the lanes' values of item x -> the row's word
// wv: the kernel's rows_wave<kWG>(), so the lambdas and the driver see one lane index.
template <bool UA, class Fold, class StepGroup, class ItemOut>
__device__ __forceinline__ void rows_pipe(const RowsWave& wv, const uint8_t* __restrict__ base, uint64_t bstride,
                                          uint64_t rpitch, uint32_t nrows, uint64_t S, uint32_t tpb, uint32_t nsup,
                                          uint64_t nitems, Fold&& fold, StepGroup&& step_group, ItemOut&& item_out) {
    constexpr int kU = kRowsSegTiles / 2;  // tiles per unit
    const uint32_t lane = wv.lane;
    // a unit of work: tiles t0 + 4 h .. t0 + 4 h + 3 of item it (its position computed once per item)
    struct Unit {
        uint64_t it;
        RowsItem x;
        uint32_t h;
    };
    auto at = [&](uint64_t it) -> Unit { return Unit{it, rows_item(it, nsup, nrows, tpb), 0}; };
    auto next = [&](const Unit& u) -> Unit {
        if ((u.h + 1) * kU < u.x.nt) return Unit{u.it, u.x, u.h + 1};
        return at(u.it + wv.nw);
    };
    auto span = [&](const RowsItem& x) { return row_span<UA>(base + x.b * bstride + uint64_t(x.r) * rpitch, S); };
    auto issue = [&](const Unit& u, u32x4(&v)[kU]) {
        const RowSpan<UA> sp = span(u.x);
#pragma unroll
        for (int i = 0; i < kU; i++) v[i] = sp.load(u.x.t0 + u.h * kU + i, lane);
    };
    uint32_t acc = 0, gs = 0;
    auto finish = [&](const Unit& u, u32x4(&v)[kU]) {
        const RowsItem& x = u.x;
        const uint32_t u0 = u.h * kU, t0 = x.t0 + u0;
        const uint32_t nt = x.nt - u0 < uint32_t(kU) ? x.nt - u0 : uint32_t(kU);
        const RowSpan<UA> sp = span(x);
#pragma unroll
        for (int i = 0; i < kU; i++) {
            if (uint32_t(i) < nt) {
                mask_row_ends<UA>(v[i], t0 + i, lane, sp);
                gs ^= fold(kU * (u.h & 1) + i, v[i]);  // the table sets of this half of the group
            }
        }
        const bool item_end = u0 + kU >= x.nt;
        if ((u.h & 1) || item_end) {  // the group is complete
            acc = step_group(acc) ^ gs;
            gs = 0;
        }
        if (item_end) {
            item_out(acc, x, sp.mis);
            acc = 0;
        }
    };
    if (wv.it0 >= nitems) return;
    Unit cur = at(wv.it0);
    u32x4 va[kU], vb[kU];
    issue(cur, va);
    for (;;) {
        Unit nx = next(cur);
        bool more = nx.it < nitems;
        issue(more ? nx : cur, vb);
        finish(cur, va);
        if (!more) break;
        cur = nx;
        nx = next(cur);
        more = nx.it < nitems;
        issue(more ? nx : cur, va);
        finish(cur, vb);
        if (!more) break;
        cur = nx;
    }
}

// rows_pipe over the named item source.  The regular passes keep rows_pipe as it is: routing them
// through a source object changes their register allocation (tools/isa_diff.py), so
// the named kernels have this loop of their own.  It differs in where a unit comes from: at() walks
// to the wave's next item whose entry names a row, or to the end, before anything is issued for it,
// so the prefetch only ever touches a named row (past the wave's last named unit it re-reads that
// unit), and a wave none of whose items names a row issues no row load at all.
//   item_out(acc, x, mis) the lanes' values of item x -> src.word(x)
template <bool UA, class Fold, class StepGroup, class ItemOut>
__device__ __forceinline__ void rows_pipe_named(const RowsWave& wv, const NamedRows& src, uint64_t S, uint64_t nitems,
                                                Fold&& fold, StepGroup&& step_group, ItemOut&& item_out) {
    constexpr int kU = kRowsSegTiles / 2;  // tiles per unit
    const uint32_t lane = wv.lane;
    struct Unit {
        uint64_t it;  // >= nitems: the end, x unset
        NamedRows::Item x;
        uint32_t h;
    };
    auto at = [&](uint64_t it) -> Unit {
        Unit u;
        u.h = 0;
        while (it < nitems && !src.item(it, u.x)) it += wv.nw;
        u.it = it;
        return u;
    };
    auto next = [&](const Unit& u) -> Unit {
        if ((u.h + 1) * kU < u.x.nt) return Unit{u.it, u.x, u.h + 1};
        return at(u.it + wv.nw);
    };
    auto issue = [&](const Unit& u, u32x4(&v)[kU]) {
        const RowSpan<UA> sp = row_span<UA>(src.row(u.x), S);
#pragma unroll
        for (int i = 0; i < kU; i++) v[i] = sp.load(u.x.t0 + u.h * kU + i, lane);
    };
    uint32_t acc = 0, gs = 0;
    auto finish = [&](const Unit& u, u32x4(&v)[kU]) {
        const NamedRows::Item& x = u.x;
        const uint32_t u0 = u.h * kU, t0 = x.t0 + u0;
        const uint32_t nt = x.nt - u0 < uint32_t(kU) ? x.nt - u0 : uint32_t(kU);
        const RowSpan<UA> sp = row_span<UA>(src.row(x), S);
#pragma unroll
        for (int i = 0; i < kU; i++) {
            if (uint32_t(i) < nt) {
                mask_row_ends<UA>(v[i], t0 + i, lane, sp);
                gs ^= fold(kU * (u.h & 1) + i, v[i]);
            }
        }
        const bool item_end = u0 + kU >= x.nt;
        if ((u.h & 1) || item_end) {
            acc = step_group(acc) ^ gs;
            gs = 0;
        }
        if (item_end) {
            item_out(acc, x, sp.mis);
            acc = 0;
        }
    };
    Unit cur = at(wv.it0);
    if (cur.it >= nitems) return;
    u32x4 va[kU], vb[kU];
    issue(cur, va);
    for (;;) {
        Unit nx = next(cur);
        bool more = nx.it < nitems;
        issue(more ? nx : cur, vb);
        finish(cur, va);
        if (!more) break;
        cur = nx;
        nx = next(cur);
        more = nx.it < nitems;
        issue(more ? nx : cur, va);
        finish(cur, vb);
        if (!more) break;
        cur = nx;
    }
}

// The matrix-core passes' B operand: bit plane q of a chunk, one data bit per fp4 nibble (d &
// 0x11.., 0x22.., 0x44.., (d >> 1) & 0x44..; bit 3 of a nibble is the e2m1 sign).
__device__ __forceinline__ mfma_v8i fp4_bit_plane(const u32x4& d, int q) {
    mfma_v8i bd;
#pragma unroll
    for (int w = 0; w < 4; w++) bd[w] = int(q < 3 ? d[w] & (0x11111111u << q) : (d[w] >> 1) & 0x44444444u);
    bd[4] = bd[5] = bd[6] = bd[7] = 0;
    return bd;
}

// ... and their read-out: the parity of an accumulator quad's 16 x 16 counts -> class m's 16-bit
// value in lane m (< 16).  Bit n of class m is bit 16 (n >> 2) + m of ballot n & 3.
__device__ __forceinline__ uint32_t ballot_class_value(const mfma_v4f& c, uint32_t m) {
    uint32_t Y = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t bl = __builtin_amdgcn_ballot_w64((int(c[i]) & 1) != 0);
        const uint32_t lo = uint32_t(bl) >> m, hi = uint32_t(bl >> 32) >> m;
        Y |= ((lo & 0x10001u) | ((hi & 0x10001u) << 8)) << i;  // n = i, 4 + i (bit 16), 8 + i, 12 + i (bit 24)
    }
    return (Y & 0x0F0Fu) | ((Y >> 12) & 0xF0F0u);
}

// A Hillis-Steele scan over 2^LEVELS neighbouring lanes (idx: the lane's index among them), each
// lane's value relative to the end of its own 16-byte chunk: level j adds the value 2^j lanes
// down, moved by pow(j, .) = A^(16 * 2^j), so the last lane ends with the sum relative to its end.
// LEVELS = 6: the chunks of a tile (lane 63); 4: the matrix-core passes' 16 classes (lane 15).
template <int LEVELS, class Pow>
__device__ __forceinline__ uint32_t rows_scan(uint32_t acc, uint32_t idx, Pow&& pow) {
#pragma unroll
    for (int j = 0; j < LEVELS; j++) {
        const uint32_t w = pow(j, acc);
        const uint32_t t = __shfl_up(w, 1u << j);
        if (idx >= (1u << j)) acc ^= t;
    }
    return acc;
}

}  // namespace rsmi
