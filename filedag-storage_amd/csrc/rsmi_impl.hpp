// rsmi_impl.hpp -- internals shared by the C-ABI implementation files (include/rsmi.h):
//   rsmi_core.cpp      contexts, coding plans, kernel dispatch, options, device-resident calls
//   rsmi_host.cpp      host-memory calls: zero-copy single kernel, copy-engine pipeline
//   rsmi_crc.cpp       datanode CRC-16 on the GPU (separate pass and fused into the encode); the rows
//                      passes over named rows (rsmi_crc_named_rows_dev)
//   rsmi_coalesce.cpp  group commit of concurrent single-block calls
//   rsmi_verify.cpp    Encoder.Verify: stored parity checked against the data rows; what the six
//                      stripe calls share: the rows' layout test, the tile launch and its label,
//                      the scratch-encode fallback, the host paths with their results buffer and
//                      write-back leg, the verdict calls' host entries, the entry points' checks
//   rsmi_locate.cpp    rsmi_locate: the shard that breaks a stripe, from Verify's syndromes
//   rsmi_heal.cpp      rsmi_heal: locate, then the named shard rewritten on the same stream
//   rsmi_mixed.cpp     rsmi_reconstruct_mixed_*: a batch whose blocks each have their own erasure pattern
//   rsmi_pair.cpp      rsmi_locate_pair: locate, then the pair of shards that explains an UNKNOWN block
//   rsmi_heal_pair.cpp rsmi_heal_pair: locate pair, then the one or two named shards rewritten on the same stream
//   rsmi_scrub.cpp     rsmi_scrub: Verify's flags and every shard's CRC-16 from one read of the rows
//   rsmi_ragged.cpp    rsmi_encode_ragged_*: the encode of a batch whose blocks each have their own size
// No CPU compute path anywhere: every byte of parity, reconstructed data or CRC and every verify
// flag comes out of the HIP kernels (rs_kernels.hip, rs_kernels_tb.hip, rs_crc16_kernels.hip, rs_crc32_kernels.hip,
// rs_verify_kernels.hip, rs_locate_kernels.hip, rs_heal_kernels.hip, rs_mixed_kernels.hip,
// rs_mixed_fused_kernels.hip, rs_pair_kernels.hip, rs_heal_pair_kernels.hip, rs_scrub_kernels.hip, rs_ragged_kernels.hip).  Kernel headers: rs_gf_tile.hpp (the GF(2^8) tile pipeline), rs_verify_tile.hpp
// (the stripe checks' tile step), rs_crc_rows.hpp (what the CRC-16 and CRC-32 rows passes share),
// rs_crc_fold.hpp (the CRC-16 fold on the matrix cores of the fused encode, the scrub and the mixed verify).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rsmi.h"
#include "crc16.hpp"
#include "crc32.hpp"
#include "gf256.hpp"
#include "wait_hook.hpp"
#include "group_commit.hpp"
#include "rs_plan.hpp"

namespace rsmi {
namespace impl {

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The status of the exception being handled at the C-ABI boundary (the entry points' function
// try blocks): a C++ exception must not unwind into C or cgo callers.
int exception_status() noexcept;


struct DevTile {
    RsPlanDev* dev = nullptr;
    int K = 0, MT = 0;
};

struct Plan {
    std::vector<DevTile> tiles;
    int device = -1;
    ~Plan() {
        if (device >= 0) {
            (void)hipSetDevice(device);
            for (auto& t : tiles)
                if (t.dev) (void)hipFree(t.dev);
        }
    }
};

struct Staging {
    hipStream_t stream = nullptr;
    uint8_t* d_in = nullptr;
    uint8_t* d_out = nullptr;
    uint8_t* d_lin = nullptr;  // linear (pitch S) landing buffer for odd S
    size_t in_cap = 0, out_cap = 0, lin_cap = 0;
};

// Launch every tile of a plan over nblocks blocks.
// Fused CRC-16 output of an encode launch (rs_fast_kernel CRC variants): per-tile quad records
// of every shard and, for unaligned-window layouts, the rows' last chunks (rs_coding_kernels.hpp).
struct CrcFuse {
    const uint32_t* tbl = nullptr;
    uint32_t* rec = nullptr;
    uint32_t* tail = nullptr;
};

// Default and upper end of option "launch_units_max": the most tiles (launch_plan,
// launch_stripe_tiles, a segment of launch_mixed) or units (launch_plan_crc, launch_scrub) one
// launch takes; a longer batch goes in several launches of whole blocks.  A unit launch runs one
// workgroup of kWG threads per unit, and a launch stays below 2^32 threads: the
// MI355X runtime takes a larger grid without an error and wraps its thread count at 2^32, so a
// fused encode or scrub of 2^24 + 3 units coded three of them and returned RSMI_OK, and a Verify of
// 2^26 + 5 tiles strode over them with two workgroups for 10.6 s.  The tile launches run a
// workgroup per 4 tiles and stay four times further below.
constexpr uint64_t kLaunchUnitsDefault = (uint64_t(1) << 24) - 1;
static_assert(kLaunchUnitsDefault * kWG < (uint64_t(1) << 32), "a unit launch stays below 2^32 threads");
// A table launch (BlockBases) is one launch: the table holds bases, not a range that could be
// cut.  A table whose blocks pass the cap (under the default: 64 blocks of rows past 256 MiB)
// makes the table forms return RSMI_ERR_INVALID_ARG, and their callers launch per block.

}  // namespace impl
}  // namespace rsmi

// Device scratch of the fused encode + CRC-16 (records of the tiles or units, and the inline
// combine's per-block unit counters), one per stream its launches go to, so concurrent calls on
// different streams never share records or counters.  Every caller stream of the
// device-resident calls gets its own.  The context's own streams share one, and only staging[0]
// ever launches a fused (or flagged) kernel (asserted in crc_scratch and arm_flag): host calls
// hold the context lock through their synchronisation, and a pipelined coalesced batch that is
// still in flight after the lock is released (rsmi_coalesce.cpp) is ordered before the next
// launch by staging[0]'s stream order.  The same holds for the page-locked R(shard)
// areas (raw_area, pipe_area): written by staging[0]'s kernels only.
struct CrcScratch {
    uint8_t* d_chunks = nullptr;  // tile records and tails (CrcFuse) or unit records
    size_t chunks_cap = 0;
    uint32_t* d_fctr = nullptr;  // per-block unit counters of the inline combine
    size_t fctr_cap = 0;
};

// defaults of options "coalesce_lanes" / "coalesce_carry" (build macros for A/B library variants)
#ifndef RSMI_COALESCE_LANES
#define RSMI_COALESCE_LANES 2
#endif
#ifndef RSMI_COALESCE_CARRY
#define RSMI_COALESCE_CARRY 1
#endif
// default of option "coalesce_flag" (rsmi_coalesce.cpp)
#ifndef RSMI_COALESCE_FLAG
#define RSMI_COALESCE_FLAG 1
#endif
// default of option "coalesce_pipeline" (rsmi_coalesce.cpp)
#ifndef RSMI_COALESCE_PIPELINE
#define RSMI_COALESCE_PIPELINE 1
#endif
// the fewest blocks a coalesced group codes through the table kernels (R(shard) straight into
// page-locked memory, no read-back dispatch): 1, a lone caller too (build macro for A/B variants;
// 2 before profiles/r05/r/)
#ifndef RSMI_TABLE_MIN_BLOCKS
#define RSMI_TABLE_MIN_BLOCKS 1
#endif

struct rsmi_ctx {
    int k = 0, m = 0, n = 0, device = 0;
    rsmi::Matrix M;  // n x k
    std::mutex mu;
    std::atomic<bool> dev_ready_flag{false};  // dev_ready, readable without mu (coalesce)
    bool dev_ready = false;
    int dev_status = RSMI_OK;
    int num_cu = 256;
    std::map<std::string, std::shared_ptr<rsmi::impl::Plan>> plans;
    std::vector<rsmi::impl::Staging> staging;  // [0] single-block calls, [0..2] batch pipeline
    uint8_t* h_stage = nullptr;    // pinned landing area for rebuilt rows (odd S)
    size_t h_stage_cap = 0;
    uint32_t* d_crc_tbl = nullptr;  // CRC-16 device tables (crc16.hpp), uploaded on first use
    uint8_t* d_crc = nullptr;       // raw row CRCs (u32) of host batch calls
    size_t crc_cap = 0;
    uint32_t* d_crc32_tbl = nullptr;  // CRC-32 device tables (crc32.hpp), uploaded on first use
    uint8_t* d_crc32 = nullptr;       // raw row CRC-32s of host batch calls
    size_t crc32_cap = 0;
    // Encoder.Verify (rsmi_verify.cpp): the flags of host calls, and per stream the scratch its
    // fallback encodes into (shapes without an rs_verify_kernel)
    uint8_t* d_vbad = nullptr;
    size_t vbad_cap = 0;
    struct VerifyScratch {
        uint8_t* p = nullptr;
        size_t cap = 0;
    };
    std::map<hipStream_t, VerifyScratch> verify_scratch;
    // rsmi_locate (rsmi_locate.cpp): per stream the candidate words (and the flags, when the
    // caller takes none) of its launches; the fallback kernel's tables, uploaded on first use
    std::map<hipStream_t, VerifyScratch> locate_scratch;
    uint8_t* d_locate_tbl = nullptr;
    // rsmi_scrub (rsmi_scrub.cpp): per stream the unit records of rs_scrub_mfma_kernel
    std::map<hipStream_t, VerifyScratch> scrub_scratch;
    // rsmi_reconstruct_mixed_batch_* (rsmi_mixed.cpp): per stream the class lists and plan
    // pointers of its launches.  A call's words are written to the page-locked half h at head and
    // copied from there to the same offset of the device half d, both on that stream; head moves
    // on, so an earlier call's words stay until its copy and kernels have consumed them.  When a
    // call's words no longer fit behind head, the stream is waited for once and head starts over.
    struct MixedScratch {
        uint8_t* d = nullptr;
        uint8_t* h = nullptr;
        size_t cap = 0, head = 0;
    };
    std::map<hipStream_t, MixedScratch> mixed_scratch;
    // ... and of its _verify forms: per stream the unit records of rs_mixed_fused_kernel and the
    // (entry, slot) checksums their combine leaves for the scatter
    std::map<hipStream_t, VerifyScratch> mixed_verify_scratch;
    rsmi::Crc32Shift crc32_shift{};  // launch_crc32's per-S shift matrix, for crc32_shift_S
    uint64_t crc32_shift_S = ~uint64_t(0);
    CrcScratch own_scratch;  // the fused encode + CRC-16's scratch on the context's own streams
    std::map<hipStream_t, CrcScratch> stream_scratch;  // ... and on each caller stream (device-resident calls)
    // options
    int opt_crc16_fold = 1;     // CRC-16 rows pass, either layout: 0 = nibble tables, 1 = matrix cores (fp4)
    int opt_crc32_fold = RSMI_CRC32_FOLD_DEFAULT;  // CRC-32 rows pass: 0 = nibble tables, 1 = matrix cores
    int opt_fused_fold = 1;     // aligned fused encode + CRC-16: 0 = nibble tables, 1 = matrix cores (fp4)
    long opt_waves_per_cu = 0;  // grid cap (0 = one tile per wave / the CRC passes' defaults)
    // tiles or units per launch; atomic (the launchers read it through its conversion): rsmi_get_stat
    // reads it without ctx->mu
    std::atomic<long> opt_launch_units_max{long(rsmi::impl::kLaunchUnitsDefault)};
    // kernel launches of the five loops that cut a batch at opt_launch_units_max (rsmi_get_stat
    // "split_launches", read without ctx->mu)
    std::atomic<long> split_launches{0};
    int opt_zero_copy = 1;  // results into page-locked host buffers by kernel stores
    long opt_small_bytes = 2L << 20;  // host calls up to this many shard bytes run zero-copy
    uint8_t* h_small = nullptr;       // page-locked staging of small calls (pageable callers)
    size_t h_small_cap = 0;
    uint8_t* h_raw = nullptr;  // page-locked landing area of row CRCs read back by kernel (readback)
    size_t h_raw_cap = 0;
    // pipelined coalesced batches (rsmi_coalesce.cpp): two page-locked landing areas of the table
    // launches' R(shard) and an event per area, so a lane's next batch launches while this one is
    // still coded
    uint8_t* h_pipe[2] = {nullptr, nullptr};
    size_t h_pipe_cap[2] = {0, 0};
    hipEvent_t pipe_ev[2] = {nullptr, nullptr};
    int pipe_slot = 0;
    int opt_coalesce_pipeline = RSMI_COALESCE_PIPELINE;
    // completion flags of table launches (BlockBases::done_flag): two page-locked flags (64 bytes
    // apart; slot = sequence number & 1, at most two launches of a context in flight) and their
    // device counters
    uint32_t* h_done = nullptr;
    uint32_t* h_done_dev = nullptr;
    uint32_t* d_done_ctr = nullptr;
    uint32_t done_seq = 0;
    int opt_coalesce_flag = RSMI_COALESCE_FLAG;
    // the coalescer's options are read by callers without ctx->mu (coalesce), so they are atomic
    std::atomic<long> opt_coalesce_us{0};     // extra wait for more callers before a coalesced batch runs
    std::atomic<long> opt_coalesce_max{256};  // blocks per coalesced batch
    std::string last_kernel;  // diagnostics (rsmi_last_kernel), under lk_mu
    mutable std::mutex lk_mu;
    // group commit for rsmi_encode_block_coalesced (see there)
    struct CoalReq {
        // encode: block/B in, out = (k+m)*S shards, raw optional; reconstruct: out = n*S
        // shards in place, present / want flags (group key covers S, pattern, want)
        const uint8_t* block;
        size_t B;
        uint8_t* out;
        uint32_t* raw;
        uint32_t* raw32;  // encode: optional CRC-32 R32(shard) per shard
        std::string key;
        int rc;
        bool done;
    };
    // a batch that throws (std::bad_alloc from the executor's host containers) fails its
    // requests as the boundary reports host-resource exceptions (include/rsmi.h ABI v3)
    rsmi::GroupCommit<CoalReq> coal{RSMI_ERR_HOST};
    std::atomic<int> opt_inject_host_fault{0};  // test hook: the next coalesced batches or direct host encodes throw std::bad_alloc
    std::atomic<int> opt_inject_lane_fault{0};  // test hook: the next lane contexts fail to open (RSMI_ERR_DEVICE)
    uint8_t* h_coal = nullptr;  // page-locked staging of the executing batch
    size_t h_coal_cap = 0;
    // Coalesced batches run on up to opt_coalesce_lanes lanes at once: lane 0 is this context, lane
    // i > 0 the child context lanes[i - 1] (same k, m, device and options; opened on first use), so
    // one batch can be coded while the next is launched and the callers' queue stays one queue
    std::atomic<long> opt_coalesce_lanes{RSMI_COALESCE_LANES};
    std::atomic<long> opt_coalesce_carry{RSMI_COALESCE_CARRY};  // batches a lane runs after its own before handing over (group_commit.hpp)
    std::vector<rsmi_ctx*> lanes;
    mutable std::mutex lanes_mu;
};

namespace rsmi {
namespace impl {

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return hip_status(_e);    \
    } while (0)

int hip_status(hipError_t e);
hipError_t pinned_alloc(void** p, size_t bytes);
int ensure_device(rsmi_ctx* c);
int make_plan(rsmi_ctx* c, const Matrix& coef, const std::vector<int>& in_rows, const std::vector<int>& out_rows,
              std::shared_ptr<Plan>& out);
int encode_plan(rsmi_ctx* c, std::shared_ptr<Plan>& out);
int decode_rows(const rsmi_ctx* c, const uint8_t* present, Matrix& dec, std::vector<int>& used);
int reconstruct_plan(rsmi_ctx* c, const uint8_t* present, const uint8_t* want, std::shared_ptr<Plan>& out);
std::vector<uint8_t> want_mask(const rsmi_ctx* c, const uint8_t* present, int data_only);
const char* kernel_label(int K, int MT, int NT, bool fast);
int auto_cache_policy(int K, int MT);
// tb: a table of block bases, in / out then being offsets from each (at most kTableBlocks blocks,
// the table kernels only: RSMI_ERR_INVALID_ARG when the shape has none, callers then launch per block)
int launch_plan(rsmi_ctx* c, const Plan& plan, const uint8_t* in, uint64_t in_rs, uint64_t in_bs, uint8_t* out,
                uint64_t out_rs, uint64_t out_bs, uint64_t S, uint64_t nblocks, hipStream_t stream,
                const CrcFuse* fuse = nullptr, const BlockBases* tb = nullptr, bool* armed = nullptr);
uintptr_t table_alignment(const BlockBases* tb, uint64_t nblocks);  // OR of the table's first nblocks bases
void set_last_kernel(rsmi_ctx* c, const std::string& label);
CrcScratch& crc_scratch(rsmi_ctx* c, hipStream_t st);  // caller holds ctx->mu
// reserve() for device scratch a stream's kernels may still be reading: that stream is
// synchronised before the old buffer is freed
int reserve_on(uint8_t*& p, size_t& cap, size_t need, hipStream_t st);
int reserve(uint8_t*& p, size_t& cap, size_t need);
int count_present(const rsmi_ctx* c, const uint8_t* present, int& np, int& dp);
int reconstruct_precheck(const rsmi_ctx* c, const uint8_t* present, const uint8_t* want);
int reconstruct_dev_impl(rsmi_ctx* c, uint8_t* d_shards, size_t shard_stride, size_t block_stride, size_t S,
                                size_t nblocks, const uint8_t* present, const uint8_t* want, void* stream);
bool dma_2d_ok(size_t S);
int repitch(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t width, size_t rows,
            hipStream_t stream);
uint8_t* host_alias(void* p, size_t len);
uint8_t* small_stage(rsmi_ctx* c, size_t need);
uint8_t* raw_area(rsmi_ctx* c, size_t bytes);
int readback(rsmi_ctx* c, const uint32_t* d16, const uint32_t* d32, size_t sz, hipStream_t st, const uint32_t*& h16,
             const uint32_t*& h32);
int encode_small(rsmi_ctx* c, const Plan& plan, const uint8_t* data, size_t dbs, uint8_t* parity, size_t pbs,
                        size_t S, size_t nblocks, uint32_t* raw_out, uint32_t* raw32_out = nullptr);
int encode_host_impl(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, uint8_t* parity,
                            size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* raw_out, uint32_t* raw32_out = nullptr);
int reconstruct_small(rsmi_ctx* c, const Plan& plan, uint8_t* shards, size_t bs, size_t S, size_t nblocks,
                             const uint8_t* present, const uint8_t* want, uint32_t* raw16 = nullptr,
                      uint32_t* raw32 = nullptr);
int reconstruct_host_impl(rsmi_ctx* c, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                 const uint8_t* present, const uint8_t* want, uint32_t* raw16 = nullptr,
                          uint32_t* raw32 = nullptr);
// The layout of a stripe's rows (rsmi_verify.cpp), which picks the tile kernels' form: 16-byte
// aligned, unaligned windows (UA), or neither (the scratch-encode fallback).
enum class StripeLayout { kAligned, kUA, kNeither };
// The rows a call over stored stripes runs on: the first block's data and parity rows, their row
// and block strides in bytes, the shard size and the number of blocks.  Every launch function of
// the stripe calls takes one.  The rows are const, as Verify reads them; the healers, which
// rewrite rows, cast where their rows kernels' arguments are built (launch_heal_rows).
struct StripeRows {
    const uint8_t* data = nullptr;
    uint64_t data_rs = 0, data_bs = 0;
    const uint8_t* parity = nullptr;
    uint64_t parity_rs = 0, parity_bs = 0;
    uint64_t S = 0, nblocks = 0;
    // blocks [b0, b0 + nb): the one place where a block index meets a block stride
    StripeRows from(uint64_t b0, uint64_t nb) const {
        StripeRows r = *this;
        r.data += b0 * data_bs;
        r.parity += b0 * parity_bs;
        r.nblocks = nb;
        return r;
    }
    StripeLayout layout() const;
};
// A tile's kernel in a stripe call's table on a layout (null: the shape has none, or the layout is
// kNeither), and the end of a tile launch: last_kernel's "rs_<name>_kernel<K=..,MT=..>[,UA]" set,
// the status of the launches returned.
void* stripe_kernel(const StripeKernelTable& table, StripeLayout layout, const DevTile& t);
int tiles_launched(rsmi_ctx* c, const char* name, StripeLayout layout, const DevTile& t);
// Encoder.Verify of rows.nblocks blocks (rsmi_verify.cpp; caller holds ctx->mu): bad[b*m + j], device
// memory, zeroed here on the stream, then non-zero where stored parity row j of block b differs
// from the encode of the block's data rows.  Stream-ordered, no synchronisation.
// loc (rsmi_locate.cpp): where the shape has an rs_locate_kernel, that kernel runs in the place of
// rs_verify_kernel and also ANDs the shards that explain each dirty tile into cand[b] (one word
// per block, all-ones on the stream before the call; rplan: the ratio matrix's tables); fused is
// the layout it ran on, kNeither when it did not run.
struct LocateFuse {
    const RsPlanDev* rplan = nullptr;
    uint32_t* cand = nullptr;
    StripeLayout fused = StripeLayout::kNeither;
};
int launch_verify(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, uint32_t* bad, hipStream_t stream,
                  LocateFuse* loc = nullptr);
// rsmi_scrub of rows.nblocks blocks (rsmi_scrub.cpp; caller holds ctx->mu): launch_verify's flags in
// bad[b*m + j] and R(row) of every data and parity row over bytes [0, S) in raw[b*(k+m) + r], data
// rows first, both device memory, from one read of the rows (rs_scrub_mfma_kernel and the records'
// combine) or, for shapes without that kernel, from launch_verify and launch_crc in turn.
// Stream-ordered, no synchronisation unless the stream's record scratch grows.
int launch_scrub(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, uint32_t* bad, uint32_t* raw,
                 hipStream_t stream);
// One tile's kernel fn of a stripe call's table over the rows' blocks: one tile per wave unless
// waves_per_cu caps the grid, in launches of at most launch_units_max tiles.  The tile kernels share
// rs_verify_kernel's parameters and, behind them, a plan (rplan) and a second per-block output.
// Each of the two per-block outputs moves on by its own words per block from launch to launch:
//   bad    bad_wpb = m: Verify's flags; pair_words(n): the pair words of rs_locate_pair_kernel;
//          null for the heal kernels, which take none
//   words  words_wpb = 1: the candidates of rs_locate_kernel, the verdicts rs_heal_kernel and
//          rs_locate_pair_kernel read; 2: the pair verdicts of rs_heal_pair_kernel; null for
//          rs_verify_kernel
int launch_stripe_tiles(rsmi_ctx* c, void* fn, const DevTile& t, const StripeRows& rows, uint32_t* bad,
                        uint64_t bad_wpb, const RsPlanDev* rplan, void* words, uint64_t words_wpb, hipStream_t stream);
// The stream's entry of a per-stream scratch map (caller holds ctx->mu): verify_scratch, the
// fallback's encoded rows; locate_scratch; scrub_scratch.  Past 32 streams the device is drained once and every
// stream's scratch freed.
rsmi_ctx::VerifyScratch& stream_scratch(std::map<hipStream_t, rsmi_ctx::VerifyScratch>& map, hipStream_t st);
// The fallback of the shapes without a tile kernel: the encode of the data rows into the stream's
// verify_scratch (16-byte-aligned rows), at most 64 MiB of scratch rows at a time, and per chunk
// of blocks from block b0 (sub: their rows, a copy whose members a kernel argument array may
// point to) the caller's byte-granular launch, before the next encode reuses them.
using ScratchRowsFn =
    std::function<int(uint64_t b0, StripeRows sub, const uint8_t* enc, uint64_t enc_rs, uint64_t enc_bs)>;
int encode_into_scratch(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, hipStream_t stream,
                        const ScratchRowsFn& fn);
// The argument checks of the *_batch_dev entries and of the host impls (out: the output that must
// be given), and the device entries' prologue: ctx->mu taken into lock, the device bound, the
// encode plan (declared before lock by the caller, so it outlives the lock).
int check_stripe_dev_args(const rsmi_ctx* c, const void* d_data, size_t data_shard_stride, const void* d_parity,
                          size_t parity_shard_stride, size_t S, const void* out);
int check_stripe_host_args(const rsmi_ctx* c, const void* data, size_t data_block_stride, const void* parity,
                           size_t parity_block_stride, size_t S, const void* out);
int begin_stripe_dev_call(rsmi_ctx* c, std::unique_lock<std::mutex>& lock, std::shared_ptr<Plan>& plan);
// A *_batch_dev entry between its try and its catch: the checks, nothing to do for no blocks, the
// prologue, then the entry's own launch(plan, rows) under the lock.
template <class Launch>
int stripe_dev_call(rsmi_ctx* c, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                    const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                    size_t nblocks, const void* out, const Launch& launch) {
    int rc = check_stripe_dev_args(c, d_data, data_shard_stride, d_parity, parity_shard_stride, S, out);
    if (rc) return rc;
    if (nblocks == 0) return RSMI_OK;
    std::shared_ptr<Plan> plan;
    std::unique_lock<std::mutex> lock;
    if ((rc = begin_stripe_dev_call(c, lock, plan))) return rc;
    return launch(*plan, StripeRows{d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride,
                                    parity_block_stride, S, nblocks});
}
// What a host-memory call runs over stored stripes: verify_host_impl stages or uploads the rows on
// one of rsmi_verify_batch_host's three paths and calls
//   prepare()  once, under ctx->mu with the device bound: the call's device result buffers
//   launch()   per staged range of blocks from block b0, its rows visible to the device
//   fetch(st)  the results to the caller's memory: queued on st, which the caller then
//              synchronises, or (st null, every stream idle) copied synchronously
// stripe_results sets prepare and fetch.  rsmi_heal and rsmi_heal_pair alone write rows, so they
// alone set the write-back leg (stripe_write_back; unset: no step is added):
//   small_done(sd, sp)          the small staged call, after its synchronisation: the page-locked
//                               copies of the data blocks (k*S apart) and of the parity blocks
//                               (m*S apart), null for a half that was not staged
//   chunk_done(st, b0, nb, Sp)  the upload pipeline, before st's device rows (pitch Sp) of blocks
//                               b0 .. b0+nb are overwritten by a later chunk, and at the end
struct StripeCheck {
    std::function<int()> prepare;
    std::function<int(const Plan& plan, const StripeRows& rows, uint64_t b0, hipStream_t st)> launch;
    std::function<int(hipStream_t st)> fetch;
    std::function<int(const uint8_t* sd, const uint8_t* sp)> small_done;
    std::function<int(Staging& st, uint64_t b0, uint64_t nb, size_t Sp)> chunk_done;
};
int verify_host_impl(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                     size_t parity_block_stride, size_t S, size_t nblocks, const StripeCheck& chk);
// The device result buffer of a host call, in ctx->d_vbad: the flags of nblocks blocks, then W
// 32-bit words per block of the call's second output: none for Verify, the verdict of locate and
// heal, the two of locate pair and heal pair, the k + m raws of scrub.  stripe_results sets
// chk.prepare, which reserves the buffer and sets r, and chk.fetch, which copies the words to
// words_out and, when bad_out is given, the flags there.  r must outlive chk.
struct StripeResults {
    uint32_t* d_bad = nullptr;
    uint32_t* d_words = nullptr;
    int32_t* verdicts() const { return reinterpret_cast<int32_t*>(d_words); }
};
void stripe_results(rsmi_ctx* c, size_t nblocks, size_t W, void* words_out, uint32_t* bad_out, StripeResults& r,
                    StripeCheck& chk);
// The write-back leg of the healers' host calls: sets chk.small_done and chk.chunk_done, which
// return the rows that the W verdict words of every block name (verdict_out, r.verdicts()) to where
// the caller keeps them, and nothing else.
void stripe_write_back(rsmi_ctx* c, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                       size_t parity_block_stride, size_t S, size_t nblocks, size_t W, int32_t* verdict_out,
                       const StripeResults& r, StripeCheck& chk);
// The host entries of the four calls that return verdicts (locate, heal, locate pair, heal pair),
// which differ in W, the verdict words per block, in their launch (blocks' rows, verdicts and
// flags in device memory, stream-ordered) and in whether they write rows: the healers give their
// rows once more, writable (home_data, home_parity), and get the write-back leg.
// verdicts_one_block is the block-of-one wrapper around it: k + m rows S apart, out[W].
using VerdictLaunch = int (*)(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* verdicts, uint32_t* bad,
                              hipStream_t stream);
int verdicts_host_impl(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                       size_t parity_block_stride, size_t S, size_t nblocks, size_t W, VerdictLaunch launch,
                       int32_t* verdict_out, uint32_t* bad_out, uint8_t* home_data = nullptr,
                       uint8_t* home_parity = nullptr);
int verdicts_one_block(rsmi_ctx* c, const uint8_t* shards, size_t S, size_t W, VerdictLaunch launch, int* out,
                       uint8_t* home = nullptr);
// rsmi_locate of rows.nblocks blocks (rsmi_locate.cpp; caller holds ctx->mu): verdicts culprit[b] and,
// when bad is given, Verify's flags, device memory, stream-ordered.  fused: the layout
// rs_locate_kernel ran on (kNeither: m = 1, or the encode into scratch and rs_locate_rows_kernel).
int launch_locate(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* culprit, uint32_t* bad,
                  hipStream_t stream, StripeLayout* fused = nullptr);
// rsmi_heal's launch behind launch_locate's verdicts (rsmi_heal.cpp; caller holds ctx->mu, m >= 2):
// rs_heal_kernel on the layout fused names, or the encode into scratch and rs_heal_rows_kernel.
int launch_heal_named(rsmi_ctx* c, const Plan& plan, StripeLayout fused, const StripeRows& rows, int32_t* culprit,
                      hipStream_t stream);
// The healers' fallback (rsmi_heal.cpp): the data rows encoded into scratch, chunk by chunk, and
// behind each chunk's encode the byte-granular kernel (rs_heal_rows_kernel, rs_heal_pair_rows_kernel:
// one parameter list), which rewrites the rows that the W verdict words of a block name.
int launch_heal_rows(rsmi_ctx* c, const Plan& plan, void* kernel, const char* label, const StripeRows& rows,
                     const int32_t* verdict, uint64_t W, hipStream_t stream);
// rsmi_locate_pair of rows.nblocks blocks (rsmi_pair.cpp; caller holds ctx->mu): two verdict words per
// block in out and, when bad is given, Verify's flags, device memory, stream-ordered.  info: the
// layout rs_locate_kernel ran on (kNeither: the fallback) and rsmi_locate's verdicts, one word per
// block in the stream's scratch, valid until the stream's next stripe call.
struct PairLaunch {
    StripeLayout fused = StripeLayout::kNeither;
    int32_t* culprit = nullptr;
};
int launch_locate_pair(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* out, uint32_t* bad,
                       hipStream_t stream, PairLaunch* info = nullptr);
// the ratio matrix's plan "L" (output slot 0: inv(M[k][c])) and the byte-granular kernels' tables
// (ctx->d_locate_tbl: log | exp | R | inv(M[k][c])), both built on first use
int ratio_plan(rsmi_ctx* c, std::shared_ptr<Plan>& out);
int ensure_locate_tables(rsmi_ctx* c);
// rsmi_reconstruct_mixed_* (rsmi_mixed.cpp).  The host classing of a call, device-free: the
// blocks' distinct (present, want) pairs, numbered by first appearance, and per block its pair,
// its status and the number of rows the call writes in it.  A pair's key holds per row bit 0
// (present) and bit 1 (the row is rebuilt: wanted and missing).
struct MixedBatch {
    std::vector<std::string> keys;  // per pattern
    std::vector<uint8_t> key_rows;  // ... the rows it rebuilds, 0 also where too few rows are present
    std::vector<int32_t> key_status;
    std::vector<uint32_t> pat;  // per block
    size_t work = 0, too_few = 0;  // blocks with rows to rebuild; blocks with too few rows present
};
void classify_mixed(const rsmi_ctx* c, size_t nblocks, const uint8_t* present, const uint8_t* required, int data_only,
                    MixedBatch& mb);
// The launches of blocks [b0, b0 + nb) of a classed batch (caller holds ctx->mu, the device is
// bound): rs_mixed_kernel per class, launch_plan per run of fallback blocks.  base: block b0's
// first row.  Stream-ordered, no synchronisation unless the stream's scratch grows or wraps.
// d16 / d32 (device memory, either may be null): block b0's n words of the by-row checksums, zeroed
// by the caller on the stream; R / R32 of every row the launches rebuild is added there by the named
// rows pass behind them, its rows array riding in the same upload as the classes' lists.
// dver (device memory, the _verify forms; excludes d16 / d32): block b0's n words, zeroed by the
// caller on the stream; R of every row the launches read (a block's k survivors) and rebuild lands
// there.  Classes with an rs_mixed_fused_kernel get both from that kernel, its records' combine and
// the scatter (the stream's mixed_verify_scratch holds what lies between them); every other block
// is rebuilt as without dver and has its k + rows rows named to the named rows pass.
int launch_mixed(rsmi_ctx* c, const MixedBatch& mb, uint8_t* base, uint64_t rs, uint64_t bs, uint64_t S, uint64_t b0,
                 uint64_t nb, hipStream_t stream, uint32_t* d16 = nullptr, uint32_t* d32 = nullptr,
                 uint32_t* dver = nullptr);
// need bytes of the stream's entry of ctx->mixed_scratch (rsmi_mixed.cpp; caller holds ctx->mu), 16-byte
// aligned, at the same offset of the page-locked half h and the device half d: the moving head the
// mixed reconstruct and the ragged encode share.  Waits for the stream once when the scratch has to
// grow or start over; past 32 streams the device is drained once and every stream's scratch freed.
int mixed_words(rsmi_ctx* c, hipStream_t st, size_t need, uint8_t*& h, uint8_t*& d);
// rsmi_encode_ragged_batch_* (rsmi_ragged.cpp).  A block's class (RSMI_RAGGED_*) over these bases:
// launch_plan's layout test on the block's two halves, and whether k has an rs_ragged_kernel.
// tiles: the block's 1 KiB-per-row tiles, 0 for a fallback block.  Device-free.
int ragged_class(const rsmi_ctx* c, uintptr_t data_base, uintptr_t parity_base, const rsmi_ragged_block& b,
                 uint64_t& tiles);
// The launches of a ragged batch (caller holds ctx->mu, the device is bound, the blocks have passed
// the entry points' checks; data, parity: device addresses): per segment of whole blocks one upload
// of the classes' units and the blocks' descriptors, rs_ragged_kernel per non-empty class (aligned,
// then unaligned-window) and plan tile, launch_plan per fallback block behind them.  Stream-ordered,
// no synchronisation unless the stream's scratch grows or starts over.
int launch_ragged(rsmi_ctx* c, const Plan& plan, const uint8_t* data, uint8_t* parity, const rsmi_ragged_block* blocks,
                  size_t nblocks, hipStream_t stream);
int ensure_crc_tables(rsmi_ctx* c);
int ensure_crc32_tables(rsmi_ctx* c);
// R(row) / R32(row) of the rows the plan rebuilt (want && !present), one row per block at
// base + b*bstride + r*rpitch, into the device buffers d16 / d32 at [b*n + r] (either may be
// null; zeroed here), stream-ordered
int launch_rebuilt_crcs(rsmi_ctx* c, const uint8_t* base, uint64_t rpitch, uint64_t bstride, uint64_t S,
                        uint64_t nblocks, const uint8_t* present, const uint8_t* want, uint32_t* d16, uint32_t* d32,
                        hipStream_t stream);
int launch_crc32(rsmi_ctx* c, const uint8_t* base, uint64_t rpitch, uint64_t bstride, uint32_t nrows, uint64_t S,
                 uint64_t nblocks, uint32_t* out, uint64_t out_bs, hipStream_t stream);
// R(row) / R32(row) of the rows a device array names (rs_plan.hpp NamedRowsArgs) into d16 / d32
// (either may be null), by slot or by row; zero: the outputs are zeroed on the stream first
int launch_crc_named(rsmi_ctx* c, const NamedRowsArgs& a, uint64_t S, uint64_t nblocks, uint32_t* d16, uint32_t* d32,
                     hipStream_t stream, bool zero);
int launch_crc(rsmi_ctx* c, const uint8_t* base, uint64_t rpitch, uint64_t bstride, uint32_t nrows, uint64_t S,
               uint64_t nblocks, uint32_t* out, uint64_t out_bs, hipStream_t stream, bool zero = true);
int launch_encode_crc(rsmi_ctx* c, const Plan& plan, const uint8_t* in, size_t in_rs, size_t in_bs, uint8_t* out,
                             size_t out_rs, size_t out_bs, size_t S, size_t nblocks, uint32_t* raw, hipStream_t st);
int launch_plan_crc(rsmi_ctx* c, const Plan& plan, const uint8_t* in, size_t in_rs, size_t in_bs, uint8_t* out,
                    size_t out_rs, size_t out_bs, size_t S, size_t nblocks, uint32_t* raw, hipStream_t st,
                    const BlockBases* tb = nullptr, bool* armed = nullptr);
// What the launches on the matrix-core fold (rs_crc_fold.hpp: rs_fused_mfma_kernel,
// rs_scrub_mfma_kernel, rs_mixed_fused_kernel) and the records' combine behind them agree on, for
// blocks of nsh rows of S bytes: chunks and tiles per row, units of 4 tiles per block, two-row
// accumulators (a record byte per lane each), record bytes per block, and A^e, which moves a row's
// value from the end of its last unit to the row's end.
struct FoldGeometry {
    uint64_t cpb, tpb, upb, nsh, nacc, rec_per_block;
    Crc16Shift sh;
    FoldGeometry(uint64_t S, uint64_t nsh);  // device-free (rsmi_crc.cpp)
};
// rs_crc16_combine_mfma_kernel over the records of nitems blocks (or list entries), g.rec_per_block
// bytes each at rec: R(row) into out[item * g.nsh + row].  A persistent grid of up to
// RSMI_COMBINE_WGS_PER_CU workgroups per CU, 4 waves each, over (item, 4-row group) pairs.
#ifndef RSMI_COMBINE_WGS_PER_CU
#define RSMI_COMBINE_WGS_PER_CU 8
#endif
int launch_fold_combine(rsmi_ctx* c, const uint8_t* rec, const FoldGeometry& g, uint64_t nitems, uint32_t* out,
                        hipStream_t stream);
int launch_encode_rows(rsmi_ctx* c, const Plan& plan, const uint8_t* in, size_t in_bs, uint8_t* out, size_t out_bs,
                       size_t S, size_t nblocks, uint32_t* d16, uint32_t* d32, hipStream_t st);
uint8_t* coal_stage(rsmi_ctx* c, size_t need);
// completion flags of table launches (rsmi_coalesce.cpp): arm one in tb (caller holds ctx->mu),
// its host view, and the poll that replaces the stream (or event) synchronisation
int arm_flag(rsmi_ctx* c, hipStream_t st, BlockBases& tb, uint32_t& seq);
const uint32_t* done_flag(const rsmi_ctx* c, uint32_t seq);
int wait_flag(const uint32_t* flag, uint32_t seq, hipStream_t st, hipEvent_t ev);
int run_coalesced_in_place(rsmi_ctx* c, rsmi_ctx::CoalReq* const* rq, size_t nb, size_t S, std::function<void()>* fin);
void run_coalesced_group(rsmi_ctx* c, rsmi_ctx::CoalReq* const* rq, size_t nb, std::function<void()>* fin);
std::function<void()> run_coalesced(rsmi_ctx* c, int lane, std::vector<rsmi_ctx::CoalReq*>& batch);
int coalesce(rsmi_ctx* c, rsmi_ctx::CoalReq& req);
int ensure_device_fast(rsmi_ctx* c);
rsmi_ctx* lane_context(rsmi_ctx* c, int lane, int* rc);  // coalescing lane `lane`'s context (0: c)  // ensure_device without the context lock once the device is bound
int apply_option(rsmi_ctx* c, const char* key, long value);  // caller holds ctx->mu

}  // namespace impl
}  // namespace rsmi
