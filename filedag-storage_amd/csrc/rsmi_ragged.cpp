// rsmi_ragged.cpp -- rsmi_encode_ragged_* (include/rsmi.h; see rsmi_impl.hpp for the file map): the
// encode of a batch in which every block has its own shard size and its own rows.  The host classes
// each block once with launch_plan's layout test on the block's two halves (aligned, unaligned
// windows, fallback), cuts the batch into segments of whole blocks, uploads per segment the
// classes' units (block, first tile: up to 4 tiles of one block) and the blocks' descriptors
// through the stream's moving-head scratch (mixed_words, rsmi_mixed.cpp) and launches
// rs_ragged_kernel (rs_ragged_kernels.hip) once per non-empty class and tile of the encode plan.
// Blocks whose K has no rs_ragged_kernel, or whose rows are neither aligned nor at least 16 bytes
// long, take the uniform call's launch_plan one by one behind the class launches: the correctness
// path of rare shapes.

#include "rsmi_impl.hpp"

#include <limits>

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

int ragged_class(const rsmi_ctx* c, uintptr_t data_base, uintptr_t parity_base, const rsmi_ragged_block& b,
                 uint64_t& tiles) {
    tiles = 0;
    const uint64_t S = b.S, ds = b.data_shard_stride, ps = b.parity_shard_stride;
    if (!ragged_shape(c->k) || S >= (uint64_t(1) << 31)) return RSMI_RAGGED_FALLBACK;
    const uint64_t S16 = (S + 15) / 16 * 16;
    const bool aligned = (data_base + b.data_off) % 16 == 0 && (parity_base + b.parity_off) % 16 == 0 && ds % 16 == 0 &&
                         ps % 16 == 0 && ds >= S16 && ps >= S16;
    if (!aligned && S < 16) return RSMI_RAGGED_FALLBACK;
    tiles = (S16 / 16 + uint64_t(kWave) - 1) / uint64_t(kWave);
    return aligned ? RSMI_RAGGED_ALIGNED : RSMI_RAGGED_UA;
}

namespace {

// The entry points' checks, before any device access: the first bad block decides, per block in
// the uniform call's order.
int check_ragged_args(const rsmi_ctx* c, const void* data, const void* parity, const rsmi_ragged_block* blocks,
                      size_t nblocks) {
    if (!c || !data || !parity || !blocks) return RSMI_ERR_INVALID_ARG;
    for (size_t b = 0; b < nblocks; b++) {
        if (blocks[b].S == 0) return RSMI_ERR_SHARD_NO_DATA;
        if (blocks[b].data_shard_stride < blocks[b].S || blocks[b].parity_shard_stride < blocks[b].S)
            return RSMI_ERR_INVALID_ARG;
    }
    return RSMI_OK;
}

// a segment's blocks are named by the units' 32-bit word
constexpr size_t kRaggedSegBlocks = size_t(1) << 31;

}  // namespace

int launch_ragged(rsmi_ctx* c, const Plan& plan, const uint8_t* data, uint8_t* parity, const rsmi_ragged_block* blocks,
                  size_t nblocks, hipStream_t stream) {
    const int K = c->k;
    constexpr int wpg = kFastWG / kWave;
    static_assert(wpg == kRaggedUnitTiles, "a unit is a workgroup's tiles");
    uint64_t wg_cap = std::numeric_limits<uint64_t>::max();
    if (c->opt_waves_per_cu > 0) wg_cap = uint64_t(std::max(1L, long(c->num_cu) * c->opt_waves_per_cu / wpg));
    const uint64_t units_max = uint64_t(std::max(1L, long(c->opt_launch_units_max)));
    const uintptr_t db = reinterpret_cast<uintptr_t>(data), pb = reinterpret_cast<uintptr_t>(parity);
    std::vector<RaggedUnit> units[2];  // by class: RSMI_RAGGED_ALIGNED, RSMI_RAGGED_UA
    std::vector<RaggedBlockDev> descs;
    std::vector<size_t> fallback;
    for (size_t b0 = 0; b0 < nblocks;) {
        // a segment: whole blocks while the classes' units together stay within launch_units_max
        // (a block of more units is a segment of its own)
        units[0].clear();
        units[1].clear();
        descs.clear();
        fallback.clear();
        uint64_t nun = 0;
        size_t b = b0;
        for (; b < nblocks; b++) {
            const rsmi_ragged_block& rb = blocks[b];
            uint64_t tiles = 0;
            const int cls = ragged_class(c, db, pb, rb, tiles);
            if (cls == RSMI_RAGGED_FALLBACK) {
                fallback.push_back(b);
                continue;
            }
            const uint64_t u = (tiles + kRaggedUnitTiles - 1) / kRaggedUnitTiles;
            if (!descs.empty() && (nun + u > units_max || descs.size() >= kRaggedSegBlocks)) break;
            RaggedBlockDev d{};
            d.data = uint64_t(db) + rb.data_off;
            d.parity = uint64_t(pb) + rb.parity_off;
            d.data_rs = rb.data_shard_stride;
            d.parity_rs = rb.parity_shard_stride;
            d.S = uint32_t(rb.S);
            d.cpb = uint32_t((rb.S + 15) / 16);
            const uint32_t idx = uint32_t(descs.size());
            descs.push_back(d);
            for (uint64_t t = 0; t < tiles; t += kRaggedUnitTiles) units[cls].push_back(RaggedUnit{idx, uint32_t(t)});
            nun += u;
        }
        if (!descs.empty()) {
            // one upload: the descriptors, then the aligned class's units, then the UA class's
            const size_t desc_bytes = descs.size() * sizeof(RaggedBlockDev);
            const size_t u0_bytes = round_up(units[0].size() * sizeof(RaggedUnit), 16);
            const size_t u1_bytes = round_up(units[1].size() * sizeof(RaggedUnit), 16);
            uint8_t *h = nullptr, *d = nullptr;
            int rc = mixed_words(c, stream, desc_bytes + u0_bytes + u1_bytes, h, d);
            if (rc) return rc;
            std::memcpy(h, descs.data(), desc_bytes);
            if (!units[0].empty()) std::memcpy(h + desc_bytes, units[0].data(), units[0].size() * sizeof(RaggedUnit));
            if (!units[1].empty())
                std::memcpy(h + desc_bytes + u0_bytes, units[1].data(), units[1].size() * sizeof(RaggedUnit));
            HIP_TRY(hipMemcpyAsync(d, h, desc_bytes + u0_bytes + u1_bytes, hipMemcpyHostToDevice, stream));
            const RaggedBlockDev* dd = reinterpret_cast<const RaggedBlockDev*>(d);
            const size_t unit_off[2] = {desc_bytes, desc_bytes + u0_bytes};
            for (int cls = 0; cls < 2; cls++) {
                if (units[cls].empty()) continue;
                const RaggedUnit* du = reinterpret_cast<const RaggedUnit*>(d + unit_off[cls]);
                uint32_t nunits = uint32_t(units[cls].size());
                const uint32_t grid = uint32_t(std::min<uint64_t>(nunits, wg_cap));
                for (const DevTile& t : plan.tiles) {
                    void* fn = (cls == RSMI_RAGGED_ALIGNED ? ragged_kernels().fn : ragged_kernels().ua)[K][t.MT];
                    if (!fn) return RSMI_ERR_DEVICE;  // ragged_class admits only shapes with a kernel
                    const RsPlanDev* pd = t.dev;
                    void* args[] = {&pd, &du, &dd, &nunits};
                    HIP_TRY(hipLaunchKernel(fn, dim3(grid), dim3(uint32_t(kFastWG)), args, 0, stream));
                    c->split_launches.fetch_add(1, std::memory_order_relaxed);
                    char buf[96];
                    std::snprintf(buf, sizeof buf, "rs_ragged_kernel<K=%d,MT=%d>%s", K, t.MT,
                                  cls == RSMI_RAGGED_UA ? ",UA" : "");
                    set_last_kernel(c, buf);
                }
            }
        }
        // the fallback: the uniform call's launch, block by block
        for (size_t fbk : fallback) {
            const rsmi_ragged_block& rb = blocks[fbk];
            int rc = launch_plan(c, plan, data + rb.data_off, rb.data_shard_stride, 0, parity + rb.parity_off,
                                 rb.parity_shard_stride, 0, rb.S, 1, stream);
            if (rc) return rc;
        }
        b0 = b;
    }
    return hip_status(hipGetLastError());
}

namespace {

// The host-memory call on encode_host_impl's decisions: both halves page-locked, one kernel in
// place over PCIe; everything else is staged through the page-locked small_stage by CPU copies, in
// chunks of whole blocks of at most small_call_bytes of rows, each block's k + m rows packed at
// pitch roundup(S, 16) (the aligned form runs), coded there in place, and bytes [0, S) of its
// parity rows copied back.  No copy-engine pipeline: this leg is not tuned.
int ragged_host_impl(rsmi_ctx* c, const uint8_t* data, uint8_t* parity, const rsmi_ragged_block* blocks,
                     size_t nblocks) {
    int rc = check_ragged_args(c, data, parity, blocks, nblocks);
    if (rc) return rc;
    if (nblocks == 0) return RSMI_OK;
    std::lock_guard<std::mutex> g(c->mu);
    if ((rc = ensure_device(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::shared_ptr<Plan> plan;
    if ((rc = encode_plan(c, plan))) return rc;
    const size_t k = size_t(c->k), m = size_t(c->m);
    hipStream_t st = c->staging[0].stream;
    // the spans of the blocks' rows in the two halves
    uint64_t dlo = ~uint64_t(0), dhi = 0, plo = ~uint64_t(0), phi = 0;
    for (size_t b = 0; b < nblocks; b++) {
        const rsmi_ragged_block& rb = blocks[b];
        dlo = std::min(dlo, rb.data_off);
        dhi = std::max(dhi, rb.data_off + (k - 1) * rb.data_shard_stride + rb.S);
        plo = std::min(plo, rb.parity_off);
        phi = std::max(phi, rb.parity_off + (m - 1) * rb.parity_shard_stride + rb.S);
    }
    const uint8_t* din = c->opt_zero_copy ? host_alias(const_cast<uint8_t*>(data) + dlo, dhi - dlo) : nullptr;
    uint8_t* dout = din ? host_alias(parity + plo, phi - plo) : nullptr;
    if (din && dout) {
        // the aliases of the bases themselves (never dereferenced: every row lies inside the spans)
        const uint8_t* dbase = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(din) - dlo);
        uint8_t* pbase = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(dout) - plo);
        if ((rc = launch_ragged(c, *plan, dbase, pbase, blocks, nblocks, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return RSMI_OK;
    }
    const size_t limit = size_t(std::max(1L, c->opt_small_bytes));
    std::vector<rsmi_ragged_block> sb;
    for (size_t b0 = 0; b0 < nblocks;) {
        sb.clear();
        size_t bytes = 0, b = b0;
        for (; b < nblocks; b++) {
            const size_t P = round_up(size_t(blocks[b].S), 16), need = (k + m) * P;
            if (b > b0 && bytes + need > limit) break;
            sb.push_back(rsmi_ragged_block{blocks[b].S, bytes, P, bytes + k * P, P});
            bytes += need;
        }
        uint8_t* hs = small_stage(c, bytes);
        if (!hs) return RSMI_ERR_DEVICE;
        for (size_t i = 0; i < sb.size(); i++) {
            const rsmi_ragged_block& rb = blocks[b0 + i];
            for (size_t r = 0; r < k; r++)
                std::memcpy(hs + sb[i].data_off + r * sb[i].data_shard_stride, data + rb.data_off + r * rb.data_shard_stride,
                            size_t(rb.S));
        }
        uint8_t* dev = host_alias(hs, bytes);
        if (!dev) return RSMI_ERR_DEVICE;
        if ((rc = launch_ragged(c, *plan, dev, dev, sb.data(), sb.size(), st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < sb.size(); i++) {
            const rsmi_ragged_block& rb = blocks[b0 + i];
            for (size_t j = 0; j < m; j++)
                std::memcpy(parity + rb.parity_off + j * rb.parity_shard_stride,
                            hs + sb[i].parity_off + j * sb[i].parity_shard_stride, size_t(rb.S));
        }
        b0 = b;
    }
    return RSMI_OK;
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_encode_ragged_classify(const rsmi_ctx* c, const void* data_base, const void* parity_base,
                                const rsmi_ragged_block* blocks, size_t nblocks, uint8_t* class_out,
                                uint64_t* tiles_out) try {
    if (!c || !blocks) return RSMI_ERR_INVALID_ARG;
    // the bases may be null here: only their alignment counts
    int rc = check_ragged_args(c, blocks, blocks, blocks, nblocks);
    if (rc) return rc;
    for (size_t b = 0; b < nblocks; b++) {
        uint64_t tiles = 0;
        const int cls = ragged_class(c, reinterpret_cast<uintptr_t>(data_base), reinterpret_cast<uintptr_t>(parity_base),
                                     blocks[b], tiles);
        if (class_out) class_out[b] = uint8_t(cls);
        if (tiles_out) tiles_out[b] = tiles;
    }
    return RSMI_OK;
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_encode_ragged_batch_dev(rsmi_ctx* c, const uint8_t* d_data, uint8_t* d_parity, const rsmi_ragged_block* blocks,
                                 size_t nblocks, void* stream) try {
    int rc = check_ragged_args(c, d_data, d_parity, blocks, nblocks);
    if (rc) return rc;
    if (nblocks == 0) return RSMI_OK;
    std::shared_ptr<Plan> plan;  // declared before the lock, so it outlives it
    std::lock_guard<std::mutex> g(c->mu);
    if ((rc = ensure_device(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = encode_plan(c, plan))) return rc;
    return launch_ragged(c, *plan, d_data, d_parity, blocks, nblocks, static_cast<hipStream_t>(stream));
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_encode_ragged_batch_host(rsmi_ctx* c, const uint8_t* data, uint8_t* parity, const rsmi_ragged_block* blocks,
                                  size_t nblocks) try {
    return ragged_host_impl(c, data, parity, blocks, nblocks);
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
