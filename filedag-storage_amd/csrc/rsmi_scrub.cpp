// rsmi_scrub.cpp -- rsmi_scrub* (include/rsmi.h; see rsmi_impl.hpp for the file map): the first
// pass of a scrub over stored stripes.  Both questions a scrub asks of every shard it reads, from
// one read of the k + m rows: Encoder.Verify's flags (do the shards belong together?) and R(shard)
// of the datanode entry checksum (is each shard the bytes that were stored?).
// rs_scrub_mfma_kernel (rs_scrub_kernels.hip) writes the flags and the units' CRC records, and
// rs_crc16_combine_mfma_kernel turns the records into R(row); shapes without a scrub kernel run
// Verify and the CRC-16 rows pass one after the other.  The host paths are verify_host_impl's, the
// raws the second output of stripe_results.

#include "rsmi_impl.hpp"

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

int launch_scrub(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, uint32_t* bad, uint32_t* raw,
                 hipStream_t stream) {
    const uint64_t S = rows.S, nblocks = rows.nblocks;
    if (nblocks == 0 || S == 0) return RSMI_OK;
    const uint64_t k = uint64_t(c->k), m = uint64_t(c->m), n = k + m;
    int rc;
    const StripeLayout layout = rows.layout();
    void* fn = plan.tiles.size() == 1 ? stripe_kernel(scrub_kernels(), layout, plan.tiles[0]) : nullptr;
    if (!fn) {
        // m > 4, a K without an rs_scrub_mfma_kernel, unaligned rows shorter than 16 bytes: the two
        // passes on this stream.  The correctness path of rare shapes.
        if ((rc = launch_verify(c, plan, rows, bad, stream))) return rc;
        HIP_TRY(hipMemsetAsync(raw, 0, nblocks * n * sizeof(uint32_t), stream));
        if ((rc = launch_crc(c, rows.data, rows.data_rs, rows.data_bs, uint32_t(k), S, nblocks, raw, n, stream, false)))
            return rc;
        return launch_crc(c, rows.parity, rows.parity_rs, rows.parity_bs, uint32_t(m), S, nblocks, raw + k, n, stream,
                          false);
    }
    if ((rc = ensure_crc_tables(c))) return rc;
    const DevTile& tile = plan.tiles[0];
    const FoldGeometry g(S, n);
    const uint64_t upb = g.upb, rec_per_block = g.rec_per_block;
    // the units' records, per stream (the host pipeline runs on three)
    rsmi_ctx::VerifyScratch& sc = stream_scratch(c->scrub_scratch, stream);
    if ((rc = reserve_on(sc.p, sc.cap, nblocks * rec_per_block, stream))) return rc;
    HIP_TRY(hipMemsetAsync(bad, 0, nblocks * m * sizeof(uint32_t), stream));
    const RsPlanDev* pd = tile.dev;
    uint32_t S32 = uint32_t(S), cpb32 = uint32_t(g.cpb), tpb32 = uint32_t(g.tpb), upb32 = uint32_t(upb), m32 = uint32_t(m);
    const uint32_t* ctb = c->d_crc_tbl;
    // launches of at most launch_units_max units (a workgroup each)
    const uint64_t max_blocks = std::max<uint64_t>(1, uint64_t(c->opt_launch_units_max) / upb);
    for (uint64_t b0 = 0; b0 < nblocks; b0 += max_blocks) {
        const uint64_t nb = std::min(max_blocks, nblocks - b0);
        uint32_t nunits = uint32_t(nb * upb);
        StripeRows r = rows.from(b0, nb);
        uint32_t* badb = bad + b0 * m;
        uint8_t* rb = sc.p + b0 * rec_per_block;
        void* args[] = {&pd,    &r.data, &r.parity, &r.data_bs, &r.data_rs, &r.parity_bs, &r.parity_rs, &S32,
                        &cpb32, &tpb32,  &upb32,    &nunits,    &badb,      &m32,         &ctb,         &rb};
        HIP_TRY(hipLaunchKernel(fn, dim3(nunits), dim3(kWG), args, 0, stream));  // a workgroup per unit
        c->split_launches.fetch_add(1, std::memory_order_relaxed);
    }
    // the records' combine, as behind rs_fused_mfma_kernel (launch_plan_crc)
    if ((rc = launch_fold_combine(c, sc.p, g, nblocks, raw, stream))) return rc;
    return tiles_launched(c, "scrub_mfma", layout, tile);
}

namespace {

// Host-memory scrub on verify_host_impl's paths: the flags and, beside them in ctx->d_vbad, the raws.
int scrub_host(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
               size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* bad_out, uint32_t* raw_out) {
    if (int rc = check_stripe_host_args(c, data, data_block_stride, parity, parity_block_stride, S,
                                        bad_out && raw_out ? bad_out : nullptr))
        return rc;
    if (nblocks == 0) return RSMI_OK;
    const size_t m = size_t(c->m), n = size_t(c->k) + m;
    StripeResults r;
    StripeCheck chk;
    stripe_results(c, nblocks, n, raw_out, bad_out, r, chk);
    chk.launch = [&](const Plan& plan, const StripeRows& rows, uint64_t b0, hipStream_t st) -> int {
        return launch_scrub(c, plan, rows, r.d_bad + b0 * m, r.d_words + b0 * n, st);
    };
    return verify_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, chk);
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_scrub_batch_dev(rsmi_ctx* c, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                         const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                         size_t nblocks, uint32_t* d_bad_out, uint32_t* d_raw_out, void* stream) try {
    return stripe_dev_call(
        c, d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride, parity_block_stride, S, nblocks,
        d_bad_out && d_raw_out ? d_bad_out : nullptr, [&](const Plan& plan, const StripeRows& rows) {
            return launch_scrub(c, plan, rows, d_bad_out, d_raw_out, static_cast<hipStream_t>(stream));
        });
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_scrub_batch_host(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                          size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* bad_out,
                          uint32_t* raw16_out) try {
    return scrub_host(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, bad_out, raw16_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_scrub(rsmi_ctx* c, const uint8_t* shards, size_t S, int* ok_out, uint32_t* raw_out) try {
    if (!c || !shards || !ok_out || !raw_out) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    const size_t k = size_t(c->k), m = size_t(c->m);
    std::vector<uint32_t> bad(m, 0), raw(k + m, 0);
    int rc = scrub_host(c, shards, k * S, shards + k * S, m * S, S, 1, bad.data(), raw.data());
    if (rc) return rc;
    *ok_out = std::all_of(bad.begin(), bad.end(), [](uint32_t x) { return x == 0; }) ? 1 : 0;
    std::copy(raw.begin(), raw.end(), raw_out);
    return RSMI_OK;
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
