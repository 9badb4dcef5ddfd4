// rsmi_heal.cpp -- rsmi_heal* (include/rsmi.h; see rsmi_impl.hpp for the file map): rewrite the
// shard that breaks a stripe.  The call is rsmi_locate's launch (launch_locate, rsmi_locate.cpp)
// and, behind rs_locate_verdict_kernel on the same stream, rs_heal_kernel (rs_heal_kernels.hip),
// which reads the verdicts and rewrites the named row of every block that has one; there is no
// host round trip in between.  Shapes without an rs_locate_kernel encode the data rows into
// scratch once more, chunk by chunk, and run the byte-granular rs_heal_rows_kernel
// (launch_heal_rows, which rsmi_heal_pair shares).  The host entries are verdicts_host_impl's
// (rsmi_verify.cpp) with the write-back leg for the rewritten rows.

#include "rsmi_impl.hpp"

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

// The fallback's scratch rows are gone (every 64 MiB chunk reuses them): the data rows are
// encoded again, chunk by chunk, and each chunk healed before the next one's encode.  A
// healed data row differs from the stored one only in blocks of earlier chunks.
int launch_heal_rows(rsmi_ctx* c, const Plan& plan, void* kernel, const char* label, const StripeRows& rows,
                     const int32_t* verdict, uint64_t W, hipStream_t stream) {
    int rc = ensure_locate_tables(c);
    if (rc) return rc;
    rc = encode_into_scratch(
        c, plan, rows, stream,
        [&](uint64_t b0, StripeRows r, const uint8_t* enc, uint64_t enc_rs, uint64_t enc_bs) -> int {
            // the rows are the caller's own (in place) or the call's staging: writable either way
            uint8_t* datab = const_cast<uint8_t*>(r.data);
            uint8_t* parb = const_cast<uint8_t*>(r.parity);
            uint32_t k32 = uint32_t(c->k), m32 = uint32_t(c->m);
            const int32_t* verdictb = verdict + W * b0;
            const uint8_t* tbl = c->d_locate_tbl;
            const uint32_t gx = uint32_t(std::min<uint64_t>((r.S + kWG - 1) / kWG, 4096));
            const uint32_t gy = uint32_t(std::min<uint64_t>(r.nblocks, 65535));
            void* args[] = {&enc,         &enc_rs, &enc_bs, &datab, &r.data_rs, &r.data_bs, &parb,     &r.parity_rs,
                            &r.parity_bs, &r.S,    &k32,    &m32,   &r.nblocks, &verdictb,  &tbl};
            HIP_TRY(hipLaunchKernel(kernel, dim3(gx, gy), dim3(kWG), args, 0, stream));
            return RSMI_OK;
        });
    if (rc) return rc;
    set_last_kernel(c, label);
    return hip_status(hipGetLastError());
}

// The heal launch behind launch_locate's verdicts (caller holds ctx->mu, the device is bound; m >= 2):
// the named row of every block whose verdict culprit[b] names one, rewritten.  fused: the layout
// launch_locate reports.  rsmi_heal_pair (rsmi_heal_pair.cpp) runs it for m = 2, where no pair is
// ever named.
int launch_heal_named(rsmi_ctx* c, const Plan& plan, StripeLayout fused, const StripeRows& rows, int32_t* culprit,
                      hipStream_t stream) {
    if (fused != StripeLayout::kNeither) {
        // the heal kernel of the layout rs_locate_kernel ran on
        const DevTile& t = plan.tiles[0];
        void* fn = stripe_kernel(heal_kernels(), fused, t);
        if (!fn) return RSMI_ERR_DEVICE;  // a locate kernel without its heal kernel: a build error
        std::shared_ptr<Plan> rp;
        int rc = ratio_plan(c, rp);
        if (rc) return rc;
        // rs_heal_kernel takes rs_locate_kernel's arguments, the verdicts in the candidates' place
        if ((rc = launch_stripe_tiles(c, fn, t, rows, nullptr, 0, rp->tiles[0].dev, culprit, 1, stream))) return rc;
        return tiles_launched(c, "heal", fused, t);
    }
    return launch_heal_rows(c, plan, heal_rows_kernel(), "rs_heal_rows_kernel", rows, culprit, 1, stream);
}

namespace {

// Heal of rows.nblocks blocks (caller holds ctx->mu, the device is bound): launch_locate's outputs,
// then the heal launch, stream-ordered.  culprit is the caller's verdicts and the heal kernel's
// input at once.
int launch_heal(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* culprit, uint32_t* bad,
                hipStream_t stream) {
    if (rows.nblocks == 0 || rows.S == 0) return RSMI_OK;
    StripeLayout fused = StripeLayout::kNeither;
    int rc = launch_locate(c, plan, rows, culprit, bad, stream, &fused);
    if (rc) return rc;
    // every shard explains any damage: nothing is ever named, the launches were Verify's
    if (c->m == 1) return RSMI_OK;
    return launch_heal_named(c, plan, fused, rows, culprit, stream);
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_heal_batch_dev(rsmi_ctx* c, uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                        uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                        size_t nblocks, int32_t* d_culprit_out, uint32_t* d_bad_out, void* stream) try {
    return stripe_dev_call(
        c, d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride, parity_block_stride, S, nblocks,
        d_culprit_out, [&](const Plan& plan, const StripeRows& rows) {
            return launch_heal(c, plan, rows, d_culprit_out, d_bad_out, static_cast<hipStream_t>(stream));
        });
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal_batch_host(rsmi_ctx* c, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                         size_t parity_block_stride, size_t S, size_t nblocks, int32_t* culprit_out,
                         uint32_t* bad_out) try {
    return verdicts_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, 1, launch_heal,
                              culprit_out, bad_out, data, parity);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal(rsmi_ctx* c, uint8_t* shards, size_t S, int* culprit_out) try {
    return verdicts_one_block(c, shards, S, 1, launch_heal, culprit_out, shards);
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
