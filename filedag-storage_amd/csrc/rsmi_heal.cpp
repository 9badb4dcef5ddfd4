// rsmi_heal.cpp -- rsmi_heal* (include/rsmi.h; see rsmi_impl.hpp for the file map): rewrite the
// shard that breaks a stripe.  The call is rsmi_locate's launch (launch_locate, rsmi_locate.cpp)
// and, behind rs_locate_verdict_kernel on the same stream, rs_heal_kernel (rs_heal_kernels.hip),
// which reads the verdicts and rewrites the named row of every block that has one; there is no
// host round trip in between.  Shapes without an rs_locate_kernel encode the data rows into
// scratch once more, chunk by chunk, and run the byte-granular rs_heal_rows_kernel.  The host
// paths are Verify's (verify_host_impl) with a write-back leg for the rewritten rows.

#include "rsmi_impl.hpp"

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

// The heal launch behind launch_locate's verdicts (caller holds ctx->mu, the device is bound; m >= 2):
// the named row of every block whose verdict culprit[b] names one, rewritten.  fused: the layout
// launch_locate reports.  rsmi_heal_pair (rsmi_heal_pair.cpp) runs it for m = 2, where no pair is
// ever named.
int launch_heal_named(rsmi_ctx* c, const Plan& plan, StripeLayout fused, uint8_t* data, uint64_t data_rs,
                      uint64_t data_bs, uint8_t* parity, uint64_t parity_rs, uint64_t parity_bs, uint64_t S,
                      uint64_t nblocks, int32_t* culprit, hipStream_t stream) {
    int rc = RSMI_OK;
    if (fused != StripeLayout::kNeither) {
        // the heal kernel of the layout rs_locate_kernel ran on
        const bool aligned = fused == StripeLayout::kAligned;
        const DevTile& t = plan.tiles[0];
        void* fn = (aligned ? heal_kernels().fn : heal_kernels().ua)[t.K][t.MT];
        if (!fn) return RSMI_ERR_DEVICE;  // a locate kernel without its heal kernel: a build error
        std::shared_ptr<Plan> rp;
        if ((rc = ratio_plan(c, rp))) return rc;
        // rs_heal_kernel takes rs_locate_kernel's arguments, the verdicts in the candidates' place
        rc = launch_stripe_tiles(c, fn, t, data, data_rs, data_bs, parity, parity_rs, parity_bs, S, nblocks, nullptr,
                                 rp->tiles[0].dev, culprit, stream);
        if (rc) return rc;
        char buf[96];
        std::snprintf(buf, sizeof buf, "rs_heal_kernel<K=%d,MT=%d>%s", t.K, t.MT, aligned ? "" : ",UA");
        set_last_kernel(c, buf);
        return hip_status(hipGetLastError());
    }
    // The fallback's scratch rows are gone (every 64 MiB chunk reuses them): the data rows are
    // encoded again, chunk by chunk, and each chunk healed before the next one's encode.  A
    // healed data row differs from the stored one only in blocks of earlier chunks.
    if ((rc = ensure_locate_tables(c))) return rc;
    rc = encode_into_scratch(
        c, plan, data, data_rs, data_bs, S, nblocks, stream,
        [&](uint64_t b0, uint64_t nb, const uint8_t* enc, uint64_t enc_rs, uint64_t enc_bs) -> int {
            uint8_t* datab = data + b0 * data_bs;
            uint8_t* parb = parity + b0 * parity_bs;
            uint32_t k32 = uint32_t(c->k), m32 = uint32_t(c->m);
            const int32_t* verdict = culprit + b0;
            const uint8_t* tbl = c->d_locate_tbl;
            const uint32_t gx = uint32_t(std::min<uint64_t>((S + kWG - 1) / kWG, 4096));
            const uint32_t gy = uint32_t(std::min<uint64_t>(nb, 65535));
            void* args[] = {&enc,  &enc_rs,    &enc_bs,    &datab, &data_rs, &data_bs, &parb, &parity_rs,
                            &parity_bs, &S, &k32,   &m32,     &nb,      &verdict, &tbl};
            HIP_TRY(hipLaunchKernel(heal_rows_kernel(), dim3(gx, gy), dim3(kWG), args, 0, stream));
            return RSMI_OK;
        });
    if (rc) return rc;
    set_last_kernel(c, "rs_heal_rows_kernel");
    return hip_status(hipGetLastError());
}

namespace {

// Heal of nblocks blocks (caller holds ctx->mu, the device is bound): launch_locate's outputs,
// then the heal launch, stream-ordered.  culprit is the caller's verdicts and the heal kernel's
// input at once.
int launch_heal(rsmi_ctx* c, const Plan& plan, uint8_t* data, uint64_t data_rs, uint64_t data_bs, uint8_t* parity,
                uint64_t parity_rs, uint64_t parity_bs, uint64_t S, uint64_t nblocks, int32_t* culprit, uint32_t* bad,
                hipStream_t stream) {
    if (nblocks == 0 || S == 0) return RSMI_OK;
    StripeLayout fused = StripeLayout::kNeither;
    int rc = launch_locate(c, plan, data, data_rs, data_bs, parity, parity_rs, parity_bs, S, nblocks, culprit, bad,
                           stream, &fused);
    if (rc) return rc;
    // every shard explains any damage: nothing is ever named, the launches were Verify's
    if (c->m == 1) return RSMI_OK;
    return launch_heal_named(c, plan, fused, data, data_rs, data_bs, parity, parity_rs, parity_bs, S, nblocks, culprit,
                             stream);
}

// Host-memory heal on Verify's host paths: locate_host_impl's buffers, and the write-back leg.
int heal_host_impl(rsmi_ctx* c, uint8_t* data, size_t data_block_stride, uint8_t* parity, size_t parity_block_stride,
                   size_t S, size_t nblocks, int32_t* culprit_out, uint32_t* bad_out) {
    if (int rc = check_stripe_host_args(c, data, data_block_stride, parity, parity_block_stride, S, culprit_out))
        return rc;
    if (nblocks == 0) return RSMI_OK;
    const size_t k = size_t(c->k), m = size_t(c->m);
    // where the caller keeps row x of block b
    auto home = [&](size_t b, size_t x) -> uint8_t* {
        return x < k ? data + b * data_block_stride + x * S : parity + b * parity_block_stride + (x - k) * S;
    };
    StripeResults r;
    StripeCheck chk;
    stripe_results(c, nblocks, culprit_out, bad_out, r, chk);
    chk.launch = [&](const Plan& plan, const uint8_t* d, uint64_t d_rs, uint64_t d_bs, const uint8_t* p, uint64_t p_rs,
                     uint64_t p_bs, uint64_t nb, uint64_t b0, hipStream_t st) -> int {
        // the rows are the caller's own (in place) or the call's staging: writable either way
        return launch_heal(c, plan, const_cast<uint8_t*>(d), d_rs, d_bs, const_cast<uint8_t*>(p), p_rs, p_bs, S, nb,
                           r.d_culprit + b0, r.d_bad + b0 * m, st);
    };
    // the small staged call: the verdicts are in culprit_out, the healed rows in the staging
    chk.small_done = [&](const uint8_t* sd, const uint8_t* sp) -> int {
        for (size_t b = 0; b < nblocks; b++) {
            const int32_t v = culprit_out[b];
            if (v < 0) continue;
            const size_t x = size_t(v);
            if (x < k && sd) std::memcpy(home(b, x), sd + (b * k + x) * S, S);
            if (x >= k && sp) std::memcpy(home(b, x), sp + (b * m + (x - k)) * S, S);
        }
        return RSMI_OK;
    };
    // the upload pipeline: a chunk's verdicts, then its healed rows from the device pitch to the
    // caller's, before the staging slot is filled again
    chk.chunk_done = [&](Staging& st, uint64_t b0, uint64_t nb, size_t Sp) -> int {
        HIP_TRY(hipMemcpyAsync(culprit_out + b0, r.d_culprit + b0, nb * sizeof(int32_t), hipMemcpyDeviceToHost,
                               st.stream));
        HIP_TRY(hipStreamSynchronize(st.stream));
        for (uint64_t b = 0; b < nb; b++) {
            const int32_t v = culprit_out[b0 + b];
            if (v < 0) continue;
            const size_t x = size_t(v);
            const uint8_t* src = x < k ? st.d_in + (b * k + x) * Sp : st.d_out + (b * m + (x - k)) * Sp;
            HIP_TRY(hipMemcpyAsync(home(b0 + b, x), src, S, hipMemcpyDeviceToHost, st.stream));
        }
        HIP_TRY(hipStreamSynchronize(st.stream));
        return RSMI_OK;
    };
    return verify_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, chk);
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_heal_batch_dev(rsmi_ctx* c, uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                        uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                        size_t nblocks, int32_t* d_culprit_out, uint32_t* d_bad_out, void* stream) try {
    int rc = check_stripe_dev_args(c, d_data, data_shard_stride, d_parity, parity_shard_stride, S, d_culprit_out);
    if (rc) return rc;
    if (nblocks == 0) return RSMI_OK;
    std::shared_ptr<Plan> plan;
    std::unique_lock<std::mutex> lock;
    if ((rc = begin_stripe_dev_call(c, lock, plan))) return rc;
    return launch_heal(c, *plan, d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride,
                       parity_block_stride, S, nblocks, d_culprit_out, d_bad_out, static_cast<hipStream_t>(stream));
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal_batch_host(rsmi_ctx* c, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                         size_t parity_block_stride, size_t S, size_t nblocks, int32_t* culprit_out,
                         uint32_t* bad_out) try {
    return heal_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, culprit_out, bad_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal(rsmi_ctx* c, uint8_t* shards, size_t S, int* culprit_out) try {
    if (!c || !shards || !culprit_out) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    const size_t k = size_t(c->k), m = size_t(c->m);
    int32_t v = RSMI_LOCATE_UNKNOWN;
    int rc = heal_host_impl(c, shards, k * S, shards + k * S, m * S, S, 1, &v, nullptr);
    if (rc) return rc;
    *culprit_out = int(v);
    return RSMI_OK;
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
