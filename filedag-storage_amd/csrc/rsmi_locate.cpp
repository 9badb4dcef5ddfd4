// rsmi_locate.cpp -- rsmi_locate* (include/rsmi.h; see rsmi_impl.hpp for the file map): which
// shard breaks a stripe?  Verify's syndromes syn_j = encode(data)_j ^ stored parity_j name it: over
// the byte columns with a non-zero syndrome, data shard c explains the stripe iff
// syn_j == R[j][c] * syn_0 for every j >= 1 (R = rsmi_locate_matrix), parity shard j iff every
// other syndrome is zero.  rs_locate_kernel (rs_locate_kernels.hip) forms flags and candidates in
// one pass over the k + m rows; shapes it is not built for take Verify's launch for the flags,
// the encode into scratch and rs_locate_rows_kernel; rs_locate_verdict_kernel ends every launch.
// The host entries are verdicts_host_impl's (rsmi_verify.cpp), one verdict word per block.

#include "rsmi_impl.hpp"

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

namespace {

// R[j][c] = M[k+j][c] / M[k][c]; false when a first-row coefficient is zero (no MDS matrix has one)
bool locate_ratios(const rsmi_ctx* c, Matrix& R) {
    R = Matrix(c->m, c->k);
    for (int col = 0; col < c->k; col++) {
        const uint8_t d = c->M.at(c->k, col);
        if (!d) return false;
        for (int j = 0; j < c->m; j++) R.at(j, col) = gf().div(c->M.at(c->k + j, col), d);
    }
    return true;
}

}  // namespace

// the v_perm tables of R, laid out as the encode plan's (cached beside it).  Row 0 of R is all
// ones and no locate kernel reads its tables (locate_tile starts at row 1), so output slot 0
// carries inv(M[k][c]) instead, the factor rs_heal_kernel turns syn_0 into a data row's error with
int ratio_plan(rsmi_ctx* c, std::shared_ptr<Plan>& out) {
    auto it = c->plans.find("L");
    if (it != c->plans.end()) {
        out = it->second;
        return RSMI_OK;
    }
    Matrix R;
    if (!locate_ratios(c, R)) return RSMI_ERR_SINGULAR;
    for (int col = 0; col < c->k; col++) R.at(0, col) = gf().div(1, c->M.at(c->k, col));
    std::vector<int> in_rows(c->k), out_rows(c->m);
    for (int i = 0; i < c->k; i++) in_rows[i] = i;
    for (int j = 0; j < c->m; j++) out_rows[j] = j;
    int rc = make_plan(c, R, in_rows, out_rows, out);
    if (rc == RSMI_OK) c->plans["L"] = out;
    return rc;
}

// rs_locate_rows_kernel's tables: log[256] | exp[512] | R[m][k], and behind them
// rs_heal_rows_kernel's inv(M[k][c])[k]
int ensure_locate_tables(rsmi_ctx* c) {
    if (c->d_locate_tbl) return RSMI_OK;
    Matrix R;
    if (!locate_ratios(c, R)) return RSMI_ERR_SINGULAR;
    std::vector<uint8_t> h(768 + R.v.size() + size_t(c->k));
    std::memcpy(h.data(), gf().log.data(), 256);
    std::memcpy(h.data() + 256, gf().exp.data(), 512);
    std::memcpy(h.data() + 768, R.v.data(), R.v.size());
    for (int col = 0; col < c->k; col++) h[768 + R.v.size() + size_t(col)] = gf().div(1, c->M.at(c->k, col));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_locate_tbl), h.size()));
    HIP_TRY(hipMemcpy(c->d_locate_tbl, h.data(), h.size(), hipMemcpyHostToDevice));
    return RSMI_OK;
}

// Locate of nblocks blocks (caller holds ctx->mu, the device is bound): culprit[b] and, when bad
// is given, Verify's flags bad[b*m + j], both device memory.  Stream-ordered; the candidate words
// (and the flags, when the caller takes none) live in the stream's scratch.  fused (rsmi_heal.cpp):
// the layout rs_locate_kernel ran on (kNeither: m = 1 or the fallback).
int launch_locate(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* culprit, uint32_t* bad,
                  hipStream_t stream, StripeLayout* fused) {
    if (fused) *fused = StripeLayout::kNeither;
    const uint64_t nblocks = rows.nblocks;
    if (nblocks == 0 || rows.S == 0) return RSMI_OK;
    const uint64_t k = uint64_t(c->k), m = uint64_t(c->m);
    uint32_t n32 = uint32_t(c->n), m32 = uint32_t(m), words = (n32 + 31u) / 32u;
    const size_t cand_bytes = nblocks * words * sizeof(uint32_t);
    rsmi_ctx::VerifyScratch& ls = stream_scratch(c->locate_scratch, stream);
    int rc = reserve_on(ls.p, ls.cap, cand_bytes + (bad ? 0 : nblocks * m * sizeof(uint32_t)), stream);
    if (rc) return rc;
    uint32_t* cand = reinterpret_cast<uint32_t*>(ls.p);
    if (!bad) bad = cand + nblocks * words;

    if (m == 1) {
        // every shard explains any damage: the verdict follows from Verify's flag alone
        if ((rc = launch_verify(c, plan, rows, bad, stream))) return rc;
        cand = nullptr;
    } else {
        HIP_TRY(hipMemsetAsync(cand, 0xFF, cand_bytes, stream));
        // Verify's launch, with rs_locate_kernel in the place of rs_verify_kernel where the shape
        // has one (a one-tile plan, m <= 4: the ratio tables are one tile as well)
        LocateFuse loc;
        std::shared_ptr<Plan> rp;
        if (plan.tiles.size() == 1) {
            if ((rc = ratio_plan(c, rp))) return rc;
            loc.rplan = rp->tiles[0].dev;
            loc.cand = cand;
        }
        if ((rc = launch_verify(c, plan, rows, bad, stream, rp ? &loc : nullptr))) return rc;
        if (fused) *fused = loc.fused;
        if (loc.fused == StripeLayout::kNeither) {
            // m > 4, K > 16 or not instantiated, unaligned rows shorter than 16 bytes: Verify's
            // launch gave the flags; now the parity rows encoded into scratch (as Verify's own
            // fallback does) and the byte-granular kernel over the blocks whose flags are set.
            // The correctness path of rare shapes.
            if ((rc = ensure_locate_tables(c))) return rc;
            rc = encode_into_scratch(
                c, plan, rows, stream,
                [&](uint64_t b0, StripeRows r, const uint8_t* enc, uint64_t enc_rs, uint64_t enc_bs) -> int {
                    uint32_t k32 = uint32_t(k);
                    const uint32_t* badb = bad + b0 * m;
                    const uint8_t* tbl = c->d_locate_tbl;
                    uint32_t* candb = cand + b0 * words;
                    const uint32_t gx = uint32_t(std::min<uint64_t>((r.S + kWG - 1) / kWG, 4096));
                    const uint32_t gy = uint32_t(std::min<uint64_t>(r.nblocks, 65535));
                    void* args[] = {&enc, &enc_rs, &enc_bs,    &r.parity, &r.parity_rs, &r.parity_bs, &r.S,
                                    &k32, &m32,    &r.nblocks, &badb,     &tbl,         &candb};
                    HIP_TRY(hipLaunchKernel(locate_rows_kernel(), dim3(gx, gy), dim3(kWG), args, size_t(m * k),
                                            stream));
                    return RSMI_OK;
                });
            if (rc) return rc;
            set_last_kernel(c, "rs_locate_rows_kernel");
        }
    }
    const uint32_t* cbad = bad;
    const uint32_t* ccand = cand;
    uint64_t nbl = nblocks;
    void* args[] = {&cbad, &ccand, &m32, &n32, &words, &nbl, &culprit};
    HIP_TRY(hipLaunchKernel(locate_verdict_kernel(), dim3(uint32_t((nblocks + kWG - 1) / kWG)), dim3(kWG), args, 0,
                            stream));
    return hip_status(hipGetLastError());
}

namespace {

// the host entries' launch (verdicts_host_impl): one verdict word per block
int locate_launch(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* culprit, uint32_t* bad,
                  hipStream_t stream) {
    return launch_locate(c, plan, rows, culprit, bad, stream);
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_locate_batch_dev(rsmi_ctx* c, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                          const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                          size_t nblocks, int32_t* d_culprit_out, uint32_t* d_bad_out, void* stream) try {
    return stripe_dev_call(
        c, d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride, parity_block_stride, S, nblocks,
        d_culprit_out, [&](const Plan& plan, const StripeRows& rows) {
            return launch_locate(c, plan, rows, d_culprit_out, d_bad_out, static_cast<hipStream_t>(stream));
        });
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_locate_batch_host(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                           size_t parity_block_stride, size_t S, size_t nblocks, int32_t* culprit_out,
                           uint32_t* bad_out) try {
    return verdicts_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, 1, locate_launch,
                              culprit_out, bad_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_locate(rsmi_ctx* c, const uint8_t* shards, size_t S, int* culprit_out) try {
    return verdicts_one_block(c, shards, S, 1, locate_launch, culprit_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_locate_matrix(const rsmi_ctx* c, uint8_t* out) try {
    if (!c || !out) return RSMI_ERR_INVALID_ARG;
    Matrix R;
    if (!locate_ratios(c, R)) return RSMI_ERR_SINGULAR;
    std::memcpy(out, R.v.data(), R.v.size());
    return RSMI_OK;
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
