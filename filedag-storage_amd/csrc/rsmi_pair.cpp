// rsmi_pair.cpp -- rsmi_locate_pair* (include/rsmi.h; see rsmi_impl.hpp for the file map): which
// two shards break a stripe?  The call is rsmi_locate's launch (launch_locate, rsmi_locate.cpp)
// with its verdicts in the stream's scratch and, behind rs_locate_verdict_kernel on the same
// stream, rs_locate_pair_kernel (rs_pair_kernels.hip), which tests every pair of shards against
// the syndromes of the blocks whose verdict is UNKNOWN; rs_locate_pair_verdict_kernel ends every
// call.  Shapes without an rs_locate_kernel encode the data rows into scratch once more, chunk by
// chunk, and run the byte-granular rs_locate_pair_rows_kernel.  m <= 2 names no pair: rsmi_locate's
// verdicts are widened to two words and nothing else is launched.  The host entries are
// verdicts_host_impl's (rsmi_verify.cpp), two verdict words per block.

#include "rsmi_impl.hpp"

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

namespace {

// rsmi_locate_pair_checks: the m - 2 rows C (m columns) with C h_x = C h_y = 0, in the form the
// kernels test them (R[l][c] = M[l][c] / M[0][c], the parity part M of the encode matrix):
//   {k+i, k+j}        for l other than i, j:      C = e_l
//   {c, k+j}, j >= 1  for l >= 1 other than j:    C = e_l + R[l][c] e_0
//   {c, k+0}          for l >= 2:                 C = e_l + (R[l][c] / R[1][c]) e_1
//   {c, d}            for l >= 2:                 C = e_l + g e_1 + (R[l][c] + g R[1][c]) e_0,
//                     g = q_l / q_1, q_l = M[l][d] + R[l][c] M[0][d]
// (+ is XOR).  False when a coefficient that must not be zero is (no MDS matrix has one).
bool pair_checks(const rsmi_ctx* c, int x, int y, Matrix& C) {
    const int k = c->k, m = c->m;
    const GF256& g = gf();
    if (x > y) std::swap(x, y);
    C = Matrix(std::max(0, m - 2), m);
    if (m <= 2) return true;
    auto M = [&](int l, int col) { return c->M.at(k + l, col); };
    auto R = [&](int l, int col) { return g.div(M(l, col), M(0, col)); };
    for (int col : {x, y})
        if (col < k && (!M(0, col) || !M(1, col))) return false;
    int r = 0;
    if (x >= k) {
        for (int l = 0; l < m; l++)
            if (l != x - k && l != y - k) C.at(r++, l) = 1;
    } else if (y >= k && y - k >= 1) {
        for (int l = 1; l < m; l++)
            if (l != y - k) {
                C.at(r, l) = 1;
                C.at(r++, 0) = R(l, x);
            }
    } else if (y >= k) {
        for (int l = 2; l < m; l++) {
            C.at(r, l) = 1;
            C.at(r++, 1) = g.div(R(l, x), R(1, x));
        }
    } else {
        auto q = [&](int l) { return uint8_t(M(l, y) ^ g.mul(R(l, x), M(0, y))); };
        if (!q(1)) return false;
        for (int l = 2; l < m; l++) {
            const uint8_t gl = g.div(q(l), q(1));
            C.at(r, l) = 1;
            C.at(r, 1) = gl;
            C.at(r++, 0) = uint8_t(R(l, x) ^ g.mul(gl, R(1, x)));
        }
    }
    return r == m - 2;
}

// Plan "P", cached beside "L": rs_locate_pair_kernel's tables behind the encode plan's.  Columns
// 0 .. k-1 are plan "L"'s (the ratios, inv(M[k][c]) in output slot 0); the pair columns follow,
// four coefficients to a column, in the order of the kernel's tests (rs_plan.hpp pair_tests): per
// data shard c the test of {c, k+0}, then of {c, d} for d > c, each with the coefficients of e_1
// in its m - 2 check rows.
int pair_plan(rsmi_ctx* c, std::shared_ptr<Plan>& out) {
    auto it = c->plans.find("P");
    if (it != c->plans.end()) {
        out = it->second;
        return RSMI_OK;
    }
    const int k = c->k, m = c->m, nc = m - 2;
    const int np = pair_blocks(k, m);
    Matrix T(kMaxMT, k + np);
    for (int col = 0; col < k; col++) {
        const uint8_t d = c->M.at(k, col);
        if (!d) return RSMI_ERR_SINGULAR;
        T.at(0, col) = gf().div(1, d);
        for (int j = 1; j < m; j++) T.at(j, col) = gf().div(c->M.at(k + j, col), d);
    }
    int e = 0;  // the coefficient's number: output slot e % 4 of pair column e / 4
    Matrix C;
    for (int x = 0; x < k; x++)
        for (int y = x; y < k; y++) {
            // y == x stands for the parity shard k + 0
            if (!pair_checks(c, x, y == x ? k : y, C)) return RSMI_ERR_SINGULAR;
            for (int i = 0; i < nc; i++, e++) T.at(e % 4, k + e / 4) = C.at(i, 1);
        }
    std::vector<int> in_rows(size_t(k + np), 0), out_rows(kMaxMT, 0);
    for (int i = 0; i < k; i++) in_rows[size_t(i)] = i;
    int rc = make_plan(c, T, in_rows, out_rows, out);
    if (rc == RSMI_OK) c->plans["P"] = out;
    return rc;
}

int launch_pair_verdict(const int32_t* culprit, const uint32_t* pairw, uint32_t n, uint32_t words, uint64_t nblocks,
                        int32_t* out, hipStream_t stream) {
    void* args[] = {&culprit, &pairw, &n, &words, &nblocks, &out};
    HIP_TRY(hipLaunchKernel(pair_verdict_kernel(), dim3(uint32_t((nblocks + kWG - 1) / kWG)), dim3(kWG), args, 0,
                            stream));
    return RSMI_OK;
}

}  // namespace

// Pair locate of nblocks blocks (caller holds ctx->mu, the device is bound): out[2b], out[2b+1]
// and, when bad is given, Verify's flags, device memory.  Stream-ordered.  The stream's
// locate_scratch holds, behind launch_locate's candidate words, rsmi_locate's verdicts, the pair
// words and (when the caller takes none) the flags.  info (rsmi_heal_pair.cpp): the layout
// rs_locate_kernel ran on and where rsmi_locate's verdicts lie.
int launch_locate_pair(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* out, uint32_t* bad,
                       hipStream_t stream, PairLaunch* info) {
    if (info) *info = PairLaunch{};
    const uint64_t nblocks = rows.nblocks;
    if (nblocks == 0 || rows.S == 0) return RSMI_OK;
    const uint64_t m = uint64_t(c->m);
    const uint32_t n32 = uint32_t(c->n);
    // a shape rs_locate_kernel may run on has pair words (n <= 20); the fallback needs none
    const bool tiled = plan.tiles.size() == 1 && c->m >= 3 && c->m <= kMaxMT && c->k <= 16;
    const uint32_t words = tiled ? uint32_t(pair_words(c->n)) : 0u;
    const size_t cand_bytes = round_up(nblocks * ((n32 + 31u) / 32u) * sizeof(uint32_t), 16);
    const size_t verdict_bytes = round_up(nblocks * sizeof(int32_t), 16);
    const size_t pair_bytes = nblocks * words * sizeof(uint32_t);
    rsmi_ctx::VerifyScratch& ls = stream_scratch(c->locate_scratch, stream);
    int rc = reserve_on(ls.p, ls.cap,
                        cand_bytes + verdict_bytes + pair_bytes + (bad ? 0 : nblocks * m * sizeof(uint32_t)), stream);
    if (rc) return rc;
    int32_t* culprit = reinterpret_cast<int32_t*>(ls.p + cand_bytes);
    uint32_t* pairw = reinterpret_cast<uint32_t*>(ls.p + cand_bytes + verdict_bytes);
    if (!bad) bad = pairw + nblocks * words;

    StripeLayout fused = StripeLayout::kNeither;
    if ((rc = launch_locate(c, plan, rows, culprit, bad, stream, &fused))) return rc;
    if (info) {
        info->fused = fused;
        info->culprit = culprit;
    }
    // every pair explains everything: rsmi_locate's verdicts, widened
    if (c->m <= 2) {
        if ((rc = launch_pair_verdict(culprit, nullptr, n32, 0, nblocks, out, stream))) return rc;
        return hip_status(hipGetLastError());
    }
    if (fused != StripeLayout::kNeither) {
        const DevTile& t = plan.tiles[0];
        void* fn = stripe_kernel(pair_kernels(), fused, t);
        if (!fn || !words) return RSMI_ERR_DEVICE;  // a locate kernel without its pair kernel: a build error
        std::shared_ptr<Plan> pp;
        if ((rc = pair_plan(c, pp))) return rc;
        HIP_TRY(hipMemsetAsync(pairw, 0xFF, pair_bytes, stream));
        // the pair words in the flags' place, rsmi_locate's verdicts in the candidates'
        if ((rc = launch_stripe_tiles(c, fn, t, rows, pairw, words, pp->tiles[0].dev, culprit, 1, stream))) return rc;
        if ((rc = launch_pair_verdict(culprit, pairw, n32, words, nblocks, out, stream))) return rc;
        return tiles_launched(c, "locate_pair", fused, t);
    }
    // The fallback's scratch rows are gone (every 64 MiB chunk reuses them): the verdicts are
    // widened, then the data rows are encoded again, chunk by chunk, and each chunk's UNKNOWN
    // blocks tested before the next one's encode.
    if ((rc = launch_pair_verdict(culprit, nullptr, n32, 0, nblocks, out, stream))) return rc;
    if ((rc = ensure_locate_tables(c))) return rc;
    rc = encode_into_scratch(
        c, plan, rows, stream,
        [&](uint64_t b0, StripeRows r, const uint8_t* enc, uint64_t enc_rs, uint64_t enc_bs) -> int {
            uint32_t k32 = uint32_t(c->k), m32 = uint32_t(c->m);
            const int32_t* verdict = culprit + b0;
            const uint8_t* tbl = c->d_locate_tbl;
            int32_t* outb = out + 2 * b0;
            const uint32_t gx = uint32_t(std::min<uint64_t>(r.nblocks, 65535));
            void* args[] = {&enc, &enc_rs, &enc_bs,    &r.parity, &r.parity_rs, &r.parity_bs, &r.S,
                            &k32, &m32,    &r.nblocks, &verdict,  &tbl,         &outb};
            HIP_TRY(hipLaunchKernel(pair_rows_kernel(), dim3(gx), dim3(kWG), args, size_t(m32) * k32, stream));
            return RSMI_OK;
        });
    if (rc) return rc;
    set_last_kernel(c, "rs_locate_pair_rows_kernel");
    return hip_status(hipGetLastError());
}

namespace {

// the host entries' launch (verdicts_host_impl): two verdict words per block
int locate_pair_launch(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* out, uint32_t* bad,
                       hipStream_t stream) {
    return launch_locate_pair(c, plan, rows, out, bad, stream);
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_locate_pair_batch_dev(rsmi_ctx* c, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                               const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride,
                               size_t S, size_t nblocks, int32_t* d_pair_out, uint32_t* d_bad_out, void* stream) try {
    return stripe_dev_call(
        c, d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride, parity_block_stride, S, nblocks,
        d_pair_out, [&](const Plan& plan, const StripeRows& rows) {
            return launch_locate_pair(c, plan, rows, d_pair_out, d_bad_out, static_cast<hipStream_t>(stream));
        });
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_locate_pair_batch_host(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                                size_t parity_block_stride, size_t S, size_t nblocks, int32_t* pair_out,
                                uint32_t* bad_out) try {
    return verdicts_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, 2,
                              locate_pair_launch, pair_out, bad_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_locate_pair(rsmi_ctx* c, const uint8_t* shards, size_t S, int pair_out[2]) try {
    return verdicts_one_block(c, shards, S, 2, locate_pair_launch, pair_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_locate_pair_checks(const rsmi_ctx* c, int x, int y, uint8_t* out) try {
    if (!c || !out) return RSMI_ERR_INVALID_ARG;
    if (x == y || x < 0 || y < 0 || x >= c->n || y >= c->n) return RSMI_ERR_INVALID_ARG;
    Matrix C;
    if (!pair_checks(c, x, y, C)) return RSMI_ERR_SINGULAR;
    if (!C.v.empty()) std::memcpy(out, C.v.data(), C.v.size());
    return RSMI_OK;
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
