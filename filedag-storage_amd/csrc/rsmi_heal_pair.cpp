// rsmi_heal_pair.cpp -- rsmi_heal_pair* (include/rsmi.h; see rsmi_impl.hpp for the file map):
// rewrite the one or two shards that break a stripe.  The call is rsmi_locate_pair's launch
// (launch_locate_pair, rsmi_pair.cpp) and, behind rs_locate_pair_verdict_kernel on the same
// stream, rs_heal_pair_kernel (rs_heal_pair_kernels.hip), which reads the two verdict words of
// every block and rewrites the rows they name; there is no host round trip in between.  Shapes
// without an rs_locate_kernel encode the data rows into scratch once more, chunk by chunk, and
// run the byte-granular rs_heal_pair_rows_kernel (launch_heal_rows, rsmi_heal.cpp).  m = 2 names
// no pair: rs_heal_kernel runs on rsmi_locate's verdicts (launch_heal_named, rsmi_heal.cpp).  The
// host entries are verdicts_host_impl's (rsmi_verify.cpp) with the write-back leg, up to two rows
// per block.

#include "rsmi_impl.hpp"

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

namespace {

// rsmi_heal_pair_matrix in the form the kernels use it: columns l0, l1 of D and the four
// coefficients d = {D[0][l0], D[0][l1], D[1][l0], D[1][l1]}, every other entry of D being zero, for
// x < y (M: the parity part of the encode matrix, syn = M data ^ parity):
//   {k+i, k+j}   l0 = i, l1 = j: the errors are the two syndromes
//   {c, k+j}     l1 = j, l0 = 0 (1 when j = 0): e_c = syn_l0 / M[l0][c], e_{k+j} = syn_j ^ M[j][c] e_c
//   {c, d}       l0 = 0, l1 = 1: the inverse of the minor [M[0][c] M[0][d]; M[1][c] M[1][d]]
// y < 0, the single shard x, is rsmi_heal's update as the first row of a D whose second is zero:
// a parity row's own syndrome, a data row's syn_0 / M[0][x].  False when a coefficient that must
// not be zero is (no MDS matrix has one).
bool heal_pair_coefs(const rsmi_ctx* c, int x, int y, int& l0, int& l1, uint8_t (&d)[4]) {
    const int k = c->k;
    const GF256& g = gf();
    auto M = [&](int l, int col) { return c->M.at(k + l, col); };
    d[0] = d[1] = d[2] = d[3] = 0;
    if (y < 0) {
        l0 = l1 = x >= k ? x - k : 0;
        if (x < k && !M(0, x)) return false;
        d[0] = x >= k ? uint8_t(1) : g.div(1, M(0, x));
    } else if (x >= k) {
        l0 = x - k;
        l1 = y - k;
        d[0] = d[3] = 1;
    } else if (y >= k) {
        l1 = y - k;
        l0 = l1 == 0 ? 1 : 0;
        if (!M(l0, x)) return false;
        d[0] = g.div(1, M(l0, x));
        d[2] = g.mul(M(l1, x), d[0]);
        d[3] = 1;
    } else {
        l0 = 0;
        l1 = 1;
        const uint8_t a = M(0, x), b = M(0, y), cc = M(1, x), dd = M(1, y);
        const uint8_t det = uint8_t(g.mul(a, dd) ^ g.mul(b, cc));
        if (!det) return false;
        d[0] = g.div(dd, det);
        d[1] = g.div(b, det);
        d[2] = g.div(cc, det);
        d[3] = g.div(a, det);
    }
    return true;
}

// Plan "H", cached beside "L" and "P": one column per explanation of a block (rs_plan.hpp
// heal_pair_entry: the C(n, 2) pairs in the order of the pair words, then the n single shards),
// the four coefficients of heal_pair_coefs in the column's output slots and l0 | l1 << 8 in its
// in_row word.  n <= 20 where rs_heal_pair_kernel runs: 210 columns at the most.
int heal_pair_plan(rsmi_ctx* c, std::shared_ptr<Plan>& out) {
    auto it = c->plans.find("H");
    if (it != c->plans.end()) {
        out = it->second;
        return RSMI_OK;
    }
    const int n = c->n, ne = heal_pair_entries(n);
    if (ne > kMaxK) return RSMI_ERR_DEVICE;
    Matrix T(kMaxMT, ne);
    std::vector<int> in_rows(size_t(ne), 0), out_rows(kMaxMT, 0);
    auto put = [&](int x, int y) -> bool {
        int l0 = 0, l1 = 0;
        uint8_t d[4];
        if (!heal_pair_coefs(c, x, y, l0, l1, d)) return false;
        const int e = heal_pair_entry(n, x, y);
        for (int j = 0; j < 4; j++) T.at(j, e) = d[j];
        in_rows[size_t(e)] = l0 | (l1 << 8);
        return true;
    };
    for (int x = 0; x < n; x++) {
        if (!put(x, -1)) return RSMI_ERR_SINGULAR;
        for (int y = x + 1; y < n; y++)
            if (!put(x, y)) return RSMI_ERR_SINGULAR;
    }
    int rc = make_plan(c, T, in_rows, out_rows, out);
    if (rc == RSMI_OK) c->plans["H"] = out;
    return rc;
}

// Pair heal of nblocks blocks (caller holds ctx->mu, the device is bound): launch_locate_pair's
// outputs, then the heal launch, stream-ordered.  out is the caller's verdicts and the heal
// kernel's input at once.
int launch_heal_pair(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, int32_t* out, uint32_t* bad,
                     hipStream_t stream) {
    if (rows.nblocks == 0 || rows.S == 0) return RSMI_OK;
    PairLaunch pl;
    int rc = launch_locate_pair(c, plan, rows, out, bad, stream, &pl);
    if (rc) return rc;
    // m = 1: nothing is ever named.  m = 2: no pair is; rsmi_heal's launch on rsmi_locate's verdicts
    if (c->m == 1) return RSMI_OK;
    if (c->m == 2) return launch_heal_named(c, plan, pl.fused, rows, pl.culprit, stream);
    if (pl.fused != StripeLayout::kNeither) {
        // the heal kernel of the layout rs_locate_kernel ran on
        const DevTile& t = plan.tiles[0];
        void* fn = stripe_kernel(heal_pair_kernels(), pl.fused, t);
        if (!fn) return RSMI_ERR_DEVICE;  // a pair kernel without its heal kernel: a build error
        std::shared_ptr<Plan> hp;
        if ((rc = heal_pair_plan(c, hp))) return rc;
        // rs_heal_kernel's arguments, the verdicts two words per block
        if ((rc = launch_stripe_tiles(c, fn, t, rows, nullptr, 0, hp->tiles[0].dev, out, 2, stream))) return rc;
        return tiles_launched(c, "heal_pair", pl.fused, t);
    }
    // the fallback, as rsmi_heal's
    return launch_heal_rows(c, plan, heal_pair_rows_kernel(), "rs_heal_pair_rows_kernel", rows, out, 2, stream);
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_heal_pair_batch_dev(rsmi_ctx* c, uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                             uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                             size_t nblocks, int32_t* d_pair_out, uint32_t* d_bad_out, void* stream) try {
    return stripe_dev_call(
        c, d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride, parity_block_stride, S, nblocks,
        d_pair_out, [&](const Plan& plan, const StripeRows& rows) {
            return launch_heal_pair(c, plan, rows, d_pair_out, d_bad_out, static_cast<hipStream_t>(stream));
        });
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal_pair_batch_host(rsmi_ctx* c, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                              size_t parity_block_stride, size_t S, size_t nblocks, int32_t* pair_out,
                              uint32_t* bad_out) try {
    return verdicts_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, 2, launch_heal_pair,
                              pair_out, bad_out, data, parity);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal_pair(rsmi_ctx* c, uint8_t* shards, size_t S, int pair_out[2]) try {
    return verdicts_one_block(c, shards, S, 2, launch_heal_pair, pair_out, shards);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal_pair_matrix(const rsmi_ctx* c, int x, int y, uint8_t* out) try {
    if (!c || !out) return RSMI_ERR_INVALID_ARG;
    if (c->m < 2 || x == y || x < 0 || y < 0 || x >= c->n || y >= c->n) return RSMI_ERR_INVALID_ARG;
    const int m = c->m;
    int l0 = 0, l1 = 0;
    uint8_t d[4];
    if (!heal_pair_coefs(c, std::min(x, y), std::max(x, y), l0, l1, d)) return RSMI_ERR_SINGULAR;
    // row 0 is x's, row 1 y's, in the order the caller names them
    const int rx = x < y ? 0 : 1, ry = 1 - rx;
    std::memset(out, 0, size_t(2 * m));
    out[rx * m + l0] = d[0];
    out[rx * m + l1] = d[1];
    out[ry * m + l0] = d[2];
    out[ry * m + l1] = d[3];
    return RSMI_OK;
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
