// rsmi_heal_pair.cpp -- rsmi_heal_pair* (include/rsmi.h; see rsmi_impl.hpp for the file map):
// rewrite the one or two shards that break a stripe.  The call is rsmi_locate_pair's launch
// (launch_locate_pair, rsmi_pair.cpp) and, behind rs_locate_pair_verdict_kernel on the same
// stream, rs_heal_pair_kernel (rs_heal_pair_kernels.hip), which reads the two verdict words of
// every block and rewrites the rows they name; there is no host round trip in between.  Shapes
// without an rs_locate_kernel encode the data rows into scratch once more, chunk by chunk, and
// run the byte-granular rs_heal_pair_rows_kernel.  m = 2 names no pair: rs_heal_kernel runs on
// rsmi_locate's verdicts (launch_heal_named, rsmi_heal.cpp).  The host paths are Verify's
// (verify_host_impl) with a write-back leg of up to two rows per block.

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
int launch_heal_pair(rsmi_ctx* c, const Plan& plan, uint8_t* data, uint64_t data_rs, uint64_t data_bs, uint8_t* parity,
                     uint64_t parity_rs, uint64_t parity_bs, uint64_t S, uint64_t nblocks, int32_t* out, uint32_t* bad,
                     hipStream_t stream) {
    if (nblocks == 0 || S == 0) return RSMI_OK;
    PairLaunch pl;
    int rc = launch_locate_pair(c, plan, data, data_rs, data_bs, parity, parity_rs, parity_bs, S, nblocks, out, bad,
                                stream, &pl);
    if (rc) return rc;
    // m = 1: nothing is ever named.  m = 2: no pair is; rsmi_heal's launch on rsmi_locate's verdicts
    if (c->m == 1) return RSMI_OK;
    if (c->m == 2)
        return launch_heal_named(c, plan, pl.fused, data, data_rs, data_bs, parity, parity_rs, parity_bs, S, nblocks,
                                 pl.culprit, stream);
    if (pl.fused != StripeLayout::kNeither) {
        // the heal kernel of the layout rs_locate_kernel ran on
        const bool aligned = pl.fused == StripeLayout::kAligned;
        const DevTile& t = plan.tiles[0];
        void* fn = (aligned ? heal_pair_kernels().fn : heal_pair_kernels().ua)[t.K][t.MT];
        if (!fn) return RSMI_ERR_DEVICE;  // a pair kernel without its heal kernel: a build error
        std::shared_ptr<Plan> hp;
        if ((rc = heal_pair_plan(c, hp))) return rc;
        // launch_stripe_tiles' own split (a launch's tile count fits 32 bits), made here as
        // launch_locate_pair makes it: the verdicts are two words per block
        const uint64_t tpb = ((S + 15) / 16 + uint64_t(kWave) - 1) / uint64_t(kWave);
        const uint64_t max_blocks = std::max<uint64_t>(1, (uint64_t(1) << 31) / tpb);
        for (uint64_t b0 = 0; b0 < nblocks; b0 += max_blocks) {
            const uint64_t nb = std::min(max_blocks, nblocks - b0);
            rc = launch_stripe_tiles(c, fn, t, data + b0 * data_bs, data_rs, data_bs, parity + b0 * parity_bs, parity_rs,
                                     parity_bs, S, nb, nullptr, hp->tiles[0].dev, out + 2 * b0, stream);
            if (rc) return rc;
        }
        char buf[96];
        std::snprintf(buf, sizeof buf, "rs_heal_pair_kernel<K=%d,MT=%d>%s", t.K, t.MT, aligned ? "" : ",UA");
        set_last_kernel(c, buf);
        return hip_status(hipGetLastError());
    }
    // The fallback's scratch rows are gone (every 64 MiB chunk reuses them): the data rows are
    // encoded again, chunk by chunk, and each chunk healed before the next one's encode, as
    // rsmi_heal's fallback does.
    if ((rc = ensure_locate_tables(c))) return rc;
    rc = encode_into_scratch(
        c, plan, data, data_rs, data_bs, S, nblocks, stream,
        [&](uint64_t b0, uint64_t nb, const uint8_t* enc, uint64_t enc_rs, uint64_t enc_bs) -> int {
            uint8_t* datab = data + b0 * data_bs;
            uint8_t* parb = parity + b0 * parity_bs;
            uint32_t k32 = uint32_t(c->k), m32 = uint32_t(c->m);
            const int32_t* verdict = out + 2 * b0;
            const uint8_t* tbl = c->d_locate_tbl;
            const uint32_t gx = uint32_t(std::min<uint64_t>((S + kWG - 1) / kWG, 4096));
            const uint32_t gy = uint32_t(std::min<uint64_t>(nb, 65535));
            void* args[] = {&enc,  &enc_rs,    &enc_bs,    &datab, &data_rs, &data_bs, &parb, &parity_rs,
                            &parity_bs, &S, &k32,   &m32,     &nb,      &verdict, &tbl};
            HIP_TRY(hipLaunchKernel(heal_pair_rows_kernel(), dim3(gx, gy), dim3(kWG), args, 0, stream));
            return RSMI_OK;
        });
    if (rc) return rc;
    set_last_kernel(c, "rs_heal_pair_rows_kernel");
    return hip_status(hipGetLastError());
}

// Host-memory pair heal on Verify's host paths: locate_pair_host_impl's buffers (the context's
// device result buffer holds the flags, then two verdict words per block), and the write-back leg.
int heal_pair_host_impl(rsmi_ctx* c, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                        size_t parity_block_stride, size_t S, size_t nblocks, int32_t* pair_out, uint32_t* bad_out) {
    if (int rc = check_stripe_host_args(c, data, data_block_stride, parity, parity_block_stride, S, pair_out)) return rc;
    if (nblocks == 0) return RSMI_OK;
    const size_t k = size_t(c->k), m = size_t(c->m);
    const size_t flag_bytes = nblocks * m * sizeof(uint32_t), verdict_bytes = 2 * nblocks * sizeof(int32_t);
    // where the caller keeps row x of block b
    auto home = [&](size_t b, size_t x) -> uint8_t* {
        return x < k ? data + b * data_block_stride + x * S : parity + b * parity_block_stride + (x - k) * S;
    };
    uint32_t* d_bad = nullptr;
    int32_t* d_pair = nullptr;
    StripeCheck chk;
    chk.prepare = [&]() -> int {
        int rc = reserve(c->d_vbad, c->vbad_cap, flag_bytes + verdict_bytes);
        d_bad = reinterpret_cast<uint32_t*>(c->d_vbad);
        d_pair = reinterpret_cast<int32_t*>(d_bad + nblocks * m);
        return rc;
    };
    chk.launch = [&](const Plan& plan, const uint8_t* d, uint64_t d_rs, uint64_t d_bs, const uint8_t* p, uint64_t p_rs,
                     uint64_t p_bs, uint64_t nb, uint64_t b0, hipStream_t st) -> int {
        // the rows are the caller's own (in place) or the call's staging: writable either way
        return launch_heal_pair(c, plan, const_cast<uint8_t*>(d), d_rs, d_bs, const_cast<uint8_t*>(p), p_rs, p_bs, S,
                                nb, d_pair + 2 * b0, d_bad + b0 * m, st);
    };
    chk.fetch = [&](hipStream_t st) -> int {
        if (st) {
            HIP_TRY(hipMemcpyAsync(pair_out, d_pair, verdict_bytes, hipMemcpyDeviceToHost, st));
            if (bad_out) HIP_TRY(hipMemcpyAsync(bad_out, d_bad, flag_bytes, hipMemcpyDeviceToHost, st));
        } else {
            HIP_TRY(hipMemcpy(pair_out, d_pair, verdict_bytes, hipMemcpyDeviceToHost));
            if (bad_out) HIP_TRY(hipMemcpy(bad_out, d_bad, flag_bytes, hipMemcpyDeviceToHost));
        }
        return RSMI_OK;
    };
    // the small staged call: the verdicts are in pair_out, the healed rows in the staging
    chk.small_done = [&](const uint8_t* sd, const uint8_t* sp) -> int {
        for (size_t b = 0; b < nblocks; b++)
            for (int i = 0; i < 2; i++) {
                const int32_t v = pair_out[2 * b + i];
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
        HIP_TRY(hipMemcpyAsync(pair_out + 2 * b0, d_pair + 2 * b0, 2 * nb * sizeof(int32_t), hipMemcpyDeviceToHost,
                               st.stream));
        HIP_TRY(hipStreamSynchronize(st.stream));
        for (uint64_t b = 0; b < nb; b++)
            for (int i = 0; i < 2; i++) {
                const int32_t v = pair_out[2 * (b0 + b) + i];
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

int rsmi_heal_pair_batch_dev(rsmi_ctx* c, uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                             uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                             size_t nblocks, int32_t* d_pair_out, uint32_t* d_bad_out, void* stream) try {
    int rc = check_stripe_dev_args(c, d_data, data_shard_stride, d_parity, parity_shard_stride, S, d_pair_out);
    if (rc) return rc;
    if (nblocks == 0) return RSMI_OK;
    std::shared_ptr<Plan> plan;
    std::unique_lock<std::mutex> lock;
    if ((rc = begin_stripe_dev_call(c, lock, plan))) return rc;
    return launch_heal_pair(c, *plan, d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride,
                            parity_block_stride, S, nblocks, d_pair_out, d_bad_out, static_cast<hipStream_t>(stream));
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal_pair_batch_host(rsmi_ctx* c, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                              size_t parity_block_stride, size_t S, size_t nblocks, int32_t* pair_out,
                              uint32_t* bad_out) try {
    return heal_pair_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, pair_out, bad_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_heal_pair(rsmi_ctx* c, uint8_t* shards, size_t S, int pair_out[2]) try {
    if (!c || !shards || !pair_out) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    const size_t k = size_t(c->k), m = size_t(c->m);
    int32_t v[2] = {RSMI_LOCATE_UNKNOWN, RSMI_LOCATE_UNKNOWN};
    int rc = heal_pair_host_impl(c, shards, k * S, shards + k * S, m * S, S, 1, v, nullptr);
    if (rc) return rc;
    pair_out[0] = int(v[0]);
    pair_out[1] = int(v[1]);
    return RSMI_OK;
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
