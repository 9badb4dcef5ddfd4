// rsmi_verify.cpp -- Encoder.Verify (include/rsmi.h rsmi_verify*; see rsmi_impl.hpp for the file
// map): do the k + m shards of a block belong together, that is, is every stored parity row what
// the encode of the data rows produces?  The check reads k + m rows and writes only flags:
// rs_verify_kernel (rs_verify_kernels.hip) over the tiles of the cached encode plan, or, for
// shapes it is not built for, the encode into scratch followed by rs_compare_rows_kernel.
// rsmi_locate (rsmi_locate.cpp) shares the launch (launch_verify with a LocateFuse).  What the six
// calls over stored stripes share lives here as well: StripeRows::layout, stripe_kernel and
// tiles_launched, launch_stripe_tiles, encode_into_scratch, the host paths (verify_host_impl with
// each call's StripeCheck), stripe_results and stripe_write_back, the verdict calls' host entries
// (verdicts_host_impl, verdicts_one_block), the entry points' argument checks and
// begin_stripe_dev_call.

#include "rsmi_impl.hpp"

#include <limits>

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

rsmi_ctx::VerifyScratch& stream_scratch(std::map<hipStream_t, rsmi_ctx::VerifyScratch>& map, hipStream_t st) {
    auto it = map.find(st);
    if (it != map.end()) return it->second;
    if (map.size() >= 32) {
        (void)hipDeviceSynchronize();
        for (auto& e : map)
            if (e.second.p) (void)hipFree(e.second.p);
        map.clear();
    }
    return map[st];
}

int launch_stripe_tiles(rsmi_ctx* c, void* fn, const DevTile& t, const StripeRows& rows, uint32_t* bad,
                        uint64_t bad_wpb, const RsPlanDev* rplan, void* words, uint64_t words_wpb, hipStream_t stream) {
    const uint64_t S = rows.S, nblocks = rows.nblocks;
    const uint64_t cpb = (S + 15) / 16;
    const uint64_t tpb = (cpb + uint64_t(kWave) - 1) / uint64_t(kWave);
    constexpr int wpg = kFastWG / kWave;
    long wg_cap = std::numeric_limits<long>::max();
    if (c->opt_waves_per_cu > 0) wg_cap = std::max(1L, long(c->num_cu) * c->opt_waves_per_cu / wpg);
    // split into launches whose tile count stays within option launch_units_max
    const uint64_t max_blocks = std::max<uint64_t>(1, uint64_t(c->opt_launch_units_max) / tpb);
    for (uint64_t b0 = 0; b0 < nblocks; b0 += max_blocks) {
        const uint64_t nb = std::min(max_blocks, nblocks - b0);
        uint32_t ntiles = uint32_t(nb * tpb);
        uint32_t S32 = uint32_t(S), cpb32 = uint32_t(cpb), tpb32 = uint32_t(tpb), m32 = uint32_t(c->m);
        const RsPlanDev* pd = t.dev;
        StripeRows r = rows.from(b0, nb);
        uint32_t* badb = bad ? bad + b0 * bad_wpb : nullptr;
        void* wordsb = words ? static_cast<uint8_t*>(words) + b0 * words_wpb * sizeof(uint32_t) : nullptr;
        // rs_locate_kernel's and rs_heal_kernel's parameters are rs_verify_kernel's and these two more
        void* args[] = {&pd,    &r.data, &r.parity, &r.data_bs, &r.data_rs, &r.parity_bs, &r.parity_rs, &S32,
                        &cpb32, &tpb32,  &ntiles,   &badb,      &m32,       &rplan,       &wordsb};
        const uint64_t wgs = std::min<uint64_t>((ntiles + wpg - 1) / wpg, uint64_t(wg_cap));
        HIP_TRY(hipLaunchKernel(fn, dim3(uint32_t(wgs)), dim3(uint32_t(wpg * kWave)), args, 0, stream));
        c->split_launches.fetch_add(1, std::memory_order_relaxed);
    }
    return RSMI_OK;
}

// the alignment test of launch_plan, the stored parity rows in the place of the output rows
StripeLayout StripeRows::layout() const {
    const bool aligned = reinterpret_cast<uintptr_t>(data) % 16 == 0 && reinterpret_cast<uintptr_t>(parity) % 16 == 0 &&
                         data_rs % 16 == 0 && data_bs % 16 == 0 && parity_rs % 16 == 0 && parity_bs % 16 == 0 &&
                         data_rs >= round_up(S, 16) && parity_rs >= round_up(S, 16) && S < (uint64_t(1) << 31);
    const bool ua = !aligned && S >= 16 && S < (uint64_t(1) << 31) && data_rs >= S && parity_rs >= S;
    return aligned ? StripeLayout::kAligned : ua ? StripeLayout::kUA : StripeLayout::kNeither;
}

void* stripe_kernel(const StripeKernelTable& table, StripeLayout layout, const DevTile& t) {
    if (layout == StripeLayout::kNeither || t.K > 16) return nullptr;
    return (layout == StripeLayout::kAligned ? table.fn : table.ua)[t.K][t.MT];
}

int tiles_launched(rsmi_ctx* c, const char* name, StripeLayout layout, const DevTile& t) {
    char buf[96];
    std::snprintf(buf, sizeof buf, "rs_%s_kernel<K=%d,MT=%d>%s", name, t.K, t.MT,
                  layout == StripeLayout::kUA ? ",UA" : "");
    set_last_kernel(c, buf);
    return hip_status(hipGetLastError());
}

int encode_into_scratch(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, hipStream_t stream,
                        const ScratchRowsFn& fn) {
    const uint64_t m = uint64_t(c->m);
    const uint64_t Sp = round_up(rows.S, 16);
    const uint64_t chunk = std::max<uint64_t>(1, (uint64_t(64) << 20) / (m * Sp));
    rsmi_ctx::VerifyScratch& vs = stream_scratch(c->verify_scratch, stream);
    int rc = reserve_on(vs.p, vs.cap, std::min(chunk, rows.nblocks) * m * Sp, stream);
    if (rc) return rc;
    for (uint64_t b0 = 0; b0 < rows.nblocks; b0 += chunk) {
        const StripeRows sub = rows.from(b0, std::min(chunk, rows.nblocks - b0));
        rc = launch_plan(c, plan, sub.data, sub.data_rs, sub.data_bs, vs.p, Sp, m * Sp, sub.S, sub.nblocks, stream);
        if (rc) return rc;
        if ((rc = fn(b0, sub, vs.p, Sp, m * Sp))) return rc;
    }
    return RSMI_OK;
}

int launch_verify(rsmi_ctx* c, const Plan& plan, const StripeRows& rows, uint32_t* bad, hipStream_t stream,
                  LocateFuse* loc) {
    if (loc) loc->fused = StripeLayout::kNeither;
    if (rows.nblocks == 0 || rows.S == 0) return RSMI_OK;
    const uint64_t m = uint64_t(c->m);
    HIP_TRY(hipMemsetAsync(bad, 0, rows.nblocks * m * sizeof(uint32_t), stream));
    const StripeLayout layout = rows.layout();
    bool fast = true;
    for (const DevTile& t : plan.tiles)
        if (!stripe_kernel(verify_kernels(), layout, t)) fast = false;
    if (fast) {
        // rsmi_locate: a one-tile plan whose shape has an rs_locate_kernel (2 <= m <= 4) runs it in
        // the place of rs_verify_kernel, the same launch with the candidates formed as well
        void* lfn = loc && plan.tiles.size() == 1 ? stripe_kernel(locate_kernels(), layout, plan.tiles[0]) : nullptr;
        for (const DevTile& t : plan.tiles) {
            void* fn = lfn ? lfn : stripe_kernel(verify_kernels(), layout, t);
            int rc = launch_stripe_tiles(c, fn, t, rows, bad, m, lfn ? loc->rplan : nullptr,
                                         lfn ? loc->cand : nullptr, 1, stream);
            if (rc) return rc;
        }
        if (lfn) loc->fused = layout;
        return tiles_launched(c, lfn ? "locate" : "verify", layout, plan.tiles.back());
    }
    // Shapes without an rs_verify_kernel (K > 16 or not instantiated, unaligned rows shorter than
    // 16 bytes): the parity rows are encoded into scratch and compared with the stored ones.  The
    // correctness path of rare shapes.
    int rc = encode_into_scratch(
        c, plan, rows, stream,
        [&](uint64_t b0, StripeRows r, const uint8_t* enc, uint64_t enc_rs, uint64_t enc_bs) -> int {
            uint32_t m32 = uint32_t(m);
            uint32_t* badb = bad + b0 * m;
            const uint64_t groups = (r.S + 3) / 4;
            const uint32_t gx = uint32_t(std::min<uint64_t>((groups + kWG - 1) / kWG, 4096));
            const uint32_t gy = uint32_t(std::min<uint64_t>(r.nblocks, 65535));
            void* args[] = {&enc, &enc_rs, &enc_bs, &r.parity, &r.parity_rs, &r.parity_bs, &r.S, &m32, &r.nblocks,
                            &badb};
            HIP_TRY(hipLaunchKernel(compare_rows_kernel(), dim3(gx, gy), dim3(kWG), args, 0, stream));
            return RSMI_OK;
        });
    if (rc) return rc;
    set_last_kernel(c, "rs_compare_rows_kernel");
    return hip_status(hipGetLastError());
}

// The host paths of every call over stored stripes, which differ in chk alone (arguments
// already checked, nblocks > 0).  Page-locked data and parity (and option
// zero_copy): one kernel reads them in place over PCIe, rows at pitch S.  Small pageable calls:
// the same kernel over the context's page-locked staging, filled by CPU copies (the rule of
// encode_small).  Everything else: chunks of about 64 MiB of device rows round-robin over the
// staging streams, so a chunk's upload runs while the chunk before it is checked; rows at
// rsmi_recommended_pitch(S) for the aligned kernel, as the host encode stages them.  The calls
// that only read have no write-back leg: only the results return, in one copy at the end.  The
// healers' (chk.small_done, chk.chunk_done: stripe_write_back) returns the rows they rewrote and
// nothing else.
int verify_host_impl(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                     size_t parity_block_stride, size_t S, size_t nblocks, const StripeCheck& chk) {
    std::lock_guard<std::mutex> g(c->mu);
    int rc = ensure_device(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::shared_ptr<Plan> plan;
    rc = encode_plan(c, plan);
    if (rc) return rc;
    const size_t k = size_t(c->k), m = size_t(c->m);
    if ((rc = chk.prepare())) return rc;

    const size_t total = nblocks * (k + m) * S;
    const size_t data_len = (nblocks - 1) * data_block_stride + k * S;
    const size_t parity_len = (nblocks - 1) * parity_block_stride + m * S;
    const uint8_t* zd = host_alias(const_cast<uint8_t*>(data), data_len);
    const uint8_t* zp = host_alias(const_cast<uint8_t*>(parity), parity_len);
    const bool pinned = zd && zp;
    if ((c->opt_zero_copy && pinned) ||
        (total <= size_t(c->opt_small_bytes) && (2 * total <= size_t(c->opt_small_bytes) || zd))) {
        hipStream_t st = c->staging[0].stream;
        size_t dbs = data_block_stride, pbs = parity_block_stride;
        const size_t in_sz = zd ? 0 : nblocks * k * S, par_sz = zp ? 0 : nblocks * m * S;
        if (in_sz + par_sz) {
            uint8_t* hs = small_stage(c, in_sz + par_sz);
            if (!hs) return RSMI_ERR_DEVICE;
            if (!zd) {
                for (size_t b = 0; b < nblocks; b++) std::memcpy(hs + b * k * S, data + b * data_block_stride, k * S);
                zd = host_alias(hs, in_sz);
                dbs = k * S;
            }
            if (!zp) {
                for (size_t b = 0; b < nblocks; b++)
                    std::memcpy(hs + in_sz + b * m * S, parity + b * parity_block_stride, m * S);
                zp = host_alias(hs + in_sz, par_sz);
                pbs = m * S;
            }
            if (!zd || !zp) return RSMI_ERR_DEVICE;
        }
        if ((rc = chk.launch(*plan, StripeRows{zd, S, dbs, zp, S, pbs, S, nblocks}, 0, st))) return rc;
        if ((rc = chk.fetch(st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        if (chk.small_done && in_sz + par_sz) {
            const uint8_t* hs = c->h_small;
            return chk.small_done(in_sz ? hs : nullptr, par_sz ? hs + in_sz : nullptr);
        }
        return RSMI_OK;
    }

    const size_t Sp = rsmi_recommended_pitch(S);
    const size_t in_bs = k * Sp, par_bs = m * Sp;
    const bool d2 = dma_2d_ok(S);
    const size_t chunk = std::max<size_t>(1, (size_t(64) << 20) / (in_bs + par_bs));
    const int ns = nblocks > chunk ? 3 : 1;
    // odd S: the PCIe copies stay linear (d_lin, data rows then parity rows in stream order) and
    // rs_repitch_kernel lays the rows out at the device pitch (rsmi_host.cpp)
    auto upload = [&](Staging& st, uint8_t* dst, size_t dst_bs, const uint8_t* src, size_t src_bs, size_t rows,
                      size_t nb) -> int {
        if (d2 && src_bs == rows * S) {
            HIP_TRY(hipMemcpy2DAsync(dst, Sp, src, S, S, nb * rows, hipMemcpyHostToDevice, st.stream));
        } else if (d2) {
            for (size_t b = 0; b < nb; b++)
                HIP_TRY(hipMemcpy2DAsync(dst + b * dst_bs, Sp, src + b * src_bs, S, S, rows, hipMemcpyHostToDevice,
                                         st.stream));
        } else {
            if (src_bs == rows * S)
                HIP_TRY(hipMemcpyAsync(st.d_lin, src, nb * rows * S, hipMemcpyHostToDevice, st.stream));
            else
                for (size_t b = 0; b < nb; b++)
                    HIP_TRY(hipMemcpyAsync(st.d_lin + b * rows * S, src + b * src_bs, rows * S, hipMemcpyHostToDevice,
                                           st.stream));
            return repitch(dst, Sp, st.d_lin, S, S, nb * rows, st.stream);
        }
        return RSMI_OK;
    };
    // the write-back leg (rsmi_heal): the chunk a staging slot holds is owed its chunk_done before
    // the slot's rows are reused, the last chunks at the end
    struct Owed {
        size_t b0 = 0, nb = 0;
    } owed[3];
    auto settle = [&](int s) -> int {
        const Owed o = owed[s];
        owed[s] = Owed{};
        return chk.chunk_done && o.nb ? chk.chunk_done(c->staging[s], o.b0, o.nb, Sp) : RSMI_OK;
    };
    for (size_t b0 = 0, i = 0; b0 < nblocks; b0 += chunk, i++) {
        Staging& st = c->staging[i % ns];
        const size_t nb = std::min(chunk, nblocks - b0);
        if ((rc = settle(int(i % ns)))) return rc;
        owed[i % ns].b0 = b0;
        owed[i % ns].nb = nb;
        if ((rc = reserve_on(st.d_in, st.in_cap, nb * in_bs, st.stream))) return rc;
        if ((rc = reserve_on(st.d_out, st.out_cap, nb * par_bs, st.stream))) return rc;
        if (!d2 && (rc = reserve_on(st.d_lin, st.lin_cap, nb * std::max(k, m) * S, st.stream))) return rc;
        if ((rc = upload(st, st.d_in, in_bs, data + b0 * data_block_stride, data_block_stride, k, nb))) return rc;
        if ((rc = upload(st, st.d_out, par_bs, parity + b0 * parity_block_stride, parity_block_stride, m, nb)))
            return rc;
        if ((rc = chk.launch(*plan, StripeRows{st.d_in, Sp, in_bs, st.d_out, Sp, par_bs, S, nb}, b0, st.stream)))
            return rc;
    }
    for (int s = 0; s < ns; s++)
        if ((rc = settle(s))) return rc;
    for (int s = 0; s < ns; s++) HIP_TRY(hipStreamSynchronize(c->staging[s].stream));
    return chk.fetch(nullptr);
}

// The results live in device memory on every path (no atomics aimed at host memory); every host
// call synchronises before it returns, so one buffer serves them all.
void stripe_results(rsmi_ctx* c, size_t nblocks, size_t W, void* words_out, uint32_t* bad_out, StripeResults& r,
                    StripeCheck& chk) {
    const size_t flag_bytes = nblocks * size_t(c->m) * sizeof(uint32_t);
    const size_t word_bytes = nblocks * W * sizeof(uint32_t);
    chk.prepare = [=, &r]() -> int {
        int rc = reserve(c->d_vbad, c->vbad_cap, flag_bytes + word_bytes);
        r.d_bad = reinterpret_cast<uint32_t*>(c->d_vbad);
        r.d_words = r.d_bad + nblocks * size_t(c->m);
        return rc;
    };
    chk.fetch = [=, &r](hipStream_t st) -> int {
        auto to_host = [st](void* dst, const void* src, size_t bytes) {
            return st ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)
                      : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
        };
        if (W) HIP_TRY(to_host(words_out, r.d_words, word_bytes));
        if (bad_out) HIP_TRY(to_host(bad_out, r.d_bad, flag_bytes));
        return RSMI_OK;
    };
}

void stripe_write_back(rsmi_ctx* c, uint8_t* data, size_t data_block_stride, uint8_t* parity,
                       size_t parity_block_stride, size_t S, size_t nblocks, size_t W, int32_t* verdict_out,
                       const StripeResults& r, StripeCheck& chk) {
    const size_t k = size_t(c->k), m = size_t(c->m);
    // where the caller keeps row x of block b
    auto home = [=](size_t b, size_t x) -> uint8_t* {
        return x < k ? data + b * data_block_stride + x * S : parity + b * parity_block_stride + (x - k) * S;
    };
    // the small staged call: the verdicts are in verdict_out, the healed rows in the staging
    chk.small_done = [=](const uint8_t* sd, const uint8_t* sp) -> int {
        for (size_t b = 0; b < nblocks; b++)
            for (size_t i = 0; i < W; i++) {
                const int32_t v = verdict_out[W * b + i];
                if (v < 0) continue;
                const size_t x = size_t(v);
                if (x < k && sd) std::memcpy(home(b, x), sd + (b * k + x) * S, S);
                if (x >= k && sp) std::memcpy(home(b, x), sp + (b * m + (x - k)) * S, S);
            }
        return RSMI_OK;
    };
    // the upload pipeline: a chunk's verdicts, then its healed rows from the device pitch to the
    // caller's, before the staging slot is filled again
    chk.chunk_done = [=, &r](Staging& st, uint64_t b0, uint64_t nb, size_t Sp) -> int {
        HIP_TRY(hipMemcpyAsync(verdict_out + W * b0, r.verdicts() + W * b0, W * nb * sizeof(int32_t),
                               hipMemcpyDeviceToHost, st.stream));
        HIP_TRY(hipStreamSynchronize(st.stream));
        for (uint64_t b = 0; b < nb; b++)
            for (size_t i = 0; i < W; i++) {
                const int32_t v = verdict_out[W * (b0 + b) + i];
                if (v < 0) continue;
                const size_t x = size_t(v);
                const uint8_t* src = x < k ? st.d_in + (b * k + x) * Sp : st.d_out + (b * m + (x - k)) * Sp;
                HIP_TRY(hipMemcpyAsync(home(b0 + b, x), src, S, hipMemcpyDeviceToHost, st.stream));
            }
        HIP_TRY(hipStreamSynchronize(st.stream));
        return RSMI_OK;
    };
}

int verdicts_host_impl(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                       size_t parity_block_stride, size_t S, size_t nblocks, size_t W, VerdictLaunch launch,
                       int32_t* verdict_out, uint32_t* bad_out, uint8_t* home_data, uint8_t* home_parity) {
    if (int rc = check_stripe_host_args(c, data, data_block_stride, parity, parity_block_stride, S, verdict_out))
        return rc;
    if (nblocks == 0) return RSMI_OK;
    const size_t m = size_t(c->m);
    StripeResults r;
    StripeCheck chk;
    stripe_results(c, nblocks, W, verdict_out, bad_out, r, chk);
    chk.launch = [&](const Plan& plan, const StripeRows& rows, uint64_t b0, hipStream_t st) -> int {
        return launch(c, plan, rows, r.verdicts() + W * b0, r.d_bad + b0 * m, st);
    };
    if (home_data)
        stripe_write_back(c, home_data, data_block_stride, home_parity, parity_block_stride, S, nblocks, W, verdict_out,
                          r, chk);
    return verify_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, chk);
}

int verdicts_one_block(rsmi_ctx* c, const uint8_t* shards, size_t S, size_t W, VerdictLaunch launch, int* out,
                       uint8_t* home) {
    if (!c || !shards || !out) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    const size_t k = size_t(c->k), m = size_t(c->m);
    int32_t v[2] = {RSMI_LOCATE_UNKNOWN, RSMI_LOCATE_UNKNOWN};
    int rc = verdicts_host_impl(c, shards, k * S, shards + k * S, m * S, S, 1, W, launch, v, nullptr, home,
                                home ? home + k * S : nullptr);
    if (rc) return rc;
    for (size_t i = 0; i < W; i++) out[i] = int(v[i]);
    return RSMI_OK;
}

int check_stripe_dev_args(const rsmi_ctx* c, const void* d_data, size_t data_shard_stride, const void* d_parity,
                          size_t parity_shard_stride, size_t S, const void* out) {
    if (!c || !d_data || !d_parity || !out) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    if (data_shard_stride < S || parity_shard_stride < S) return RSMI_ERR_INVALID_ARG;
    return RSMI_OK;
}

int check_stripe_host_args(const rsmi_ctx* c, const void* data, size_t data_block_stride, const void* parity,
                           size_t parity_block_stride, size_t S, const void* out) {
    if (!c || !data || !parity || !out) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    if (data_block_stride < size_t(c->k) * S || parity_block_stride < size_t(c->m) * S) return RSMI_ERR_INVALID_ARG;
    return RSMI_OK;
}

int begin_stripe_dev_call(rsmi_ctx* c, std::unique_lock<std::mutex>& lock, std::shared_ptr<Plan>& plan) {
    lock = std::unique_lock<std::mutex>(c->mu);
    int rc = ensure_device(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return encode_plan(c, plan);
}

namespace {

// Host-memory verify on verify_host_impl's paths: flags alone.
int verify_flags_host(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                      size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* bad_out) {
    if (int rc = check_stripe_host_args(c, data, data_block_stride, parity, parity_block_stride, S, bad_out)) return rc;
    if (nblocks == 0) return RSMI_OK;
    const size_t m = size_t(c->m);
    StripeResults r;
    StripeCheck chk;
    stripe_results(c, nblocks, 0, nullptr, bad_out, r, chk);
    chk.launch = [&](const Plan& plan, const StripeRows& rows, uint64_t b0, hipStream_t st) -> int {
        return launch_verify(c, plan, rows, r.d_bad + b0 * m, st);
    };
    return verify_host_impl(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, chk);
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_verify_batch_dev(rsmi_ctx* c, const uint8_t* d_data, size_t data_shard_stride, size_t data_block_stride,
                          const uint8_t* d_parity, size_t parity_shard_stride, size_t parity_block_stride, size_t S,
                          size_t nblocks, uint32_t* d_bad_out, void* stream) try {
    return stripe_dev_call(
        c, d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride, parity_block_stride, S, nblocks,
        d_bad_out, [&](const Plan& plan, const StripeRows& rows) {
            return launch_verify(c, plan, rows, d_bad_out, static_cast<hipStream_t>(stream));
        });
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_verify_batch_host(rsmi_ctx* c, const uint8_t* data, size_t data_block_stride, const uint8_t* parity,
                           size_t parity_block_stride, size_t S, size_t nblocks, uint32_t* bad_out) try {
    return verify_flags_host(c, data, data_block_stride, parity, parity_block_stride, S, nblocks, bad_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_verify(rsmi_ctx* c, const uint8_t* shards, size_t S, int* ok_out) try {
    if (!c || !shards || !ok_out) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    const size_t k = size_t(c->k), m = size_t(c->m);
    std::vector<uint32_t> bad(m, 0);
    int rc = verify_flags_host(c, shards, k * S, shards + k * S, m * S, S, 1, bad.data());
    if (rc) return rc;
    *ok_out = std::all_of(bad.begin(), bad.end(), [](uint32_t x) { return x == 0; }) ? 1 : 0;
    return RSMI_OK;
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
