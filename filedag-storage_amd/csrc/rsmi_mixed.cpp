// rsmi_mixed.cpp -- rsmi_reconstruct_mixed_* (include/rsmi.h; see rsmi_impl.hpp for the file map):
// the in-place reconstruct of a batch in which every block has its own present (and required)
// mask.  The host deduplicates the blocks' (present, want) pairs, takes each pair's plan from the
// cache the uniform call uses (reconstruct_plan), sorts the blocks into classes by the number of
// rows their plan rebuilds (1..4) and launches rs_mixed_kernel (rs_mixed_kernels.hip) once per
// class over that class's tiles; a wave finds its block and plan through the class's list.
// Blocks whose plan has more than one tile, whose K has no rs_mixed_kernel, or whose layout is
// neither aligned nor unaligned-window take the uniform call's launch_plan, one per run of
// consecutive blocks with equal masks: the correctness path of rare shapes.  The _crcs forms add the
// named rows pass (rsmi_crc.cpp launch_crc_named) over the rows just rebuilt, behind those launches.
// The _verify forms return R of every row read and rebuilt: the classes launch rs_mixed_fused_kernel
// (rs_mixed_fused_kernels.hip) in the place of rs_mixed_kernel, then the records' combine and the
// scatter to (block, row); the other blocks have their survivors and rebuilt rows named to that pass.

#include "rsmi_impl.hpp"

#include <limits>
#include <unordered_map>

using namespace rsmi;
using namespace rsmi::impl;

namespace rsmi {
namespace impl {

void classify_mixed(const rsmi_ctx* c, size_t nblocks, const uint8_t* present, const uint8_t* required, int data_only,
                    MixedBatch& mb) {
    const size_t n = size_t(c->n), k = size_t(c->k);
    mb = MixedBatch();
    mb.pat.resize(nblocks);
    std::unordered_map<std::string, uint32_t> index;
    std::string key(n, '0');
    uint32_t last = 0;
    for (size_t b = 0; b < nblocks; b++) {
        const uint8_t* p = present + b * n;
        const uint8_t* r = required ? required + b * n : nullptr;
        for (size_t i = 0; i < n; i++) {
            const bool have = p[i] != 0;
            const bool want = !have && (r ? r[i] != 0 : (i < k || !data_only));
            key[i] = char('0' + (have ? 1 : 0) + (want ? 2 : 0));
        }
        // neighbours mostly share their masks: the map is asked once per run
        if (b == 0 || key != mb.keys[last]) {
            auto it = index.find(key);
            if (it == index.end()) {
                size_t np = 0, rows = 0;
                for (size_t i = 0; i < n; i++) {
                    np += key[i] == '1';
                    rows += key[i] == '2';
                }
                // upstream reconstruct(): nothing wanted is missing -> no-op; then fewer than k present
                const bool few = rows != 0 && np < k;
                it = index.emplace(key, uint32_t(mb.keys.size())).first;
                mb.keys.push_back(key);
                mb.key_status.push_back(few ? RSMI_ERR_TOO_FEW_SHARDS : RSMI_OK);
                mb.key_rows.push_back(few ? 0 : uint8_t(rows));
            }
            last = it->second;
        }
        mb.pat[b] = last;
        if (mb.key_status[last] != RSMI_OK) mb.too_few++;
        else if (mb.key_rows[last]) mb.work++;
    }
}

namespace {

constexpr int kNoLaunch = 0, kFallback = -1;  // a pattern's class, beside 1..kMaxMT

// The stream's entry of ctx->mixed_scratch (caller holds ctx->mu), evicted past 32 streams as
// stream_scratch (rsmi_verify.cpp) evicts.
rsmi_ctx::MixedScratch& mixed_scratch(rsmi_ctx* c, hipStream_t st) {
    auto& map = c->mixed_scratch;
    auto it = map.find(st);
    if (it != map.end()) return it->second;
    if (map.size() >= 32) {
        (void)hipDeviceSynchronize();
        for (auto& e : map) {
            if (e.second.d) (void)hipFree(e.second.d);
            if (e.second.h) (void)hipHostFree(e.second.h);
        }
        map.clear();
    }
    return map[st];
}

}  // namespace

// need bytes of the stream's scratch, 16-byte aligned, at the same offset of both halves; they
// stay untouched until the stream has been waited for.  Waits for the stream once when the
// scratch has to grow or start over.  (Shared with the ragged encode, rsmi_ragged.cpp.)
int mixed_words(rsmi_ctx* c, hipStream_t st, size_t need, uint8_t*& h, uint8_t*& d) {
    rsmi_ctx::MixedScratch& ms = mixed_scratch(c, st);
    need = round_up(need, 16);
    if (ms.cap - ms.head < need) {
        if (ms.d) HIP_TRY(hipStreamSynchronize(st));
        ms.head = 0;
        if (ms.cap < need) {
            const size_t cap = std::max<size_t>(std::max(need, ms.cap + ms.cap / 2), size_t(1) << 20);
            if (ms.d) HIP_TRY(hipFree(ms.d));
            ms.d = nullptr;
            if (ms.h) HIP_TRY(hipHostFree(ms.h));
            ms.h = nullptr;
            ms.cap = 0;
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ms.d), cap));
            HIP_TRY(pinned_alloc(reinterpret_cast<void**>(&ms.h), cap));
            ms.cap = cap;
        }
    }
    h = ms.h + ms.head;
    d = ms.d + ms.head;
    ms.head += need;
    return RSMI_OK;
}

namespace {

// One class of a segment on the _verify route: rs_mixed_fused_kernel over the class's units, a
// workgroup each (at most the class's tiles, so within option launch_units_max as the segment is),
// the records' combine with the class's entries as its blocks, and the scatter of the (entry, slot)
// checksums to out[blk * n + row].  list, plans: device memory, as rs_mixed_kernel takes them; rec,
// comb: the class's share of the stream's mixed_verify_scratch.
struct MixedFusedClass {
    const MixedEntry* list;
    const RsPlanDev* const* plans;
    uint8_t* base;
    uint64_t bs, rs, S;
    int K, mt;
    bool aligned;
    uint64_t entries;
    const FoldGeometry* g;  // of (S, K + mt)
    uint8_t* rec;
    uint32_t* comb;
    uint32_t* out;
    uint32_t n;
};
int launch_mixed_fused(rsmi_ctx* c, const MixedFusedClass& a, hipStream_t stream) {
    void* fn = (a.aligned ? mixed_fused_kernels().fn : mixed_fused_kernels().ua)[a.K][a.mt];
    const MixedEntry* dl = a.list;
    const RsPlanDev* const* dp = a.plans;
    uint8_t* base = a.base;
    uint8_t* rec = a.rec;
    const uint32_t* ctb = c->d_crc_tbl;
    const FoldGeometry& g = *a.g;
    uint32_t nunits = uint32_t(a.entries * g.upb);
    uint32_t S32 = uint32_t(a.S), cpb32 = uint32_t(g.cpb), tpb32 = uint32_t(g.tpb), upb32 = uint32_t(g.upb);
    uint64_t bs64 = a.bs, rs64 = a.rs;
    void* args[] = {&dl, &dp, &base, &bs64, &rs64, &S32, &cpb32, &tpb32, &upb32, &nunits, &ctb, &rec};
    HIP_TRY(hipLaunchKernel(fn, dim3(nunits), dim3(kWG), args, 0, stream));  // a workgroup per unit
    c->split_launches.fetch_add(1, std::memory_order_relaxed);
    // the records' combine, crc16_combine_mfma_kernel() as behind the fused encode and the scrub, with
    // the class's entries as its blocks
    if (int rc = launch_fold_combine(c, a.rec, g, a.entries, a.comb, stream)) return rc;
    uint32_t nsh32 = uint32_t(g.nsh), K32 = uint32_t(a.K), n32 = a.n;
    uint32_t nitems = uint32_t(a.entries * nsh32);
    const uint32_t* ccomb = a.comb;
    uint32_t* out = a.out;
    void* sargs[] = {&dl, &dp, &ccomb, &nsh32, &K32, &n32, &nitems, &out};
    HIP_TRY(hipLaunchKernel(mixed_scatter_kernel(), dim3((nitems + kWG - 1) / kWG), dim3(kWG), sargs, 0, stream));
    char buf[96];
    std::snprintf(buf, sizeof buf, "rs_mixed_fused_kernel<K=%d,MT=%d>%s", a.K, a.mt, a.aligned ? "" : ",UA");
    set_last_kernel(c, buf);
    return RSMI_OK;
}

}  // namespace

int launch_mixed(rsmi_ctx* c, const MixedBatch& mb, uint8_t* base, uint64_t rs, uint64_t bs, uint64_t S, uint64_t b0,
                 uint64_t nb, hipStream_t stream, uint32_t* d16, uint32_t* d32, uint32_t* dver) {
    if (nb == 0 || S == 0) return RSMI_OK;
    const bool crcs = d16 || d32;
    if (crcs && dver) return RSMI_ERR_INVALID_ARG;
    const size_t n = size_t(c->n), npat = mb.keys.size();
    // launch_plan's layout test, the rows being read and written in place
    const StripeLayout layout = StripeRows{base, rs, bs, base, rs, bs, S, nb}.layout();
    const bool aligned = layout == StripeLayout::kAligned;
    const uint64_t cpb = (S + 15) / 16;
    const uint64_t tpb = (cpb + uint64_t(kWave) - 1) / uint64_t(kWave);
    constexpr int wpg = kFastWG / kWave;
    long wg_cap = std::numeric_limits<long>::max();
    if (c->opt_waves_per_cu > 0) wg_cap = std::max(1L, long(c->num_cu) * c->opt_waves_per_cu / wpg);

    // per pattern that has a block here: its plan and its class
    std::vector<std::shared_ptr<Plan>> plans(npat);
    std::vector<int> cls(npat, kNoLaunch);
    // dver: the pattern's class has an rs_mixed_fused_kernel, which also checksums what it reads
    // and writes; every other pattern with a launch has its rows named to the named rows pass
    std::vector<uint8_t> fused(npat, 0);
    std::vector<uint8_t> seen(npat, 0);
    std::vector<uint8_t> have(n), want(n);
    const int K = c->k;  // every reconstruct plan reads k survivors
    for (uint64_t b = b0; b < b0 + nb; b++) {
        const uint32_t p = mb.pat[b];
        if (seen[p]) continue;
        seen[p] = 1;
        if (!mb.key_rows[p]) continue;
        for (size_t i = 0; i < n; i++) {
            have[i] = mb.keys[p][i] == '1';
            want[i] = mb.keys[p][i] == '2';
        }
        int rc = reconstruct_plan(c, have.data(), want.data(), plans[p]);
        if (rc) return rc;
        const Plan& pl = *plans[p];
        const DevTile& t = pl.tiles[0];
        const bool fast = layout != StripeLayout::kNeither && pl.tiles.size() == 1 && t.K == K && K <= 16 &&
                          (aligned ? mixed_kernels().fn : mixed_kernels().ua)[K][t.MT] != nullptr;
        cls[p] = fast ? t.MT : kFallback;
        fused[p] = dver && fast && (aligned ? mixed_fused_kernels().fn : mixed_fused_kernels().ua)[K][t.MT] != nullptr;
    }
    const bool any_fused = std::find(fused.begin(), fused.end(), uint8_t(1)) != fused.end();
    if (any_fused)
        if (int rc = ensure_crc_tables(c)) return rc;
    // the fused classes' geometry: units of 4 tiles of one block, K + mt record slots
    std::vector<FoldGeometry> fg;
    for (int mt = 0; any_fused && mt <= kMaxMT; mt++) fg.emplace_back(S, uint64_t(K + mt));

    // segments of at most 2^22 blocks whose tile counts per class stay within option launch_units_max
    const uint64_t seg =
        std::min<uint64_t>(std::max<uint64_t>(1, uint64_t(c->opt_launch_units_max) / tpb), uint64_t(1) << 22);
    // a class's units are at most its tiles, so a segment's fused launches stay within the option too
    std::vector<MixedEntry> list[kMaxMT + 1], flist[kMaxMT + 1];
    for (uint64_t s0 = b0; s0 < b0 + nb; s0 += seg) {
        const uint64_t sn = std::min(seg, b0 + nb - s0);
        uint8_t* sbase = base + (s0 - b0) * bs;
        for (auto& l : list) l.clear();
        for (auto& l : flist) l.clear();
        size_t nfast = 0;
        for (uint64_t b = 0; b < sn; b++) {
            const uint32_t p = mb.pat[s0 + b];
            if (cls[p] > 0) {
                if (fused[p])
                    flist[cls[p]].push_back(MixedEntry{uint32_t(b), p});
                else
                    list[cls[p]].push_back(MixedEntry{uint32_t(b), p});
                nfast++;
            }
        }
        // with checksums: the rows every block of the segment rebuilds, as the named rows pass reads
        // them (slots = the most rows a block rebuilds, unused slots -1), behind the lists; dver:
        // ahead of them the k survivors, and only of the blocks no fused kernel takes
        auto named = [&](uint32_t p) { return cls[p] != kNoLaunch && (crcs || (dver && !fused[p])); };
        uint32_t slots = 0;
        if (crcs || dver)
            for (uint64_t b = 0; b < sn; b++)
                if (named(mb.pat[s0 + b]))
                    slots = std::max<uint32_t>(slots, (dver ? uint32_t(K) : 0u) + mb.key_rows[mb.pat[s0 + b]]);
        const size_t rows_bytes = size_t(sn) * slots * sizeof(int32_t);
        const int32_t* d_rows = nullptr;
        if (nfast || slots) {
            // one upload: the patterns' plan pointers, then the classes' lists in ascending MT
            // (rs_mixed_kernel's, then rs_mixed_fused_kernel's)
            const size_t ptr_bytes = round_up(npat * sizeof(const RsPlanDev*), 16);
            const size_t list_bytes = round_up(nfast * sizeof(MixedEntry), 16);
            uint8_t *h = nullptr, *d = nullptr;
            int rc = mixed_words(c, stream, ptr_bytes + list_bytes + rows_bytes, h, d);
            if (rc) return rc;
            auto* hp = reinterpret_cast<const RsPlanDev**>(h);
            for (size_t p = 0; p < npat; p++) hp[p] = cls[p] > 0 ? plans[p]->tiles[0].dev : nullptr;
            size_t off = ptr_bytes;
            size_t list_off[kMaxMT + 1] = {}, flist_off[kMaxMT + 1] = {};
            for (int mt = 1; mt <= kMaxMT; mt++) {
                list_off[mt] = off;
                if (!list[mt].empty()) std::memcpy(h + off, list[mt].data(), list[mt].size() * sizeof(MixedEntry));
                off += list[mt].size() * sizeof(MixedEntry);
            }
            for (int mt = 1; mt <= kMaxMT; mt++) {
                flist_off[mt] = off;
                if (!flist[mt].empty()) std::memcpy(h + off, flist[mt].data(), flist[mt].size() * sizeof(MixedEntry));
                off += flist[mt].size() * sizeof(MixedEntry);
            }
            if (slots) {
                off = ptr_bytes + list_bytes;
                int32_t* hr = reinterpret_cast<int32_t*>(h + off);
                for (uint64_t b = 0; b < sn; b++) {
                    const uint32_t p = mb.pat[s0 + b];
                    uint32_t s = 0;
                    if (named(p)) {
                        // dver: the first k present rows, the rows every reconstruct plan reads
                        for (size_t i = 0; dver && i < n && s < uint32_t(K); i++)
                            if (mb.keys[p][i] == '1') hr[b * slots + s++] = int32_t(i);
                        for (size_t i = 0; i < n; i++)
                            if (mb.keys[p][i] == '2') hr[b * slots + s++] = int32_t(i);
                    }
                    while (s < slots) hr[b * slots + s++] = -1;
                }
                d_rows = reinterpret_cast<const int32_t*>(d + off);
                off += rows_bytes;
            }
            HIP_TRY(hipMemcpyAsync(d, h, off, hipMemcpyHostToDevice, stream));
            for (int mt = 1; mt <= kMaxMT; mt++) {
                if (list[mt].empty()) continue;
                void* fn = (aligned ? mixed_kernels().fn : mixed_kernels().ua)[K][mt];
                const MixedEntry* dl = reinterpret_cast<const MixedEntry*>(d + list_off[mt]);
                const RsPlanDev* const* dp = reinterpret_cast<const RsPlanDev* const*>(d);
                uint32_t ntiles = uint32_t(list[mt].size() * tpb);
                uint32_t S32 = uint32_t(S), cpb32 = uint32_t(cpb), tpb32 = uint32_t(tpb);
                uint64_t bs64 = bs, rs64 = rs;
                void* args[] = {&dl, &dp, &sbase, &bs64, &rs64, &S32, &cpb32, &tpb32, &ntiles};
                const uint64_t wgs = std::min<uint64_t>((uint64_t(ntiles) + wpg - 1) / wpg, uint64_t(wg_cap));
                HIP_TRY(hipLaunchKernel(fn, dim3(uint32_t(wgs)), dim3(uint32_t(wpg * kWave)), args, 0, stream));
                c->split_launches.fetch_add(1, std::memory_order_relaxed);
                char buf[96];
                std::snprintf(buf, sizeof buf, "rs_mixed_kernel<K=%d,MT=%d>%s", K, mt, aligned ? "" : ",UA");
                set_last_kernel(c, buf);
            }
            // the fused classes: per class the tile kernel over its units, a workgroup each, the
            // records' combine with the class's entries as its blocks, and the scatter to the rows
            size_t rec_bytes = 0, comb_words = 0;
            for (int mt = 1; mt <= kMaxMT; mt++) {
                if (!flist[mt].empty()) rec_bytes += flist[mt].size() * fg[mt].rec_per_block;
                comb_words += flist[mt].size() * size_t(K + mt);
            }
            if (rec_bytes) {
                rsmi_ctx::VerifyScratch& sc = stream_scratch(c->mixed_verify_scratch, stream);
                rec_bytes = round_up(rec_bytes, 16);
                if ((rc = reserve_on(sc.p, sc.cap, rec_bytes + comb_words * sizeof(uint32_t), stream))) return rc;
                uint8_t* rec = sc.p;
                uint32_t* comb = reinterpret_cast<uint32_t*>(sc.p + rec_bytes);
                const RsPlanDev* const* dp = reinterpret_cast<const RsPlanDev* const*>(d);
                uint32_t* vout = dver + (s0 - b0) * n;
                for (int mt = 1; mt <= kMaxMT; mt++) {
                    const uint64_t ne = flist[mt].size();
                    if (!ne) continue;
                    const MixedFusedClass fc{reinterpret_cast<const MixedEntry*>(d + flist_off[mt]), dp, sbase, bs, rs, S,
                                             K, mt, aligned, ne, &fg[mt], rec, comb, vout, uint32_t(n)};
                    if ((rc = launch_mixed_fused(c, fc, stream))) return rc;
                    rec += ne * fg[mt].rec_per_block;
                    comb += ne * fg[mt].nsh;
                }
            }
        }
        // the fallback: the uniform call's launch per run of consecutive blocks with equal masks
        for (uint64_t b = 0; b < sn;) {
            const uint32_t p = mb.pat[s0 + b];
            uint64_t e = b + 1;
            while (e < sn && mb.pat[s0 + e] == p) e++;
            if (cls[p] == kFallback) {
                uint8_t* rb = sbase + b * bs;
                int rc = launch_plan(c, *plans[p], rb, rs, bs, rb, rs, bs, S, e - b, stream);
                if (rc) return rc;
            }
            b = e;
        }
        // the checksums of the rows just written, whatever rebuilt them: by row, behind the launches above
        if (slots) {
            const NamedRowsArgs a{d_rows, sbase, bs, rs, sbase + uint64_t(K) * rs, bs, rs,
                                  uint32_t(K), uint32_t(n), slots, uint32_t(n)};
            uint32_t* o16 = dver ? dver : d16;
            int rc = launch_crc_named(c, a, S, sn, o16 ? o16 + (s0 - b0) * n : nullptr,
                                      d32 ? d32 + (s0 - b0) * n : nullptr, stream, false);
            if (rc) return rc;
        }
    }
    return hip_status(hipGetLastError());
}

namespace {

void write_status(const MixedBatch& mb, size_t nblocks, int32_t* status_out) {
    if (!status_out) return;
    for (size_t b = 0; b < nblocks; b++) status_out[b] = mb.key_status[mb.pat[b]];
}

// The host-memory call on reconstruct_host_impl's three decisions: page-locked shards in place,
// small pageable calls through the page-locked staging, everything else uploaded in ~64 MiB
// chunks of whole blocks over the three staging slots.  Only wanted rows of blocks with status OK
// are written into the caller's memory.  crcs: raw16 / raw32[b*(k+m) + r] (host memory, not both
// null) receive R / R32 of every row the call rebuilt and 0 elsewhere: the named rows pass runs where
// the rows were rebuilt (in place, over the staging, over the chunk's device rows on its slot's
// stream before the slot is reused), into ctx->d_crc / d_crc32, read back once at the end.
// rawv (the _verify form, in place of raw16 / raw32): R of every row the call read or rebuilt, by
// the same route (launch_mixed's dver), ctx->d_crc being its device side.
int mixed_host_impl(rsmi_ctx* c, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                    const uint8_t* present, const uint8_t* required, int data_only, int32_t* status_out,
                    bool crcs = false, uint32_t* raw16 = nullptr, uint32_t* raw32 = nullptr, uint32_t* rawv = nullptr) {
    if (!c || !shards || !present || (crcs && !raw16 && !raw32 && !rawv)) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    if (block_stride < size_t(c->n) * S) return RSMI_ERR_INVALID_ARG;
    if (nblocks == 0) return RSMI_OK;
    MixedBatch mb;
    classify_mixed(c, nblocks, present, required, data_only, mb);
    if (mb.too_few && !status_out) return RSMI_ERR_TOO_FEW_SHARDS;
    const size_t raw_sz = nblocks * size_t(c->n) * 4;
    if (raw16) std::memset(raw16, 0, raw_sz);
    if (raw32) std::memset(raw32, 0, raw_sz);
    if (!mb.work) {
        if (rawv) std::memset(rawv, 0, raw_sz);  // with work every word comes back from the device
        write_status(mb, nblocks, status_out);
        return RSMI_OK;
    }
    std::lock_guard<std::mutex> g(c->mu);
    int rc = ensure_device(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = size_t(c->n), blk = n * S;
    if ((raw16 || rawv) && (rc = reserve(c->d_crc, c->crc_cap, raw_sz))) return rc;
    if (raw32 && (rc = reserve(c->d_crc32, c->crc32_cap, raw_sz))) return rc;
    uint32_t* d16 = raw16 ? reinterpret_cast<uint32_t*>(c->d_crc) : nullptr;
    uint32_t* d32 = raw32 ? reinterpret_cast<uint32_t*>(c->d_crc32) : nullptr;
    uint32_t* dv = rawv ? reinterpret_cast<uint32_t*>(c->d_crc) : nullptr;
    // the rows of block b the call moves: in, the present rows; out, the rows it rebuilt
    auto each_row = [&](size_t b, char which, auto&& fn) {
        const uint32_t p = mb.pat[b];
        if (!mb.key_rows[p]) return;
        for (size_t i = 0; i < n; i++)
            if (mb.keys[p][i] == which) fn(i);
    };
    uint8_t* dev = c->opt_zero_copy ? host_alias(shards, (nblocks - 1) * block_stride + blk) : nullptr;
    if (dev || nblocks * blk <= size_t(c->opt_small_bytes)) {
        hipStream_t st = c->staging[0].stream;
        uint8_t* hs = nullptr;
        size_t dbs = block_stride;
        if (!dev) {
            hs = small_stage(c, nblocks * blk);
            if (!hs) return RSMI_ERR_DEVICE;
            for (size_t b = 0; b < nblocks; b++)
                each_row(b, '1', [&](size_t i) { std::memcpy(hs + b * blk + i * S, shards + b * block_stride + i * S, S); });
            dev = host_alias(hs, nblocks * blk);
            dbs = blk;
            if (!dev) return RSMI_ERR_DEVICE;
        }
        if (d16) HIP_TRY(hipMemsetAsync(d16, 0, raw_sz, st));
        if (d32) HIP_TRY(hipMemsetAsync(d32, 0, raw_sz, st));
        if (dv) HIP_TRY(hipMemsetAsync(dv, 0, raw_sz, st));
        if ((rc = launch_mixed(c, mb, dev, S, dbs, S, 0, nblocks, st, d16, d32, dv))) return rc;
        const uint32_t *h16, *h32;
        if ((rc = readback(c, dv ? dv : d16, d32, raw_sz, st, h16, h32))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        if (rawv) std::memcpy(rawv, h16, raw_sz);
        if (raw16) std::memcpy(raw16, h16, raw_sz);
        if (raw32) std::memcpy(raw32, h32, raw_sz);
        if (hs)
            for (size_t b = 0; b < nblocks; b++)
                each_row(b, '2', [&](size_t i) { std::memcpy(shards + b * block_stride + i * S, hs + b * blk + i * S, S); });
        write_status(mb, nblocks, status_out);
        return RSMI_OK;
    }
    // Whole blocks go up linearly at pitch S (the kernels take that pitch as it is: the
    // unaligned-window form, or the aligned one when S is a multiple of 16), so every row crosses
    // PCIe on the way in, missing ones included; the rebuilt rows come back one copy each, behind
    // the chunk's kernels on its slot's stream, before a later chunk's upload reuses the slot.
    const size_t chunk = std::max<size_t>(1, (size_t(64) << 20) / blk);
    const int ns = nblocks > chunk ? 3 : 1;
    for (size_t b0 = 0, i = 0; b0 < nblocks; b0 += chunk, i++) {
        Staging& st = c->staging[i % ns];
        const size_t nb = std::min(chunk, nblocks - b0);
        if ((rc = reserve(st.d_lin, st.lin_cap, nb * blk))) return rc;
        const uint8_t* h = shards + b0 * block_stride;
        if (block_stride == blk)
            HIP_TRY(hipMemcpyAsync(st.d_lin, h, nb * blk, hipMemcpyHostToDevice, st.stream));
        else
            for (size_t b = 0; b < nb; b++)
                HIP_TRY(hipMemcpyAsync(st.d_lin + b * blk, h + b * block_stride, blk, hipMemcpyHostToDevice, st.stream));
        if (d16) HIP_TRY(hipMemsetAsync(d16 + b0 * n, 0, nb * n * 4, st.stream));
        if (d32) HIP_TRY(hipMemsetAsync(d32 + b0 * n, 0, nb * n * 4, st.stream));
        if (dv) HIP_TRY(hipMemsetAsync(dv + b0 * n, 0, nb * n * 4, st.stream));
        if ((rc = launch_mixed(c, mb, st.d_lin, S, blk, S, b0, nb, st.stream, d16 ? d16 + b0 * n : nullptr,
                               d32 ? d32 + b0 * n : nullptr, dv ? dv + b0 * n : nullptr)))
            return rc;
        for (size_t b = 0; b < nb; b++) {
            hipError_t e = hipSuccess;
            each_row(b0 + b, '2', [&](size_t r) {
                if (e == hipSuccess)
                    e = hipMemcpyAsync(shards + (b0 + b) * block_stride + r * S, st.d_lin + b * blk + r * S, S,
                                       hipMemcpyDeviceToHost, st.stream);
            });
            HIP_TRY(e);
        }
    }
    for (int s = 0; s < ns; s++) HIP_TRY(hipStreamSynchronize(c->staging[s].stream));
    if (raw16) HIP_TRY(hipMemcpy(raw16, d16, raw_sz, hipMemcpyDeviceToHost));
    if (raw32) HIP_TRY(hipMemcpy(raw32, d32, raw_sz, hipMemcpyDeviceToHost));
    if (rawv) HIP_TRY(hipMemcpy(rawv, dv, raw_sz, hipMemcpyDeviceToHost));
    write_status(mb, nblocks, status_out);
    return RSMI_OK;
}

}  // namespace

}  // namespace impl
}  // namespace rsmi

extern "C" {

int rsmi_reconstruct_mixed_classify(const rsmi_ctx* c, size_t nblocks, const uint8_t* present, const uint8_t* required,
                                    int data_only, int32_t* status_out, uint8_t* rows_out, uint32_t* pattern_out,
                                    size_t* npatterns_out) try {
    if (!c || (nblocks && !present)) return RSMI_ERR_INVALID_ARG;
    MixedBatch mb;
    classify_mixed(c, nblocks, present, required, data_only, mb);
    for (size_t b = 0; b < nblocks; b++) {
        const uint32_t p = mb.pat[b];
        if (status_out) status_out[b] = mb.key_status[p];
        if (rows_out) rows_out[b] = mb.key_rows[p];
        if (pattern_out) pattern_out[b] = p;
    }
    if (npatterns_out) *npatterns_out = mb.keys.size();
    return RSMI_OK;
} catch (...) {
    return rsmi::impl::exception_status();
}

namespace {

// rsmi_reconstruct_mixed_batch_dev, and with crcs its _crcs form: d16 / d32 (device memory, not
// both null) are zeroed on the stream, so that form needs the device even with nothing to rebuild;
// dver in their place: the _verify form, the same in every other respect
int mixed_dev_impl(rsmi_ctx* c, uint8_t* d_shards, size_t shard_stride, size_t block_stride, size_t S, size_t nblocks,
                   const uint8_t* present, const uint8_t* required, int data_only, int32_t* status_out, bool crcs,
                   uint32_t* d16, uint32_t* d32, void* stream, uint32_t* dver = nullptr) {
    if (!c || !d_shards || !present || (crcs && !d16 && !d32 && !dver)) return RSMI_ERR_INVALID_ARG;
    if (S == 0) return RSMI_ERR_SHARD_NO_DATA;
    if (shard_stride < S) return RSMI_ERR_INVALID_ARG;
    if (nblocks == 0) return RSMI_OK;
    MixedBatch mb;
    classify_mixed(c, nblocks, present, required, data_only, mb);
    if (mb.too_few && !status_out) return RSMI_ERR_TOO_FEW_SHARDS;
    if (mb.work || crcs) {
        std::lock_guard<std::mutex> g(c->mu);
        int rc = ensure_device(c);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        hipStream_t st = static_cast<hipStream_t>(stream);
        const size_t raw_sz = nblocks * size_t(c->n) * 4;
        if (d16) HIP_TRY(hipMemsetAsync(d16, 0, raw_sz, st));
        if (d32) HIP_TRY(hipMemsetAsync(d32, 0, raw_sz, st));
        if (dver) HIP_TRY(hipMemsetAsync(dver, 0, raw_sz, st));
        if (mb.work &&
            (rc = launch_mixed(c, mb, d_shards, shard_stride, block_stride, S, 0, nblocks, st, d16, d32, dver)))
            return rc;
    }
    write_status(mb, nblocks, status_out);
    return RSMI_OK;
}

}  // namespace

int rsmi_reconstruct_mixed_batch_dev(rsmi_ctx* c, uint8_t* d_shards, size_t shard_stride, size_t block_stride, size_t S,
                                     size_t nblocks, const uint8_t* present, const uint8_t* required, int data_only,
                                     int32_t* status_out, void* stream) try {
    return mixed_dev_impl(c, d_shards, shard_stride, block_stride, S, nblocks, present, required, data_only, status_out,
                          false, nullptr, nullptr, stream);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_reconstruct_mixed_batch_dev_crcs(rsmi_ctx* c, uint8_t* d_shards, size_t shard_stride, size_t block_stride,
                                          size_t S, size_t nblocks, const uint8_t* present, const uint8_t* required,
                                          int data_only, int32_t* status_out, uint32_t* d_raw16_out,
                                          uint32_t* d_raw32_out, void* stream) try {
    return mixed_dev_impl(c, d_shards, shard_stride, block_stride, S, nblocks, present, required, data_only, status_out,
                          true, d_raw16_out, d_raw32_out, stream);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_reconstruct_mixed_batch_dev_verify(rsmi_ctx* c, uint8_t* d_shards, size_t shard_stride, size_t block_stride,
                                            size_t S, size_t nblocks, const uint8_t* present, const uint8_t* required,
                                            int data_only, int32_t* status_out, uint32_t* d_raw16_rows,
                                            void* stream) try {
    return mixed_dev_impl(c, d_shards, shard_stride, block_stride, S, nblocks, present, required, data_only, status_out,
                          true, nullptr, nullptr, stream, d_raw16_rows);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_reconstruct_mixed_batch_host_verify(rsmi_ctx* c, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                             const uint8_t* present, const uint8_t* required, int data_only,
                                             int32_t* status_out, uint32_t* raw16_rows) try {
    return mixed_host_impl(c, shards, block_stride, S, nblocks, present, required, data_only, status_out, true, nullptr,
                           nullptr, raw16_rows);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_reconstruct_mixed_batch_host_crcs(rsmi_ctx* c, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                           const uint8_t* present, const uint8_t* required, int data_only,
                                           int32_t* status_out, uint32_t* raw16_out, uint32_t* raw32_out) try {
    return mixed_host_impl(c, shards, block_stride, S, nblocks, present, required, data_only, status_out, true,
                           raw16_out, raw32_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

int rsmi_reconstruct_mixed_batch_host(rsmi_ctx* c, uint8_t* shards, size_t block_stride, size_t S, size_t nblocks,
                                      const uint8_t* present, const uint8_t* required, int data_only,
                                      int32_t* status_out) try {
    return mixed_host_impl(c, shards, block_stride, S, nblocks, present, required, data_only, status_out);
} catch (...) {
    return rsmi::impl::exception_status();
}

}  // extern "C"
