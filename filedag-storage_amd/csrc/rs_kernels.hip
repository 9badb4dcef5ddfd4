// rs_kernels.hip -- the coding kernels' table-less instantiations and their dispatch table
// (templates: rs_coding_kernels.hpp), the generic coding kernel and the row re-pitch copy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rs_coding_kernels.hpp"

namespace rsmi {

// Any K (<= 256), MT <= 4, any alignment: one byte-group of 4 per lane, bytewise memory
// access.  Correctness path for layouts the fast kernel does not accept.
__global__ __launch_bounds__(kWG) void rs_generic_kernel(const RsPlanDev* __restrict__ plan, const uint8_t* in,
                                                         uint8_t* out, uint64_t in_bs, uint64_t in_rs,
                                                         uint64_t out_bs, uint64_t out_rs, uint64_t S,
                                                         uint64_t nblocks) {
    __shared__ u32x4 s_tbl[kMaxK * kColDwords / 4];
    const int K = int(plan->k), MT = int(plan->mt);
    {
        const uint32_t* src = plan->tbl;
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_tbl);
        for (int i = threadIdx.x; i < K * kColDwords; i += kWG) dst[i] = src[i];
    }
    __syncthreads();
    const uint64_t groups = (S + 3) / 4;
    for (uint64_t b = blockIdx.y; b < nblocks; b += gridDim.y) {
        for (uint64_t g = uint64_t(blockIdx.x) * kWG + threadIdx.x; g < groups; g += uint64_t(gridDim.x) * kWG) {
            const uint64_t x0 = g * 4;
            const int nb = int(S - x0 < 4 ? S - x0 : 4);
            uint32_t acc[4] = {0, 0, 0, 0};
            for (int c = 0; c < K; c++) {
                const uint8_t* p = in + b * in_bs + uint64_t(plan->in_row[c]) * in_rs + x0;
                uint32_t x = 0;
                for (int i = 0; i < nb; i++) x |= uint32_t(p[i]) << (8 * i);
                const uint32_t s1 = x & 0x07070707u, s2 = (x >> 3) & 0x07070707u, s3 = (x >> 6) & 0x03030303u;
                const u32x4 T0 = s_tbl[c * 5 + 0], T1 = s_tbl[c * 5 + 1], T2 = s_tbl[c * 5 + 2],
                            T3 = s_tbl[c * 5 + 3], T4 = s_tbl[c * 5 + 4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    acc[j] ^= __builtin_amdgcn_perm(u4get(T1, j), u4get(T0, j), s1) ^
                              __builtin_amdgcn_perm(u4get(T3, j), u4get(T2, j), s2) ^
                              __builtin_amdgcn_perm(u4get(T4, j), u4get(T4, j), s3);
                }
            }
            for (int j = 0; j < MT; j++) {
                uint8_t* p = out + b * out_bs + uint64_t(plan->out_row[j]) * out_rs + x0;
                for (int i = 0; i < nb; i++) p[i] = uint8_t(acc[j] >> (8 * i));
            }
        }
    }
}

// Strided byte-row copy on the device (any src/dst alignment): rows x width bytes from
// src (row pitch spitch) to dst (row pitch dpitch).  Host staging uses it to turn the
// contiguous Split layout (pitch S, often odd) into the 16-B-aligned pitched layout and
// back, so PCIe transfers stay linear (odd-width 2-D DMA runs at 3-9 GB/s on MI355X).
// Each thread writes one naturally aligned destination dword; its 4 source bytes are
// funnel-shifted out of the two aligned source dwords that cover them.  A row's first
// and last dwords may be shared with a neighbouring row, so they are written bytewise.
__global__ __launch_bounds__(kWG) void rs_repitch_kernel(const uint8_t* __restrict__ src, uint64_t spitch,
                                                         uint8_t* __restrict__ dst, uint64_t dpitch, uint64_t width,
                                                         uint64_t rows) {
    const uint64_t dw_per_row = (width + 6) / 4 + 1;  // upper bound of dwords a row can touch
    const uint64_t total = dw_per_row * rows;
    for (uint64_t i = uint64_t(blockIdx.x) * kWG + threadIdx.x; i < total; i += uint64_t(gridDim.x) * kWG) {
        const uint64_t r = i / dw_per_row, q = i - r * dw_per_row;
        const uintptr_t drow = reinterpret_cast<uintptr_t>(dst + r * dpitch);
        const uintptr_t a = (drow & ~uintptr_t(3)) + 4 * q;  // aligned destination dword
        if (a >= drow + width) continue;
        const uint8_t* srow = src + r * spitch;
        const int64_t off = int64_t(a) - int64_t(drow);     // row offset of the dword's byte 0
        if (off >= 0 && uint64_t(off) + 4 <= width) {
            const uintptr_t sa = reinterpret_cast<uintptr_t>(srow) + uint64_t(off);
            const uint32_t* p = reinterpret_cast<const uint32_t*>(sa & ~uintptr_t(3));
            const uint32_t sh = uint32_t(sa & 3);
            const uint32_t lo = p[0];
            const uint32_t hi = sh ? p[1] : 0u;  // a second dword only when straddling
            *reinterpret_cast<uint32_t*>(a) = __builtin_amdgcn_alignbyte(hi, lo, sh);
        } else {
            for (int b = 0; b < 4; b++) {
                const int64_t o = off + b;
                if (o >= 0 && uint64_t(o) < width) reinterpret_cast<uint8_t*>(a)[b] = srow[o];
            }
        }
    }
}

void* repitch_kernel() { return reinterpret_cast<void*>(&rs_repitch_kernel); }

// ------------------------------------------------------------------ dispatch table
template <int K, int MT>
static void fill_km(FastKernelTable& t) {
    constexpr int NT = auto_nt(K, MT);
    t.fn[K][MT] = reinterpret_cast<void*>(&rs_fast_kernel<K, MT, NT>);
    // the rows of the grouped order run the shape's own kernel where it has one (store_policy,
    // waves_cap, rs_plan.hpp)
    if constexpr (grouped_kernel_shape(K, MT, NT))
        t.fn_sp[K][MT] = reinterpret_cast<void*>(&rs_fast_kernel<K, MT, NT, kMinWavesPerSimd, false, false, false,
                                                                 store_policy(K, MT, NT), waves_cap(K, MT)>);
    t.ua[K][MT] = reinterpret_cast<void*>(&rs_fast_kernel<K, MT, ua_nt(K, MT), kMinWavesPerSimd, true>);
    t.crc[K][MT] = reinterpret_cast<void*>(&rs_fast_kernel<K, MT, NT, kMinWavesPerSimd, false, true>);
    t.ua_crc[K][MT] = reinterpret_cast<void*>(&rs_fast_kernel<K, MT, NT, kMinWavesPerSimd, true, true>);
    t.fused[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd>);
    t.fused_ua[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, true>);
}

// the in-kernel combine for small launches, for the encode shapes of the BASELINE configs (other
// shapes take the two-launch form)
template <int K, int MT>
static void fill_inl(FastKernelTable& t) {
    constexpr int NT = auto_nt(K, MT);
    t.fused_inl[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, false, true>);
    t.fused_ua_inl[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, true, true>);
}

template <int K>
static void fill_k(FastKernelTable& t) {
    fill_km<K, 1>(t);
    fill_km<K, 2>(t);
    fill_km<K, 3>(t);
    fill_km<K, 4>(t);
}

const FastKernelTable& fast_kernels() {
    static const FastKernelTable t = [] {
        FastKernelTable x{};
        fill_k<1>(x);
        fill_k<2>(x);
        fill_k<3>(x);
        fill_k<4>(x);
        fill_k<5>(x);
        fill_k<6>(x);
        fill_k<8>(x);
        fill_k<10>(x);
        fill_k<12>(x);
        fill_k<16>(x);
        fill_inl<2, 1>(x);
        fill_inl<4, 2>(x);
        fill_inl<10, 4>(x);
        fill_inl<16, 4>(x);
        fill_table_kernels(x);
        return x;
    }();
    return t;
}

void* generic_kernel() { return reinterpret_cast<void*>(&rs_generic_kernel); }

}  // namespace rsmi
