// rs_kernels_tb.hip -- the table-of-bases forms of the coding kernels (rs_coding_kernels.hpp TB: a
// coalesced group of DagNode.Put / Get callers' own page-locked buffers coded by one kernel
// launch), in a translation unit of their own so the build compiles them beside rs_kernels.hip:
// for the BASELINE shapes' encodes (K = k, MT = m) and their reconstructs of up to 4 rows; other
// shapes code a coalesced group with one launch per block.
#include "rs_coding_kernels.hpp"

namespace rsmi {

template <int K, int MT>
static void fill_tb_km(FastKernelTable& t) {
    constexpr int NT = auto_nt(K, MT);
    t.fn_tb[K][MT] = reinterpret_cast<void*>(&rs_fast_kernel<K, MT, NT, kMinWavesPerSimd, false, false, true>);
    t.ua_tb[K][MT] = reinterpret_cast<void*>(&rs_fast_kernel<K, MT, ua_nt(K, MT), kMinWavesPerSimd, true, false, true>);
}
template <int K, int MT>
static void fill_tb_fused(FastKernelTable& t) {
    constexpr int NT = auto_nt(K, MT);
    t.fused_tb[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, false, false, true>);
    t.fused_ua_tb[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, true, false, true>);
    t.fused_inl_tb[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, false, true, true>);
    t.fused_ua_inl_tb[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, true, true, true>);
}
template <int K, int MT>
static void fill_tb_fused_inl(FastKernelTable& t) {
    constexpr int NT = auto_nt(K, MT);
    t.fused_inl_tb[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, false, true, true>);
    t.fused_ua_inl_tb[K][MT] = reinterpret_cast<void*>(&rs_fused_mfma_kernel<K, MT, NT, kFusedWavesPerSimd, true, true, true>);
}
template <int K>
static void fill_tb_k(FastKernelTable& t) {
    fill_tb_km<K, 1>(t);
    fill_tb_km<K, 2>(t);
    fill_tb_km<K, 3>(t);
    fill_tb_km<K, 4>(t);
}
void fill_table_kernels(FastKernelTable& t) {
    fill_tb_k<2>(t);
    fill_tb_k<4>(t);
    fill_tb_k<10>(t);
    fill_tb_k<16>(t);
    fill_tb_fused<2, 1>(t);
    fill_tb_fused<4, 2>(t);
    fill_tb_fused<10, 4>(t);
    fill_tb_fused<16, 4>(t);
    // the verified reconstructs of a lone degraded read (the survivors' R(row) with the rebuilt
    // rows, one block: the in-kernel combine and its completion flag) of fewer rows than m
    fill_tb_fused_inl<4, 1>(t);
    fill_tb_fused_inl<10, 1>(t);
    fill_tb_fused_inl<10, 2>(t);
    fill_tb_fused_inl<10, 3>(t);
    fill_tb_fused_inl<16, 1>(t);
    fill_tb_fused_inl<16, 2>(t);
    fill_tb_fused_inl<16, 3>(t);
}

}  // namespace rsmi
