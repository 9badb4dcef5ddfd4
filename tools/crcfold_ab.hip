// crcfold_ab.hip -- diagnostic A/B (not part of the product): two ways to fold a 16-byte chunk
// into its datanode CRC-16 value R(chunk) (howeyc IBM, reflected 0xA001, crc16.hpp).
//
//   nib   -- the product's fold (rs_crc16_kernels.hip crc_nib_chunk): 32 positional nibble lookups per
//            chunk in 16-entry u16 LDS tables (conflict-free), one byte extract per lookup.
//   vperm -- byte-transposed v_perm fold (VERDICT r1 item 3's candidate): a lane holds the same
//            chunk of 4 rows, transposes them so one dword carries byte p of all 4 rows, and runs
//            the byte-serial CRC on the 4 rows at once: per byte, the 3/3/2-bit split of
//            (state ^ byte) selects the table bytes of t[x] with 6 v_perm_b32 (low and high byte
//            of the 16-bit entry, three groups), as the encode kernel's GF tables do.  No LDS.
//
// Every lane folds chunk i of 4 rows for i = gid, gid + grid, ... and XORs the chunk values per
// row; both kernels must give identical results, and the small run checks every chunk value
// against a host byte loop.  Timed with HIP events over rows of BYTES bytes each (4 rows).
// Usage: crcfold_ab [MiB per row = 384] [iterations = 10]
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x)                                                                                    \
    do {                                                                                         \
        hipError_t e_ = (x);                                                                     \
        if (e_ != hipSuccess) {                                                                  \
            std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));       \
            std::exit(2);                                                                        \
        }                                                                                        \
    } while (0)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

static uint16_t T[256];
static void make_table() {
    for (int i = 0; i < 256; i++) {
        uint16_t c = uint16_t(i);
        for (int k = 0; k < 8; k++) c = (c & 1) ? uint16_t((c >> 1) ^ 0xA001) : uint16_t(c >> 1);
        T[i] = c;
    }
}
static uint16_t zbyte(uint16_t s) { return uint16_t((s >> 8) ^ T[s & 0xFF]); }  // one zero byte
static uint16_t host_chunk(const uint8_t* p) {
    uint16_t s = 0;
    for (int i = 0; i < 16; i++) s = uint16_t((s >> 8) ^ T[(s ^ p[i]) & 0xFF]);
    return s;
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// ---- nib: N[2p][v] = Z^(15-p)(t[v]), N[2p+1][v] = Z^(15-p)(t[16 v]); 32 x 16 u16 = 1 KiB
__device__ __forceinline__ uint32_t nib_chunk(const uint8_t* nb, const u32x4& v) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        uint32_t lo = (v[w] << 1) & 0x1E1E1E1Eu, hi = (v[w] >> 3) & 0x1E1E1E1Eu;
        asm volatile("" : "+v"(lo), "+v"(hi));
        uint32_t l[8];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int p = 4 * w + q;
            l[2 * q] = *reinterpret_cast<const uint16_t*>(nb + 64 * p + ((lo >> (8 * q)) & 0xFF));
            l[2 * q + 1] = *reinterpret_cast<const uint16_t*>(nb + 64 * p + 32 + ((hi >> (8 * q)) & 0xFF));
        }
        c = xor3(c, xor3(l[0], l[1], l[2]), xor3(l[3], l[4], l[5])) ^ (l[6] ^ l[7]);
    }
    return c;
}

__global__ __launch_bounds__(256) void k_nib(const uint16_t* __restrict__ ntbl, const uint8_t* __restrict__ rows,
                                             uint64_t row_bytes, uint64_t nchunks, uint32_t* __restrict__ out) {
    __shared__ uint16_t s[512];
    for (int i = threadIdx.x; i < 512; i += 256) s[i] = ntbl[i];
    __syncthreads();
    const uint8_t* nb = reinterpret_cast<const uint8_t*>(s);
    const uint64_t gid = uint64_t(blockIdx.x) * 256 + threadIdx.x, g = uint64_t(gridDim.x) * 256;
    uint32_t acc[4] = {0, 0, 0, 0};
    for (uint64_t i = gid; i < nchunks; i += g) {
        u32x4 v[4];
#pragma unroll
        for (int r = 0; r < 4; r++)
            v[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rows + r * row_bytes) + i);
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] ^= nib_chunk(nb, v[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) out[gid * 4 + r] = acc[r];
}

// ---- vperm: tables tv[0..9] = {L1 lo, L1 hi, L2 lo, L2 hi, L3, H1 lo, H1 hi, H2 lo, H2 hi, H3}
// L/H = low / high byte of t[i] (group 1), t[8 i] (group 2), t[64 i] (group 3), 4 entries a dword
__global__ __launch_bounds__(256) void k_vperm(const uint32_t* __restrict__ tv, const uint8_t* __restrict__ rows,
                                               uint64_t row_bytes, uint64_t nchunks, uint32_t* __restrict__ out) {
    uint32_t t[10];
#pragma unroll
    for (int i = 0; i < 10; i++) t[i] = __builtin_amdgcn_readfirstlane(tv[i]);
    const uint64_t gid = uint64_t(blockIdx.x) * 256 + threadIdx.x, g = uint64_t(gridDim.x) * 256;
    uint32_t accL = 0, accH = 0;  // byte r = row r
    for (uint64_t i = gid; i < nchunks; i += g) {
        u32x4 v[4];
#pragma unroll
        for (int r = 0; r < 4; r++)
            v[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rows + r * row_bytes) + i);
        uint32_t SL = 0, SH = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            // 4x4 byte transpose: D[q] byte r = byte q of row r's dword w
            const uint32_t ab_lo = __builtin_amdgcn_perm(v[1][w], v[0][w], 0x05010400u);
            const uint32_t ab_hi = __builtin_amdgcn_perm(v[1][w], v[0][w], 0x07030602u);
            const uint32_t cd_lo = __builtin_amdgcn_perm(v[3][w], v[2][w], 0x05010400u);
            const uint32_t cd_hi = __builtin_amdgcn_perm(v[3][w], v[2][w], 0x07030602u);
            uint32_t D[4];
            D[0] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u);
            D[1] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);
            D[2] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u);
            D[3] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t x = SL ^ D[q];
                const uint32_t s1 = x & 0x07070707u, s2 = (x >> 3) & 0x07070707u, s3 = (x >> 6) & 0x03030303u;
                const uint32_t l1 = __builtin_amdgcn_perm(t[1], t[0], s1), l2 = __builtin_amdgcn_perm(t[3], t[2], s2),
                               l3 = __builtin_amdgcn_perm(t[4], t[4], s3);
                const uint32_t h1 = __builtin_amdgcn_perm(t[6], t[5], s1), h2 = __builtin_amdgcn_perm(t[8], t[7], s2),
                               h3 = __builtin_amdgcn_perm(t[9], t[9], s3);
                SL = xor3(xor3(SH, l1, l2), l3, 0u);
                SH = xor3(h1, h2, h3);
            }
        }
        accL ^= SL;
        accH ^= SH;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) out[gid * 4 + r] = ((accL >> (8 * r)) & 0xFF) | (((accH >> (8 * r)) & 0xFF) << 8);
}

int main(int argc, char** argv) {
    const uint64_t mib = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 384;
    const int iters = argc > 2 ? std::atoi(argv[2]) : 10;
    make_table();
    // nibble tables
    std::vector<uint16_t> nt(512);
    for (int p = 0; p < 16; p++)
        for (int v = 0; v < 16; v++) {
            uint16_t a = T[v], b = T[v << 4];
            for (int z = 0; z < 15 - p; z++) {
                a = zbyte(a);
                b = zbyte(b);
            }
            nt[size_t(2 * p) * 16 + v] = a;
            nt[size_t(2 * p + 1) * 16 + v] = b;
        }
    // v_perm byte tables
    uint32_t tv[10] = {};
    for (int i = 0; i < 8; i++) {
        tv[0 + i / 4] |= uint32_t(T[i] & 0xFF) << (8 * (i % 4));
        tv[2 + i / 4] |= uint32_t(T[i << 3] & 0xFF) << (8 * (i % 4));
        tv[5 + i / 4] |= uint32_t(T[i] >> 8) << (8 * (i % 4));
        tv[7 + i / 4] |= uint32_t(T[i << 3] >> 8) << (8 * (i % 4));
    }
    for (int i = 0; i < 4; i++) {
        tv[4] |= uint32_t(T[i << 6] & 0xFF) << (8 * i);
        tv[9] |= uint32_t(T[i << 6] >> 8) << (8 * i);
    }
    uint16_t* d_nt;
    uint32_t* d_tv;
    CK(hipMalloc(&d_nt, 1024));
    CK(hipMalloc(&d_tv, 40));
    CK(hipMemcpy(d_nt, nt.data(), 1024, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_tv, tv, 40, hipMemcpyHostToDevice));
    int dev;
    CK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, dev));
    const int ncu = prop.multiProcessorCount;

    // 1) exactness: every chunk value of a small run against the host loop (grid = nchunks lanes)
    {
        const uint64_t nch = 1 << 16, rb = nch * 16;
        std::vector<uint8_t> h(4 * rb);
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (auto& b : h) {
            x ^= x << 13;
            x ^= x >> 7;
            x ^= x << 17;
            b = uint8_t(x);
        }
        uint8_t* d;
        uint32_t *o1, *o2;
        CK(hipMalloc(&d, 4 * rb));
        CK(hipMalloc(&o1, nch * 16));
        CK(hipMalloc(&o2, nch * 16));
        CK(hipMemcpy(d, h.data(), 4 * rb, hipMemcpyHostToDevice));
        k_nib<<<nch / 256, 256>>>(d_nt, d, rb, nch, o1);
        k_vperm<<<nch / 256, 256>>>(d_tv, d, rb, nch, o2);
        CK(hipDeviceSynchronize());
        std::vector<uint32_t> a(nch * 4), b(nch * 4);
        CK(hipMemcpy(a.data(), o1, nch * 16, hipMemcpyDeviceToHost));
        CK(hipMemcpy(b.data(), o2, nch * 16, hipMemcpyDeviceToHost));
        uint64_t bad = 0;
        for (uint64_t i = 0; i < nch; i++)
            for (int r = 0; r < 4; r++) {
                const uint32_t want = host_chunk(h.data() + r * rb + i * 16);
                bad += (a[i * 4 + r] != want) + (b[i * 4 + r] != want);
            }
        std::printf("exactness: %llu chunk values x 2 folds, %llu wrong\n", (unsigned long long)(nch * 4),
                    (unsigned long long)bad);
        CK(hipFree(d));
        CK(hipFree(o1));
        CK(hipFree(o2));
        if (bad) return 1;
    }
    // 2) throughput over 4 rows of `mib` MiB in HBM, a persistent grid of 8 waves per SIMD
    const uint64_t rb = mib << 20, nch = rb / 16;
    uint8_t* d;
    CK(hipMalloc(&d, 4 * rb));
    CK(hipMemset(d, 0x5A, 4 * rb));
    const uint32_t grid = uint32_t(ncu) * 8;
    uint32_t *o1, *o2;
    CK(hipMalloc(&o1, size_t(grid) * 256 * 16));
    CK(hipMalloc(&o2, size_t(grid) * 256 * 16));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int kind = 0; kind < 2; kind++) {
        auto run = [&] {
            if (kind == 0)
                k_nib<<<grid, 256>>>(d_nt, d, rb, nch, o1);
            else
                k_vperm<<<grid, 256>>>(d_tv, d, rb, nch, o2);
        };
        run();
        CK(hipEventRecord(e0));
        for (int i = 0; i < iters; i++) run();
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        const double us = 1e3 * ms / iters;
        std::printf("%-6s %10.1f us  %8.1f GB/s of row bytes (4 x %llu MiB)\n", kind ? "vperm" : "nib", us,
                    4.0 * double(rb) / (us * 1e3), (unsigned long long)mib);
    }
    std::vector<uint32_t> a(size_t(grid) * 1024), b(size_t(grid) * 1024);
    CK(hipMemcpy(a.data(), o1, a.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), o2, b.size() * 4, hipMemcpyDeviceToHost));
    std::printf("large run: folds agree: %s\n", a == b ? "yes" : "NO");
    return a == b ? 0 : 1;
}
