// The coding kernels' workgroup -> tile-group mapping (rs_plan.hpp: tile_group, launch_head) on the
// host, with its own main: built plain and with -fsanitize=address,undefined by
// tests/test_tile_order.py.  Exit status 0 and a last line "ok" on success.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rs_plan.hpp"

using namespace rsmi;

static int fails = 0;
#define CHECK(cond, ...)                        \
    do {                                        \
        if (!(cond)) {                          \
            if (fails++ < 20) {                 \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);       \
                std::printf("\n");              \
            }                                   \
        }                                       \
    } while (0)

// tile_group over [0, grid) with this head: a permutation; within the head, the workgroups of
// one XCD (equal wg & 7) take consecutive groups starting at (wg & 7) * head / 8; past it, wg
static void check_pair(uint32_t grid, uint32_t head, std::vector<uint32_t>& stamp, uint32_t id) {
    uint32_t bad = 0, prev[8] = {};
    // the head maps onto [0, head) without a repeat, the rest onto itself: a permutation of [0, grid)
    for (uint32_t wg = 0; wg < head; wg++) {
        const uint32_t g = tile_group(wg, grid, head);
        if (g >= head) {
            bad++;
            continue;
        }
        bad += stamp[g] == id;  // hit twice
        stamp[g] = id;
        if (wg < 8) bad += g != wg * (head >> 3);
        else bad += g != prev[wg & 7u] + 1u;
        prev[wg & 7u] = g;
    }
    for (uint32_t wg = head; wg < grid; wg++) bad += tile_group(wg, grid, head) != wg;
    CHECK(bad == 0, "grid %u head %u: %u workgroups off", grid, head, bad);
}

struct Shape {
    const char* name;
    int k, m, lost;
    uint64_t block_bytes, nblocks;
};

int main() {
    constexpr uint32_t kMaxGrid = 4200;
    std::vector<uint32_t> stamp(kMaxGrid, 0);
    uint32_t id = 0, pairs = 0;
    for (uint32_t grid = 1; grid <= kMaxGrid; grid++)
        for (uint32_t head = 0; head <= grid; head += 8) {
            check_pair(grid, head, stamp, ++id);
            pairs++;
        }
    // head = 0 is the identity
    for (uint32_t grid = 1; grid <= kMaxGrid; grid++)
        for (uint32_t wg = 0; wg < grid; wg++) CHECK(tile_group(wg, grid, 0) == wg, "grid %u wg %u", grid, wg);

    // launch_head: a multiple of 8 and <= grid, for the BASELINE shapes' grids (bench.py CONFIGS:
    // S = ceil(block / k), one tile per wave) and for small and the largest grids, every layout
    const Shape shapes[] = {{"rs10_4_256k", 10, 4, 1, 256 << 10, 4096},
                            {"rs4_2_256k", 4, 2, 0, 256 << 10, 4096},
                            {"rs10_4_1m", 10, 4, 0, 1024 << 10, 1024},
                            {"rs16_4_4m", 16, 4, 2, 4096 << 10, 256},
                            {"rs2_1_256k", 2, 1, 1, 256 << 10, 4096}};
    constexpr uint32_t wpg = kFastWG / kWave;
    auto check_head = [&](uint32_t grid, int K, int MT, uint32_t S, const char* what) {
        for (int ua = 0; ua < 2; ua++)
            for (int strided = 0; strided < 2; strided++) {
                const uint32_t head = launch_head(grid, K, MT, S, ua != 0, strided != 0);
                CHECK(head % 8 == 0 && head <= grid, "%s grid %u K %d MT %d ua %d strided %d: head %u", what, grid, K,
                      MT, ua, strided, head);
                if (!ua && strided) CHECK(head == 0, "%s: strided aligned launch with head %u", what, head);
                if (ua) CHECK(head == (grid % 8 == 0 ? grid : 0), "%s: ua head %u of grid %u", what, head, grid);
            }
    };
    for (const Shape& s : shapes) {
        const uint64_t S = (s.block_bytes + s.k - 1) / s.k;
        const uint64_t tpb = ((S + 15) / 16 + kWave - 1) / kWave;
        const uint32_t grid = uint32_t((s.nblocks * tpb + wpg - 1) / wpg);
        check_head(grid, s.k, s.m, uint32_t(S), s.name);
        if (s.lost) check_head(grid, s.k, s.lost, uint32_t(S), s.name);
        // the largest launch of this shape: 2^31 / tpb blocks (launch_plan splits there)
        const uint64_t maxb = (uint64_t(1) << 31) / tpb;
        check_head(uint32_t((maxb * tpb + wpg - 1) / wpg), s.k, s.m, uint32_t(S), s.name);
        for (uint32_t g : {1u, 7u, 8u, 9u}) check_head(g, s.k, s.m, uint32_t(S), s.name);
    }
    // any shape at the largest grids a launch can have, where grid * num must not wrap
    for (int K : {1, 2, 4, 10, 16})
        for (int MT = 1; MT <= 4; MT++)
            for (uint32_t g : {1u, 7u, 8u, 9u, (1u << 31) / wpg, (1u << 31) / wpg + 1, 0xFFFFFFF8u, 0xFFFFFFFFu})
                check_head(g, K, MT, 26215, "any");

    std::printf("%u (grid, head) pairs, %d failures\n", pairs, fails);
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
