// Stand-alone check of the loss-term planner (wild_deep_mvs_amd/csrc/loss_plan.h), meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/dev/loss_plan_check.cpp -o loss_plan_check && ./loss_plan_check
// Walks the planner over good and bad tables (exact-size heap arrays, so that a read past n entries is an error the sanitizer
// sees) and checks the block prefix: every term owns ceil(pixels / chunk) blocks, at most LOSS_MAX_BLOCKS_PER_TERM.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../wild_deep_mvs_amd/csrc/loss_plan.h"

using namespace pscv;

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool plan_of(const std::vector<int>& kinds, const std::vector<long>& dims, LossPlan& plan, int n = -1) {
    // exact-size copies on the heap: one element too far is a heap-buffer-overflow
    int* k = (int*)std::malloc(kinds.size() * sizeof(int) + (kinds.empty() ? 1 : 0));
    long* d = (long*)std::malloc(dims.size() * sizeof(long) + (dims.empty() ? 1 : 0));
    if (!kinds.empty()) std::memcpy(k, kinds.data(), kinds.size() * sizeof(int));
    if (!dims.empty()) std::memcpy(d, dims.data(), dims.size() * sizeof(long));
    const bool ok = loss_plan(n < 0 ? (int)kinds.size() : n, k, d, plan);
    std::free(k);
    std::free(d);
    return ok;
}

int main() {
    LossPlan plan;
    // the fixture's shapes: 2304 pixels = 3 blocks (the last one ragged), 144 pixels = 1 block, an L term of 6912 = 7 blocks
    EXPECT(plan_of({0, 1, 3}, {2, 24, 48, 24, 48, 2, 6, 12, 24, 48, 6912, 1, 1, 0, 0}, plan));
    EXPECT(plan.n_terms == 3 && plan.blk_start[0] == 0 && plan.blk_start[1] == 3 && plan.blk_start[2] == 4 && plan.blk_start[3] == 11);
    EXPECT(plan.rh[0] == 1 && plan.rw[0] == 1 && plan.rh[1] == 4 && plan.rw[1] == 4 && plan.rh[2] == 1 && plan.npix[2] == 6912);
    // mixed ratios, exact multiples of the chunk, the cap
    EXPECT(plan_of({0, 0, 2, 2}, {1, 12, 48, 24, 48, 1, 2, 4, 24, 8, LOSS_CHUNK, 1, 1, 0, 0, (long)LOSS_CHUNK * 1000 + 1, 1, 1, 0, 0}, plan));
    EXPECT(plan.rh[0] == 2 && plan.rw[0] == 1 && plan.rh[1] == 12 && plan.rw[1] == 2);
    EXPECT(plan.blk_start[3] - plan.blk_start[2] == 1 && plan.blk_start[4] - plan.blk_start[3] == LOSS_MAX_BLOCKS_PER_TERM);
    // 32 terms of the largest size: the prefix stays in range
    {
        std::vector<int> kinds(LOSS_MAX_TERMS, 3);
        std::vector<long> dims;
        for (int t = 0; t < LOSS_MAX_TERMS; ++t) { const long d[5] = {0x7fffffffL, 1, 1, 0, 0}; dims.insert(dims.end(), d, d + 5); }
        EXPECT(plan_of(kinds, dims, plan) && plan.blk_start[LOSS_MAX_TERMS] == LOSS_MAX_TERMS * LOSS_MAX_BLOCKS_PER_TERM);
        for (int t = 0; t < LOSS_MAX_TERMS; ++t) EXPECT(plan.blk_start[t + 1] > plan.blk_start[t]);
        kinds.push_back(3);
        dims.insert(dims.end(), {4, 1, 1, 0, 0});
        EXPECT(!plan_of(kinds, dims, plan) && plan.error && std::strstr(plan.error, "32 terms") && plan.n_terms == 0);
    }
    // every rejection
    EXPECT(!loss_plan(1, nullptr, nullptr, plan) && std::strstr(plan.error, "null pointer"));
    EXPECT(!plan_of({}, {}, plan, 0) && std::strstr(plan.error, "no terms"));
    EXPECT(!plan_of({}, {}, plan, -3) && std::strstr(plan.error, "no terms"));
    EXPECT(!plan_of({0, 5}, {2, 6, 12, 24, 48, 2, 6, 12, 24, 48}, plan) && std::strstr(plan.error, "unknown kind") && plan.error_term == 1);
    EXPECT(!plan_of({-1}, {2, 6, 12, 24, 48}, plan) && std::strstr(plan.error, "unknown kind"));
    EXPECT(!plan_of({0}, {2, 7, 12, 24, 48}, plan) && std::strstr(plan.error, "non-integer ratio") && plan.error_term == 0);
    EXPECT(!plan_of({1}, {2, 6, 13, 24, 48}, plan) && std::strstr(plan.error, "non-integer ratio"));
    EXPECT(!plan_of({1}, {2, 48, 96, 24, 48}, plan) && std::strstr(plan.error, "non-integer ratio"));       // an upsampling "ratio" of 1/2
    EXPECT(plan_of({2}, {2, 7, 13, 24, 48}, plan));                                                            // the L kinds ignore H, W
    const long bad[][5] = {{0, 6, 12, 24, 48}, {2, 0, 12, 24, 48}, {2, 6, 0, 24, 48}, {2, 6, 12, 0, 48}, {2, 6, 12, 24, 0}, {-2, 6, 12, 24, 48},
                           {2, 6, 12, -24, 48}};
    for (const auto& d : bad) EXPECT(!plan_of({0}, std::vector<long>(d, d + 5), plan) && std::strstr(plan.error, "size"));
    EXPECT(!plan_of({2}, {0x80000000L, 1, 1, 0, 0}, plan) && std::strstr(plan.error, "2^31"));
    EXPECT(!plan_of({2}, {1L << 40, 1L << 40, 1L << 40, 0, 0}, plan) && std::strstr(plan.error, "2^31"));       // no overflow on the way
    EXPECT(!plan_of({2}, {65536, 65536, 1, 0, 0}, plan) && std::strstr(plan.error, "2^31"));
    EXPECT(!plan_of({0}, {1, 1, 1, 1L << 20, 1L << 20}, plan) && std::strstr(plan.error, "2^31"));
    std::printf(failures ? "%d checks FAILED\n" : "loss_plan: all checks passed\n", failures);
    return failures ? 1 : 0;
}
