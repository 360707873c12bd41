// Unit checks of object_slam_amd/csrc/loop_parent_check.h (host C++, no HIP, no GPU): the walk over a spanning-tree `parent` array that the host entry
// point of the map update after global BA runs before it launches anything.  Built with -fsanitize=address,undefined by tests/test_loop_closing_cpu.py.
// Every array lives in an exactly sized heap block, so a read past either end is an error the sanitizer reports.  Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../object_slam_amd/csrc/loop_parent_check.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

static int run(std::initializer_list<int32_t> parent) {
    std::vector<int32_t> p(parent);
    p.shrink_to_fit();
    std::vector<uint8_t> mark;
    return oslam::parent_tree_check(p.data(), (int)p.size(), mark);
}

int main() {
    using namespace oslam;
    // valid trees: empty, a single root, a chain, a chain stored backwards, a branching tree, two roots
    CHECK(run({}) == kParentOk);
    CHECK(run({-1}) == kParentOk);
    CHECK(run({-1, 0, 1, 2, 3, 4}) == kParentOk);
    CHECK(run({1, 2, 3, 4, 5, -1}) == kParentOk);
    CHECK(run({-1, 0, 0, 1, 1, 2, 2, 3, 5, 5}) == kParentOk);
    CHECK(run({-1, 0, 1, -1, 3, 4, 4}) == kParentOk);
    // cycles: a self-parent, a pair, a ring of every keyframe, a ring behind a valid root, a tail that leads into a ring
    CHECK(run({0}) == kParentCycle);
    CHECK(run({-1, 1}) == kParentCycle);
    CHECK(run({1, 0}) == kParentCycle);
    CHECK(run({1, 2, 3, 0}) == kParentCycle);
    CHECK(run({-1, 0, 1, 4, 3, 4}) == kParentCycle);
    CHECK(run({-1, 2, 3, 4, 2, 1}) == kParentCycle);
    // indices out of range: below -1, n, far outside either way (never followed)
    CHECK(run({-2}) == kParentOutOfRange);
    CHECK(run({-1, 2}) == kParentOutOfRange);
    CHECK(run({-1, 0, 3}) == kParentOutOfRange);
    CHECK(run({-1, 0, 2147483647}) == kParentOutOfRange);
    CHECK(run({-1, -2147483647 - 1, 0}) == kParentOutOfRange);
    // a long chain: the walk is a loop, not a recursion
    {
        const int n = 200000;
        std::vector<int32_t> p((size_t)n);
        for (int k = 0; k < n; k++) p[(size_t)k] = k + 1 < n ? k + 1 : -1;
        std::vector<uint8_t> mark;
        CHECK(parent_tree_check(p.data(), n, mark) == kParentOk);
        p[(size_t)n - 1] = 0;
        CHECK(parent_tree_check(p.data(), n, mark) == kParentCycle);
    }
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("loop_parent_check: ok\n");
    return 0;
}
