// Unit checks of object_slam_amd/csrc/stage_layout.h (host C++, no HIP, no GPU): the layout rules every host-pointer entry point of the batched
// solver operators relies on, one case pinned by hand, and the put / get round trip.  Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/oslam_hip.h"
#include "../object_slam_amd/csrc/stage_layout.h"

using oslam::Field;
using oslam::StageLayout;

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

struct Span { size_t off, bytes; };
template <class T> static Span span(const Field<T>& f) { return {f.off, f.bytes}; }
static size_t round256(size_t b) { return (b + 255) / 256 * 256; }

// every offset a multiple of 256; fields disjoint and in declaration order; a zero-byte field takes no room (it shares its offset with the next field);
// the total is the sum of the rounded sizes
static void check_rules(const std::vector<Span>& f, size_t total) {
    size_t sum = 0;
    for (size_t i = 0; i < f.size(); i++) {
        CHECK(f[i].off % 256 == 0);
        CHECK(f[i].off == sum);   // in order, nothing between the fields but the rounding
        const size_t next = i + 1 < f.size() ? f[i + 1].off : total;
        CHECK(f[i].off + f[i].bytes <= next);
        if (f[i].bytes == 0) CHECK(next == f[i].off);
        sum += round256(f[i].bytes);
    }
    CHECK(total == sum);
}

// oslam_sim3_iterate_batch's block for 3 problems, 70 correspondences, max_iterations = 300 and no optional array, worked out by hand from the chain of
// align_up(.., 256) links the entry point had before this header
static void check_sim3_case() {
    const size_t np = 3, nc = 70, its = 300;
    const bool samples = false, iter_inliers = false, hypotheses = false;
    StageLayout lay;
    const auto fProb = lay.add<oslam_sim3_problem_t>(np);
    const auto fX1 = lay.add<float>(nc * 3), fX2 = lay.add<float>(nc * 3), fS1 = lay.add<float>(nc), fS2 = lay.add<float>(nc);
    const auto fSam = lay.add<int32_t>(np * its * 3, samples);
    const auto fState = lay.add<oslam_sim3_state_t>(np);
    const auto fSt = lay.add<int32_t>(np * 4);
    const auto fT = lay.add<float>(np * 16);
    const auto fIn = lay.add<uint8_t>(nc);
    const auto fIt = lay.add<int32_t>(np * its, iter_inliers);
    const auto fHy = lay.add<float>(np * its * 13, hypotheses);
    const std::vector<Span> f = {span(fProb), span(fX1), span(fX2), span(fS1), span(fS2), span(fSam), span(fState), span(fSt), span(fT), span(fIn), span(fIt), span(fHy)};
    const size_t bytes[12] = {144, 840, 840, 280, 280, 0, 192, 48, 192, 70, 0, 0};
    const size_t offs[12] = {0, 256, 1280, 2304, 2816, 3328, 3328, 3584, 3840, 4096, 4352, 4352};
    for (int i = 0; i < 12; i++) { CHECK(f[i].bytes == bytes[i]); CHECK(f[i].off == offs[i]); }
    CHECK(lay.total() == 4352);
    check_rules(f, lay.total());
    uint8_t base[1] = {0};
    CHECK(at(fSam, base) == nullptr && at(fIt, base) == nullptr && at(fHy, base) == nullptr);   // an absent optional array is a NULL pointer
    CHECK((void*)at(fProb, base) == (void*)base);

    // the same block with all three optional arrays
    StageLayout all;
    all.add<oslam_sim3_problem_t>(np); all.add<float>(nc * 3); all.add<float>(nc * 3); all.add<float>(nc); all.add<float>(nc);
    const auto gSam = all.add<int32_t>(np * its * 3, true);
    const auto gState = all.add<oslam_sim3_state_t>(np);
    CHECK(gSam.off == 3328 && gSam.bytes == 10800 && gState.off == 3328 + 11008);   // 10800 = 42 * 256 + 48
}

// odd sizes, sizes on both sides of a multiple of 256, empty fields at the start, in the middle, next to each other and at the end
static void check_general() {
    const size_t counts[] = {0, 1, 255, 256, 257, 0, 0, 3, 512, 1000, 0};
    StageLayout lay;
    std::vector<Span> f;
    for (size_t c : counts) {
        f.push_back(span(lay.add<uint8_t>(c)));
        f.push_back(span(lay.add<double>(c)));
        f.push_back(span(lay.add<float>(c * 3, c % 2 == 1)));
    }
    check_rules(f, lay.total());
    CHECK(StageLayout().total() == 0);
    StageLayout empty;
    const auto e = empty.add<float>(0);
    uint8_t base[1] = {0};
    CHECK(e.off == 0 && e.bytes == 0 && empty.total() == 0);
    CHECK((void*)at(e, base) == (void*)base);   // present with zero elements: an address, not NULL
}

// two typed fields through a plain byte vector standing in for the pinned block
static void check_round_trip() {
    StageLayout lay;
    const auto fA = lay.add<float>(5);
    const auto fNone = lay.add<int32_t>(7, false);
    const auto fB = lay.add<int32_t>(100);
    std::vector<uint8_t> blk(lay.total(), 0xAB);
    const float a[5] = {1.5f, -2.f, 3.25f, 0.f, 1e-3f};
    int32_t b[100];
    for (int i = 0; i < 100; i++) b[i] = i * i - 50;
    put(fA, blk.data(), a);
    put(fNone, blk.data(), (const int32_t*)nullptr);   // skipped: no read through the NULL pointer
    put(fB, blk.data(), b);
    for (size_t i = fA.end(); i < fB.off; i++) CHECK(blk[i] == 0xAB);   // the padding between the fields is not written
    for (size_t i = fB.end(); i < blk.size(); i++) CHECK(blk[i] == 0xAB);
    float a2[5] = {0};
    int32_t b2[100] = {0};
    get(fA, blk.data(), a2);
    get(fNone, blk.data(), (int32_t*)nullptr);
    get(fB, blk.data(), b2);
    for (int i = 0; i < 5; i++) CHECK(a2[i] == a[i]);
    for (int i = 0; i < 100; i++) CHECK(b2[i] == b[i]);
    CHECK(at(fB, blk.data())[99] == 99 * 99 - 50 && at(fA, blk.data())[2] == 3.25f);
}

int main() {
    check_sim3_case();
    check_general();
    check_round_trip();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("stage_layout_check: ok\n");
    return 0;
}
