// Unit checks of object_slam_amd/csrc/stage_layout.h (host C++, no HIP, no GPU): the layout rules every host-pointer entry point of the batched
// solver operators and every operator of the driver's table relies on, one case pinned by hand, the put / get round trip, the row helper of the
// slot-major fields, and the byte layout of the resident keyframe record (kf_record_layout.h) at two capacities.  Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/oslam_hip.h"
#include "../object_slam_amd/csrc/kf_record_layout.h"
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

// a slot-major field: 3 rows of stride 5 of a 12-byte element behind a 4-byte field, worked out by hand; an absent field has no rows
static void check_rows() {
    struct P3 { float x, y, z; };
    static_assert(sizeof(P3) == 12, "12-byte element");
    StageLayout lay;
    const auto fHead = lay.add<int32_t>(1);
    const auto fRows = lay.add<P3>(3 * 5);
    const auto fNone = lay.add<P3>(3 * 5, false);
    CHECK(fHead.off == 0 && fRows.off == 256 && lay.total() == 512);
    std::vector<uint8_t> blk(lay.total(), 0xAB);
    CHECK((uint8_t*)row(fRows, blk.data(), 5, 2) == blk.data() + 256 + 2 * 5 * 12);
    CHECK((uint8_t*)row(fRows, blk.data(), 5, 0) == (uint8_t*)at(fRows, blk.data()));
    CHECK(row(fNone, blk.data(), 5, 2) == nullptr && row(fNone, blk.data(), 5, 0) == nullptr);
    // a job's share of its row, in and out: 4 of the 5 elements; the fifth and the neighbouring rows stay as they were
    const P3 src[4] = {{1, 2, 3}, {4, 5, 6}, {7, 8, 9}, {10, 11, 12}};
    oslam::copy_elems(row(fRows, blk.data(), 5, 1), src, 4);
    oslam::copy_elems(row(fRows, blk.data(), 5, 1), (const P3*)nullptr, 0);   // nothing to copy: no read through the NULL pointer
    for (size_t i = 0; i < blk.size(); i++) if (i < 256 + 5 * 12 || i >= 256 + 5 * 12 + 4 * 12) CHECK(blk[i] == 0xAB);
    P3 back[4] = {};
    oslam::copy_elems(back, (const P3*)row(fRows, blk.data(), 5, 1), 4);
    for (int i = 0; i < 4; i++) CHECK(back[i].x == src[i].x && back[i].y == src[i].y && back[i].z == src[i].z);
}

// the resident keyframe record: offsets worked out by hand from the chain of align_up(.., 256) links the operator table had before kf_record_layout.h
// (28-byte keypoints, 32-byte descriptors, 3072 16-bit cell ends, 16-byte candidates, int32 point list, 64-bit observer cells, one depth bit per keypoint)
static void check_kf_record() {
    static_assert(sizeof(oslam_keypoint_t) == 28, "the offsets below are for 28-byte keypoints");
    struct Want { size_t cap, keys, desc, ur, cell_end, cand, mp, okf, good, bytes, okf_from_mp, good_from_mp; };
    const Want want[2] = {
        {1000, 0, 28160, 60160, 64256, 70400, 86528, 90624, 98816, 99072, 4096, 12288},
        // 1033 (no multiple of 64): 28924 -> 28928, 33056 -> 33280, 4132 -> 4352, 6144, 16528 -> 16640, 4132 -> 4352, 8264 -> 8448, 33 words = 132 -> 256
        {1033, 0, 28928, 62208, 66560, 72704, 89344, 93696, 102144, 102400, 4352, 12800},
    };
    for (const Want& w : want) {
        const oslam::KfRecordLayout r(w.cap);
        CHECK(r.keys.off == w.keys && r.desc.off == w.desc && r.ur.off == w.ur && r.cell_end.off == w.cell_end && r.cand.off == w.cand);
        CHECK(r.mp.off == w.mp && r.core_bytes() == w.mp && r.okf.off == w.okf && r.good.off == w.good && r.bytes == w.bytes);
        CHECK(r.okf_from_mp() == w.okf_from_mp && r.good_from_mp() == w.good_from_mp);
        CHECK(r.keys.bytes == w.cap * 28 && r.desc.bytes == w.cap * 32 && r.ur.bytes == w.cap * 4 && r.cell_end.bytes == 6144 && r.cand.bytes == w.cap * 16);
        CHECK(r.mp.bytes == w.cap * 4 && r.okf.bytes == w.cap * 8 && r.good.bytes == (w.cap + 31) / 32 * 4);
        check_rules({span(r.keys), span(r.desc), span(r.ur), span(r.cell_end), span(r.cand), span(r.mp), span(r.okf), span(r.good)}, r.bytes);
    }
    CHECK(oslam::KfRecordLayout().bytes == 6144);   // a handle without a capacity yet: only the grid's fixed cell table
}

int main() {
    check_sim3_case();
    check_general();
    check_round_trip();
    check_rows();
    check_kf_record();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("stage_layout_check: ok\n");
    return 0;
}
