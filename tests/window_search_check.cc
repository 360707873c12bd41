// Unit checks of object_slam_amd/csrc/window_search_host.h (host C++, no HIP, no GPU): the code and the precedence of every refusal the windowed projection
// searches share, the boundary values that must be accepted, and the camera block.  Exit status 0 = all checks passed.
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../object_slam_amd/csrc/window_search_host.h"

static std::string g_error;
void oslam::set_error(const char* fmt, ...) {   // the library's keeps the message per thread; this one keeps the last
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

using namespace oslam::kf_stage;

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (last error: %s)\n", __FILE__, __LINE__, #cond, g_error.c_str()); g_failed++; } \
    } while (0)

static bool said(const char* part) { return g_error.find(part) != std::string::npos; }

struct Handle { int max_problems, max_kps, max_pts; };
struct Rows { int n_rows; };

static const oslam_camera_t kCam = {500.f, 510.f, 320.f, 240.f, 0.f, 0.f};
static const float kBounds[4] = {-10.f, -20.f, 630.f, 460.f};
static const float kScale[3] = {1.f, 1.2f, 1.44f};
static const float kLog = 0.18232156f;

// the call's refusals in their order: every later fault is present too, and the earlier one is reported
static void check_call_refusals() {
    const Handle h = {4, 100, 50};
    const Rows kp = {10}, pts = {20};
    const float empty_x[4] = {5.f, 0.f, 5.f, 10.f}, empty_y[4] = {0.f, 7.f, 10.f, 7.f}, nan_b[4] = {0.f, 0.f, NAN, 10.f};
    const auto call = [&](const Handle* hh, int n_problems, const Rows* k, const Rows* p, int n_pt_out, int n_kp_out, const oslam_camera_t* cam, const float* bounds, const float* sf, int nlevels,
                          float logsf) { return check_proj_call("fn", hh, n_problems, k, "frame", p, n_pt_out, "skip", n_kp_out, cam, bounds, sf, nlevels, logsf); };
    CHECK(call(&h, 4, &kp, &pts, 50, 7, &kCam, kBounds, kScale, 3, kLog) == OSLAM_OK);   // at every capacity
    CHECK(call(&h, 0, &kp, &pts, 0, 0, &kCam, kBounds, kScale, 1, kLog) == OSLAM_OK && call(&h, 1, &kp, &pts, 0, 0, &kCam, kBounds, kScale, OSLAM_MAX_LEVELS, kLog) == OSLAM_OK);
    // 1. NULL before everything (the counts are bad too)
    const Rows neg = {-1};
    CHECK(call(nullptr, -1, &kp, &pts, 0, 0, &kCam, kBounds, kScale, 3, kLog) == OSLAM_E_INVALID && said("fn: NULL argument"));
    CHECK(call(&h, -1, nullptr, &pts, 0, 0, &kCam, kBounds, kScale, 3, kLog) == OSLAM_E_INVALID && call(&h, -1, &kp, nullptr, 0, 0, &kCam, kBounds, kScale, 3, kLog) == OSLAM_E_INVALID);
    CHECK(call(&h, -1, &kp, &pts, 0, 0, nullptr, kBounds, kScale, 3, kLog) == OSLAM_E_INVALID && call(&h, -1, &kp, &pts, 0, 0, &kCam, nullptr, kScale, 3, kLog) == OSLAM_E_INVALID);
    CHECK(call(&h, -1, &kp, &pts, 0, 0, &kCam, kBounds, nullptr, 3, kLog) == OSLAM_E_INVALID && said("NULL argument"));
    // 2. a negative count (too many problems, too)
    CHECK(call(&h, -1, &kp, &pts, 0, 0, &kCam, kBounds, kScale, 0, kLog) == OSLAM_E_CAPACITY && said("none may be negative") && said("10 frame rows"));
    CHECK(call(&h, 9, &neg, &pts, 0, 0, &kCam, kBounds, kScale, 3, kLog) == OSLAM_E_CAPACITY && said("none may be negative"));
    CHECK(call(&h, 9, &kp, &neg, 0, 0, &kCam, kBounds, kScale, 3, kLog) == OSLAM_E_CAPACITY && said("none may be negative"));
    CHECK(call(&h, 9, &kp, &pts, -1, 0, &kCam, kBounds, kScale, 3, kLog) == OSLAM_E_CAPACITY && said("none may be negative"));
    CHECK(call(&h, 9, &kp, &pts, 0, INT_MIN, &kCam, kBounds, kScale, 3, kLog) == OSLAM_E_CAPACITY && said("none may be negative"));
    // 3. more problems than the handle has (more points, too)
    const Rows many = {51};
    CHECK(call(&h, 5, &kp, &many, 0, 0, &kCam, kBounds, kScale, 3, kLog) == OSLAM_E_CAPACITY && said("5 problems exceed the handle's 4"));
    // 4. more points than the handle has (bad nlevels, too)
    CHECK(call(&h, 4, &kp, &many, 0, 0, &kCam, kBounds, kScale, 0, kLog) == OSLAM_E_CAPACITY && said("51 point rows / 0 skip rows exceed the handle's max_points_total 50"));
    CHECK(call(&h, 4, &kp, &pts, 51, 0, &kCam, kBounds, kScale, 0, kLog) == OSLAM_E_CAPACITY && said("max_points_total"));
    // 5. nlevels (empty bounds, too)
    CHECK(call(&h, 4, &kp, &pts, 0, 0, &kCam, empty_x, kScale, 0, kLog) == OSLAM_E_INVALID && said("nlevels = 0 outside [1, 16]"));
    CHECK(call(&h, 4, &kp, &pts, 0, 0, &kCam, empty_x, kScale, OSLAM_MAX_LEVELS + 1, kLog) == OSLAM_E_INVALID && said("nlevels"));
    // 6. empty bounds (bad logScaleFactor, too); NaN is empty
    CHECK(call(&h, 4, &kp, &pts, 0, 0, &kCam, empty_x, kScale, 3, 0.f) == OSLAM_E_INVALID && said("empty image bounds"));
    CHECK(call(&h, 4, &kp, &pts, 0, 0, &kCam, empty_y, kScale, 3, 0.f) == OSLAM_E_INVALID && said("empty image bounds"));
    CHECK(call(&h, 4, &kp, &pts, 0, 0, &kCam, nan_b, kScale, 3, 0.f) == OSLAM_E_INVALID && said("empty image bounds"));
    // 7. logScaleFactor
    CHECK(call(&h, 4, &kp, &pts, 0, 0, &kCam, kBounds, kScale, 3, 0.f) == OSLAM_E_INVALID && said("logScaleFactor must be positive"));
    CHECK(call(&h, 4, &kp, &pts, 0, 0, &kCam, kBounds, kScale, 3, -1.f) == OSLAM_E_INVALID && call(&h, 4, &kp, &pts, 0, 0, &kCam, kBounds, kScale, 3, NAN) == OSLAM_E_INVALID);
    // the three camera refusals alone, as SearchBySim3 makes them after its own
    CHECK(check_window("fn", kBounds, 3, kLog) == OSLAM_OK && check_window("fn", empty_x, 17, 0.f) == OSLAM_E_INVALID && said("nlevels"));
    CHECK(check_window("fn", empty_x, 3, 0.f) == OSLAM_E_INVALID && said("bounds") && check_window("fn", kBounds, 3, 0.f) == OSLAM_E_INVALID && said("logScaleFactor"));
}

template <class P> static P record(int n_kp, int kp_off, int n_pts, int pt_off, int kp_out_off, int pt_out_off) {
    P p;
    memset(&p, 0, sizeof p);
    p.n_kp = n_kp; p.kp_off = kp_off; p.n_pts = n_pts; p.pt_off = pt_off; p.kp_out_off = kp_out_off; p.pt_out_off = pt_out_off;
    return p;
}

template <class P> static void check_records() {
    const auto none = [](int, const P&) { return (int)OSLAM_OK; };
    const ProjExtent e = {100, 300, 500, 40, 60, true};          // 300 keypoint rows, 500 point rows, 40 / 60 output rows
    const ProjExtent fuse = {100, 300, 500, 0, 60, false};       // Fuse: no per-keypoint output rows
    const auto one = [&](const P& p, const ProjExtent& ex) { return check_proj_records("fn", &p, 1, ex, "keyframe", none); };
    const auto fits = [&](const P& p, const ProjExtent& ex) { return record_counts_fit(p, ex) && record_lies_inside(p, ex); };   // what the kernel asks
    // accepted: offsets exactly at rows - n, n = 0 at the end of the arrays, n_kp at the capacity
    const P ok[] = {record<P>(40, 260, 60, 440, 0, 0), record<P>(0, 300, 0, 500, 40, 60), record<P>(0, 0, 0, 0, 0, 0), record<P>(100, 200, 1, 499, 0, 59) /* kp_out: see below */};
    for (int i = 0; i < 3; i++) { CHECK(one(ok[i], e) == OSLAM_OK); CHECK(fits(ok[i], e)); }
    CHECK(one(ok[3], e) == OSLAM_E_INVALID && !fits(ok[3], e));   // 100 keypoints do not fit 40 output rows ...
    CHECK(one(ok[3], fuse) == OSLAM_OK && fits(ok[3], fuse));     // ... which Fuse does not have
    CHECK(check_proj_records("fn", ok, 0, e, "keyframe", none) == OSLAM_OK && check_proj_records("fn", (const P*)nullptr, 0, e, "keyframe", none) == OSLAM_OK);
    // counts: OSLAM_E_CAPACITY, before the offsets (which are bad too)
    const P bad_n[] = {record<P>(-1, -1, 0, 0, 0, 0), record<P>(0, -1, -1, 0, 0, 0), record<P>(101, -1, 0, 0, 0, 0), record<P>(INT_MIN, 0, 0, 0, 0, 0), record<P>(INT_MAX, 0, 0, 0, 0, 0)};
    for (const P& p : bad_n) { CHECK(one(p, e) == OSLAM_E_CAPACITY && said("none may be negative")); CHECK(!fits(p, e)); }
    // offsets: OSLAM_E_INVALID; one step beyond every boundary, negative ones, and INT_MAX (rows - n must not be formed as off + n)
    const P bad_off[] = {record<P>(40, 261, 0, 0, 0, 0), record<P>(0, 0, 60, 441, 0, 0), record<P>(40, 0, 0, 0, 1, 0), record<P>(0, 0, 60, 0, 0, 1), record<P>(0, 301, 0, 0, 0, 0),
                         record<P>(0, 0, 0, 501, 0, 0), record<P>(0, 0, 0, 0, 41, 0), record<P>(0, 0, 0, 0, 0, 61), record<P>(0, -1, 0, 0, 0, 0), record<P>(0, 0, 0, -1, 0, 0),
                         record<P>(0, 0, 0, 0, -1, 0), record<P>(0, 0, 0, 0, 0, -1), record<P>(1, INT_MAX, 0, 0, 0, 0), record<P>(0, 0, INT_MAX, INT_MAX, 0, 0),
                         record<P>(100, 0, 0, 0, INT_MAX, 0), record<P>(0, 0, INT_MAX, 0, 0, INT_MAX), record<P>(0, 0, INT_MAX, 0, 0, 0), record<P>(0, INT_MIN, 0, INT_MIN, INT_MIN, INT_MIN)};
    for (const P& p : bad_off) { CHECK(one(p, e) == OSLAM_E_INVALID && said("lies outside the 300 keyframe rows / 500 point rows / 40 and 60 output rows")); CHECK(!fits(p, e)); }
    // Fuse skips the kp_out terms, and only those
    CHECK(one(record<P>(40, 0, 0, 0, 41, 0), fuse) == OSLAM_OK && one(record<P>(40, 0, 0, 0, -1, 0), fuse) == OSLAM_OK && one(record<P>(40, 0, 0, 0, INT_MAX, 0), fuse) == OSLAM_OK);
    CHECK(one(record<P>(40, 0, 60, 0, 0, 1), fuse) == OSLAM_E_INVALID && one(record<P>(40, 261, 0, 0, 0, 0), fuse) == OSLAM_E_INVALID);
    // the first bad record is reported; the operator's own refusal comes after the shared ones of the same record and before the next record
    const P three[3] = {record<P>(1, 0, 1, 0, 0, 0), record<P>(1, 300, 1, 0, 0, 0), record<P>(-1, 0, 0, 0, 0, 0)};
    CHECK(check_proj_records("fn", three, 3, e, "keyframe", none) == OSLAM_E_INVALID && said("problem 1 "));
    CHECK(check_proj_records("fn", three, 1, e, "keyframe", none) == OSLAM_OK);
    std::vector<int> seen;
    const auto own = [&](int b, const P&) { seen.push_back(b); return b == 0 ? -77 : 0; };
    CHECK(check_proj_records("fn", three, 3, e, "keyframe", own) == -77 && seen == std::vector<int>{0});
    seen.clear();
    CHECK(check_proj_records("fn", three + 1, 2, e, "keyframe", own) == OSLAM_E_INVALID && seen.empty());   // not asked about a record the shared check refuses
}

static void check_camera_block() {
    WindowCam w;
    memset(&w, 0xFF, sizeof w);   // (NaN in every float: what fill leaves untouched would show)
    fill_window_cam(w, &kCam, kBounds, kScale, 3, kLog);
    CHECK(w.fx == 500.f && w.fy == 510.f && w.cx == 320.f && w.cy == 240.f);
    CHECK(w.minX == -10.f && w.minY == -20.f && w.maxX == 630.f && w.maxY == 460.f);
    CHECK(w.invW == 64.f / 640.f && w.invH == 48.f / 480.f && w.invW == 0.1f && w.invH == 0.1f);
    CHECK(w.scale[0] == 1.f && w.scale[1] == 1.2f && w.scale[2] == 1.44f && w.nlevels == 3 && w.logScale == kLog);
    for (int i = 3; i < OSLAM_MAX_LEVELS; i++) CHECK(w.scale[i] == 0.f);   // zero from nlevels on: scaleFactors holds only nlevels entries
    // the reference divides in float (src/Frame.cc:160-161): bounds whose difference is no exact float quotient
    const float odd[4] = {0.25f, 0.5f, 752.75f, 480.125f};
    float all[OSLAM_MAX_LEVELS];
    for (int i = 0; i < OSLAM_MAX_LEVELS; i++) all[i] = 1.f + i;
    fill_window_cam(w, &kCam, odd, all, OSLAM_MAX_LEVELS, 1.f);
    CHECK(w.invW == 64.f / (752.75f - 0.25f) && w.invH == 48.f / (480.125f - 0.5f) && w.scale[OSLAM_MAX_LEVELS - 1] == (float)OSLAM_MAX_LEVELS);
    CHECK(sizeof(WindowCam) == (10 + OSLAM_MAX_LEVELS + 2) * 4);   // no padding: the block is the tail of a kernel's arguments
}

int main() {
    check_call_refusals();
    check_records<oslam_sim3_proj_problem_t>();
    check_records<oslam_reloc_proj_problem_t>();
    check_camera_block();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("window_search_check: ok\n");
    return 0;
}
