// The host arithmetic the windowed projection searches share (window_search.h has the device code; sim3_match.hip, sim3_project.hip and reloc_project.hip are
// the operators): the camera block of their kernel arguments and how it is filled, the refusals of a call they make alike, and the range check of the problem
// records of the two projection operators, which the kernels repeat per record.  No HIP and no runtime call: tests/window_search_check.cc compiles this
// header alone.
#pragma once
#include <cstdint>

#include "../../include/oslam_hip.h"

#ifdef __HIPCC__
#define OSLAM_HD __host__ __device__
#else
#define OSLAM_HD
#endif

namespace oslam {

void set_error(const char* fmt, ...);   // (common.h declares it too; the stand-alone check defines its own)

namespace kf_stage {

constexpr int kGridCols = 64, kGridRows = 48;   // reference include/Frame.h:43-44 (KeyFrame copies the Frame's grid, src/KeyFrame.cc:33-55)

// What a kernel needs to project a point, predict its level and find its window: the tail of every operator's argument block
struct WindowCam {
    float fx, fy, cx, cy;
    float minX, minY, maxX, maxY, invW, invH;   // mnMinX .. mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv
    float scale[OSLAM_MAX_LEVELS];              // mvScaleFactors, 0 from nlevels on
    int nlevels;
    float logScale;
};

// The refusals of the camera arguments, in the order every operator makes them (after its own NULL, count and capacity refusals)
static inline int check_window(const char* fn, const float* bounds, int nlevels, float logScaleFactor) {
    if (nlevels < 1 || nlevels > OSLAM_MAX_LEVELS) { set_error("%s: nlevels = %d outside [1, %d]", fn, nlevels, OSLAM_MAX_LEVELS); return OSLAM_E_INVALID; }
    if (!(bounds[2] > bounds[0]) || !(bounds[3] > bounds[1])) { set_error("%s: empty image bounds", fn); return OSLAM_E_INVALID; }
    if (!(logScaleFactor > 0.0f)) { set_error("%s: logScaleFactor must be positive", fn); return OSLAM_E_INVALID; }
    return OSLAM_OK;
}

// (after check_window)
static inline void fill_window_cam(WindowCam& w, const oslam_camera_t* cam, const float* bounds, const float* scaleFactors, int nlevels, float logScaleFactor) {
    w.fx = cam->fx; w.fy = cam->fy; w.cx = cam->cx; w.cy = cam->cy;
    w.minX = bounds[0]; w.minY = bounds[1]; w.maxX = bounds[2]; w.maxY = bounds[3];
    w.invW = (float)kGridCols / (float)(w.maxX - w.minX);   // src/Frame.cc:160-161
    w.invH = (float)kGridRows / (float)(w.maxY - w.minY);
    for (int i = 0; i < OSLAM_MAX_LEVELS; i++) w.scale[i] = i < nlevels ? scaleFactors[i] : 0.f;
    w.nlevels = nlevels; w.logScale = logScaleFactor;
}

// ---- the two projection operators: their calls have the same shape (problems, keypoint rows, point rows, per-point and per-keypoint output rows) ----

// The first seven refusals of a call.  h: the handle (max_problems, max_pts); kp, pts: the row structs (n_rows).  kp_noun names the keypoint rows ("keyframe" /
// "frame"), out_noun the per-point output rows ("point output" / "skip").
template <class H, class KpRows, class PtRows>
static inline int check_proj_call(const char* fn, const H* h, int n_problems, const KpRows* kp, const char* kp_noun, const PtRows* pts, int n_pt_out, const char* out_noun, int n_kp_out,
                                  const oslam_camera_t* cam, const float* bounds, const float* scaleFactors, int nlevels, float logScaleFactor) {
    if (!h || !kp || !pts || !cam || !bounds || !scaleFactors) { set_error("%s: NULL argument", fn); return OSLAM_E_INVALID; }
    if (n_problems < 0 || kp->n_rows < 0 || pts->n_rows < 0 || n_pt_out < 0 || n_kp_out < 0) {
        set_error("%s: %d problems, %d %s rows, %d point rows, %d / %d output rows: none may be negative", fn, n_problems, kp->n_rows, kp_noun, pts->n_rows, n_pt_out, n_kp_out);
        return OSLAM_E_CAPACITY;
    }
    if (n_problems > h->max_problems) { set_error("%s: %d problems exceed the handle's %d", fn, n_problems, h->max_problems); return OSLAM_E_CAPACITY; }
    if (pts->n_rows > h->max_pts || n_pt_out > h->max_pts) {
        set_error("%s: %d point rows / %d %s rows exceed the handle's max_points_total %d", fn, pts->n_rows, n_pt_out, out_noun, h->max_pts);
        return OSLAM_E_CAPACITY;
    }
    return check_window(fn, bounds, nlevels, logScaleFactor);
}

// The arrays one call's problem records index.  kp_out: the operator writes per-keypoint output rows (Fuse does not)
struct ProjExtent { int max_kps, kp_rows, pt_rows, n_kp_out, n_pt_out; bool kp_out; };

// One record (oslam_sim3_proj_problem_t, oslam_reloc_proj_problem_t: the same six leading ints) against the extent.  `off <= rows - n` with 0 <= n and
// 0 <= rows cannot overflow, whatever off is.
template <class P> static OSLAM_HD inline bool record_counts_fit(const P& p, const ProjExtent& e) { return p.n_kp >= 0 && p.n_pts >= 0 && p.n_kp <= e.max_kps; }
template <class P> static OSLAM_HD inline bool record_lies_inside(const P& p, const ProjExtent& e) {   // (after record_counts_fit)
    bool inside = p.kp_off >= 0 && p.pt_off >= 0 && p.pt_out_off >= 0 && p.kp_off <= e.kp_rows - p.n_kp && p.pt_off <= e.pt_rows - p.n_pts && p.pt_out_off <= e.n_pt_out - p.n_pts;
    if (e.kp_out) inside = inside && p.kp_out_off >= 0 && p.kp_out_off <= e.n_kp_out - p.n_kp;
    return inside;
}

// The record check of a host-pointer entry point, which refuses the call where the kernel would answer -2 for the record.  more(b, p): the operator's own
// refusal of record b, made after the shared ones of the same record (0 = none).
template <class P, class More>
static inline int check_proj_records(const char* fn, const P* problems, int n_problems, const ProjExtent& e, const char* kp_noun, More more) {
    for (int b = 0; b < n_problems; b++) {
        const P& p = problems[b];
        if (!record_counts_fit(p, e)) {
            set_error("%s: problem %d has %d keypoints (at most %d) and %d points: none may be negative", fn, b, p.n_kp, e.max_kps, p.n_pts);
            return OSLAM_E_CAPACITY;
        }
        if (!record_lies_inside(p, e)) {
            set_error("%s: problem %d (kp_off %d, pt_off %d, kp_out_off %d, pt_out_off %d) lies outside the %d %s rows / %d point rows / %d and %d output rows", fn, b, p.kp_off,
                      p.pt_off, p.kp_out_off, p.pt_out_off, e.kp_rows, kp_noun, e.pt_rows, e.n_kp_out, e.n_pt_out);
            return OSLAM_E_INVALID;
        }
        const int rc = more(b, p);
        if (rc) return rc;
    }
    return OSLAM_OK;
}

}  // namespace kf_stage
}  // namespace oslam
