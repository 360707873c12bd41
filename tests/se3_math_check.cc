// csrc/se3_math.h as a stand-alone host program (no GPU): the four bodies of the matrix -> quaternion conversion, on both sides of each boundary between
// them and at the exact ties; the sign rule of the quaternion (w >= 0) through se3_from_T and through an update that carries w across zero; the float
// round trip.  Built by tests/test_far_pose_cpu.py:  g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include tests/se3_math_check.cc
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../object_slam_amd/csrc/se3_math.h"

using namespace oslam;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            failures++;                                   \
            std::printf("FAIL %s:%d  ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

// Rodrigues' formula, written out here: nothing of the header under test
static void rodrigues(double ax, double ay, double az, double deg, double R[9]) {
    const double n = std::sqrt(ax * ax + ay * ay + az * az), x = ax / n, y = ay / n, z = az / n;
    const double th = deg * 3.14159265358979323846 / 180.0, c = std::cos(th), s = std::sin(th), C = 1 - c;
    R[0] = c + x * x * C;     R[1] = x * y * C - z * s; R[2] = x * z * C + y * s;
    R[3] = y * x * C + z * s; R[4] = c + y * y * C;     R[5] = y * z * C - x * s;
    R[6] = z * x * C - y * s; R[7] = z * y * C + x * s; R[8] = c + z * z * C;
}

static void mul3(const double A[9], const double B[9], double o[9]) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) o[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// Eigen's rule (Eigen/src/Geometry/Quaternion.h): 0 = positive trace, 1 + i otherwise, ties to the lower index
static int eigen_body(const double m[9]) {
    if (m[0] + m[4] + m[8] > 0) return 0;
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[i * 4]) i = 2;
    return 1 + i;
}

static int seen[4] = {0, 0, 0, 0};

// se3_R(quat_from_R(R)) == R to 1e-14, the quaternion has unit length, and the body Eigen's rule names put its own component first
static void round_trip(const double R[9], int want_body, const char* what) {
    const int body = eigen_body(R);
    seen[body]++;
    CHECK(want_body < 0 || body == want_body, "%s: the case sits in body %d, meant for %d", what, body, want_body);
    SE3 s;
    quat_from_R(R, s.q);
    s.t[0] = s.t[1] = s.t[2] = 0;
    const double n2 = s.q[0] * s.q[0] + s.q[1] * s.q[1] + s.q[2] * s.q[2] + s.q[3] * s.q[3];
    CHECK(std::fabs(n2 - 1.0) <= 1e-14, "%s: |q|^2 = %.17g", what, n2);
    // the component the body computes from the square root is positive and (in a non-trace body) the largest of x, y, z
    if (body == 0) CHECK(s.q[3] > 0, "%s: trace body with w = %g", what, s.q[3]);
    else {
        const int i = body - 1;
        CHECK(s.q[i] > 0 && s.q[i] >= std::fabs(s.q[(i + 1) % 3]) - 1e-15 && s.q[i] >= std::fabs(s.q[(i + 2) % 3]) - 1e-15, "%s: body %d with q = %g %g %g %g", what, body, s.q[0],
              s.q[1], s.q[2], s.q[3]);
    }
    double B[9];
    se3_R(s, B);
    double worst = 0;
    for (int k = 0; k < 9; k++) worst = std::fmax(worst, std::fabs(B[k] - R[k]));
    CHECK(worst <= 1e-14, "%s (body %d): |se3_R(quat_from_R(R)) - R| = %.3g", what, body, worst);
}

static void float_pose(const double R[9], const double t[3], float T[16]) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)R[r * 3 + c];
        T[r * 4 + 3] = (float)t[r];
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

// se3_from_T: w >= 0, unit norm; se3_to_T(se3_from_T(T)) == T to float rounding (the float rotation is orthonormal to 1e-7 only: 4e-7 absolute)
static void pose_round_trip(const double R[9], const char* what) {
    const double t[3] = {1.25, -7.5, 144.0};
    float T[16], B[16];
    float_pose(R, t, T);
    const SE3 s = se3_from_T(T);
    const double n2 = s.q[0] * s.q[0] + s.q[1] * s.q[1] + s.q[2] * s.q[2] + s.q[3] * s.q[3];
    CHECK(s.q[3] >= 0, "%s: se3_from_T gives w = %g", what, s.q[3]);
    CHECK(std::fabs(n2 - 1.0) <= 1e-14, "%s: se3_from_T gives |q|^2 = %.17g", what, n2);
    se3_to_T(s, B);
    double worst = 0;
    for (int k = 0; k < 12; k++) worst = std::fmax(worst, std::fabs((double)B[k] - (double)T[k]) / std::fmax(1.0, std::fabs((double)T[k])));
    CHECK(worst <= 4e-7, "%s: |se3_to_T(se3_from_T(T)) - T| = %.3g", what, worst);
    CHECK(B[3] == T[3] && B[7] == T[7] && B[11] == T[11] && B[12] == 0.f && B[13] == 0.f && B[14] == 0.f && B[15] == 1.f, "%s: translation / last row", what);
    // the pose maps a point as the matrix does
    const double X[3] = {0.5, -2.0, 3.0};
    double p[3];
    se3_map(s, X, p);
    for (int r = 0; r < 3; r++) {
        const double want = (double)T[r * 4] * X[0] + (double)T[r * 4 + 1] * X[1] + (double)T[r * 4 + 2] * X[2] + (double)T[r * 4 + 3];
        CHECK(std::fabs(p[r] - want) <= 4e-6, "%s: se3_map row %d: %.9g, the matrix gives %.9g", what, r, p[r], want);
    }
}

int main() {
    double R[9], A[9], B[9];
    char what[128];
    // ---- inside each body: rotations about the axes, the diagonal and general axes
    const double axes[][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}, {1, -2, 0.5}, {-0.3, 0.2, 1}, {2, 1, -0.1}, {0.1, 3, 0.4}};
    const double angles[] = {0.0, 5.0, 60.0, 100.0, 119.5, 120.5, 130.0, 150.0, 170.0, 175.0, 179.999, 180.0, 185.0, 240.0, 359.0};
    for (const auto& ax : axes)
        for (double deg : angles) {
            rodrigues(ax[0], ax[1], ax[2], deg, R);
            std::snprintf(what, sizeof what, "%g deg about (%g, %g, %g)", deg, ax[0], ax[1], ax[2]);
            round_trip(R, -1, what);
            pose_round_trip(R, what);
        }
    // ---- both sides of trace = 0: about each axis the trace is 1 + 2 cos(theta), zero at 120 degrees
    for (int a = 0; a < 3; a++)
        for (double deg : {120.0 - 1e-6, 120.0 + 1e-6}) {
            rodrigues(a == 0, a == 1, a == 2, deg, R);
            std::snprintf(what, sizeof what, "%.7f deg about axis %d", deg, a);
            round_trip(R, deg < 120 ? 0 : 1 + a, what);
            pose_round_trip(R, what);
        }
    // ---- both sides of each boundary between the non-trace bodies: pi about an axis between two coordinate axes, tilted to either
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            if (i == j) continue;
            double ax[3] = {0, 0, 0};
            ax[i] = 1.0 + 1e-6;   // the larger component decides: m_ii = 2 ax_i^2 - 1 (normalised)
            ax[j] = 1.0;
            rodrigues(ax[0], ax[1], ax[2], 180.0, R);
            std::snprintf(what, sizeof what, "pi about the axis between %d and %d, nearer %d", i, j, i);
            round_trip(R, 1 + i, what);
            pose_round_trip(R, what);
            rodrigues(ax[0], ax[1], ax[2], 170.0, R);   // and with w != 0
            round_trip(R, 1 + i, what);
        }
    // ---- the exact ties
    const double pix[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1}, piy[9] = {-1, 0, 0, 0, 1, 0, 0, 0, -1}, piz[9] = {-1, 0, 0, 0, -1, 0, 0, 0, 1};
    const double cyc[9] = {0, 0, 1, 1, 0, 0, 0, 1, 0}, cyc2[9] = {0, 1, 0, 0, 0, 1, 1, 0, 0};
    round_trip(pix, 1, "diag(1, -1, -1)");      // m11 == m22
    round_trip(piy, 2, "diag(-1, 1, -1)");      // m00 == m22
    round_trip(piz, 3, "diag(-1, -1, 1)");      // m00 == m11
    round_trip(cyc, 1, "cyclic permutation");   // trace exactly 0 (not > 0), all diagonal entries equal: i = 0
    round_trip(cyc2, 1, "cyclic permutation, transposed");
    for (const double* M : {pix, piy, piz, cyc, cyc2}) pose_round_trip(M, "exact tie");
    // pi about (1, 1, 0): m00 == m11 == 0 > m22 = -1: the tie goes to i = 0; pi about (0, 1, 1): i = 1; pi about (1, 0, 1): m00 == m22: i = 0
    const double xy[9] = {0, 1, 0, 1, 0, 0, 0, 0, -1}, yz[9] = {-1, 0, 0, 0, 0, 1, 0, 1, 0}, xz[9] = {0, 0, 1, 0, -1, 0, 1, 0, 0};
    round_trip(xy, 1, "pi about (1, 1, 0)");
    round_trip(yz, 2, "pi about (0, 1, 1)");
    round_trip(xz, 1, "pi about (1, 0, 1)");
    {   // w = 0 exactly at the start
        SE3 s;
        quat_from_R(pix, s.q);
        CHECK(s.q[0] == 1 && s.q[1] == 0 && s.q[2] == 0 && s.q[3] == 0, "diag(1, -1, -1): q = %g %g %g %g", s.q[0], s.q[1], s.q[2], s.q[3]);
        quat_from_R(piy, s.q);
        CHECK(s.q[0] == 0 && s.q[1] == 1 && s.q[2] == 0 && s.q[3] == 0, "diag(-1, 1, -1): q = %g %g %g %g", s.q[0], s.q[1], s.q[2], s.q[3]);
        quat_from_R(piz, s.q);
        CHECK(s.q[0] == 0 && s.q[1] == 0 && s.q[2] == 1 && s.q[3] == 0, "diag(-1, -1, 1): q = %g %g %g %g", s.q[0], s.q[1], s.q[2], s.q[3]);
        quat_from_R(cyc, s.q);
        CHECK(s.q[0] == 0.5 && s.q[1] == 0.5 && s.q[2] == 0.5 && s.q[3] == 0.5, "cyclic permutation: q = %g %g %g %g", s.q[0], s.q[1], s.q[2], s.q[3]);
    }
    CHECK(seen[0] > 0 && seen[1] > 0 && seen[2] > 0 && seen[3] > 0, "bodies reached: %d %d %d %d", seen[0], seen[1], seen[2], seen[3]);

    // ---- w across zero in an update: T has 179 degrees about an axis (w = cos(89.5 deg) > 0), the update adds 2 degrees about the same axis: the product's
    // w is cos(90.5 deg) < 0 before SE3Quat::normalizeRotation, which must return the quaternion with w >= 0 — and the same rotation matrix
    for (const auto& ax : axes) {
        const double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        for (double step : {2.0, -2.0}) {
            const double base = step > 0 ? 179.0 : 181.0;   // (181 degrees: se3_from_T has already flipped the sign; -2 degrees crosses back)
            rodrigues(ax[0], ax[1], ax[2], base, A);
            const double t[3] = {0.5, -1.0, 2.0};
            float T[16];
            float_pose(A, t, T);
            const SE3 s0 = se3_from_T(T);
            const double th = step * 3.14159265358979323846 / 180.0;
            const double u[6] = {th * ax[0] / n, th * ax[1] / n, th * ax[2] / n, 0.01, -0.02, 0.03};
            const SE3 up = se3_exp(u);
            const SE3 s1 = se3_mul(up, s0);
            CHECK(s1.q[3] >= 0, "update of %g degrees on %g about (%g, %g, %g): w = %g", step, base, ax[0], ax[1], ax[2], s1.q[3]);
            const double n2 = s1.q[0] * s1.q[0] + s1.q[1] * s1.q[1] + s1.q[2] * s1.q[2] + s1.q[3] * s1.q[3];
            CHECK(std::fabs(n2 - 1.0) <= 1e-14, "update: |q|^2 = %.17g", n2);
            // the raw product has w < 0: the case does cross
            const double raw_w = up.q[3] * s0.q[3] - up.q[0] * s0.q[0] - up.q[1] * s0.q[1] - up.q[2] * s0.q[2];
            CHECK(raw_w < 0, "the case does not cross w = 0: raw w = %g", raw_w);
            // rotation of the product == product of the rotations (float T is orthonormal to 1e-7: compare with the rotation of s0, not with A)
            double R0[9], Ru[9], R1[9];
            se3_R(s0, R0);
            se3_R(up, Ru);
            se3_R(s1, R1);
            mul3(Ru, R0, B);
            double worst = 0;
            for (int k = 0; k < 9; k++) worst = std::fmax(worst, std::fabs(R1[k] - B[k]));
            CHECK(worst <= 1e-14, "update across w = 0: |R(up * T) - R(up) R(T)| = %.3g", worst);
            // and the translation: R(up) t0 + t(up)
            for (int r = 0; r < 3; r++) {
                const double want = Ru[r * 3] * s0.t[0] + Ru[r * 3 + 1] * s0.t[1] + Ru[r * 3 + 2] * s0.t[2] + up.t[r];
                CHECK(std::fabs(s1.t[r] - want) <= 1e-14, "update across w = 0: t[%d] = %.17g, want %.17g", r, s1.t[r], want);
            }
        }
    }
    // se3_exp of a rotation beyond 120 degrees takes the non-trace bodies itself
    for (int a = 0; a < 3; a++) {
        const double th = 170.0 * 3.14159265358979323846 / 180.0;
        const double u[6] = {a == 0 ? th : 0, a == 1 ? th : 0, a == 2 ? th : 0, 0, 0, 0};
        const SE3 s = se3_exp(u);
        rodrigues(a == 0, a == 1, a == 2, 170.0, R);
        se3_R(s, B);
        double worst = 0;
        for (int k = 0; k < 9; k++) worst = std::fmax(worst, std::fabs(B[k] - R[k]));
        CHECK(worst <= 1e-14 && s.q[3] >= 0, "se3_exp of 170 degrees about axis %d: |R - Rodrigues| = %.3g, w = %g", a, worst, s.q[3]);
    }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("se3_math host checks passed (bodies reached: %d %d %d %d)\n", seen[0], seen[1], seen[2], seen[3]);
    return failures ? 1 : 0;
}
