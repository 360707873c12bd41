// A caller of ORB_SLAM2::ORBmatcher::SearchByBoW(KF1, KF2) and ORB_SLAM2::LoopClosing written only against include/orb_slam2_adapter.hpp: one fixed problem
// each of the KeyFrame-pair BoW search (src/ORBmatcher.cc:522), mg2oScw (src/LoopClosing.cc:334-336), CorrectLoop's propagation (:436-517) and the map
// update after global BA (:677-738).  Prints every input and every output, floats and doubles as hexadecimal bit patterns.
// tests/test_loop_correct_gpu.py builds it, runs it and compares every output with the ctypes path on the printed inputs.
#include <cmath>
#include <cstdio>
#include <vector>

#include "orb_slam2_adapter.hpp"

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static unsigned long long bits(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }
static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static double unit() { return (rnd() % 100000) / 100000.0; }

static void pose(double ay, double ax, const double Ow[3], float* T) {   // Rcw = Rx(ax) Ry(ay), tcw = -Rcw Ow
    const double cy = std::cos(ay), sy = std::sin(ay), cx = std::cos(ax), sx = std::sin(ax);
    const double Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx};
    double R[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[3 * r + c] = Rx[3 * r] * Ry[c] + Rx[3 * r + 1] * Ry[3 + c] + Rx[3 * r + 2] * Ry[6 + c];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
        T[4 * r + 3] = (float)-(R[3 * r] * Ow[0] + R[3 * r + 1] * Ow[1] + R[3 * r + 2] * Ow[2]);
    }
    T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
}

static void print_f(const char* tag, const float* v, size_t n) { printf("%s", tag); for (size_t i = 0; i < n; i++) printf(" %08x", bits(v[i])); printf("\n"); }
static void print_d(const char* tag, const double* v, size_t n) { printf("%s", tag); for (size_t i = 0; i < n; i++) printf(" %016llx", bits(v[i])); printf("\n"); }
template <class T> static void print_i(const char* tag, const T* v, size_t n) { printf("%s", tag); for (size_t i = 0; i < n; i++) printf(" %d", (int)v[i]); printf("\n"); }

int main() {
    try {
        {   // ---- SearchByBoW(pKF1, pKF2, vpMatches12)
            const int N1 = 40, N2 = 36;
            std::vector<oslam::KeyPoint> k1(N1), k2(N2);
            std::vector<uint8_t> d1((size_t)N1 * 32), d2((size_t)N2 * 32), v1(N1), v2(N2);
            std::vector<uint32_t> node1(N1), node2(N2);
            memset(k1.data(), 0, sizeof(oslam::KeyPoint) * N1); memset(k2.data(), 0, sizeof(oslam::KeyPoint) * N2);
            for (int i = 0; i < N1; i++) {
                for (int b = 0; b < 32; b++) d1[(size_t)i * 32 + b] = (uint8_t)rnd();
                k1[i].angle = (float)(rnd() % 360); node1[i] = rnd() % 5; v1[i] = rnd() % 10 < 8;
            }
            for (int k = 0; k < N2; k++) {   // noisy copies of side-1 keypoints
                const int src = k < 28 ? k : (int)(rnd() % 28);   // the last eight contend with earlier copies
                for (int b = 0; b < 32; b++) d2[(size_t)k * 32 + b] = d1[(size_t)src * 32 + b] ^ (uint8_t)(1u << (rnd() % 8)) * (rnd() % 4 == 0);
                k2[k].angle = k1[src].angle - (float)(rnd() % 7) + (rnd() % 6 == 0 ? 90.f : 0.f);
                if (k2[k].angle < 0) k2[k].angle += 360.f;
                node2[k] = node1[src]; v2[k] = rnd() % 10 < 8;
            }
            auto flat = [](const std::vector<uint32_t>& node) {
                DBoW2::FeatureVector fv;
                for (size_t i = 0; i < node.size(); i++) fv[node[i]].push_back((unsigned)i);
                return ORB_SLAM2::ORBVocabulary::flatten(fv);
            };
            const ORB_SLAM2::ORBmatcher::FeatureVector fv1 = flat(node1), fv2 = flat(node2);
            ORB_SLAM2::FrameView KF1 = {N1, k1.data(), nullptr, d1.data(), nullptr, 0, 0, 640, 480}, KF2 = {N2, k2.data(), nullptr, d2.data(), nullptr, 0, 0, 640, 480};
            ORB_SLAM2::ORBmatcher matcher(0.75f, true);
            std::vector<int32_t> match12;
            const int nm = matcher.SearchByBoW(KF1, fv1, v1.data(), KF2, fv2, v2.data(), match12);
            for (int i = 0; i < N1; i++) { printf("bow1 %08x %u %d", bits(k1[i].angle), node1[i], (int)v1[i]); for (int b = 0; b < 32; b++) printf(" %d", d1[(size_t)i * 32 + b]); printf("\n"); }
            for (int i = 0; i < N2; i++) { printf("bow2 %08x %u %d", bits(k2[i].angle), node2[i], (int)v2[i]); for (int b = 0; b < 32; b++) printf(" %d", d2[(size_t)i * 32 + b]); printf("\n"); }
            print_i("match12", match12.data(), match12.size());
            printf("nmatches %d\n", nm);
        }
        const double c0[3] = {0.5, -0.2, 1.0};
        ORB_SLAM2::Sim3 Scw;
        {   // ---- mg2oScw
            ORB_SLAM2::Sim3 gScm;
            float Tcm[16], Tmw[16], mScw[16];
            const double o1[3] = {0.3, 0.1, -0.2};
            pose(0.2, -0.1, o1, Tcm);
            pose(-0.4, 0.15, c0, Tmw);
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) gScm.R[3 * r + c] = Tcm[4 * r + c]; gScm.t[r] = Tcm[4 * r + 3]; }
            gScm.s = 1.07;
            Scw = ORB_SLAM2::LoopClosing::ComputeScw(gScm, Tmw, mScw);
            print_d("Scm", gScm.R, 13); print_f("Tmw", Tmw, 16); print_d("Scw", Scw.R, 13); print_f("mScw", mScw, 16);
        }
        {   // ---- CorrectLoop's propagation
            const int n = 5, M = 30;
            std::vector<float> Tiw((size_t)n * 16), X((size_t)M * 3);
            for (int k = 0; k < n; k++) { const double Ow[3] = {c0[0] + 0.4 * k, c0[1], c0[2] - 0.1 * k}; pose(-0.4 + 0.1 * k, 0.15, Ow, Tiw.data() + 16 * k); }
            for (size_t i = 0; i < X.size(); i++) X[i] = (float)(4 * unit() - 2);
            std::vector<uint8_t> bad(M, 0);
            bad[3] = bad[17] = 1;
            std::vector<int32_t> ptr{0}, mp;
            for (int k = 0; k < n; k++) {
                for (int j = 0; j < 12 && k != 1; j++) mp.push_back(j % 5 == 4 ? -1 : (int32_t)((k * 5 + j) % M));
                ptr.push_back((int32_t)mp.size());
            }
            std::vector<ORB_SLAM2::Sim3> corr(n), nonc(n);
            std::vector<int32_t> cref(M, -7);
            print_f("prop_Tiw", Tiw.data(), Tiw.size()); print_f("prop_P", X.data(), X.size()); print_i("prop_bad", bad.data(), bad.size());
            print_i("prop_ptr", ptr.data(), ptr.size()); print_i("prop_mp", mp.data(), mp.size());
            ORB_SLAM2::LoopCorrectionView V = {n, 3, Tiw.data(), Scw, ptr.data(), mp.data(), M, X.data(), bad.data(), corr.data(), nonc.data(), cref.data()};
            ORB_SLAM2::LoopClosing::PropagateCorrection(V);
            printf("prop_cur %d\n", V.pCurKF);
            print_d("prop_Scorr", corr[0].R, (size_t)n * 13); print_d("prop_Snc", nonc[0].R, (size_t)n * 13); print_f("prop_Tout", Tiw.data(), Tiw.size());
            print_f("prop_Pout", X.data(), X.size()); print_i("prop_ref", cref.data(), cref.size());
        }
        {   // ---- the map update after global BA
            const int n = 7, M = 24;
            const int32_t parent[n] = {-1, 0, 1, 1, 3, 4, 2};
            const uint8_t in_ba[n] = {1, 1, 1, 0, 0, 0, 1};
            std::vector<float> Tcw((size_t)n * 16), Tg((size_t)n * 16), X((size_t)M * 3), Xg((size_t)M * 3);
            for (int k = 0; k < n; k++) {
                const double Ow[3] = {0.3 * k, 0.05 * k, 1.0 + 0.2 * k}, Og[3] = {0.3 * k + 0.02, 0.05 * k - 0.01, 1.0 + 0.2 * k + 0.03};
                pose(0.1 * k, -0.05, Ow, Tcw.data() + 16 * k);
                pose(0.1 * k + 0.01, -0.05, Og, Tg.data() + 16 * k);
            }
            for (size_t i = 0; i < X.size(); i++) { X[i] = (float)(4 * unit() - 2); Xg[i] = X[i] + (float)(0.02 * unit()); }
            std::vector<uint8_t> pin(M), bad(M, 0), reached(n, 9);
            std::vector<int32_t> ref(M);
            for (int i = 0; i < M; i++) { pin[i] = i % 3 != 0; ref[i] = i % n; }
            bad[5] = bad[6] = 1;
            print_i("gba_parent", parent, n); print_i("gba_in_ba", in_ba, n); print_f("gba_Tcw", Tcw.data(), Tcw.size()); print_f("gba_Tg", Tg.data(), Tg.size());
            print_f("gba_P", X.data(), X.size()); print_f("gba_Pg", Xg.data(), Xg.size()); print_i("gba_pin", pin.data(), pin.size()); print_i("gba_bad", bad.data(), bad.size());
            print_i("gba_ref", ref.data(), ref.size());
            ORB_SLAM2::GlobalBAUpdateView V = {n, parent, in_ba, Tcw.data(), Tg.data(), reached.data(), M, X.data(), Xg.data(), pin.data(), bad.data(), ref.data()};
            ORB_SLAM2::LoopClosing::UpdateMapAfterGlobalBA(V);
            print_f("gba_Tout", Tcw.data(), Tcw.size()); print_i("gba_reached", reached.data(), reached.size()); print_f("gba_Pout", X.data(), X.size());
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "adapter_loop_correct_program: %s\n", e.what());
        return 1;
    }
    return 0;
}
