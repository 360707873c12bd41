// A caller of ORB_SLAM2::Optimizer::OptimizeEssentialGraph written only against include/orb_slam2_adapter.hpp: the call of LoopClosing::CorrectLoop
// (src/LoopClosing.cc:568) on a small hand-built map: twelve keyframes on an arc, a spanning tree, covisibility lists, an old loop edge, the new loop
// between the last keyframe and keyframe 0 with its connections, drifted poses and a corrected Sim3 for the current keyframe and its neighbour.  Prints the
// map ("parent", "children k ...", "loops k ...", "covis k ...", "conn k (j w)..."), the helper's edges ("edge i j kind"), the operator's inputs as the
// adapter forms them ("Scw", "Snc", "has_nc", "fixed": floats as hexadecimal bit patterns), and the results ("Tcw", "Pin", "ref", "Pout").
// tests/test_essential_graph_gpu.py builds it, runs it and compares every line with the ctypes path.
#include <cmath>
#include <cstdio>
#include <vector>

#include "orb_slam2_adapter.hpp"

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

static void rot_y(double a, double R[9]) {
    const double c = std::cos(a), s = std::sin(a);
    const double M[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    memcpy(R, M, sizeof(M));
}

struct Csr {
    std::vector<int32_t> ptr{0}, val, w;
    void row(std::initializer_list<int32_t> v, std::initializer_list<int32_t> weights = {}) {
        val.insert(val.end(), v); w.insert(w.end(), weights); ptr.push_back((int32_t)val.size());
    }
};

int main() {
    try {
        const int n = 12;
        std::vector<float> Tcw((size_t)n * 16, 0.f);
        std::vector<ORB_SLAM2::Sim3> corrected(n), noncorrected(n);
        std::vector<uint8_t> has_c(n, 0), has_nc(n, 0);
        for (int k = 0; k < n; k++) {
            const double a = 0.5 * k, drift = 0.004 * k;   // the estimate turns and moves a little more than the truth with every keyframe
            double R[9], Rt[9];
            rot_y(-(a + drift), R);
            rot_y(-a, Rt);
            const double Ow[3] = {4 * std::sin(a) + 3 * drift, 0.1 * k * 0.1, 4 - 4 * std::cos(a) - 2 * drift}, Owt[3] = {4 * std::sin(a), 0.01 * k, 4 - 4 * std::cos(a)};
            float* T = Tcw.data() + (size_t)k * 16;
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
                T[4 * r + 3] = (float)-(R[3 * r] * Ow[0] + R[3 * r + 1] * Ow[1] + R[3 * r + 2] * Ow[2]);
            }
            T[15] = 1.f;
            if (k >= n - 2) {   // CorrectLoop corrects the current keyframe and its neighbours
                has_c[k] = has_nc[k] = 1;
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++) { corrected[k].R[3 * r + c] = Rt[3 * r + c]; noncorrected[k].R[3 * r + c] = T[4 * r + c]; }
                    corrected[k].t[r] = -(Rt[3 * r] * Owt[0] + Rt[3 * r + 1] * Owt[1] + Rt[3 * r + 2] * Owt[2]);
                    noncorrected[k].t[r] = T[4 * r + 3];
                }
                corrected[k].s = 1.0; noncorrected[k].s = 1.0;
            }
        }
        std::vector<int32_t> parent(n);
        Csr children, loops, covis, conn;
        for (int k = 0; k < n; k++) parent[k] = k - 1;
        parent[7] = 5;   // a branch of the spanning tree
        for (int k = 0; k < n; k++) {
            std::vector<int32_t> c;
            for (int m = 0; m < n; m++) if (parent[m] == k) c.push_back(m);
            children.val.insert(children.val.end(), c.begin(), c.end()); children.ptr.push_back((int32_t)children.val.size());
        }
        for (int k = 0; k < n; k++) {   // an old loop between 8 and 2
            if (k == 8) loops.row({2}); else if (k == 2) loops.row({8}); else loops.row({});
        }
        for (int k = 0; k < n; k++) {   // covisibles by weight: the neighbours two and one steps away, parent and child among them
            std::vector<int32_t> c;
            for (int m : {k - 2, k + 2, k - 1, k + 1, k - 3}) if (m >= 0 && m < n) c.push_back(m);
            if (k == 8) c.push_back(2);
            if (k == 11) c.push_back(1);   // also a loop connection: sInsertedEdges keeps it out
            covis.val.insert(covis.val.end(), c.begin(), c.end()); covis.ptr.push_back((int32_t)covis.val.size());
        }
        for (int k = 0; k < n; k++) {   // LoopConnections: the current keyframe and its neighbour gained links across the loop
            if (k == 11) conn.row({0, 1, 2}, {30, 120, 99});   // (cur, loop) is kept below 100; 1 is kept; 2 is dropped
            else if (k == 10) conn.row({0}, {150});
            else conn.row({});
        }
        std::vector<float> Xw;
        std::vector<int32_t> ref;
        for (int m = 0; m < 30; m++) {
            Xw.push_back(0.3f * m - 4.f); Xw.push_back(0.1f * (m % 7)); Xw.push_back(6.f - 0.2f * m);
            ref.push_back(m % 5 == 4 ? -1 : m % n);
        }
        const std::vector<float> Xin = Xw;
        ORB_SLAM2::EssentialGraphView G;
        G.nKF = n; G.Tcw = Tcw.data(); G.parent = parent.data();
        G.children_ptr = children.ptr.data(); G.children = children.val.data(); G.loop_ptr = loops.ptr.data(); G.loop_edges = loops.val.data();
        G.covis_ptr = covis.ptr.data(); G.covisibles = covis.val.data(); G.conn_ptr = conn.ptr.data(); G.conn = conn.val.data(); G.conn_weight = conn.w.data();
        G.has_corrected = has_c.data(); G.Corrected = corrected.data(); G.has_noncorrected = has_nc.data(); G.NonCorrected = noncorrected.data();
        G.pLoopKF = 0; G.pCurKF = 11; G.nMP = (int)ref.size(); G.Xw = Xw.data(); G.ref = ref.data();
        const bool mbFixScale = true;

        printf("nKF %d\ncur %d\nloop %d\nfixScale %d\nparent", n, G.pCurKF, G.pLoopKF, mbFixScale ? 1 : 0);
        for (int k = 0; k < n; k++) printf(" %d", parent[k]);
        printf("\n");
        auto dump = [&](const char* tag, const Csr& c, bool weights) {
            for (int k = 0; k < n; k++) {
                if (weights && c.ptr[k] == c.ptr[k + 1]) continue;
                printf("%s %d", tag, k);
                for (int q = c.ptr[k]; q < c.ptr[k + 1]; q++) { printf(" %d", c.val[q]); if (weights) printf(" %d", c.w[q]); }
                printf("\n");
            }
        };
        dump("children", children, false); dump("loops", loops, false); dump("covis", covis, false); dump("conn", conn, true);
        const std::vector<int32_t> edges = ORB_SLAM2::Optimizer::EssentialGraphEdges(G);
        for (size_t e = 0; e < edges.size(); e += 3) printf("edge %d %d %d\n", edges[e], edges[e + 1], edges[e + 2]);
        // the operator's inputs, as the adapter forms them (:818-832)
        printf("has_nc"); for (int k = 0; k < n; k++) printf(" %d", has_nc[k]); printf("\n");
        printf("fixed"); for (int k = 0; k < n; k++) printf(" %d", k == G.pLoopKF ? 1 : 0); printf("\n");
        for (int pass = 0; pass < 2; pass++)
            for (int k = 0; k < n; k++) {
                float o[13] = {0};
                const bool use = pass == 0 ? has_c[k] != 0 : has_nc[k] != 0;
                const ORB_SLAM2::Sim3& S = pass == 0 ? corrected[k] : noncorrected[k];
                if (use) {
                    o[0] = (float)S.s;
                    for (int q = 0; q < 9; q++) o[1 + q] = (float)S.R[q];
                    for (int q = 0; q < 3; q++) o[10 + q] = (float)S.t[q];
                } else if (pass == 0) {
                    const float* T = Tcw.data() + (size_t)k * 16;
                    o[0] = 1.f;
                    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o[1 + 3 * r + c] = T[4 * r + c]; o[10 + r] = T[4 * r + 3]; }
                }
                printf(pass == 0 ? "Scw" : "Snc");
                for (int q = 0; q < 13; q++) printf(" %08x", bits(o[q]));
                printf("\n");
            }
        ORB_SLAM2::Optimizer::OptimizeEssentialGraph(G, mbFixScale);
        for (int k = 0; k < n; k++) {
            printf("Tcw");
            for (int q = 0; q < 16; q++) printf(" %08x", bits(Tcw[(size_t)k * 16 + q]));
            printf("\n");
        }
        printf("ref"); for (size_t m = 0; m < ref.size(); m++) printf(" %d", ref[m]); printf("\n");
        for (size_t m = 0; m < ref.size(); m++) printf("Pin %08x %08x %08x\n", bits(Xin[3 * m]), bits(Xin[3 * m + 1]), bits(Xin[3 * m + 2]));
        for (size_t m = 0; m < ref.size(); m++) printf("Pout %08x %08x %08x\n", bits(Xw[3 * m]), bits(Xw[3 * m + 1]), bits(Xw[3 * m + 2]));
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
