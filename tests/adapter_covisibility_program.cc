// A caller of ORB_SLAM2::KeyFrameGraph and ORB_SLAM2::LoopClosing::LoopConnections written only against include/orb_slam2_adapter.hpp: one sequence whose
// keyframes arrive one after the other (src/LocalMapping.cc hands each to KeyFrame::UpdateConnections, src/Tracking.cc:1496 asks for the local keyframes),
// closed by the loop of src/LoopClosing.cc:549-565.  Reads <ops file>, one operation per line:
//   E <type> <a> <b> <c>                           an event: 0 AddObservation(point a, keyframe b, idx c), 1 EraseObservation(a, b), 2 SetBadFlag(point a),
//                                                  3 AddConnection(a, b, weight c), 4 EraseConnection(a, b), 5 keyframe a is bad, 6 ChangeParent(a, parent b)
//   U <keyframe> <n> {<point id>} x n              UpdateConnections
//   T <n> {<point id>} x n                         UpdateLocalKeyFrames
//   L <m> {<keyframe>} x m  m x (<n> {<point id>} x n)   LoopConnections over mvpCurrentConnectedKFs and the mvpMapPoints of each
// and prints per U "U <kf> | <vector covisibles> | <best 10> | <by weight 15> | <by weight 1> | <connected> | <parent> | <weight to kf - 1>", per T
// "T <reference> | <local keyframes> | <slots set to NULL>", per L one line "L <keyframe> <links>" for each entry of the map; every list as "<n> ids".
// tests/test_covisibility_gpu.py builds it, runs it and compares the lines with the restatement's.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "orb_slam2_adapter.hpp"

static std::vector<int32_t> read_ids(std::istream& in) {
    int m = 0;
    in >> m;
    std::vector<int32_t> ids(m);
    for (int i = 0; i < m; i++) in >> ids[i];
    return ids;
}

template <class List> static void print_ids(const List& ids) {
    printf("%zu ", ids.size());
    size_t i = 0;
    for (auto it = ids.begin(); it != ids.end(); ++it, ++i) printf("%s%d", i ? " " : "", *it);
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    try {
        ORB_SLAM2::KeyFrameGraph graph(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream in(line);
            char op = 0;
            in >> op;
            if (op == 'E') {
                int type, a, b, c;
                in >> type >> a >> b >> c;
                switch (type) {
                    case 0: graph.AddObservation(a, b, c); break;
                    case 1: graph.EraseObservation(a, b); break;
                    case 2: graph.SetBadFlag(a); break;
                    case 3: graph.AddConnection(a, b, c); break;
                    case 4: graph.EraseConnection(a, b); break;
                    case 5: graph.SetKeyFrameBad(a); break;
                    case 6: graph.ChangeParent(a, b); break;
                    default: throw std::runtime_error("ops: unknown event");
                }
            } else if (op == 'U') {
                int kf = 0;
                in >> kf;
                graph.UpdateConnections(kf, read_ids(in));
                printf("U %d | ", kf);
                print_ids(graph.GetVectorCovisibleKeyFrames(kf));
                printf(" | ");
                print_ids(graph.GetBestCovisibilityKeyFrames(kf, 10));
                printf(" | ");
                print_ids(graph.GetCovisiblesByWeight(kf, 15));
                printf(" | ");
                print_ids(graph.GetCovisiblesByWeight(kf, 1));
                printf(" | ");
                print_ids(graph.GetConnectedKeyFrames(kf));
                printf(" | %d | %d\n", graph.GetParent(kf), graph.GetWeight(kf, kf > 0 ? kf - 1 : 0));
            } else if (op == 'T') {
                std::vector<int32_t> points = read_ids(in);
                const std::vector<int32_t> before = points;
                if (!graph.UpdateLocalKeyFrames(points)) { printf("T empty\n"); continue; }
                std::vector<int32_t> nulled;
                for (size_t i = 0; i < points.size(); i++)
                    if (points[i] != before[i]) nulled.push_back((int32_t)i);
                printf("T %d | ", graph.mpReferenceKF);
                print_ids(graph.mvpLocalKeyFrames);
                printf(" | ");
                print_ids(nulled);
                printf("\n");
            } else if (op == 'L') {
                const std::vector<int32_t> connected = read_ids(in);
                std::vector<std::vector<int32_t> > pointsOfEach;
                for (size_t i = 0; i < connected.size(); i++) pointsOfEach.push_back(read_ids(in));
                const std::map<int32_t, std::set<int32_t> > LoopConnections = ORB_SLAM2::LoopClosing::LoopConnections(graph, connected, pointsOfEach);
                for (const auto& e : LoopConnections) {
                    printf("L %d ", e.first);
                    print_ids(e.second);
                    printf("\n");
                }
            } else {
                throw std::runtime_error("ops: unknown operation");
            }
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
