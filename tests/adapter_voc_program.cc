// A small caller written ONLY against ORB_SLAM2::ORBVocabulary and ORBmatcher of include/orb_slam2_adapter.hpp, the way the reference's System /
// Frame / KeyFrame code uses the vocabulary: loadFromTextFile, transform(desc, BowVector, FeatureVector, 4) for two frames, score, and SearchByBoW
// with the two FeatureVectors.  It reads the vocabulary file and raw arrays from a directory (written by tests/test_vocabulary_gpu.py) and dumps what it
// got; the test compares the dump with the ctypes path.  Usage: adapter_voc_program <dir>;  a second argument = a file that must NOT load.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "../include/orb_slam2_adapter.hpp"

static std::string g_dir;
template <class T>
static std::vector<T> rd(const std::string& name) {
    std::ifstream f(g_dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!f) { std::cerr << "missing " << name << "\n"; exit(2); }
    const size_t n = (size_t)f.tellg();
    std::vector<T> v(n / sizeof(T));
    f.seekg(0);
    f.read((char*)v.data(), n);
    return v;
}
template <class T>
static void wr(const std::string& name, const std::vector<T>& v) {
    std::ofstream f(g_dir + "/out_" + name + ".bin", std::ios::binary);
    f.write((const char*)v.data(), v.size() * sizeof(T));
}

static void dump(const std::string& tag, const DBoW2::BowVector& v, const DBoW2::FeatureVector& fv) {
    std::vector<uint32_t> ids, nodes, count, items;
    std::vector<double> vals;
    for (const auto& e : v) { ids.push_back(e.first); vals.push_back(e.second); }
    for (const auto& e : fv) {
        nodes.push_back(e.first); count.push_back((uint32_t)e.second.size());
        items.insert(items.end(), e.second.begin(), e.second.end());
    }
    wr(tag + "_bow_ids", ids); wr(tag + "_bow_vals", vals); wr(tag + "_fv_nodes", nodes); wr(tag + "_fv_count", count); wr(tag + "_fv_items", items);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    g_dir = argv[1];
    using namespace ORB_SLAM2;
    try {
        ORBVocabulary voc;
        if (argc > 2) {   // System.cc:68-74: a file that does not load
            const bool ok = voc.loadFromTextFile(argv[2]);
            std::cout << (ok ? "loaded" : "refused") << " " << oslam_last_error() << "\n";
            return ok ? 1 : 0;
        }
        if (!voc.loadFromTextFile(g_dir + "/voc.txt")) { std::cerr << "Wrong path to vocabulary: " << oslam_last_error() << "\n"; return 1; }
        std::vector<oslam::KeyPoint> kA = rd<oslam::KeyPoint>("keysA"), kB = rd<oslam::KeyPoint>("keysB");
        std::vector<uint8_t> dA = rd<uint8_t>("descA"), dB = rd<uint8_t>("descB");
        DBoW2::BowVector bowA, bowB;
        DBoW2::FeatureVector fvA, fvB;
        voc.transform(dA, bowA, fvA, 4);
        voc.transform(dB, bowB, fvB, 4);
        dump("A", bowA, fvA);
        dump("B", bowB, fvB);
        const ORBmatcher::FeatureVector fA = ORBVocabulary::flatten(fvA), fB = ORBVocabulary::flatten(fvB);
        wr("A_qidx", fA.q_idx); wr("A_qnode", fA.q_node); wr("B_nodes", fB.nodes); wr("B_start", fB.start); wr("B_items", fB.items);
        FrameView KF = {(int)kA.size(), kA.data(), nullptr, dA.data(), nullptr, 0.f, 0.f, 640.f, 480.f};
        FrameView F = {(int)kB.size(), kB.data(), nullptr, dB.data(), nullptr, 0.f, 0.f, 640.f, 480.f};
        std::vector<uint8_t> good(kA.size(), 1);
        std::vector<int32_t> match;
        ORBmatcher m(0.7f, true);
        const int nm = m.SearchByBoW(KF, fA, good.data(), F, fB, match);
        wr("bow_match", match);
        std::ofstream r(g_dir + "/out_results.txt");
        r.precision(17);
        r << "nbow " << nm << "\nscoreAB " << voc.score(bowA, bowB) << "\nscoreAA " << voc.score(bowA, bowA) << "\n";
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    return 0;
}
