// Compile-only check of ORB_SLAM2::Initializer of include/orb_slam2_adapter.hpp (no OpenCV, no GPU needed), in the manner of adapter_compile_check.cc:
// the class is instantiated in dead code so that its inline bodies are compiled and the C ABI symbols they use must resolve at link time.
#include "../include/orb_slam2_adapter.hpp"
int main(int argc, char**) {
    if (argc > 1000) {   // never taken
        ORB_SLAM2::InitFrameView f{};
        ORB_SLAM2::Initializer init(f, 1.0f, 200);
        std::vector<int> vMatches12;
        std::vector<ORB_SLAM2::Point3f> vP3D;
        std::vector<bool> vbTriangulated;
        float R21[9], t21[3];
        (void)init.Initialize(f, vMatches12, R21, t21, vP3D, vbTriangulated);
    }
    return sizeof(ORB_SLAM2::Point3f) == 12 && sizeof(oslam_init_problem_t) == 48 && sizeof(oslam_init_params_t) == 16 ? 0 : 1;
}
