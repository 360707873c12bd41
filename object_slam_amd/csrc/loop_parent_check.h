// The check of a spanning-tree `parent` array that the host entry point of the map update after global BA runs before it launches anything
// (include/oslam_hip.h, "LoopClosing: map corrections").  Pure host arithmetic: no HIP, no runtime call; tests/loop_parent_check.cc runs it under the
// address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>
#include <vector>

namespace oslam {

enum { kParentOk = 0, kParentOutOfRange = 1, kParentCycle = 2 };

// parent[k] is -1 (a root) or the index in [0, n) of k's parent.  Answers kParentOutOfRange for an index outside [-1, n), kParentCycle when following
// parents from some keyframe comes back to a keyframe already on the way (a self-parent included), kParentOk otherwise.  O(n): every keyframe is walked
// over at most twice.  `mark` is scratch (resized here): 0 not seen, 1 on the path being walked, 2 known to end at a root.
inline int parent_tree_check(const int32_t* parent, int n, std::vector<uint8_t>& mark) {
    if (n <= 0) return kParentOk;
    for (int k = 0; k < n; k++)
        if (parent[k] < -1 || parent[k] >= n) return kParentOutOfRange;
    mark.assign((size_t)n, 0);
    for (int k = 0; k < n; k++) {
        int j = k;
        while (j >= 0 && mark[(size_t)j] == 0) { mark[(size_t)j] = 1; j = parent[j]; }
        if (j >= 0 && mark[(size_t)j] == 1) return kParentCycle;
        j = k;
        while (j >= 0 && mark[(size_t)j] == 1) { mark[(size_t)j] = 2; j = parent[j]; }
    }
    return kParentOk;
}

}  // namespace oslam
