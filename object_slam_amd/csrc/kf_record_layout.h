// Byte layout of one resident keyframe record of the driver's operator table (slam_ops_hip.hip), stated ONCE: every array of a record starts on a 256-byte
// boundary, in this order.  The host accessors, the record size of the chunk allocations and the geometry the mirror kernels receive all read this object;
// kernels of other translation units get pointers into records, so the order and the rounding are part of the table's contract with them.
// Pure host arithmetic on top of stage_layout.h: no HIP (tests/stage_layout_check.cc pins two capacities by hand).
#pragma once
#include "../../include/oslam_hip.h"
#include "stage_layout.h"

namespace oslam {

struct KfRecordLayout {
    Field<oslam_keypoint_t> keys;   // mvKeysUn [cap]
    Field<uint8_t> desc;            // mDescriptors [cap][32]
    Field<float> ur;                // mvuRight [cap]
    Field<uint16_t> cell_end;       // feature grid: end of every cell's candidate run [3072]
    Field<float> cand;              // feature grid: candidates sorted by cell, 16 bytes each [cap][4]
    Field<int32_t> mp;              // mirror of the observation graph: the keyframe's point list [cap]; everything before it is the record's core
    Field<uint64_t> okf;            // "which point observes keypoint i": event number << 32 | point [cap]
    Field<uint32_t> good;           // usable-depth bits [(cap + 31) / 32]
    size_t bytes = 0;               // one record

    explicit KfRecordLayout(size_t cap = 0) {
        StageLayout lay;
        keys = lay.add<oslam_keypoint_t>(cap); desc = lay.add<uint8_t>(cap * 32); ur = lay.add<float>(cap); cell_end = lay.add<uint16_t>(3072); cand = lay.add<float>(cap * 4);
        mp = lay.add<int32_t>(cap); okf = lay.add<uint64_t>(cap); good = lay.add<uint32_t>((cap + 31) / 32);
        bytes = lay.total();
    }
    size_t core_bytes() const { return mp.off; }
    // the mirror kernels address okf and good from the point list
    size_t okf_from_mp() const { return okf.off - mp.off; }
    size_t good_from_mp() const { return good.off - mp.off; }
};

}  // namespace oslam
