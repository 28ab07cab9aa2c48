// warped_bricks.hpp — the brick of the warped TSDF sweeps (tsdf_warped.hip) and of the k-NN field (knn_field.hip), the
// field's size arithmetic and the launchers' dispatch over K.  Host-only code: no HIP header, plain g++ compiles it
// (tests/cpp/test_knn_field_size.cpp drives the arithmetic on the CPU).
#pragma once
#include <cstddef>
#include <cstdint>

namespace dfa {

// A brick, in voxels.  One slice deep: a lane's voxels are searched one after the other, and the searches of a brick far from
// the nodes are long (shells beyond the 3 x 3 x 3 block), so deeper bricks are fewer, longer workgroups with a long tail —
// measured at 512^3, 2 048 nodes, k = 8 (tools/warped_integrate_timing.py, SKIP mode): 8 slices 9.39 ms, 4: 7.80, 2: 6.98,
// 1: 4.47.  The code of the sweeps holds for any depth that divides the occupancy box's 8.
constexpr int WBX = 64, WBY = 4, WBZ = 1;
constexpr int WB_VOXELS = WBX * WBY * WBZ;

// ---- the k-NN field's sizes.  size_t throughout: a 1024^3 volume with k = 16 is 64 GiB when every brick is stored.
inline size_t knn_field_bricks(int X, int Y, int Z) {
    return (size_t)((X + WBX - 1) / WBX) * (size_t)((Y + WBY - 1) / WBY) * (size_t)((Z + WBZ - 1) / WBZ);
}
// one brick record: k slots of one int32 per voxel of the brick
inline size_t knn_field_record_bytes(int k) { return (size_t)WB_VOXELS * (size_t)k * sizeof(int32_t); }
// records are numbered by int32 (the per-brick table), and so are the bricks
constexpr size_t KNN_FIELD_MAX_RECORDS = 0x7fffffffu;
// the bytes of `records` records; false when that many records cannot be numbered or their bytes overflow size_t
inline bool knn_field_bytes(size_t records, int k, size_t* bytes) {
    const size_t rec = knn_field_record_bytes(k);
    if (records > KNN_FIELD_MAX_RECORDS || (rec != 0 && records > (size_t)-1 / rec)) return false;
    *bytes = records * rec;
    return true;
}
// may a field capped at max_bytes (0: no cap) hold `records` records?
inline bool knn_field_fits(size_t records, int k, size_t max_bytes) {
    size_t bytes;
    return knn_field_bytes(records, k, &bytes) && (max_bytes == 0 || bytes <= max_bytes);
}

}  // namespace dfa

// ---- the dispatch of the launchers over K (tsdf_warped.hip, knn_field.hip): a statement that names KK, with KK the
// smallest of {4, 8, 16} — {4, 8} — that holds k (as K6DISPATCH of solve6_internal.hpp, for kernel templates with further
// parameters):  KDISPATCH16(k, kernel<KK, true><<<...>>>(...));
#define KDISPATCH_AS_(value, ...)  \
    {                              \
        constexpr int KK = value;  \
        __VA_ARGS__;               \
    }
#define KDISPATCH16(k, ...)                               \
    do {                                                  \
        if ((k) <= 4) KDISPATCH_AS_(4, __VA_ARGS__)       \
        else if ((k) <= 8) KDISPATCH_AS_(8, __VA_ARGS__)  \
        else KDISPATCH_AS_(16, __VA_ARGS__)               \
    } while (0)
#define KDISPATCH8(k, ...)                           \
    do {                                             \
        if ((k) <= 4) KDISPATCH_AS_(4, __VA_ARGS__)  \
        else KDISPATCH_AS_(8, __VA_ARGS__)           \
    } while (0)
