// test_knn_field_size.cpp — the size arithmetic of the k-NN field (dynfu_amd/csrc/warped_bricks.hpp) on the CPU: no HIP, no
// library.  Brick counts, record bytes, the byte count past 2^31 and past size_t, and the max_bytes compare.
#include <cstdint>

#include "../../dynfu_amd/csrc/warped_bricks.hpp"
#include "minitest.hpp"

using namespace dfa;

static_assert(sizeof(size_t) == 8, "the field's sizes are 64-bit");
static_assert(WB_VOXELS == 256, "a record slot is one 256-voxel brick");

TEST(KnnFieldSize, BricksOfAVolume) {
    ASSERT_EQ(knn_field_bricks(32, 32, 32), (size_t)256);    // 1 x 8 x 32
    ASSERT_EQ(knn_field_bricks(50, 38, 44), (size_t)440);    // 1 x 10 x 44
    ASSERT_EQ(knn_field_bricks(9, 7, 14), (size_t)28);       // 1 x 2 x 14
    ASSERT_EQ(knn_field_bricks(1, 2, 12), (size_t)12);
    ASSERT_EQ(knn_field_bricks(65, 5, 1), (size_t)4);        // partial bricks count
    ASSERT_EQ(knn_field_bricks(512, 512, 512), (size_t)524288);
    ASSERT_EQ(knn_field_bricks(1024, 1024, 1024), (size_t)4194304);
}

TEST(KnnFieldSize, RecordBytes) {
    ASSERT_EQ(knn_field_record_bytes(1), (size_t)1024);
    ASSERT_EQ(knn_field_record_bytes(8), (size_t)8192);
    ASSERT_EQ(knn_field_record_bytes(16), (size_t)16384);
}

TEST(KnnFieldSize, BytesPastTwoToThe31AndPastSizeT) {
    size_t bytes = 0;
    // the first record count whose bytes no longer fit 31 bits at k = 8
    ASSERT_TRUE(knn_field_bytes(262143, 8, &bytes) && bytes == 2147475456ull);
    ASSERT_TRUE(knn_field_bytes(262144, 8, &bytes) && bytes == 2147483648ull);
    ASSERT_TRUE(knn_field_bytes(262145, 8, &bytes) && bytes == 2147491840ull);
    // 1024^3, k = 16, every brick stored: 64 GiB
    ASSERT_TRUE(knn_field_bytes(knn_field_bricks(1024, 1024, 1024), 16, &bytes) && bytes == (64ull << 30));
    // 512^3, k = 8: 4 GiB
    ASSERT_TRUE(knn_field_bytes(knn_field_bricks(512, 512, 512), 8, &bytes) && bytes == (4ull << 30));
    // records are numbered by int32
    ASSERT_TRUE(knn_field_bytes(KNN_FIELD_MAX_RECORDS, 16, &bytes) && bytes == 0x7fffffffull * 16384ull);
    bytes = 7;
    ASSERT_TRUE(!knn_field_bytes(KNN_FIELD_MAX_RECORDS + 1, 1, &bytes) && bytes == 7);
    ASSERT_TRUE(!knn_field_bytes((size_t)-1, 16, &bytes) && !knn_field_bytes((size_t)-1 / 16384 + 1, 16, &bytes) && bytes == 7);
    ASSERT_TRUE(knn_field_bytes(0, 16, &bytes) && bytes == 0);
}

TEST(KnnFieldSize, TheCap) {
    ASSERT_TRUE(knn_field_fits(230, 8, 0));  // 0: no cap
    ASSERT_TRUE(knn_field_fits(230, 8, 230 * 8192) && !knn_field_fits(230, 8, 230 * 8192 - 1) && !knn_field_fits(231, 8, 230 * 8192));
    ASSERT_TRUE(knn_field_fits(0, 8, 1));
    const size_t dense = knn_field_bricks(1024, 1024, 1024);
    ASSERT_TRUE(!knn_field_fits(dense, 16, (64ull << 30) - 1) && knn_field_fits(dense, 16, 64ull << 30));
    ASSERT_TRUE(!knn_field_fits(dense, 16, 0xffffffffull));  // a cap of 4 GiB - 1 is not compared in 32 bits
    ASSERT_TRUE(!knn_field_fits(dense, 16, 1));
    ASSERT_TRUE(!knn_field_fits(KNN_FIELD_MAX_RECORDS + 1, 1, 0));  // without a cap, too many records are still refused
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
