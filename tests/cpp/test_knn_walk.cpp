// test_knn_walk.cpp — dynfu_amd/csrc/knn_walk.hpp on the CPU: no HIP, no library.  A lane's walk over the nine row ranges of
// the 3 x 3 x 3 block exactly as knn_grid_query runs it (plan, then `steps` steps of one batch each, the slots in an array of
// the lane's own), on hand-made and random range sets: every index of every non-empty range exactly once and in range order,
// no more steps than the trip count computed before the loop, every index a load would form inside the sorted array —
// damaged tables included —, and a wave of 64 such lanes leaving after the longest lane's trip count.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <random>

#include "../../dynfu_amd/csrc/knn_walk.hpp"
#include "minitest.hpp"

using namespace dfa;

namespace {
constexpr int POISON = INT_MIN / 2;  // a slot that was never stored: fetching it shows in every check below

struct Lane {
    int sb[KNN_WALK_ROWS], se[KNN_WALK_ROWS];  // the lane's slots
    int stored_max = -1, steps = 0, fetched = 0;
    KnnWalk w;
    std::vector<int> visited;  // candidates pushed, in order
    std::vector<int> loaded;   // every index a (clamped) load formed
};

void plan(Lane& l, const int (&rb)[KNN_WALK_ROWS], const int (&re)[KNN_WALK_ROWS], int count) {
    std::fill(l.sb, l.sb + KNN_WALK_ROWS, POISON), std::fill(l.se, l.se + KNN_WALK_ROWS, POISON);
    l.steps = knn_walk_plan(rb, re, count, [&](int slot, int b, int e) {
        ASSERT_TRUE(slot >= 0 && slot < KNN_WALK_ROWS);
        l.sb[slot] = b, l.se[slot] = e;
        l.stored_max = std::max(l.stored_max, slot);
    });
    knn_walk_begin(l.w);
}

// one step as the kernel's loop body runs it for a lane with s < steps
void step(Lane& l) {
    int j, e;
    knn_walk_step(l.w, [&](int slot, int& b, int& en) {
        ASSERT_TRUE(slot >= 0 && slot <= l.stored_max);
        ASSERT_TRUE(l.sb[slot] != POISON);
        b = l.sb[slot], en = l.se[slot];
        ++l.fetched;
    }, j, e);
    ASSERT_TRUE(j < e);  // a fetched range is never empty, a batch never starts behind its range
    for (int t = 0; t < KNN_WALK_BATCH; ++t) l.loaded.push_back(std::min(j + t, e - 1));
    for (int t = 0; t < KNN_WALK_BATCH; ++t)
        if (j + t < e) l.visited.push_back(j + t);
}

int clampi(int v, int count) { return std::min(std::max(v, 0), count); }

// what the nine loops of scan_block3 visit on the same (clamped) table: the rows in walk order, each range front to back
std::vector<int> expected(const int (&rb)[KNN_WALK_ROWS], const int (&re)[KNN_WALK_ROWS], int count, int* batches, int* kept) {
    std::vector<int> out;
    *batches = *kept = 0;
    for (int i = 0; i < KNN_WALK_ROWS; ++i) {
        const int b = clampi(rb[KNN_WALK_ORDER[i]], count), e = clampi(re[KNN_WALK_ORDER[i]], count);
        for (int j = b; j < e; ++j) out.push_back(j);
        if (e > b) *batches += (e - b + KNN_WALK_BATCH - 1) / KNN_WALK_BATCH, ++*kept;
    }
    return out;
}

void check_lane(const int (&rb)[KNN_WALK_ROWS], const int (&re)[KNN_WALK_ROWS], int count) {
    Lane l;
    plan(l, rb, re, count);
    int batches, kept;
    const std::vector<int> want = expected(rb, re, count, &batches, &kept);
    ASSERT_EQ(l.steps, batches);
    ASSERT_TRUE(l.steps <= KNN_WALK_ROWS * ((count + KNN_WALK_BATCH - 1) / KNN_WALK_BATCH));
    for (int s = 0; s < l.steps; ++s) step(l);
    ASSERT_TRUE(l.visited == want);  // every index once, in range order, after exactly `steps` steps
    ASSERT_EQ(l.fetched, kept);
    for (int i : l.loaded) ASSERT_TRUE(i >= 0 && i < count);
}

void set_lengths(int (&rb)[KNN_WALK_ROWS], int (&re)[KNN_WALK_ROWS], const int (&len)[KNN_WALK_ROWS], int first) {
    int at = first;
    for (int i = 0; i < KNN_WALK_ROWS; ++i) rb[i] = at, re[i] = at + len[i], at += len[i] + 2;
}
}  // namespace

TEST(KnnWalk, OrderIsOwnRowThenFacesThenCorners) {
    bool seen[KNN_WALK_ROWS] = {};
    for (int i = 0; i < KNN_WALK_ROWS; ++i) ASSERT_TRUE(KNN_WALK_ORDER[i] >= 0 && KNN_WALK_ORDER[i] < KNN_WALK_ROWS), seen[KNN_WALK_ORDER[i]] = true;
    for (bool s : seen) ASSERT_TRUE(s);
    ASSERT_EQ(KNN_WALK_ORDER[0], 4);
    for (int i = 1; i < 5; ++i) ASSERT_TRUE(KNN_WALK_ORDER[i] % 2 == 1);               // dy == 0 or dz == 0
    for (int i = 5; i < 9; ++i) ASSERT_TRUE(KNN_WALK_ORDER[i] % 2 == 0 && KNN_WALK_ORDER[i] != 4);
}

TEST(KnnWalk, HandMadeRangeSets) {
    int rb[KNN_WALK_ROWS], re[KNN_WALK_ROWS];
    // all nine empty: no step, no slot fetched
    for (int i = 0; i < KNN_WALK_ROWS; ++i) rb[i] = re[i] = 7 * i;
    check_lane(rb, re, 100);
    {
        Lane l;
        plan(l, rb, re, 100);
        ASSERT_EQ(l.steps, 0);
    }
    // a single candidate in the row walked last (row 8), which is also the last element of the sorted array
    for (int i = 0; i < KNN_WALK_ROWS; ++i) rb[i] = re[i] = 0;
    rb[8] = 99, re[8] = 100;
    check_lane(rb, re, 100);
    // lengths 0, 1, 3, 4, 5 and 9 (empty ranges between kept ones, partial and full batches, more than two batches)
    const int mixed[KNN_WALK_ROWS] = {0, 1, 3, 4, 5, 9, 0, 0, 2};
    set_lengths(rb, re, mixed, 3);
    check_lane(rb, re, 64);
    // nine full ranges, and nine of one candidate each
    const int full[KNN_WALK_ROWS] = {12, 12, 12, 12, 12, 12, 12, 12, 12}, ones[KNN_WALK_ROWS] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    set_lengths(rb, re, full, 0);
    check_lane(rb, re, 200);
    set_lengths(rb, re, ones, 0);
    check_lane(rb, re, 200);
    // only the own row (all nodes in one x-row of cells)
    for (int i = 0; i < KNN_WALK_ROWS; ++i) rb[i] = re[i] = 0;
    rb[4] = 10, re[4] = 31;
    check_lane(rb, re, 40);
}

TEST(KnnWalk, DamagedTablesStayInsideTheArrayAndTheTripCount) {
    const int count = 37;
    int rb[KNN_WALK_ROWS] = {-5, 30, 20, INT_MIN, 0, 36, 40, 10, -1};
    int re[KNN_WALK_ROWS] = {3, 1000, 10, INT_MAX, INT_MAX, 37, 50, 10, INT_MIN};
    check_lane(rb, re, count);
    Lane l;
    plan(l, rb, re, count);
    ASSERT_TRUE(l.steps <= KNN_WALK_ROWS * ((count + KNN_WALK_BATCH - 1) / KNN_WALK_BATCH));
    // an empty array: nothing can be walked, whatever the table says
    check_lane(rb, re, 0);
}

TEST(KnnWalk, RandomRangeSets) {
    std::mt19937 rng(20240613u);
    for (int rep = 0; rep < 20000; ++rep) {
        const int count = 1 + (int)(rng() % 300);
        int rb[KNN_WALK_ROWS], re[KNN_WALK_ROWS];
        for (int i = 0; i < KNN_WALK_ROWS; ++i) {
            const int kind = (int)(rng() % 8);
            rb[i] = (int)(rng() % (unsigned)(count + 1));
            re[i] = kind < 3 ? rb[i] : std::min(count, rb[i] + (int)(rng() % 14));        // empty rows are common on a surface
            if (kind == 7) rb[i] -= (int)(rng() % 5), re[i] += (int)(rng() % 5) - 2;      // now and then outside / reversed
        }
        check_lane(rb, re, count);
    }
}

// 64 lanes in the kernel's loop: `for (s = 0; s < cap && any(s < steps); ++s) if (s < steps) step`
TEST(KnnWalk, AWaveLeavesWithItsLongestLane) {
    std::mt19937 rng(7u);
    for (int rep = 0; rep < 300; ++rep) {
        const int count = 500;
        std::vector<Lane> lanes(64);
        std::vector<std::vector<int>> want(64);
        int longest = 0, nine_loops = 0, row_max[KNN_WALK_ROWS] = {};
        for (int l = 0; l < 64; ++l) {
            int rb[KNN_WALK_ROWS], re[KNN_WALK_ROWS], len[KNN_WALK_ROWS];
            // (rep 0: one lane with nine full ranges beside 63 lanes with one candidate each)
            for (int i = 0; i < KNN_WALK_ROWS; ++i) len[i] = rep == 0 ? (l == 17 ? 16 : (i == 4 ? 1 : 0)) : (rng() % 3 ? (int)(rng() % 11) : 0);
            set_lengths(rb, re, len, (int)(rng() % 50));
            plan(lanes[l], rb, re, count);
            int batches, kept;
            want[l] = expected(rb, re, count, &batches, &kept);
            longest = std::max(longest, lanes[l].steps);
            for (int i = 0; i < KNN_WALK_ROWS; ++i) row_max[i] = std::max(row_max[i], (len[i] + KNN_WALK_BATCH - 1) / KNN_WALK_BATCH);
        }
        for (int i = 0; i < KNN_WALK_ROWS; ++i) nine_loops += row_max[i];
        const int cap = KNN_WALK_ROWS * ((count + KNN_WALK_BATCH - 1) / KNN_WALK_BATCH);
        int trips = 0;
        for (int s = 0; s < cap; ++s) {
            bool any = false;
            for (auto& l : lanes) any = any || s < l.steps;
            if (!any) break;
            ++trips;
            for (auto& l : lanes)
                if (s < l.steps) step(l);
        }
        ASSERT_EQ(trips, longest);
        ASSERT_TRUE(longest <= nine_loops);  // never more than the nine wave-wide loops take
        if (rep == 0) ASSERT_TRUE(longest == 36 && nine_loops == 36);
        for (int l = 0; l < 64; ++l) ASSERT_TRUE(lanes[l].visited == want[l]);
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
