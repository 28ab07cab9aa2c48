// knn_walk.hpp — one candidate loop per lane over the nine x-rows of the 3 x 3 x 3 block of knn_grid_query (knn_device.hpp),
// as host/device code: no HIP runtime call, plain g++ compiles it (tests/cpp/test_knn_walk.cpp drives it on the CPU), and
// every lane of the one-lane-per-query searches runs it on the device.
//
// Nine wave-wide loops, one per row, each last as long as the longest lane of the wave in THAT row: a wave pays
// sum_rows max_lanes(batches of the row) where any one lane needs sum_rows(its own batches).  Here a lane walks its own rows
// in one loop, and the wave leaves when its last lane has finished: max_lanes sum_rows (tools/knn_walk_count.py counts both).
//
//   the plan (knn_walk_plan)   the nine [beg, end) ranges in walk order, each clamped to [0, count] (count = the length of
//                              the sorted array), the non-empty ones stored to consecutive slots 0, 1, ...; returns the
//                              lane's trip count, sum ceil(length / KNN_WALK_BATCH) <= 9 ceil(count / KNN_WALK_BATCH).  The
//                              trip count is known BEFORE the loop — a lane takes exactly that many steps, whatever the
//                              table held — and every index a step forms lies in [0, count).
//   a step (knn_walk_step)     the lane's next batch [j, min(j + KNN_WALK_BATCH, e)): a batch stays inside its range; a lane
//                              whose range is exhausted takes the next slot first.  A lane that has steps left has a slot
//                              left: the slots hold non-empty ranges only and the trip count is the sum of their batches.
//
// Where the slots live is the caller's: `store(slot, beg, end)` / `fetch(slot, beg, end)`.  On the device they are LDS words
// of the lane's own (ranges picked by a computed index out of registers would be scratch memory); the test keeps an array.
#pragma once

#if defined(__HIPCC__)
#define DFA_WALK_HD __host__ __device__ __forceinline__
#define DFA_WALK_UNROLL _Pragma("unroll")
#else
#define DFA_WALK_HD inline
#define DFA_WALK_UNROLL
#endif

namespace dfa {

constexpr int KNN_WALK_ROWS  = 9;
constexpr int KNN_WALK_BATCH = 4;  // candidates requested together (knn_grid_query's KNN_BATCH)

// the walk order of the rows i = 3 (dz + 1) + (dy + 1): the row of the query's own cell first, then the four rows that share
// a face with it, then the corners (the list fills with near candidates early)
constexpr int KNN_WALK_ORDER[KNN_WALK_ROWS] = {4, 1, 3, 5, 7, 0, 2, 6, 8};

struct KnnWalk {
    int j, e;  // the next candidate of the current range and the range's end
    int next;  // the slot taken when the current range is exhausted
};

DFA_WALK_HD int knn_walk_clamp(int v, int count) { return v < 0 ? 0 : (v > count ? count : v); }

// rbeg / rend: the rows' ranges indexed by row; returns the lane's trip count
template <class Store>
DFA_WALK_HD int knn_walk_plan(const int (&rbeg)[KNN_WALK_ROWS], const int (&rend)[KNN_WALK_ROWS], int count, Store&& store) {
    int steps = 0, slot = 0;
    DFA_WALK_UNROLL for (int i = 0; i < KNN_WALK_ROWS; ++i) {
        const int b = knn_walk_clamp(rbeg[KNN_WALK_ORDER[i]], count), e = knn_walk_clamp(rend[KNN_WALK_ORDER[i]], count);
        // (stored whether empty or not — no branch per row —, but an empty range does not keep its slot: the next one
        // overwrites it, and one that stays behind the last kept slot is never fetched)
        store(slot, b, e);
        const int n = e > b ? (int)((unsigned)(e - b + KNN_WALK_BATCH - 1) / (unsigned)KNN_WALK_BATCH) : 0;
        slot += n > 0 ? 1 : 0;
        steps += n;
    }
    return steps;
}

DFA_WALK_HD void knn_walk_begin(KnnWalk& w) { w.j = w.e = w.next = 0; }

// one of the lane's `steps` steps: the batch is [j, min(j + KNN_WALK_BATCH, e)), e the end of its range
template <class Fetch>
DFA_WALK_HD void knn_walk_step(KnnWalk& w, Fetch&& fetch, int& j, int& e) {
    if (w.j >= w.e) {
        fetch(w.next, w.j, w.e);
        ++w.next;
    }
    j = w.j, e = w.e;
    w.j += KNN_WALK_BATCH;
}

}  // namespace dfa
