// device_memory.hpp — the owners of the C ABI layer's device memory (host-only; included by the capi*.cpp units through capi_internal.hpp, and by tsdf.hip):
// grow-only scratch buffers and their per-stream table, the arena of a solver plan, the pool of timing events.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)  // internal to the library: nothing here joins its exported symbols
namespace dfa {

// A typed device buffer that grows on demand and never shrinks.  Growing releases first and then allocates (hipFree
// waits for the device, and a fresh hipMalloc costs milliseconds: callers whose sizes creep upwards ask for headroom);
// after a failed allocation the buffer is empty.  No destructor: the per-stream table below lives until the process
// ends, behind the HIP runtime's own teardown, and plans release theirs.
template <class T>
struct DeviceBuffer {
    T* data    = nullptr;
    size_t cap = 0;  // elements
    void release() {
        (void)hipFree(data);
        data = nullptr, cap = 0;
    }
    // room for `count` elements; a buffer that has to grow for them is allocated with `headroom` more
    hipError_t reserve(size_t count, size_t headroom = 0) {
        if (count <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void**)&data, sizeof(T) * (count + headroom));
        if (e == hipSuccess) cap = count + headroom;
        else data = nullptr;
        return e;
    }
    // as reserve, but the first `keep` elements survive the move (copied on `s`, which is waited for before the old
    // block goes); after a failed allocation the buffer is what it was
    hipError_t grow_keep(size_t count, size_t keep, size_t headroom, hipStream_t s) {
        if (count <= cap) return hipSuccess;
        T* fresh     = nullptr;
        hipError_t e = hipMalloc((void**)&fresh, sizeof(T) * (count + headroom));
        if (e != hipSuccess) return e;
        if (keep) e = hipMemcpyAsync(fresh, data, sizeof(T) * keep, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(fresh);
            return e;
        }
        (void)hipFree(data);
        data = fresh, cap = count + headroom;
        return hipSuccess;
    }
};

// Scratch of the entry points that have no plan to keep it in (dfa_knn, dfa_warp_to_live, dfa_correspond,
// dfa_marching_cubes, dfa_icp_sums, the tile table of the TSDF sweeps ...): one instance of T per (device, stream),
// created on first use and kept.  Work on one stream is ordered, so a call never overwrites the scratch of a call still
// running — whichever host threads and however many streams the caller uses (round 1 kept these per host THREAD: two
// streams driven by one thread shared them).  The C ABI's caller owns every buffer it passes; these are internal.
template <class T>
T& stream_scratch(hipStream_t s) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, T> table;  // (device, stream): the null stream exists on every device
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    return table[std::make_pair(dev, s)];  // std::map nodes never move
}

// Every device array and pinned host block of one solver plan: a hipMalloc per array (never one large block cut up:
// where the buffers lie is part of what the benchmark measured), freed together with the plan.  The first failure sticks — later
// requests do nothing — so a plan's field list reads as a list, with one check behind it.
class PlanArena {
    std::vector<void*> device_, pinned_;

  public:
    hipError_t error = hipSuccess;  // the first failure
    const char* what = "";          // the call attempted last: behind a failure, the one that failed
    PlanArena()      = default;
    PlanArena(const PlanArena&)            = delete;
    PlanArena& operator=(const PlanArena&) = delete;
    ~PlanArena() {
        for (void* p : device_) (void)hipFree(p);
        for (void* p : pinned_) (void)hipHostFree(p);
    }

    bool ok() const { return error == hipSuccess; }

    // *out = `count` elements of T (an empty array is one element long), zero-filled on request
    template <class T>
    void alloc(T** out, size_t count, bool zero = false) {
        if (!ok()) return;
        const size_t bytes = sizeof(T) * (count ? count : 1);
        void* p            = nullptr;
        what               = "hipMalloc (plan memory)";
        if ((error = hipMalloc(&p, bytes)) != hipSuccess) return;
        device_.push_back(p);
        *out = (T*)p;
        what = "hipMemset (plan memory)";
        if (zero) error = hipMemset(p, 0, bytes);
    }

    // `count` zeroed elements of pinned host memory, or null: what a plan can do without is the plan's decision
    template <class T>
    T* pinned(size_t count) {
        void* p = nullptr;
        if (!ok() || hipHostMalloc(&p, sizeof(T) * count, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        pinned_.push_back(p);
        std::memset(p, 0, sizeof(T) * count);
        return (T*)p;
    }
};

// Timing events of a plan, created as they are needed and kept until the plan goes: a measurement rewinds the pool and
// takes them again in order.
struct EventPool {
    std::vector<hipEvent_t> events;
    size_t used = 0;
    EventPool() = default;
    EventPool(const EventPool&) = delete;
    ~EventPool() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }

    // the next `count` events (created where the pool is exhausted): the index of the first, or -1 and none taken
    int take(int count) {
        while (events.size() < used + (size_t)count) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return -1;
            events.push_back(e);
        }
        used += (size_t)count;
        return (int)used - count;
    }
    // records the next event on st: its index, or -1 (no event to be had: the bracket is not taken)
    int record(hipStream_t st) {
        const int i = take(1);
        if (i >= 0) (void)hipEventRecord(events[i], st);
        return i;
    }
    void rewind() { used = 0; }
};

}  // namespace dfa
#pragma GCC visibility pop
