// stage_clock.hpp — DFA_HOST_PROFILE=1: wall time of the stages of a frame (device synchronised at every mark) on stderr.
// Private to the units of DynFusion (dyn_fusion.cpp, dyn_fusion_northstar.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>

#include <dfa_host/device.hpp>

namespace dfa {
struct StageClock {
    bool on = host_switch("DFA_HOST_PROFILE");
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char* what) {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[dfa host] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};
}  // namespace dfa
