// The host-side timers of the junc driver (PJB_PROFILE_HOST): one object for the workers and the device threads.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <mutex>
#include <string>
#include <vector>

namespace portcullis {

struct HostProfile {  // PJB_PROFILE_HOST=1: where the host side of findJuncs spends its time
    bool on = getenv("PJB_PROFILE_HOST") != nullptr;
    double t0 = now();  // (static initialisation: about when the process starts)
    void mark(const char* what) {
        if (!on) return;
        std::lock_guard<std::mutex> lk(mu);
        std::cerr << "[host profile] t=" << (now() - t0) << " s: " << what << std::endl;
    }
    std::mutex mu;
    // PJB_PROFILE_HOST=2: every command of the device threads and every step of the workers with its start and end
    struct Event {
        double a, b;
        std::string what;
    };
    bool events_on = on && atoi(getenv("PJB_PROFILE_HOST")) >= 2;
    std::vector<Event> events;
    void event(double a, double b, const std::string& what) {
        if (!events_on) return;
        std::lock_guard<std::mutex> lk(mu);
        events.push_back({a - t0, b - t0, what});
    }
    void dumpEvents() {
        if (!events_on) return;
        std::lock_guard<std::mutex> lk(mu);
        std::sort(events.begin(), events.end(), [](const Event& x, const Event& y) { return x.a < y.a; });
        for (auto& e : events) {
            char line[256];
            snprintf(line, sizeof line, "[host event] %8.4f %8.4f %7.1f ms  %s", e.a, e.b, (e.b - e.a) * 1e3, e.what.c_str());
            std::cerr << line << "\n";
        }
    }
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};
extern HostProfile g_prof;  // (device_thread.cc)

}  // namespace portcullis
