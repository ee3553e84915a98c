// devunit_host.h — the host side every entry point of the TEST-ONLY device library shares (devunit.hip,
// devunit_linalg.hip, devunit_stats.hip, devunit_optim.hip): the device buffers of one call, whose first error sticks.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace devunit {

struct Bufs {
    std::vector<void*> p;
    hipError_t e = hipSuccess;
    ~Bufs() {
        for (void* q : p) (void)hipFree(q);
    }
    void chk(hipError_t r) {
        if (e == hipSuccess) e = r;
    }
    // n uninitialised device elements
    template <class T>
    T* alloc(size_t n) {
        if (e != hipSuccess) return nullptr;
        void* d = nullptr;
        chk(hipMalloc(&d, n * sizeof(T)));
        if (e != hipSuccess) return nullptr;
        p.push_back(d);
        return (T*)d;
    }
    // device copy of n host elements (output buffers too: entries a kernel leaves alone keep the host's values)
    template <class T>
    T* put(const T* h, size_t n) {
        if (e != hipSuccess || h == nullptr) return nullptr;
        T* d = alloc<T>(n);
        if (e != hipSuccess) return nullptr;
        chk(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <class T>
    void get(T* h, const T* d, size_t n) {
        if (e == hipSuccess && h != nullptr && d != nullptr) chk(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
    }
    void done() {
        chk(hipGetLastError());
        chk(hipDeviceSynchronize());
    }
};

}  // namespace devunit
