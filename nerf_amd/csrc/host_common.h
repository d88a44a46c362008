// Host-side launch helpers shared by the kernel translation units.  Everything here is keyed by the CURRENT DEVICE and guarded by a
// mutex: hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies per device, so one process driving several GPUs (or several host
// threads) must opt in once per (device, kernel function), and the CU count that sizes the persistent grids is a per-device fact.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>

namespace nerf_host {

inline std::mutex& table_mutex() { static std::mutex m; return m; }

inline int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return dev;
}

// Dynamic LDS above 64 KiB is an opt-in per kernel function AND device; done once for each pair (and again if a larger size is asked).
inline int allow_dynamic_lds(const void* fn, size_t lds) {
    struct Entry { int dev; const void* fn; size_t lds; };
    static std::vector<Entry> done;
    const int dev = current_device();
    std::lock_guard<std::mutex> lock(table_mutex());
    for (auto& e : done)
        if (e.dev == dev && e.fn == fn) {
            if (e.lds >= lds) return 0;
            hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (err != hipSuccess) return (int)err;
            e.lds = lds;
            return 0;
        }
    hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return (int)err;
    done.push_back({dev, fn, lds});
    return 0;
}

// compute units of the current device (256 on MI355X); persistent kernels launch one workgroup per CU
inline int cu_count() {
    static int n_cu[64] = {0};
    const int dev = current_device();
    std::lock_guard<std::mutex> lock(table_mutex());
    int& slot = n_cu[dev & 63];
    if (!slot) {
        hipDeviceProp_t p;
        slot = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
    }
    return slot;
}

// Tile counters of the render MLP kernels that hand their tiles out dynamically (mlp_kernels.hip, "Elastic tiles"): one 32-bit counter
// per STREAM that launches such a kernel, in a small pool that the library owns per device.  Launches of one stream are ordered, so they
// may share a counter -- the launcher zeroes it with a stream-ordered memset ahead of each launch that needs it --; launches in flight on
// different streams never do.  The pool, described once:
constexpr int TILE_COUNTER_SLOTS = 32;            // streams per device that hold a counter at one time
constexpr size_t TILE_COUNTER_STRIDE = 128;       // bytes from one counter to the next (each in a cache line of its own)
constexpr size_t TILE_COUNTER_POOL_BYTES = TILE_COUNTER_SLOTS * TILE_COUNTER_STRIDE;
// When a further stream finds the pool full, the device is synchronised -- nothing that counts is in flight any more -- and the pool is
// handed out afresh.
inline int tile_counter(hipStream_t st, unsigned** counter) {
    struct Pool { int dev; char* base; int used; hipStream_t owner[TILE_COUNTER_SLOTS]; };
    static std::vector<Pool> pools;
    const int dev = current_device();
    std::lock_guard<std::mutex> lock(table_mutex());
    Pool* p = nullptr;
    for (auto& q : pools)
        if (q.dev == dev) p = &q;
    if (!p) {
        void* mem = nullptr;
        if (hipError_t err = hipMalloc(&mem, TILE_COUNTER_POOL_BYTES)) return (int)err;
        pools.push_back(Pool{dev, reinterpret_cast<char*>(mem), 0, {}});
        p = &pools.back();
    }
    int k = 0;
    while (k < p->used && p->owner[k] != st) ++k;
    if (k == p->used) {
        if (p->used == TILE_COUNTER_SLOTS) {
            if (hipError_t err = hipDeviceSynchronize()) return (int)err;
            p->used = 0;
            k = 0;
        }
        p->owner[p->used++] = st;
    }
    *counter = reinterpret_cast<unsigned*>(p->base + (size_t)k * TILE_COUNTER_STRIDE);
    return 0;
}

}  // namespace nerf_host
