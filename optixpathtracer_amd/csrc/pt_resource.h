// pt_resource.h — owners of the HIP resources the host code holds, the C-ABI driver (pt_capi*.cpp)
// and the BVH builders' host stages (pt_build.hip, pt_sah_gpu.hip) alike: each releases what it holds
// in its destructor, none can be copied.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <utility>
#include <vector>

namespace pt {

// n elements of device memory (hipMalloc / hipFree).  hipFree waits for the work that may still
// read the memory.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    // Frees what it held first, so that memory is available to the new allocation.  On failure it
    // is left empty, and a later launch's hipGetLastError does not see the failure.
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, sizeof(T) * n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            return e;
        }
        n_ = n;
        return hipSuccess;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }
    void swap(DevBuf& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
    }
};

// The first failure among results listed in order, e.g. first_error({a.alloc(n), b.alloc(n)}).
inline hipError_t first_error(std::initializer_list<hipError_t> results) {
    for (hipError_t e : results)
        if (e != hipSuccess) return e;
    return hipSuccess;
}

// Waits for `s` when it goes out of scope.  Declared after a function's scratch buffers it is
// destroyed before them, so on every return path the stream is idle when they are freed.
struct StreamIdle {
    hipStream_t s;
    explicit StreamIdle(hipStream_t stream) : s(stream) {}
    StreamIdle(const StreamIdle&) = delete;
    StreamIdle& operator=(const StreamIdle&) = delete;
    ~StreamIdle() { (void)hipStreamSynchronize(s); }
};

// The adaptive sampler's device state (pt_render_adaptive, pt_internal.h AdaptiveBuffers): the
// image-sized arrays, the per-tile ones, the next round's pixel list with its length, the per-pixel
// mean and the scan's scratch.  All or none exist.
struct AdaptiveStore {
    DevBuf<uint32_t> n;
    DevBuf<double> moments;
    DevBuf<float> err, tile_err, mean;
    DevBuf<int> tile_rounds, tile_state, tile_cnt, tile_off, pixel_map, count;
    DevBuf<unsigned char> scan_tmp;
    size_t pixels() const { return n.size(); }
    size_t tiles() const { return tile_state.size(); }
    hipError_t alloc(size_t pixels, size_t tiles, size_t scan_bytes) {
        hipError_t e = moments.alloc(2 * pixels);
        for (DevBuf<float>* b : {&err, &mean})
            if (e == hipSuccess) e = b->alloc(b == &mean ? 3 * pixels : pixels);
        if (e == hipSuccess) e = tile_err.alloc(tiles);
        for (DevBuf<int>* b : {&tile_rounds, &tile_state, &tile_cnt, &tile_off})
            if (e == hipSuccess) e = b->alloc(tiles);
        if (e == hipSuccess) e = pixel_map.alloc(pixels);
        if (e == hipSuccess) e = count.alloc(1);
        if (e == hipSuccess) e = scan_tmp.alloc(std::max<size_t>(scan_bytes, 16));
        if (e == hipSuccess) e = n.alloc(pixels);  // last: its size says that all of them exist
        if (e != hipSuccess) release();
        return e;
    }
    void release() {
        n.reset();
        moments.reset();
        for (DevBuf<float>* b : {&err, &tile_err, &mean}) b->reset();
        for (DevBuf<int>* b : {&tile_rounds, &tile_state, &tile_cnt, &tile_off, &pixel_map, &count}) b->reset();
        scan_tmp.reset();
    }
};

// The pixel filter's device tables (pt_set_pixel_filter, DevLaunch::ss_cells / ss_taps): the
// sub-pixel cell of every cell index (x, y pairs; empty without supersampling) and the cells' tap
// rows (empty for a filter no wider than the box).
struct FilterStore {
    DevBuf<int> cells;
    DevBuf<float> taps;
    void swap(FilterStore& o) noexcept {
        cells.swap(o.cells);
        taps.swap(o.taps);
    }
};

// One word of pinned host memory that kernels read over PCIe: `h` on the host, `d` the same word's
// device address.
struct PinnedWord {
    unsigned* h = nullptr;
    unsigned* d = nullptr;
    PinnedWord() = default;
    PinnedWord(const PinnedWord&) = delete;
    PinnedWord& operator=(const PinnedWord&) = delete;
    ~PinnedWord() { reset(); }
    hipError_t alloc(unsigned init) {  // the host word alone; map() completes it
        reset();
        const hipError_t e = hipHostMalloc((void**)&h, sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) {
            h = nullptr;
            return e;
        }
        *h = init;
        return hipSuccess;
    }
    hipError_t map() {  // on failure the word is released
        void* p = nullptr;
        const hipError_t e = hipHostGetDevicePointer(&p, h, 0);
        if (e != hipSuccess) reset();
        else d = static_cast<unsigned*>(p);
        return e;
    }
    void reset() {
        if (h) (void)hipHostFree(h);
        h = d = nullptr;
    }
};

// A HIP event, created at its first use.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t ensure(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

// A non-blocking HIP stream.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

// Reusable HIP event pairs, one pair per timed launch; summed once the launches retire.
struct EventPool {
    std::vector<hipEvent_t> start, stop;
    size_t used = 0;
    EventPool() = default;
    EventPool(const EventPool&) = delete;
    EventPool& operator=(const EventPool&) = delete;
    ~EventPool() {
        for (hipEvent_t e : start) (void)hipEventDestroy(e);
        for (hipEvent_t e : stop) (void)hipEventDestroy(e);
    }
    hipError_t next(hipEvent_t* a, hipEvent_t* b) {
        if (used == start.size()) {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            hipError_t e = hipEventCreate(&e0);
            if (e == hipSuccess) e = hipEventCreate(&e1);
            if (e != hipSuccess) return e;
            start.push_back(e0);
            stop.push_back(e1);
        }
        *a = start[used];
        *b = stop[used];
        used++;
        return hipSuccess;
    }
    hipError_t collect(double* ms_sum, size_t* n) {
        *ms_sum = 0.0;
        *n = used;
        if (used == 0) return hipSuccess;
        hipError_t e = hipEventSynchronize(stop[used - 1]);
        for (size_t i = 0; i < used && e == hipSuccess; ++i) {
            float ms = 0.0f;
            e = hipEventElapsedTime(&ms, start[i], stop[i]);
            *ms_sum += ms;
        }
        used = 0;
        return e;
    }
};

}  // namespace pt
