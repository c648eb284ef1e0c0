// The device memory of one runner handle (host code).  Every runner allocates all it will ever need while it is created -- packed
// weights, one forward's activations, the backward's gradient streams -- one hipMalloc per buffer, and frees it when the handle goes.
// The handle struct holds a DevArena MEMBER, so `delete handle` frees the device memory on every path: prx_*_destroy, and the
// std::unique_ptr that guards a create which fails half way.  An allocation that fails is an error of the call, never an abort:
// -1, the sticky HIP error cleared (it would otherwise surface at the next PRX_LAUNCH_CHECK), and a message with the figures,
//   "<who>: device allocation of N bytes failed (<hip error>) with M bytes already held by this handle<note>".
#pragma once
#include "common.h"
#include <stdarg.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

class DevArena {
public:
    DevArena() = default;
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    ~DevArena() { for (void* p : ptrs_) (void)hipFree(p); }

    // set once at the start of a create: the name the message begins with, and the runner's own sentence on what it keeps
    void describe(const char* who, const char* note_fmt, ...) __attribute__((format(printf, 3, 4))) {
        who_ = who;
        va_list ap;
        va_start(ap, note_fmt);
        vsnprintf(note_, sizeof(note_), note_fmt, ap);
        va_end(ap);
    }
    int alloc_bytes(void** p, size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            prx_set_error("%s: device allocation of %zu bytes failed (%s) with %zu bytes already held by this handle%s", who_, bytes,
                          hipGetErrorString(e), bytes_, note_);
            return -1;
        }
        ptrs_.push_back(q);
        bytes_ += bytes;
        *p = q;
        return 0;
    }
    // `count` elements; a count of 0 allocates one element, so that every buffer has an address
    template <typename T>
    int alloc(T** p, size_t count) {
        void* q = nullptr;
        if (int r = alloc_bytes(&q, std::max<size_t>(count, 1) * sizeof(T))) return r;
        *p = (T*)q;
        return 0;
    }
    int alloc_op(void** p, size_t count, int f32) { return alloc_bytes(p, std::max<size_t>(count, 1) * op_esz(f32)); }   // operand elements
    // a device copy of `n` floats (a weight the runner keeps in fp32)
    int copy_f32(float** dst, const float* src, size_t n, hipStream_t s) {
        if (int r = alloc(dst, n)) return r;
        PRX_CHECK_HIP(hipMemcpyAsync(*dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    size_t bytes() const { return bytes_; }   // device bytes held

private:
    std::vector<void*> ptrs_;
    size_t bytes_ = 0;
    const char* who_ = "create";
    char note_[256] = "";
};

// DEV_ALLOC(arena, alloc, ptr, count) / DEV_ALLOC(arena, alloc_op, ptr, count, f32): allocate or return the error from the enclosing function
#define DEV_ALLOC(arena, how, ptr, ...) do { if (int _r = (arena).how(&(ptr), __VA_ARGS__)) return _r; } while (0)
