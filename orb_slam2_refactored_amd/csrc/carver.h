// The cursor behind every buffer layout of the library (ba_layout.h, orbp_layout.h): plain C++, so that
// the CPU tests under tests/native share it.
#pragma once
#include <algorithm>
#include <cstddef>

namespace orbamd_host {

// A field takes max(n, 1) elements rounded up to 256 bytes (ba_fill_kernel needs 16-byte aligned segments).
// A null base is a dry run for the size: offsets only, every field null.
struct Carver {
    char* base;
    size_t off = 0;
    template <class T>
    void take(T*& p, size_t n) {
        p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (std::max<size_t>(n, 1) * sizeof(T) + 255) / 256 * 256;
    }
};

}  // namespace orbamd_host
