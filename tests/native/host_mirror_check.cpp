// csrc/host_mirror.h on the CPU: the "device" is a heap slab, the copier memcpy with a counter per direction.
// Built with AddressSanitizer by tests/test_host_mirror_native.py: a zero-count field is a zero-length heap block, so a
// single byte read from it is a reported error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_mirror.h"

using orbamd_host::Mirror;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static int n_to_device = 0, n_to_host = 0;
static size_t bytes_to_device = 0, bytes_to_host = 0;
static int to_device(void* dst, const void* src, size_t bytes) {
    n_to_device++;
    bytes_to_device += bytes;
    std::memcpy(dst, src, bytes);
    return 0;
}
static int to_host(void* dst, const void* src, size_t bytes) {
    n_to_host++;
    bytes_to_host += bytes;
    std::memcpy(dst, src, bytes);
    return 0;
}
static void reset_counts() { n_to_device = n_to_host = 0; bytes_to_device = bytes_to_host = 0; }

struct Slab {   // what orbamd::DevBuf offers
    char* ptr = nullptr;
    size_t bytes = 0;
    int reserves = 0;
    int reserve(size_t need) {
        reserves++;
        std::free(ptr);
        ptr = nullptr;
        // 256-byte aligned like hipMalloc; 0xEE marks what upload did not write
        if (posix_memalign(reinterpret_cast<void**>(&ptr), 256, need ? need : 1)) return 3;
        std::memset(ptr, 0xEE, need);
        bytes = need;
        return 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(ptr); }
    ~Slab() { std::free(ptr); }
};

struct P3 { float x, y, z; };   // a 12-byte element
static_assert(sizeof(P3) == 12, "P3");

template <class T>
static T* heap(size_t n, int seed) {   // n == 0: a zero-length block
    T* p = static_cast<T*>(std::malloc(n * sizeof(T)));
    for (size_t i = 0; i < n * sizeof(T); i++) reinterpret_cast<unsigned char*>(p)[i] = (unsigned char)(seed + 7 * i);
    return p;
}

static bool inside(const Slab& s, const void* p, size_t bytes) {
    const char* c = static_cast<const char*>(p);
    return c >= s.ptr && c + bytes <= s.ptr + s.bytes && (reinterpret_cast<uintptr_t>(p) & 255) == 0;
}

// One struct with an input, an output, an in-out and a null field of n elements of T each.
template <class T>
static void directions(size_t n) {
    struct Args { const T* in; T* out; T* inout; const T* absent; T* absent_out; } host{}, d{};
    T* in = heap<T>(n, 1);
    host.in = in; host.out = heap<T>(n, 2); host.inout = heap<T>(n, 3);
    std::vector<unsigned char> in_before(n * sizeof(T) + 1);
    std::memcpy(in_before.data(), in, n * sizeof(T));
    d = host;
    reset_counts();
    Slab slab;
    Mirror m(to_device, to_host);
    m.add(d.in, n, true, false);            // const T*&
    m.add(d.absent, n, true, false);
    m.add(d.out, n, false, true);           // T*&
    m.add(d.absent_out, n, true, true);
    m.add(d.inout, n, true, true);
    CHECK(m.upload(slab) == 0);
    CHECK(slab.reserves == 1);
    const size_t step = (std::max<size_t>(n, 1) * sizeof(T) + 255) / 256 * 256;
    CHECK(slab.bytes == 3 * step);          // the null fields take no room
    CHECK(d.absent == nullptr && d.absent_out == nullptr);
    CHECK(inside(slab, d.in, n * sizeof(T)) && inside(slab, d.out, n * sizeof(T)) && inside(slab, d.inout, n * sizeof(T)));
    CHECK((const void*)d.in != (const void*)d.out && (const void*)d.out != (const void*)d.inout &&
          (const void*)d.in != (const void*)d.inout);
    CHECK(n_to_device == (n ? 2 : 0) && bytes_to_device == 2 * n * sizeof(T) && n_to_host == 0);
    CHECK(std::memcmp(d.in, host.in, n * sizeof(T)) == 0 && std::memcmp(d.inout, host.inout, n * sizeof(T)) == 0);
    for (size_t i = 0; i < n * sizeof(T); i++) CHECK(reinterpret_cast<unsigned char*>(d.out)[i] == 0xEE);   // not uploaded
    // the "device call": writes all three device arrays
    for (size_t i = 0; i < n * sizeof(T); i++) {
        reinterpret_cast<unsigned char*>(const_cast<T*>(d.in))[i] = 0x11;
        reinterpret_cast<unsigned char*>(d.out)[i] = 0x22;
        reinterpret_cast<unsigned char*>(d.inout)[i] = 0x33;
    }
    CHECK(m.download() == 0);
    CHECK(n_to_device == (n ? 2 : 0) && n_to_host == (n ? 2 : 0) && bytes_to_host == 2 * n * sizeof(T));
    CHECK(std::memcmp(in, in_before.data(), n * sizeof(T)) == 0);   // an input is not copied back
    for (size_t i = 0; i < n * sizeof(T); i++) {
        CHECK(reinterpret_cast<unsigned char*>(host.out)[i] == 0x22);
        CHECK(reinterpret_cast<unsigned char*>(host.inout)[i] == 0x33);
    }
    std::free(in); std::free(host.out); std::free(host.inout);
}

// A zero-count field between two others: an address of its own, nothing read or written.
static void zero_count_between_neighbours() {
    int32_t *a = heap<int32_t>(65, 1), *z = heap<int32_t>(0, 2), *b = heap<int32_t>(63, 3);
    int32_t *da = a, *dz = z, *db = b;
    reset_counts();
    Slab slab;
    Mirror m(to_device, to_host);
    m.add(da, 65, true, true); m.add(dz, 0, true, true); m.add(db, 63, true, true);
    CHECK(m.upload(slab) == 0);
    CHECK(inside(slab, dz, 0) && dz != da && dz != db && (char*)dz >= (char*)da + 65 * 4 && (char*)db >= (char*)dz + 256);
    CHECK(slab.bytes == 512 + 256 + 256);
    CHECK(m.download() == 0);
    CHECK(n_to_device == 2 && n_to_host == 2 && bytes_to_device == (65 + 63) * 4 && bytes_to_host == (65 + 63) * 4);
    std::free(a); std::free(z); std::free(b);
}

// Two fields naming one host array: shared on request (one address, one copy each way), else two arrays.
static void one_host_array_twice() {
    for (int share = 0; share < 2; share++) {
        uint8_t* flags = heap<uint8_t>(65, 5);
        uint8_t *d1 = flags, *d2 = flags;
        const uint8_t* d3 = flags;
        reset_counts();
        Slab slab;
        Mirror m(to_device, to_host);
        m.add(d1, 65, true, true);
        m.add(d2, 65, true, true, share != 0);
        m.add(d3, 65, true, false, share != 0);
        CHECK(m.upload(slab) == 0);
        if (share) {
            CHECK(d1 == d2 && d3 == d1 && slab.bytes == 256 && n_to_device == 1);
            d2[64] = 0x5A;
            CHECK(m.download() == 0);
            CHECK(n_to_host == 1 && flags[64] == 0x5A);
        } else {
            CHECK(d1 != d2 && d3 != d1 && d3 != d2 && slab.bytes == 3 * 256 && n_to_device == 3);
            CHECK(m.download() == 0);
            CHECK(n_to_host == 2);
        }
        std::free(flags);
    }
}

// A copier's error code comes back from upload / download.
static void a_failed_copy_is_reported() {
    float* a = heap<float>(4, 1);
    float* d = a;
    Slab slab;
    Mirror up([](void*, const void*, size_t) { return 7; }, to_host);
    up.add(d, 4, true, true);
    CHECK(up.upload(slab) == 7);
    d = a;
    Mirror down(to_device, [](void*, const void*, size_t) { return 9; });
    down.add(d, 4, true, true);
    CHECK(down.upload(slab) == 0 && down.download() == 9);
    std::free(a);
}

int main() {
    for (size_t n : {size_t(0), size_t(1), size_t(63), size_t(65)}) {
        directions<uint8_t>(n);
        directions<int32_t>(n);
        directions<P3>(n);
    }
    zero_count_between_neighbours();
    one_host_array_twice();
    a_failed_copy_is_reported();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
