// The host arrays of one call mirrored in one device slab: the plan behind every host entry that takes host pointers
// (common.h's run_host does the copies with hipMemcpy).  Plain C++, so that the CPU tests under tests/native share it.
#pragma once
#include <cstddef>
#include <vector>

#include "carver.h"

namespace orbamd_host {

// add() records a pointer field of the caller's copy of the argument struct; upload() lays the fields out with Carver
// (256-byte steps), copies the `in` ones and points every field at its device address; download() copies the `out`
// ones back.  A null field is skipped and stays null.  A field of count 0 has an address of its own and is never
// copied.  Two fields that name one host array are two device arrays (a call that reads one and writes the other keeps
// doing so) unless the second is added with share: then it takes the first one's address and its one copy each way.
struct Mirror {
    using Copy = int (*)(void* dst, const void* src, size_t bytes);   // 0, or the error code upload/download return
    Copy to_device, to_host;
    Mirror(Copy to_device, Copy to_host) : to_device(to_device), to_host(to_host) {}

    template <class T>
    void add(T*& field, size_t count, bool in, bool out, bool share = false) {
        if (!field) return;
        const size_t bytes = count * sizeof(T);
        int first = -1;
        for (size_t i = 0; share && i < items.size() && first < 0; i++)
            if (items[i].host == (const void*)field && items[i].alias < 0) first = (int)i;
        if (first >= 0) {
            Item& f = items[first];
            f.bytes = bytes > f.bytes ? bytes : f.bytes;
            f.in |= in;
            f.out |= out;
        }
        items.push_back(Item{&field, (const void*)field, bytes, in, out, first, nullptr,
                             [](void* f, char* dev) { *static_cast<T**>(f) = reinterpret_cast<T*>(dev); }});
    }

    size_t bytes() const {
        Carver c{nullptr};
        char* p;
        for (const Item& i : items)
            if (i.alias < 0) c.take(p, i.bytes);
        return c.off;
    }

    // Slab: int reserve(size_t) (0 on success) and as<char>(), as orbamd::DevBuf
    template <class Slab>
    int upload(Slab& slab) {
        if (int rc = slab.reserve(bytes())) return rc;
        Carver c{slab.template as<char>()};
        for (Item& i : items) {
            if (i.alias >= 0) continue;
            c.take(i.dev, i.bytes);
            if (i.in && i.bytes)
                if (int rc = to_device(i.dev, i.host, i.bytes)) return rc;
        }
        for (Item& i : items) i.bind(i.field, i.alias < 0 ? i.dev : items[i.alias].dev);
        return 0;
    }

    int download() {
        for (Item& i : items)
            if (i.alias < 0 && i.out && i.bytes)
                if (int rc = to_host(const_cast<void*>(i.host), i.dev, i.bytes)) return rc;
        return 0;
    }

    struct Item {
        void* field;        // the T*& given to add()
        const void* host;
        size_t bytes;
        bool in, out;
        int alias;          // the earlier item with the same host array, or -1
        char* dev;
        void (*bind)(void* field, char* dev);
    };
    std::vector<Item> items;
};

}  // namespace orbamd_host
