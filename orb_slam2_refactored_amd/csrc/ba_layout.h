// LocalBA's buffer regions (orbba.hip), plain C++ so that a CPU test (tests/native/ba_layout_check.cpp)
// shares them.  Each region is one struct of typed pointers whose carve() lays the fields out from a
// base pointer, in the order written there, and returns the bytes used: the device view, the pinned
// staging view and the byte count of a region all come from that one list.  A null base is a dry run
// for the size: offsets only, every field null.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "carver.h"

namespace orbamd_host {

// (int2 / int4 as the kernels read them: same size, fields at multiples of 256)
struct Int2 {
    int x, y;
};
struct Int4 {
    int x, y, z, w;
};

// What the host provides, built in pinned staging and uploaded with a single copy.
struct UploadLayout {
    uint8_t* fixed;    // P
    int* ep;           // E
    int* ek;           // E
    uint8_t* stereo;   // E
    double* obs;       // E x 3
    double* info;      // E
    double* cam;       // one_cam: 5, else E x 5
    double* q;         // P x 4
    double* t;         // P x 3
    double* X;         // N x 3
    size_t carve(char* base, size_t P, size_t N, size_t E, bool one_cam) {
        Carver c{base};
        c.take(fixed, P); c.take(ep, E); c.take(ek, E); c.take(stereo, E); c.take(obs, 3 * E); c.take(info, E);
        c.take(cam, one_cam ? 5 : 5 * E); c.take(q, 4 * P); c.take(t, 3 * P); c.take(X, 3 * N);
        return c.off;
    }
};

// Device-only per-call state: the push / pop copies and the per-edge flags and errors.
struct StateLayout {
    double* q_sv;      // P x 4
    double* t_sv;      // P x 3
    double* X_sv;      // N x 3
    uint8_t* robust;   // E
    uint8_t* level;    // E
    double* err;       // E x 3
    size_t carve(char* base, size_t P, size_t N, size_t E) {
        Carver c{base};
        c.take(q_sv, 4 * P); c.take(t_sv, 3 * P); c.take(X_sv, 3 * N); c.take(robust, E); c.take(level, E);
        c.take(err, 3 * E);
        return c.off;
    }
};

// What the final gather writes (mapped pinned memory: the kernel's view and the host's).
struct ResultLayout {
    double* q;          // P x 4
    double* t;          // P x 3
    double* X;          // N x 3
    uint8_t* outlier;   // E
    double* chi2;       // E
    size_t carve(char* base, size_t P, size_t N, size_t E) {
        Carver c{base};
        c.take(q, 4 * P); c.take(t, 3 * P); c.take(X, 3 * N); c.take(outlier, E); c.take(chi2, E);
        return c.off;
    }
};

struct StructDims {
    size_t P, N, Ea, np, nl, nblk, nps, npairs;
    bool dev_build;   // the device fills the four lists: the slot table follows
};
// The active structure.  Three nested extents: the host-built arrays (all the device build uploads) end
// at small_bytes, the four lists (the host build uploads them too) at list_bytes; the rest is
// device-only.
struct StructLayout {
    int* hp;         // P
    int* hl;         // N
    int* pt_beg;     // nl + 1
    int* pt_id;      // nl
    int* ps_beg;     // np + 1
    int* ps_id;      // np
    int* blk_i1;     // nblk
    int* blk_i2;     // nblk
    int* blk_beg;    // nblk + 1
    int* blk_diag;   // np
    size_t small_bytes;
    int* act;         // Ea
    int* pt_slot;     // Ea
    int* ps_slot;     // nps
    Int2* blk_pair;   // npairs
    size_t list_bytes;
    Int4* pt_rec;   // Ea
    int* slot;      // dev_build: np x nl (free pose, point) slot table, else null
    size_t carve(char* base, const StructDims& d) {
        Carver c{base};
        c.take(hp, d.P); c.take(hl, d.N); c.take(pt_beg, d.nl + 1); c.take(pt_id, d.nl);
        c.take(ps_beg, d.np + 1); c.take(ps_id, d.np); c.take(blk_i1, d.nblk); c.take(blk_i2, d.nblk);
        c.take(blk_beg, d.nblk + 1); c.take(blk_diag, d.np);
        small_bytes = c.off;
        c.take(act, d.Ea); c.take(pt_slot, d.Ea); c.take(ps_slot, d.nps); c.take(blk_pair, d.npairs);
        list_bytes = c.off;
        c.take(pt_rec, d.Ea);
        slot = nullptr;
        if (d.dev_build) c.take(slot, d.np * d.nl);
        return c.off;
    }
};

struct SystemDims {
    size_t Ea, np, nl, nblk;
    size_t spart_n;   // the Schur-block parts' partials (+ the Hpp part)
    size_t sg_n;      // the global solve's padded working copy, Dp x (Dp + 1); 0: solved in LDS
};
// The linear system of an LM trial (D = 6 np).
struct SystemLayout {
    double* J;            // Ea x 72
    double* W;            // Ea x 24
    double* Hll;          // nl x 9
    double* Dinv;         // nl x 9
    double* bl;           // nl x 3
    double* Hpp;          // np x 36
    double* bp;           // np x 6
    double* S;            // D x D
    double* Spart;        // spart_n
    unsigned* blk_done;   // nblk
    double* bs;           // D
    double* x;            // D + 3 nl
    double* rchi;         // max(Ea, nl)
    double* part;         // nl + np
    double* Sg;           // sg_n, or null
    double* wgpart;       // 2 per point-update workgroup (8 points each)
    size_t carve(char* base, const SystemDims& d) {
        const size_t D = 6 * d.np;
        Carver c{base};
        c.take(J, 72 * d.Ea); c.take(W, 24 * d.Ea); c.take(Hll, 9 * d.nl); c.take(Dinv, 9 * d.nl);
        c.take(bl, 3 * d.nl); c.take(Hpp, 36 * d.np); c.take(bp, 6 * d.np); c.take(S, D * D);
        c.take(Spart, d.spart_n); c.take(blk_done, d.nblk); c.take(bs, D); c.take(x, D + 3 * d.nl);
        c.take(rchi, std::max(d.Ea, d.nl)); c.take(part, d.nl + d.np);
        Sg = nullptr;
        if (d.sg_n) c.take(Sg, d.sg_n);
        c.take(wgpart, 2 * ((d.nl * 8 + 63) / 64));
        return c.off;
    }
};

}  // namespace orbamd_host
