// The undirected-edge hash table of mesh_topo.hip, mesh_fill.hip, mesh_smooth.hip, mesh_subdivide.hip and mesh_collapse.hip (DESIGN.md, section
// "mesh_edges.h").
// Open addressing over 64-bit keys (lo << 32 | hi), 4 F slots rounded up to a power of two (at most 3 F keys: never full), claimed by
// atomicCAS.  The value counts the faces that run lo -> hi in its low word and hi -> lo in its high word by one 64-bit integer add; the
// halves cannot carry into each other (3 F < 2^32).  In a workspace the table is slots * 16 bytes: the keys, then the values.
// Everything lives in an unnamed namespace, as in mesh_common.h.
#pragma once
#include "mesh_common.h"

namespace {

constexpr u64 EDGE_EMPTY = ~0ull;
constexpr uint32_t NO_SLOT = 0xffffffffu;                           // (slots <= 2^31)

int64_t edge_slots(int64_t F) {
    int64_t cap = 1024;
    while (cap < 4 * F) cap <<= 1;
    return cap;
}

struct EdgeTable {
    u64 *keys, *vals;
    u64 mask;
    int shift;                                                     // slots = 2^(64 - shift)
    int64_t slots;
};

// the table for F faces at p (p may be nullptr where only the sizes are wanted)
EdgeTable edge_table_at(void *p, int64_t F) {
    EdgeTable t;
    t.slots = edge_slots(F);
    t.keys = static_cast<u64 *>(p);
    t.vals = t.keys + t.slots;
    t.mask = (u64)(t.slots - 1);
    t.shift = 64;
    for (int64_t s = t.slots; s > 1; s >>= 1) --t.shift;
    return t;
}

int edge_table_clear(const EdgeTable &t, hipStream_t st) {
    const int rc = vt_fill32(t.keys, 0xffffffffu, (size_t)t.slots * 8, st);
    return rc ? rc : vt_fill32(t.vals, 0u, (size_t)t.slots * 8, st);
}

__device__ inline u64 edge_key(int a, int b) { return a < b ? ((u64)(unsigned)a << 32 | (unsigned)b) : ((u64)(unsigned)b << 32 | (unsigned)a); }
__device__ inline u64 edge_home(const EdgeTable &t, u64 key) { return (key * 0x9E3779B97F4A7C15ull) >> t.shift; }

// the uses of an edge, both directions added
__device__ inline u64 edge_uses(u64 val) { return (val & 0xffffffffull) + (val >> 32); }

// counts one use of a -> b and returns the edge's slot; NO_SLOT for a == b (no edge) and for a full table
__device__ inline uint32_t edge_insert(const EdgeTable &t, int a, int b) {
    if (a == b) return NO_SLOT;
    const u64 key = edge_key(a, b);
    const u64 inc = a < b ? 1ull : (1ull << 32);
    u64 slot = edge_home(t, key);
    for (u64 probes = 0; probes <= t.mask; ++probes) {            // (at most 3 F of the >= 4 F slots are ever claimed: a free one is met)
        const u64 old = atomicCAS(t.keys + slot, EDGE_EMPTY, key);
        if (old == EDGE_EMPTY || old == key) { atomicAdd(t.vals + slot, inc); return (uint32_t)slot; }
        slot = (slot + 1) & t.mask;
    }
    return NO_SLOT;
}

// the uses of {a, b} in a table that is no longer written; 0 for a == b and for a key that is not in the table
__device__ inline u64 edge_uses(const EdgeTable &t, int a, int b) {
    if (a == b) return 0;
    const u64 key = edge_key(a, b);
    u64 slot = edge_home(t, key);
    for (u64 probes = 0; probes <= t.mask; ++probes) {
        const u64 k = t.keys[slot];
        if (k == key) return edge_uses(t.vals[slot]);
        if (k == EDGE_EMPTY) return 0;
        slot = (slot + 1) & t.mask;
    }
    return 0;
}

// the three edges of every face.  A face with an index outside [0, V) takes no part; with REPORT it sets bit 0 of *bad.
template <bool REPORT>
__global__ void __launch_bounds__(MT_THREADS) edge_insert_kernel(const int32_t *faces, int F, int V, EdgeTable t, int32_t *bad) {
    __shared__ int32_t lds[MT_THREADS * 3];
    int f, a, b, c;
    bool ok;
    if (!load_face(faces, F, V, lds, f, a, b, c, ok)) return;
    if (!ok) { if (REPORT) atomicOr(bad, 1); return; }
    edge_insert(t, a, b);
    edge_insert(t, b, c);
    edge_insert(t, c, a);
}

}  // namespace
