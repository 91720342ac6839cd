// What mc.hip (count, emit) and mc_normals.hip share: the workspace a count leaves behind and an emit completes, the cell geometry and
// the corner loads.  Everything lives in an unnamed namespace: each translation unit has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr double MC_EPS = 2.220446049250313e-16;   // skimage's "FLT_EPSILON" = np.spacing(1.0)
constexpr int CELLS_PER_BLOCK = 256;

struct McHeader {
    unsigned unused0;      // (formerly the atomic min / max keys)
    unsigned unused1;
    int nverts;
    int nfaces;
    double level;
    int reserved[10];
};
static_assert(sizeof(McHeader) == 64, "header is 64 bytes");

struct McDims {
    int n0, n1, n2;        // volume extents (axis 0,1,2); x runs along axis 2
    int c1, c2;            // cells along axis 1 and 2
    unsigned ncells;
};

struct McWs {
    McHeader *hdr;
    uint16_t *cnt;         // ntri | nnew << 8
    uint32_t *desc;        // offset of the cell's triangle list in MC_LUT (active cells only)
    uint64_t *rank;        // 13 nibbles: 1 + rank of owned edge e (0 = not owned / unused)
    uint32_t *vbase;       // first vertex id owned by the cell (active cells only)
    uint2 *bsum;           // per block (tri, vert) sums
    uint2 *boff;           // per block exclusive offsets
};

// corner k -> (dx,dy,dz), Lewiner order
__device__ __forceinline__ int cx(int k) { return (0x66 >> k) & 1; }   // 0,1,1,0,0,1,1,0
__device__ __forceinline__ int cy(int k) { return (0xCC >> k) & 1; }   // 0,0,1,1,0,0,1,1
__device__ __forceinline__ int cz(int k) { return k >> 2; }

__device__ __forceinline__ void load_cell(const float *vol, const McDims &d, int x, int y, int z, double level, double v[8]) {
    const size_t s1 = (size_t)d.n2, s0 = (size_t)d.n1 * d.n2;
    const float *p = vol + (size_t)z * s0 + (size_t)y * s1 + x;
    v[0] = (double)p[0] - level;          v[1] = (double)p[1] - level;
    v[3] = (double)p[s1] - level;         v[2] = (double)p[s1 + 1] - level;
    v[4] = (double)p[s0] - level;         v[5] = (double)p[s0 + 1] - level;
    v[7] = (double)p[s0 + s1] - level;    v[6] = (double)p[s0 + s1 + 1] - level;
}

// select v[k] with a runtime k without sending the array to scratch
__device__ __forceinline__ double pick(const double v[8], int k) {
    double r = v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) r = (k == i) ? v[i] : r;
    return r;
}

__device__ __forceinline__ void cell_xyz(unsigned c, const McDims &d, int &x, int &y, int &z) {
    const unsigned t = c / (unsigned)d.c2;
    x = (int)(c - t * (unsigned)d.c2);
    z = (int)(t / (unsigned)d.c1);
    y = (int)(t - (unsigned)z * (unsigned)d.c1);
}

__host__ size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

__host__ bool mc_layout(int n0, int n1, int n2, McDims &d, size_t off[8], size_t &total, unsigned &nblk) {
    if (n0 < 2 || n1 < 2 || n2 < 2) return false;
    const uint64_t nc = (uint64_t)(n0 - 1) * (n1 - 1) * (n2 - 1);
    if (nc >= (1ull << 31)) return false;
    d.n0 = n0; d.n1 = n1; d.n2 = n2; d.c1 = n1 - 1; d.c2 = n2 - 1; d.ncells = (unsigned)nc;
    nblk = (unsigned)((nc + CELLS_PER_BLOCK - 1) / CELLS_PER_BLOCK);
    size_t p = 0;
    off[0] = p; p = align_up(p + sizeof(McHeader), 256);
    off[1] = p; p = align_up(p + nc * sizeof(uint16_t), 256);
    off[2] = p; p = align_up(p + nc * sizeof(uint32_t), 256);
    off[3] = p; p = align_up(p + nc * sizeof(uint64_t), 256);
    off[4] = p; p = align_up(p + nc * sizeof(uint32_t), 256);
    off[5] = p; p = align_up(p + (size_t)nblk * sizeof(uint2), 256);
    off[6] = p; p = align_up(p + (size_t)nblk * sizeof(uint2), 256);
    total = p;
    return true;
}

__host__ McWs mc_ws(void *base, const size_t off[8]) {
    char *b = (char *)base;
    McWs w;
    w.hdr = (McHeader *)(b + off[0]); w.cnt = (uint16_t *)(b + off[1]); w.desc = (uint32_t *)(b + off[2]);
    w.rank = (uint64_t *)(b + off[3]); w.vbase = (uint32_t *)(b + off[4]);
    w.bsum = (uint2 *)(b + off[5]); w.boff = (uint2 *)(b + off[6]);
    return w;
}

}  // namespace
