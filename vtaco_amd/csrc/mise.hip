// Multiresolution isosurface extraction (MISE, Occupancy Networks): the device half of one refinement step.  The reference keeps
// the algorithm as numpy code nothing calls (src/utils/mesh.py:7-84 MultiGridExtractor, src/utils/voxels.py:222-257
// check_voxel_boundary); vtaco_amd/mise.py drives these passes and decodes the compacted query points through the point path.
//
// Level k-1 holds nc = r0 * 2^(k-1) + 1 values per axis, level k nf = 2 nc - 1.  One step:
//   classify  coarse voxel active  <=>  its 8 corners do not all fall on the same side of `level`, side = (double)v - level > 0:
//             marching cubes' own predicate (mc.hip load_cell + the cube index), so a voxel judged inactive here can never emit
//             a triangle there.  (The reference's rule is values < threshold; the two differ only where a value equals the level.)
//   refine    every fine point takes coarse (x>>1, y>>1, z>>1) (upsample3d_nn(...)[:-1,:-1,:-1]); fine point (2i,2j,2l) is known
//             when coarse (i,j,l) was (value_known[::2,::2,::2] = value_known), every other one is not.  An unknown fine point
//             becomes a query point when it is a corner of a fine voxel whose parent coarse voxel is active.  Query points are compacted (64-bit ballot, one atomicAdd per wave on a device word) into a list of
//             lattice ids (int32) and coordinates (lattice_point's arithmetic at nf: coarse point i and fine point 2i coincide bit
//             for bit, since the step at nf is the coarse step halved exactly).  The list order varies from run to run; its set does not.
//   scatter   the decoded logits of the list into the fine grid at their ids.
// Every pass is a grid-stride walk over 256-element chunks (4 consecutive elements per lane, 16-byte stores where aligned).
#include "decode_common.h"

namespace {

constexpr int MISE_THREADS = 256;
constexpr int MISE_PER_LANE = 4;
constexpr int MISE_CHUNK = 64 * MISE_PER_LANE;                     // elements per wave and chunk

__device__ __forceinline__ bool mise_side(float v, double level) { return (double)v - level > 0.0; }

__device__ __forceinline__ DecodeArgs mise_lattice(int n, float box) {
    DecodeArgs d;
    d.grid = nullptr; d.pts = nullptr; d.c_img = nullptr; d.blob = nullptr; d.out = nullptr; d.out2 = nullptr; d.save = nullptr;
    d.c_direct = nullptr; d.cimg_ids = nullptr; d.cimg_table = nullptr; d.cimg_nf = 0; d.brick = 0; d.N = 0; d.total = 0;
    d.lattice_first = 0; d.R = 2; d.nx = n; d.box = box; d.divisor = 1.0f; d.status = nullptr; d.clk = nullptr; d.claim = 0;
    return d;
}

// active[v] = 1 for the coarse voxels (nc-1)^3 the surface at `level` crosses
__global__ void __launch_bounds__(MISE_THREADS) mise_classify_kernel(const float *__restrict__ coarse, int nc, double level,
                                                                       unsigned char *__restrict__ active) {
    const uint32_t m = (uint32_t)(nc - 1), total = m * m * m;
    const size_t s1 = (size_t)nc, s0 = (size_t)nc * nc;
    for (uint32_t base = (blockIdx.x * MISE_THREADS + threadIdx.x) * MISE_PER_LANE; base < total;
         base += gridDim.x * MISE_THREADS * MISE_PER_LANE) {
        unsigned char r[MISE_PER_LANE];
#pragma unroll
        for (int j = 0; j < MISE_PER_LANE; ++j) {
            const uint32_t v = base + j;
            r[j] = 0;
            if (v < total) {
                const uint32_t t = v / m, z = v - t * m, x = t / m, y = t - x * m;
                const float *p = coarse + x * s0 + y * s1 + z;
                const bool s = mise_side(p[0], level);
                const bool mixed = (mise_side(p[1], level) != s) | (mise_side(p[s1], level) != s) | (mise_side(p[s1 + 1], level) != s) |
                                   (mise_side(p[s0], level) != s) | (mise_side(p[s0 + 1], level) != s) |
                                   (mise_side(p[s0 + s1], level) != s) | (mise_side(p[s0 + s1 + 1], level) != s);
                r[j] = mixed ? 1 : 0;
            }
        }
        if (base + MISE_PER_LANE <= total && (base & 3) == 0) {
            *reinterpret_cast<uchar4 *>(active + base) = make_uchar4(r[0], r[1], r[2], r[3]);
        } else {
            for (int j = 0; j < MISE_PER_LANE; ++j)
                if (base + j < total) active[base + j] = r[j];
        }
    }
}

// parents of fine coordinate c along one axis: odd c -> {c>>1}; even c -> {c/2-1, c/2}, clipped to [0, nc-2]
__device__ __forceinline__ void mise_parents(uint32_t c, uint32_t nc, int &lo, int &hi) {
    const int h = (int)(c >> 1);
    if (c & 1u) { lo = h; hi = h; }
    else { lo = h > 0 ? h - 1 : 0; hi = h < (int)nc - 2 ? h : (int)nc - 2; }
}

struct RefineArgs {
    const float *coarse;          // [nc]^3
    const unsigned char *coarse_known;   // [nc]^3, or null: every coarse point known
    const unsigned char *active;  // [nc-1]^3
    float *fine;                  // [nf]^3
    unsigned char *known;         // [nf]^3 or null
    int *qids;                    // [capacity]
    float *qpts;                  // [capacity][3]
    int *count;                   // device word: query points found (may exceed capacity; only the first `capacity` are written)
    uint32_t nc, nf;
    uint32_t capacity;
    float box;
};

__global__ void __launch_bounds__(MISE_THREADS) mise_refine_kernel(RefineArgs a) {
    const uint32_t nf = a.nf, nc = a.nc, total = nf * nf * nf;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (MISE_THREADS / 64);
    const DecodeArgs lat = mise_lattice((int)nf, a.box);
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t mc = nc - 1;
    // the chunk index is uniform over the wave: every lane takes part in every ballot
    for (uint32_t chunk = blockIdx.x * (MISE_THREADS / 64) + (threadIdx.x >> 6); chunk * (uint32_t)MISE_CHUNK < total; chunk += waves) {
        const uint32_t base = chunk * MISE_CHUNK + lane * MISE_PER_LANE;
        float val[MISE_PER_LANE];
        unsigned char kn[MISE_PER_LANE];
        unsigned q = 0;                                             // bit j: element base+j is a query point
        // (x, y, z) of base once; the next elements step z with a carry (one division pair per lane and chunk)
        const uint32_t t0 = base / nf;
        const uint32_t z0 = base - t0 * nf, x0 = t0 / nf, y0 = t0 - x0 * nf;
        uint32_t x = x0, y = y0, z = z0;
#pragma unroll
        for (int j = 0; j < MISE_PER_LANE; ++j) {
            val[j] = 0.0f; kn[j] = 0;
            if (base + j < total) {
                const size_t ci = ((size_t)(x >> 1) * nc + (y >> 1)) * nc + (z >> 1);
                val[j] = a.coarse[ci];
                if (((x | y | z) & 1u) == 0) kn[j] = a.coarse_known ? a.coarse_known[ci] : 1;
                if (!kn[j]) {
                    int xl, xh, yl, yh, zl, zh;
                    mise_parents(x, nc, xl, xh); mise_parents(y, nc, yl, yh); mise_parents(z, nc, zl, zh);
                    // the (up to 8) parent voxels, without loops: a repeated parent is read twice and OR-ed in again
                    const unsigned char *r0 = a.active + ((size_t)xl * mc + yl) * mc, *r1 = a.active + ((size_t)xl * mc + yh) * mc;
                    const unsigned char *r2 = a.active + ((size_t)xh * mc + yl) * mc, *r3 = a.active + ((size_t)xh * mc + yh) * mc;
                    const unsigned hit = r0[zl] | r0[zh] | r1[zl] | r1[zh] | r2[zl] | r2[zh] | r3[zl] | r3[zh];
                    q |= (hit ? 1u : 0u) << j;
                }
            }
            if (++z == nf) { z = 0; if (++y == nf) { y = 0; ++x; } }
        }
        // this lane's query count (0..4) as three bit planes: the wave's exclusive prefix and total from three ballots
        const unsigned cnt = __popc(q);
        unsigned before = 0, sum = 0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const unsigned long long plane = __ballot((cnt >> b) & 1u);
            before += (unsigned)__popcll(plane & below) << b;
            sum += (unsigned)__popcll(plane) << b;
        }
        uint32_t slot0 = 0;
        if (sum) {
            int wbase = 0;
            if (lane == 0) wbase = atomicAdd(a.count, (int)sum);
            slot0 = (uint32_t)__shfl(wbase, 0) + before;
        }
        uint32_t slot = slot0;
        x = x0; y = y0; z = z0;
#pragma unroll
        for (int j = 0; j < MISE_PER_LANE; ++j) {
            if (((q >> j) & 1u) && slot < a.capacity) {            // past the capacity: counted, not written (the host sizes up, runs again)
                float px, py, pz;
                lattice_point(lat, x, y, z, px, py, pz);
                a.qids[slot] = (int)(base + j);
                float *o = a.qpts + (size_t)slot * 3;
                o[0] = px; o[1] = py; o[2] = pz;
            }
            slot += (q >> j) & 1u;
            if (++z == nf) { z = 0; if (++y == nf) { y = 0; ++x; } }
        }
        if (base + MISE_PER_LANE <= total) {                        // base is a multiple of 4: 16-byte / 4-byte aligned rows
            *reinterpret_cast<f32x4 *>(a.fine + base) = f32x4{val[0], val[1], val[2], val[3]};
            if (a.known) *reinterpret_cast<uchar4 *>(a.known + base) = make_uchar4(kn[0], kn[1], kn[2], kn[3]);
        } else {
            for (int j = 0; j < MISE_PER_LANE; ++j)
                if (base + j < total) {
                    a.fine[base + j] = val[j];
                    if (a.known) a.known[base + j] = kn[j];
                }
        }
    }
}

__global__ void __launch_bounds__(MISE_THREADS) mise_scatter_kernel(const int *__restrict__ ids, const float *__restrict__ vals,
                                                                      uint32_t m, float *__restrict__ fine, uint32_t total,
                                                                      unsigned char *__restrict__ known) {
    for (uint32_t i = blockIdx.x * MISE_THREADS + threadIdx.x; i < m; i += gridDim.x * MISE_THREADS) {
        const int g = ids[i];
        if (g < 0 || (uint32_t)g >= total) continue;               // never past the grid, whatever the list holds
        fine[g] = vals[i];
        if (known) known[g] = 1;
    }
}

// the whole n^3 lattice as a query list: ids 0..n^3-1 and their coordinates (level 0)
__global__ void __launch_bounds__(MISE_THREADS) mise_lattice_kernel(uint32_t n, float box, int *__restrict__ ids, float *__restrict__ pts) {
    const uint32_t total = n * n * n;
    const DecodeArgs lat = mise_lattice((int)n, box);
    for (uint32_t g = blockIdx.x * MISE_THREADS + threadIdx.x; g < total; g += gridDim.x * MISE_THREADS) {
        const uint32_t t = g / n, z = g - t * n, x = t / n, y = t - x * n;
        float px, py, pz;
        lattice_point(lat, x, y, z, px, py, pz);
        if (ids) ids[g] = (int)g;
        float *o = pts + (size_t)g * 3;
        o[0] = px; o[1] = py; o[2] = pz;
    }
}

unsigned mise_blocks(uint64_t elems, uint64_t per_block) {
    uint64_t g = (elems + per_block - 1) / per_block;
    const uint64_t cap = (uint64_t)vt_num_cus() * 8;
    if (g > cap) g = cap;
    return (unsigned)(g ? g : 1);
}

bool mise_size_ok(int64_t n) { return n >= 2 && n <= VT_MISE_MAX_N; }

}  // namespace

extern "C" int vt_mise_lattice(int n, float box, int *ids, float *pts, void *stream) {
    if (!pts) return vt_fail(VT_ERR_INVALID, "vt_mise_lattice: null argument");
    if (!mise_size_ok(n)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_mise_lattice: n must be in [2, VT_MISE_MAX_N]");
    const uint64_t total = (uint64_t)n * n * n;
    hipLaunchKernelGGL(mise_lattice_kernel, dim3(mise_blocks(total, MISE_THREADS)), dim3(MISE_THREADS), 0, (hipStream_t)stream,
                       (uint32_t)n, box, ids, pts);
    return vt_check(hipGetLastError(), "vt_mise_lattice");
}

extern "C" int vt_mise_refine(const float *coarse, const unsigned char *coarse_known, int nc, double level, float box, unsigned char *active, float *fine,
                              unsigned char *known, int *qids, float *qpts, int64_t capacity, int *count, void *stream) {
    if (!coarse || !active || !fine || !qids || !qpts || !count) return vt_fail(VT_ERR_INVALID, "vt_mise_refine: null argument");
    const int64_t nf = 2 * (int64_t)nc - 1;
    if (nc < 2 || !mise_size_ok(nf)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_mise_refine: 2 nc - 1 must be in [3, VT_MISE_MAX_N]");
    if (capacity < 0 || capacity >= ((int64_t)1 << 31)) return vt_fail(VT_ERR_INVALID, "vt_mise_refine: capacity must be in [0, 2^31)");
    hipStream_t st = (hipStream_t)stream;
    int rc = vt_fill32(count, 0u, sizeof(int), st);
    if (rc) return rc;
    const uint64_t voxels = (uint64_t)(nc - 1) * (nc - 1) * (nc - 1);
    hipLaunchKernelGGL(mise_classify_kernel, dim3(mise_blocks(voxels, MISE_THREADS * MISE_PER_LANE)), dim3(MISE_THREADS), 0, st,
                       coarse, nc, level, active);
    rc = vt_check(hipGetLastError(), "vt_mise_refine: classify");
    if (rc) return rc;
    RefineArgs a;
    a.coarse = coarse; a.coarse_known = coarse_known; a.active = active; a.fine = fine; a.known = known; a.qids = qids; a.qpts = qpts; a.count = count;
    a.nc = (uint32_t)nc; a.nf = (uint32_t)nf; a.capacity = (uint32_t)capacity; a.box = box;
    const uint64_t total = (uint64_t)nf * nf * nf;
    hipLaunchKernelGGL(mise_refine_kernel, dim3(mise_blocks(total, MISE_THREADS * MISE_PER_LANE)), dim3(MISE_THREADS), 0, st, a);
    return vt_check(hipGetLastError(), "vt_mise_refine");
}

extern "C" int vt_mise_scatter(const int *ids, const float *vals, int64_t m, float *fine, int64_t total, unsigned char *known,
                               void *stream) {
    if (m == 0) return 0;
    if (!ids || !vals || !fine) return vt_fail(VT_ERR_INVALID, "vt_mise_scatter: null argument");
    if (m < 0 || total <= 0 || total > (int64_t)VT_MISE_MAX_N * VT_MISE_MAX_N * VT_MISE_MAX_N || m > total)
        return vt_fail(VT_ERR_INVALID, "vt_mise_scatter: bad size");
    hipLaunchKernelGGL(mise_scatter_kernel, dim3(mise_blocks((uint64_t)m, MISE_THREADS)), dim3(MISE_THREADS), 0, (hipStream_t)stream,
                       ids, vals, (uint32_t)m, fine, (uint32_t)total, known);
    return vt_check(hipGetLastError(), "vt_mise_scatter");
}
