// The normals and values scikit-image's Lewiner marching cubes returns next to its vertices and faces
//     vertices, faces, normals, values = measure.marching_cubes(value_grid, gradient_direction='ascent')
// (reference src/conv_onet/generation.py:270), for the vertices vt_mc_emit numbered: one launch behind vt_mc_count / vt_mc_emit on the
// same volume and workspace, which still holds every cell's triangle list (desc, cnt), owned-edge ranks and first vertex id.
// tests/mc_normals_ref.py restates the rule in float64; DESIGN.md, section "mc_normals / mesh_normals", says what was fitted and how.
//   gradient   per cell, v = vol - level in double: G(k) = the three one-sided differences inside the cell at corner k, low minus high.
//              A corner with y = 1 uses the gradient of the corner mirrored in x (scikit-image indexes its gradient table, kept in
//              Lewiner's corner order, with a binary corner index): G'.
//   edge       every triangle corner of a cell that names the vertex on cell edge (a, b) adds w_a G'(a), then w_b G'(b), with
//              w = 1 / (eps + |v|), the weights of the vertex position.  The count is per triangle corner, not per cell.
//   centre     every triangle corner that names a cell's centre vertex adds w_k (G_z(k), G_y(k), 0) in (x, y, z) for the eight corners k:
//              scikit-image's centre normals carry the z sum in the x slot and nothing along axis 0 (fitted on single cells).
//   normal     the sum, normalised, in array-axis order (z, y, x); (0,0,0) where it is zero or not finite.
//   value      the largest (cell max - cell min) of v, rounded to float, over the cells that reference the vertex.
// One lane per emitted vertex: the owner cells of a 256-cell chunk are compacted, their owned vertices dealt over the workgroup, and each
// lane gathers from the at most four cells around its lattice edge in ascending cell order, adding in double in the order scikit-image
// adds.  No atomics, no dependence on the launch geometry: equal bits from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vt_common.h"
#include "vtaco_hip.h"

namespace {
#define MC_TABLE_QUALIFIER __device__ const
#include "mc_tables.inc"
}  // namespace
#include "mc_common.h"

namespace {

// Lewiner corner at offsets (dx, dy, dz)
__device__ __forceinline__ int corner_at(int dx, int dy, int dz) { return 4 * dz + (dy ? 3 - dx : dx); }

// G(k): (x, y, z) components
__device__ __forceinline__ void gradient(const double v[8], int k, double &gx, double &gy, double &gz) {
    const int dx = cx(k), dy = cy(k), dz = cz(k);
    gx = pick(v, corner_at(0, dy, dz)) - pick(v, corner_at(1, dy, dz));
    gy = pick(v, corner_at(dx, 0, dz)) - pick(v, corner_at(dx, 1, dz));
    gz = pick(v, corner_at(dx, dy, 0)) - pick(v, corner_at(dx, dy, 1));
}

__device__ __forceinline__ int mirrored(int k) { return cy(k) ? corner_at(1 - cx(k), 1, cz(k)) : k; }

struct Acc { double sx, sy, sz; float value; };

// what cell `cc` at (x, y, z) adds to the vertex on its local edge `el` (12: its centre vertex)
__device__ void gather_cell(const float *vol, const McDims &d, const McWs &ws, double level, unsigned cc, int x, int y, int z, int el, Acc &acc) {
    const unsigned nt = ws.cnt[cc] & 0xffu;
    if (nt == 0 || nt > 12) return;
    const unsigned off = ws.desc[cc];
    if (off + 3 * nt > (unsigned)MC_LUT_SIZE) return;           // (a workspace no count wrote: nothing is read past the table)
    int refs = 0;
    for (unsigned i = 0; i < 3 * nt; ++i) refs += (MC_LUT[off + i] == el) ? 1 : 0;
    if (refs == 0) return;
    double v[8];
    load_cell(vol, d, x, y, z, level, v);
    double lo = v[0], hi = v[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) { lo = fmin(lo, v[q]); hi = fmax(hi, v[q]); }
    acc.value = fmaxf(acc.value, (float)(hi - lo));
    if (el == 12) {
        double ty[8], tz[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            double gx, gy, gz;
            gradient(v, q, gx, gy, gz);
            const double w = 1.0 / (MC_EPS + fabs(v[q]));
            ty[q] = w * gy; tz[q] = w * gz;
        }
        for (int r = 0; r < refs; ++r) {
#pragma unroll
            for (int q = 0; q < 8; ++q) { acc.sx += tz[q]; acc.sy += ty[q]; }
        }
        return;
    }
    const int a = (el < 8) ? el : el - 8;                          // E0
    const int b = (el < 8) ? ((el & 4) | ((el + 1) & 3)) : el - 4; // E1
    const double wa = 1.0 / (MC_EPS + fabs(pick(v, a))), wb = 1.0 / (MC_EPS + fabs(pick(v, b)));
    double ax, ay, az, bx, by, bz;
    gradient(v, mirrored(a), ax, ay, az);
    gradient(v, mirrored(b), bx, by, bz);
    ax *= wa; ay *= wa; az *= wa; bx *= wb; by *= wb; bz *= wb;
    for (int r = 0; r < refs; ++r) {
        acc.sx += ax; acc.sy += ay; acc.sz += az;
        acc.sx += bx; acc.sy += by; acc.sz += bz;
    }
}

__global__ void __launch_bounds__(CELLS_PER_BLOCK)
mc_normals_kernel(const float *vol, McDims d, McWs ws, float *normals, float *values, int max_verts) {
    __shared__ int scan[CELLS_PER_BLOCK];
    __shared__ unsigned list[CELLS_PER_BLOCK], lpre[CELLS_PER_BLOCK];
    __shared__ unsigned wave_cnt[4];
    if (ws.bsum[blockIdx.x].y == 0) return;                         // no vertex is owned in this chunk (one scalar load)
    const unsigned c = blockIdx.x * CELLS_PER_BLOCK + threadIdx.x;
    const unsigned cn = (c < d.ncells) ? ws.cnt[c] : 0;
    unsigned nnew = cn >> 8;
    if (nnew > 13) nnew = 0;
    // inclusive scan of the owned-vertex counts over the workgroup
    scan[threadIdx.x] = (int)nnew;
    __syncthreads();
    for (int s = 1; s < CELLS_PER_BLOCK; s <<= 1) {
        const int t = (int)threadIdx.x >= s ? scan[threadIdx.x - s] : 0;
        __syncthreads();
        scan[threadIdx.x] += t;
        __syncthreads();
    }
    const unsigned total = (unsigned)scan[CELLS_PER_BLOCK - 1], pre = (unsigned)scan[threadIdx.x] - nnew;
    // the owner cells, compacted in cell order: (local cell id, first item of the cell)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(nnew != 0);
    if (lane == 0) wave_cnt[w] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned base = 0, nact = 0;
    for (int i = 0; i < 4; ++i) { if (i < w) base += wave_cnt[i]; nact += wave_cnt[i]; }
    if (nnew) {
        const unsigned pos = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        list[pos] = threadIdx.x; lpre[pos] = pre;
    }
    __syncthreads();
    if (nact == 0) return;
    const double level = ws.hdr->level;
    const int c0 = d.n0 - 1;
    for (unsigned item = threadIdx.x; item < total; item += CELLS_PER_BLOCK) {
        unsigned lo = 0, hi = nact;                                  // the owner whose item range holds `item`: last k with lpre[k] <= item
        while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (lpre[mid] <= item) lo = mid; else hi = mid; }
        const unsigned cc = blockIdx.x * CELLS_PER_BLOCK + list[lo], nib = item - lpre[lo] + 1;
        const uint64_t rk = ws.rank[cc];
        int e = -1;
        for (int k = 0; k < 13; ++k) e = (((unsigned)(rk >> (4 * k)) & 15u) == nib) ? k : e;
        const unsigned vid = ws.vbase[cc] + nib - 1;
        if (e < 0 || vid >= (unsigned)max_verts) continue;
        int x, y, z;
        cell_xyz(cc, d, x, y, z);
        Acc acc = {0.0, 0.0, 0.0, 0.0f};
        if (e == 12) {
            gather_cell(vol, d, ws, level, cc, x, y, z, 12, acc);
        } else {
            // the lattice edge: base point and direction (0: x, 1: y, 2: z), as mc.hip's face kernel resolves it
            const int dir = (e >= 8) ? 2 : (e & 1);
            int bx, by, bz;
            if (e >= 8) { const int k = e - 8; bx = (k == 1) | (k == 2); by = (k >> 1) & 1; bz = 0; }
            else { const int k = e & 3; bx = (k == 1); by = (k == 2); bz = e >> 2; }
            const int gx = x + bx, gy = y + by, gz = z + bz;
            // the four cells around it, in ascending cell order: (slow axis - 1, fast axis - 1), (-1, 0), (0, -1), (0, 0)
            for (int i = 0; i < 4; ++i) {
                const int ds = 1 - (i >> 1), df = 1 - (i & 1);           // how far below the edge's base point the cell starts
                int qx = gx, qy = gy, qz = gz, el;
                if (dir == 0) { qz -= ds; qy -= df; el = 2 * df + 4 * ds; }
                else if (dir == 1) { qz -= ds; qx -= df; el = (df ? 1 : 3) + 4 * ds; }
                else { qy -= ds; qx -= df; el = 8 + (ds ? (df ? 2 : 3) : df); }
                if (qx < 0 || qy < 0 || qz < 0 || qx >= d.c2 || qy >= d.c1 || qz >= c0) continue;
                const unsigned qc = ((unsigned)qz * (unsigned)d.c1 + (unsigned)qy) * (unsigned)d.c2 + (unsigned)qx;
                gather_cell(vol, d, ws, level, qc, qx, qy, qz, el, acc);
            }
        }
        const double l2 = (acc.sx * acc.sx + acc.sy * acc.sy) + acc.sz * acc.sz;
        const bool ok = l2 > 0.0 && l2 < __longlong_as_double(0x7ff0000000000000ll);
        const double len = ok ? sqrt(l2) : 1.0;
        float *dst = normals + (size_t)vid * 3;                      // array-axis order (axis0, axis1, axis2) = (z, y, x)
        dst[0] = ok ? (float)(acc.sz / len) : 0.0f;
        dst[1] = ok ? (float)(acc.sy / len) : 0.0f;
        dst[2] = ok ? (float)(acc.sx / len) : 0.0f;
        values[vid] = acc.value;
    }
}

}  // namespace

extern "C" {

int vt_mc_emit_normals(const float *vol, int n0, int n1, int n2, void *workspace, float *normals, float *values, int max_verts, void *stream) {
    if (!vol || !workspace || !normals || !values) return vt_fail(VT_ERR_INVALID, "vt_mc_emit_normals: null argument");
    if (max_verts < 0) return vt_fail(VT_ERR_INVALID, "vt_mc_emit_normals: negative capacity");
    McDims d; size_t off[8], total; unsigned nblk;
    if (!mc_layout(n0, n1, n2, d, off, total, nblk)) return vt_fail(VT_ERR_INVALID, "vt_mc_emit_normals: bad volume shape");
    McWs ws = mc_ws(workspace, off);
    hipLaunchKernelGGL(mc_normals_kernel, dim3(nblk), dim3(CELLS_PER_BLOCK), 0, (hipStream_t)stream, vol, d, ws, normals, values, max_verts);
    return vt_check(hipGetLastError(), "vt_mc_emit_normals");
}

}  // extern "C"
