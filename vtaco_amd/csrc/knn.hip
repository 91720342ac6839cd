// The k nearest points of a point set, and what a point cloud wants from them: the reference's get_nearest_neighbors_indices_batch
// (src/common.py:158-175, pykdtree's query(k)) and the normals its visualize_pointcloud draws (src/utils/visualize.py:51).  The definitions
// are DESIGN.md's section "knn.hip", restated in numpy by tests/knn_ref.py: this file's operations in this file's order.  Every number is
// float64; every product, sum, division and square root is a separate IEEE rounding in a fixed order (-ffp-contract=off).  No atomic, no
// sort whose order depends on timing: the outputs are bit-reproducible.  B problems with one N, one M and one k per call.
//   result    per query the k targets smallest in the order (d2, index), ascending, as d2 [B][N][k] f64 and idx [B][N][k] i32;
//             d2 = (dx dx + dy dy) + dz dz with d = q - p (icp.hip's, point_tree.hip's).  T [B][16] or NULL moves the queries first
//   list      starts as k entries (+inf, -1).  A target (d, m) is taken when d < worst || (d == worst && m < worst_m), (worst, worst_m) the
//             list's last entry, and is put in front of the first entry it is smaller than in the order (d2, index); the last entry
//             drops out.  The list is therefore the k smallest of the targets seen so far whatever the order they were seen in.  With
//             M < k the tail stays (+inf, -1); a NaN or infinite query takes nothing and returns all (+inf, -1)
//   storage   the list lives in LDS as [slot][lane] (doubles, then int32): a wave's lanes touch consecutive addresses whatever slot each
//             is at, and no per-lane array is indexed at run time, so nothing goes to scratch.  worst and worst_m are kept in registers:
//             a target that is not taken costs no LDS access.  Dynamic LDS: threads * k * 12 bytes
//   brute     vt_nn_points' shape: 256 queries per workgroup and one slab of targets, staged through LDS in chunks of 256 points read by
//             broadcast; one partial list per (query, slab) goes to the workspace as [slab][slot][query]; a finish pass (64 lanes per
//             workgroup) merges the lists in ascending slab order by the same rule, leaving a list at its first entry that is not
//             taken.  The result does not depend on the slab size
//   tree      octree_common.h's walk over a PointTree (point_tree.hip), 64 lanes per workgroup: a cell is skipped exactly when
//             lb > worst, lb = ot_box_d2, the box's lower bound in d2's operation order.  worst is +inf until the list holds k targets.  The
//             computed lb is <= the computed d2 of every point under the cell (monotone rounding, as in point_tree.hip), so a skipped
//             cell holds no point with d2 <= worst: none that would be taken, and none that ties with worst at a lower index.  No slack.
//             Seed leaf, near children first (VTACO_POINT_TREE_WALK), the lane permutation and stats [B][N][2] are point_tree.hip's
//   normals   one lane per query, everything in registers with static indices.  r = the first valid neighbour (idx >= 0), e_j = p_j - r
//             for the valid neighbours in ascending slot order; ebar = (sum e_j from +0.0) / count; f_j = e_j - ebar; the six sums
//             f_a f_b from +0.0 in the same order, each divided by count: C.  (Taking the differences from r first makes coincident
//             neighbours an exactly zero C.)  Cyclic Jacobi on C with V = I, KNN_SWEEPS sweeps over the pairs (0,1), (0,2), (1,2): a_pq == 0
//             skips; zeta = (a_qq - a_pp) / (2 a_pq), t = 1 / (|zeta| + sqrt(1 + zeta zeta)), negated for zeta < 0, c = 1 / sqrt(1 + t t),
//             s = c t (icp.hip's formula); a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0; a_rp, a_rq <- c a_rp - s a_rq, s a_rp + c a_rq for
//             the third index r; the same on V's columns p, q.  Diagonal and columns sorted ascending (swaps (0,1), (1,2), (0,1) on a
//             strict >).  normal = v_0 / sqrt(|v_0|^2); with a view point negated when n . (view - p_idx[0]) < 0, else so that its
//             component of largest magnitude (the lowest axis among equals) is positive.  Fewer than 3 valid neighbours or C == 0
//             exactly: normal and eigenvalues are +0.0.  Never NaN for finite points
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_common.h"
#include "mesh_common.h"
#include "octree_common.h"
#include "vt_common.h"
#include "vtaco_hip.h"

extern __shared__ __attribute__((aligned(16))) double knn_lds[];          // the lists: d [k][threads] doubles, then m [k][threads] int32

namespace {

constexpr int KNN_THREADS = 256;                // brute force: queries per workgroup and points per LDS chunk
constexpr int KNN_LANES = 64;                   // the walk and the finish pass: lanes per workgroup (one wave; 24 KB of lists at k = 32)
constexpr int KNN_MIN_CHUNKS = 2;               // chunks per slab at least (vt_nn_points')
constexpr int KNN_TARGET_BLOCKS = 2048;         // workgroups wanted per launch: 8 per CU
constexpr int KNN_SWEEPS = 8;                   // Jacobi sweeps (a symmetric 3x3 settles in 4 to 6)
constexpr int64_t KNN_MAX = 0x7fffff00;

// one lane's list among TH lanes' in LDS: d [k][TH] doubles, then m [k][TH] int32
template <int TH>
struct KList {
    double *d;
    int32_t *m;
    int k;
    double worst;
    int worst_m;
    __device__ KList(int k_, int lane) : k(k_), worst(__builtin_inf()), worst_m(-1) {
        d = knn_lds + lane;
        m = reinterpret_cast<int32_t *>(knn_lds + (size_t)TH * k_) + lane;
        for (int j = 0; j < k; ++j) { d[j * TH] = __builtin_inf(); m[j * TH] = -1; }
    }
    __device__ bool takes(double dd, int mm) const { return dd < worst || (dd == worst && mm < worst_m); }
    __device__ void insert(double dd, int mm) {
        int j = k - 1;
        while (j > 0) {
            const double pd = d[(j - 1) * TH];
            const int pm = m[(j - 1) * TH];
            if (!(dd < pd || (dd == pd && mm < pm))) break;
            d[j * TH] = pd; m[j * TH] = pm;
            --j;
        }
        d[j * TH] = dd; m[j * TH] = mm;
        worst = d[(k - 1) * TH]; worst_m = m[(k - 1) * TH];
    }
    // the list to out_d / out_m, `stride` entries apart
    __device__ void store(double *out_d, int32_t *out_m, size_t stride) const {
        for (int j = 0; j < k; ++j) { out_d[(size_t)j * stride] = d[j * TH]; out_m[(size_t)j * stride] = m[j * TH]; }
    }
};

size_t knn_lds_bytes(int threads, int k) { return (size_t)threads * k * (sizeof(double) + sizeof(int32_t)); }

struct KnnPlan { int slab_pts, slabs; size_t pidx_off, block_bytes; };

KnnPlan knn_plan(int64_t N, int64_t M, int B, int k, int slab_points) {
    const int64_t qtiles = (N + KNN_THREADS - 1) / KNN_THREADS * (B > 0 ? B : 1);
    const int64_t chunks = (M + KNN_THREADS - 1) / KNN_THREADS;
    int64_t per;
    if (slab_points > 0) per = slab_points / KNN_THREADS;
    else {
        int64_t want = KNN_TARGET_BLOCKS / (qtiles > 0 ? qtiles : 1);
        if (want < 1) want = 1;
        per = (chunks + want - 1) / want;
        if (per < KNN_MIN_CHUNKS) per = KNN_MIN_CHUNKS;
    }
    KnnPlan p;
    p.slab_pts = (int)(per * KNN_THREADS);
    const int64_t slabs = (chunks + per - 1) / per;
    p.slabs = (int)(slabs < 1 ? 1 : (slabs > 0x7fffffff ? 0x7fffffff : slabs));
    p.pidx_off = up256((size_t)N * p.slabs * k * sizeof(double));
    p.block_bytes = p.pidx_off + up256((size_t)N * p.slabs * k * sizeof(int32_t));
    return p;
}

// grid (query tiles, slabs, B): the partial list of 256 queries over one slab of targets
__global__ void __launch_bounds__(KNN_THREADS)
knn_slab_kernel(const double *src, const double *T, const double *dst, int N, int M, int k, char *ws, size_t block_bytes, size_t pidx_off, int slab_pts,
                int slabs) {
    __shared__ double pts[KNN_THREADS * 3];
    const int b = blockIdx.z;
    const int slab = blockIdx.y;
    const int m_begin = slab * slab_pts;
    if (m_begin >= M) return;                     // (uniform over the workgroup; the finish pass does not read this slab)
    const int m_end = min(M, m_begin + slab_pts);
    const int n = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool in = n < N;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (in) {
        const double *p = src + ((size_t)b * N + n) * 3;
        px = p[0]; py = p[1]; pz = p[2];
        if (T) move_point(T + (size_t)b * 16, px, py, pz, px, py, pz);
    }
    KList<KNN_THREADS> list(k, threadIdx.x);
    const double *q = dst + (size_t)b * M * 3;
    for (int m0 = m_begin; m0 < m_end; m0 += KNN_THREADS) {
        const int cnt = min(KNN_THREADS, m_end - m0);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * 3; i += KNN_THREADS) pts[i] = q[(size_t)m0 * 3 + i];
        __syncthreads();
        if (in) {
            for (int j = 0; j < cnt; ++j) {
                const double dx = px - pts[3 * j], dy = py - pts[3 * j + 1], dz = pz - pts[3 * j + 2];
                const double d = (dx * dx + dy * dy) + dz * dz;
                if (list.takes(d, m0 + j)) list.insert(d, m0 + j);
            }
        }
    }
    if (in) {
        char *block = ws + (size_t)b * block_bytes;
        const size_t at = (size_t)slab * k * N + n;
        list.store(reinterpret_cast<double *>(block) + at, reinterpret_cast<int32_t *>(block + pidx_off) + at, (size_t)N);
    }
}

// grid (query tiles of 64, 1, B): a query's partial lists in ascending slab order
__global__ void __launch_bounds__(KNN_LANES)
knn_finish_kernel(int N, int M, int k, const char *ws, size_t block_bytes, size_t pidx_off, int slab_pts, int slabs, double *d2, int32_t *idx) {
    const int b = blockIdx.z;
    const int n = blockIdx.x * KNN_LANES + threadIdx.x;
    if (n >= N) return;
    const char *block = ws + (size_t)b * block_bytes;
    const double *pd = reinterpret_cast<const double *>(block) + n;
    const int32_t *pm = reinterpret_cast<const int32_t *>(block + pidx_off) + n;
    KList<KNN_LANES> list(k, threadIdx.x);
    for (int s = 0; s < slabs && (int64_t)s * slab_pts < M; ++s) {
        for (int j = 0; j < k; ++j) {
            const size_t at = ((size_t)s * k + j) * N;
            const double d = pd[at];
            const int m = pm[at];
            if (!list.takes(d, m)) break;        // the partial list ascends: nothing after this entry is taken either
            list.insert(d, m);
        }
    }
    const size_t out = ((size_t)b * N + n) * k;
    list.store(d2 + out, idx + out, 1);
}

// grid (query tiles of 64, B).  perm NULL, or [B][N]: lane i of problem b answers query perm[b][i] (vt_point_tree_lanes)
template <bool SEED, bool ORDER>
__global__ void __launch_bounds__(KNN_LANES)
knn_walk_kernel(const char *trees, OtAt tree_at, OtBase base, int L, const double *src, const double *T, int N, int k, double *d2, int32_t *idx,
                int32_t *stats, const int32_t *perm) {
    const int b = blockIdx.y;
    const OtView<double> tv = ot_view<double>(trees, tree_at, b);
    const int lane = blockIdx.x * KNN_LANES + threadIdx.x;
    if (lane >= N) return;
    const int n = perm ? perm[(size_t)b * N + lane] : lane;
    double q[3];
    load_query(src, T, b, N, n, q);
    const double flo[3] = {tv.frame[0], tv.frame[1], tv.frame[2]}, fside = tv.frame[3];
    KList<KNN_LANES> list(k, threadIdx.x);
    int n_boxes = 0, n_points = 0, seed_rk = -1;
    // the points of leaf rk in list order
    auto leaf = [&](int rk) {
        const int o = tv.loff[rk], e = tv.loff[rk + 1];
        for (int t = o; t < e; ++t) {
            const double *p = tv.payload + (size_t)t * 3;
            const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            const int m = tv.list[t];
            if (list.takes(d, m)) list.insert(d, m);
        }
        n_points += e - o;
    };
    if (SEED) {
        seed_rk = ot_leaf_of(tv.pyr, tv.frame, L, q);
        if (seed_rk >= 0) leaf(seed_rk);
    }
    ot_walk(
        tv.pyr,
        [&](int level, int rk) {
            const double lb = ot_box_d2(tv.recs + ((size_t)base.v[level] + rk) * OT_BOX, q);
            ++n_boxes;
            if (lb > list.worst) return false;
            if (level < L) return true;
            if (rk != seed_rk) leaf(rk);
            return false;
        },
        [&](int level, unsigned actual) { return ot_near_octant<ORDER>(flo, fside, level, actual, q); });
    const size_t at = (size_t)b * N + n;
    list.store(d2 + at * k, idx + at * k, 1);
    if (stats) { stats[2 * at] = n_boxes; stats[2 * at + 1] = n_points; }
}

// one Jacobi rotation of the symmetric matrix (app, aqq, apq; arp, arq the third index's entries) and of V's columns vp, vq
__device__ inline void knn_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double *vp, double *vq) {
    if (apq == 0.0) return;
    const double zeta = (aqq - app) / (2.0 * apq);
    double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    if (zeta < 0.0) t = -t;
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double x = vp[i], y = vq[i];
        vp[i] = c * x - s * y;
        vq[i] = s * x + c * y;
    }
}

__device__ inline void knn_swap_up(double &la, double &lb, double *va, double *vb) {
    if (la > lb) {
        double t = la; la = lb; lb = t;
#pragma unroll
        for (int i = 0; i < 3; ++i) { t = va[i]; va[i] = vb[i]; vb[i] = t; }
    }
}

// grid (query tiles, B): view NULL, [B][3] (view_per_point == 0) or [B][N][3]
__global__ void __launch_bounds__(KNN_THREADS)
knn_normals_kernel(const double *pts, int M, const int32_t *idx, int N, int k, const double *view, int view_per_point, double *normal, double *eig) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * KNN_THREADS + threadIdx.x;
    if (n >= N) return;
    const double *P = pts + (size_t)b * M * 3;
    const int32_t *ix = idx + ((size_t)b * N + n) * k;
    const size_t out = ((size_t)b * N + n) * 3;
    int count = 0, first = -1;
    for (int j = 0; j < k; ++j) {
        const int m = ix[j];
        if (m >= 0 && m < M) { if (first < 0) first = m; ++count; }
    }
    double nrm[3] = {0.0, 0.0, 0.0}, lam[3] = {0.0, 0.0, 0.0};
    if (count >= 3) {
        const double r0 = P[(size_t)first * 3], r1 = P[(size_t)first * 3 + 1], r2 = P[(size_t)first * 3 + 2];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < k; ++j) {
            const int m = ix[j];
            if (m < 0 || m >= M) continue;
            s0 = s0 + (P[(size_t)m * 3] - r0); s1 = s1 + (P[(size_t)m * 3 + 1] - r1); s2 = s2 + (P[(size_t)m * 3 + 2] - r2);
        }
        const double cnt = (double)count;
        const double m0 = s0 / cnt, m1 = s1 / cnt, m2 = s2 / cnt;
        double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
        for (int j = 0; j < k; ++j) {
            const int m = ix[j];
            if (m < 0 || m >= M) continue;
            const double f0 = (P[(size_t)m * 3] - r0) - m0, f1 = (P[(size_t)m * 3 + 1] - r1) - m1, f2 = (P[(size_t)m * 3 + 2] - r2) - m2;
            c00 = c00 + f0 * f0; c01 = c01 + f0 * f1; c02 = c02 + f0 * f2;
            c11 = c11 + f1 * f1; c12 = c12 + f1 * f2; c22 = c22 + f2 * f2;
        }
        c00 = c00 / cnt; c01 = c01 / cnt; c02 = c02 / cnt; c11 = c11 / cnt; c12 = c12 / cnt; c22 = c22 / cnt;
        if (c00 != 0.0 || c01 != 0.0 || c02 != 0.0 || c11 != 0.0 || c12 != 0.0 || c22 != 0.0) {
            double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
            for (int sweep = 0; sweep < KNN_SWEEPS; ++sweep) {
                knn_rotate(c00, c11, c01, c02, c12, v0, v1);
                knn_rotate(c00, c22, c02, c01, c12, v0, v2);
                knn_rotate(c11, c22, c12, c01, c02, v1, v2);
            }
            knn_swap_up(c00, c11, v0, v1); knn_swap_up(c11, c22, v1, v2); knn_swap_up(c00, c11, v0, v1);
            const double len = sqrt((v0[0] * v0[0] + v0[1] * v0[1]) + v0[2] * v0[2]);
            nrm[0] = v0[0] / len; nrm[1] = v0[1] / len; nrm[2] = v0[2] / len;
            lam[0] = c00; lam[1] = c11; lam[2] = c22;
            bool flip;
            const int m_q = ix[0];
            if (view && m_q >= 0 && m_q < M) {
                const double *w = view + (view_per_point ? ((size_t)b * N + n) * 3 : (size_t)b * 3);
                const double *pq = P + (size_t)m_q * 3;
                flip = (nrm[0] * (w[0] - pq[0]) + nrm[1] * (w[1] - pq[1])) + nrm[2] * (w[2] - pq[2]) < 0.0;
            } else {
                double big = nrm[0];
                if (fabs(nrm[1]) > fabs(big)) big = nrm[1];
                if (fabs(nrm[2]) > fabs(big)) big = nrm[2];
                flip = big < 0.0;
            }
            if (flip) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { normal[out + a] = nrm[a]; eig[out + a] = lam[a]; }
}

bool knn_sizes_ok(int64_t N, int64_t M, int B) { return N >= 1 && M >= 1 && B >= 1 && N <= KNN_MAX && M <= KNN_MAX && B <= 65535; }
bool knn_k_ok(int k) { return k >= 1 && k <= VT_KNN_MAX_K; }
bool knn_slab_ok(int slab_points) { return slab_points == 0 || (slab_points > 0 && slab_points % KNN_THREADS == 0); }

typedef void (*KnnWalkFn)(const char *, OtAt, OtBase, int, const double *, const double *, int, int, double *, int32_t *, int32_t *, const int32_t *);
const KnnWalkFn KNN_WALK[4] = {knn_walk_kernel<false, false>, knn_walk_kernel<true, false>, knn_walk_kernel<false, true>, knn_walk_kernel<true, true>};

}  // namespace

extern "C" {

size_t vt_knn_points_workspace_bytes(int64_t N, int64_t M, int B, int k, int slab_points) {
    if (!knn_sizes_ok(N, M, B) || !knn_k_ok(k) || !knn_slab_ok(slab_points)) return 0;
    return (size_t)B * knn_plan(N, M, B, k, slab_points).block_bytes;
}

int vt_knn_points_slab_points(int64_t N, int64_t M, int B) {
    if (!knn_sizes_ok(N, M, B)) return 0;
    return knn_plan(N, M, B, 1, 0).slab_pts;
}

int vt_knn_points(const double *src, int64_t N, const double *dst, int64_t M, int B, const double *T, int k, int slab_points, double *d2, int32_t *idx,
                  void *workspace, size_t workspace_bytes, void *stream) {
    if (!knn_sizes_ok(N, M, B) || !src || !dst || !d2 || !idx)
        return vt_fail(VT_ERR_INVALID, "vt_knn_points: bad argument (N >= 1, M >= 1, 1 <= B <= 65535)");
    if (!knn_k_ok(k)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_knn_points: k outside [1, 32]");
    if (!knn_slab_ok(slab_points)) return vt_fail(VT_ERR_INVALID, "vt_knn_points: slab_points must be 0 or a multiple of 256");
    const KnnPlan pl = knn_plan(N, M, B, k, slab_points);
    if (pl.slabs > 65535) return vt_fail(VT_ERR_UNSUPPORTED, "vt_knn_points: more than 65535 slabs");
    if (!workspace || workspace_bytes < (size_t)B * pl.block_bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_knn_points");
    const size_t slab_lds = knn_lds_bytes(KNN_THREADS, k), finish_lds = knn_lds_bytes(KNN_LANES, k);
    if (hipError_t e = vt_max_dyn_lds(reinterpret_cast<const void *>(knn_slab_kernel), (int)knn_lds_bytes(KNN_THREADS, VT_KNN_MAX_K)))
        return vt_check(e, "vt_knn_points: hipFuncSetAttribute");
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    hipLaunchKernelGGL(knn_slab_kernel, dim3(blocks_of(N, KNN_THREADS), (unsigned)pl.slabs, (unsigned)B), dim3(KNN_THREADS), slab_lds, st, src, T, dst,
                       (int)N, (int)M, k, ws, pl.block_bytes, pl.pidx_off, pl.slab_pts, pl.slabs);
    hipLaunchKernelGGL(knn_finish_kernel, dim3(blocks_of(N, KNN_LANES), 1u, (unsigned)B), dim3(KNN_LANES), finish_lds, st, (int)N, (int)M, k,
                       (const char *)ws, pl.block_bytes, pl.pidx_off, pl.slab_pts, pl.slabs, d2, idx);
    return vt_check(hipGetLastError(), "vt_knn_points");
}

int vt_point_tree_knn(const void *tree, size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, const double *src, int64_t N,
                      const double *T, int k, double *d2, int32_t *idx, int32_t *stats, const int32_t *perm, void *stream) {
    if (!tree || !src || !d2 || !idx) return vt_fail(VT_ERR_INVALID, "vt_point_tree_knn: bad argument (a NULL array)");
    if (!knn_k_ok(k)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_point_tree_knn: k outside [1, 32]");
    PtQueryPlan plan;
    if (int rc = pt_query_plan(tree_bytes, M, depth, B, state_host, N, &plan)) return rc;
    OtBase base;
    for (int l = 0; l <= OT_LEVELS; ++l) base.v[l] = plan.base[l];
    hipLaunchKernelGGL(KNN_WALK[plan.kernel], dim3(blocks_of(N, KNN_LANES), (unsigned)B), dim3(KNN_LANES), knn_lds_bytes(KNN_LANES, k),
                       (hipStream_t)stream, static_cast<const char *>(tree), OtAt{plan.stride, plan.pyr, plan.box, plan.loff, plan.list, plan.pts},
                       base, plan.depth, src, T, (int)N, k, d2, idx, stats, perm);
    return vt_check(hipGetLastError(), "vt_point_tree_knn");
}

int vt_knn_normals(const double *pts, int64_t M, const int32_t *idx, int64_t N, int k, int B, const double *view, int view_per_point, double *normal,
                   double *eig, void *stream) {
    if (!knn_sizes_ok(N, M, B) || !pts || !idx || !normal || !eig)
        return vt_fail(VT_ERR_INVALID, "vt_knn_normals: bad argument (N >= 1, M >= 1, 1 <= B <= 65535)");
    if (!knn_k_ok(k)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_knn_normals: k outside [1, 32]");
    hipLaunchKernelGGL(knn_normals_kernel, dim3(blocks_of(N, KNN_THREADS), (unsigned)B), dim3(KNN_THREADS), 0, (hipStream_t)stream, pts, (int)M, idx,
                       (int)N, k, view, view_per_point, normal, eig);
    return vt_check(hipGetLastError(), "vt_knn_normals");
}

}  // extern "C"
