// Evaluation metrics of the visualise block (reference src/conv_onet/generation.py:274-284, src/common.py:45-91) on the device:
//   vt_chamfer_nn    nearest neighbour of every point in the other set, both directions in one launch (naive Chamfer distance);
//   vt_emd_auction   the optimal assignment of scipy.optimize.linear_sum_assignment over the cdist cost matrix, by an
//                    epsilon-scaling auction: one workgroup per problem, every per-problem array in LDS, no grid-wide barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vt_common.h"
#include "vtaco_hip.h"

namespace {

// ---- nearest neighbour ---------------------------------------------------------------------------------------------------
constexpr int NN_THREADS = 256;       // one query point per thread
constexpr int NN_TILE = 1024;         // target points staged in LDS per pass (SoA: conflict-free broadcast reads)

// blockIdx.z = direction: 0 = queries a, targets b (d_ab, i_ab); 1 = queries b, targets a (d_ba, i_ba).  blockIdx.y = problem.
__global__ void __launch_bounds__(NN_THREADS)
chamfer_nn_kernel(const float *a, const float *b, int N, int M, float *d_ab, int *i_ab, float *d_ba, int *i_ba) {
    __shared__ float tx[NN_TILE], ty[NN_TILE], tz[NN_TILE];
    const int dir = blockIdx.z, prob = blockIdx.y;
    const int nq = dir ? M : N, nt = dir ? N : M;
    const float *q = (dir ? b : a) + (size_t)prob * nq * 3;
    const float *t = (dir ? a : b) + (size_t)prob * nt * 3;
    float *dout = (dir ? d_ba : d_ab) + (size_t)prob * nq;
    int *iout = (dir ? i_ba : i_ab) + (size_t)prob * nq;
    const int qi = blockIdx.x * NN_THREADS + threadIdx.x;
    if ((int)(blockIdx.x * NN_THREADS) >= nq) return;            // the grid covers max(N, M): whole workgroup idle in one direction
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (qi < nq) { qx = q[3 * qi]; qy = q[3 * qi + 1]; qz = q[3 * qi + 2]; }
    float best = __builtin_huge_valf();
    int arg = 0;
    for (int t0 = 0; t0 < nt; t0 += NN_TILE) {
        __syncthreads();
        for (int k = threadIdx.x; k < NN_TILE && t0 + k < nt; k += NN_THREADS) {
            const size_t j = (size_t)(t0 + k) * 3;
            tx[k] = t[j]; ty[k] = t[j + 1]; tz[k] = t[j + 2];
        }
        __syncthreads();
        const int cnt = min(NN_TILE, nt - t0);
        for (int k = 0; k < cnt; ++k) {
            const float dx = qx - tx[k], dy = qy - ty[k], dz = qz - tz[k];
            const float d = (dx * dx + dy * dy) + dz * dz;           // numpy's f32 order; -ffp-contract=off keeps it unfused
            if (d < best) { best = d; arg = t0 + k; }                // strict: the smallest index among equal minima
        }
    }
    if (qi < nq) { dout[qi] = best; iout[qi] = arg; }
}

// ---- epsilon-scaling auction -----------------------------------------------------------------------------------------------
constexpr int EMD_THREADS = 1024;
constexpr int EMD_WAVES = EMD_THREADS / 64;
constexpr float EMD_THETA = 5.f;      // epsilon divisor between phases

struct EmdStats { long long rounds, bids; int phases; float eps_last; long long pad; };     // 32 bytes per problem (the workspace)
static_assert(sizeof(EmdStats) == VT_EMD_WORKSPACE_PER_PROBLEM, "workspace record");

// bid slot u64, b xyz + price f32, owner / assign / list i16; with cache_a also a xyz f32 (the bidders' own coordinates)
constexpr int emd_lds_bytes(int n, bool cache_a) { return n * (8 + 4 * 4 + (cache_a ? 12 : 0) + 3 * 2); }
constexpr int EMD_LDS_LIMIT = 160 * 1024 - 1024;      // dynamic LDS of one workgroup (the kernel's static LDS is < 1 KiB)
static_assert(emd_lds_bytes(VT_EMD_MAX_POINTS, false) <= EMD_LDS_LIMIT, "the largest problem must fit");

__device__ __forceinline__ unsigned long long pack_bid(float bid, int person) {
    unsigned u = __float_as_uint(bid);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                         // order-preserving float -> unsigned
    return ((unsigned long long)u << 32) | (unsigned)person;
}
__device__ __forceinline__ float unpack_bid(unsigned long long s) {
    const unsigned u = (unsigned)(s >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// (best, index, second best) of two partial scans; equal bests keep the smaller index and make the second best equal to the best
__device__ __forceinline__ void merge_best(float &b1, int &i1, float &b2, float ob1, int oi1, float ob2) {
    if (ob1 < b1 || (ob1 == b1 && oi1 < i1)) {
        b2 = fminf(b1, ob2); b1 = ob1; i1 = oi1;
    } else {
        b2 = fminf(b2, ob1);
    }
}

__device__ __forceinline__ void wave_best(float &b1, int &i1, float &b2) {
    for (int o = 32; o > 0; o >>= 1) {
        const float ob1 = __shfl_xor(b1, o), ob2 = __shfl_xor(b2, o);
        const int oi1 = __shfl_xor(i1, o);
        merge_best(b1, i1, b2, ob1, oi1, ob2);
    }
}

__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

// block-wide min of v (every thread gets it); red: EMD_WAVES floats of LDS
__device__ float block_min(float v, float *red) {
    v = wave_min(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < EMD_WAVES; ++w) r = fminf(r, red[w]);
    return r;
}

// One bidder's scan over the columns j = first, first + stride, ... < n: best value c(i, j) + price[j], its column (smallest on ties)
// and the second best, reduced over the wave.  Dummy rows (i >= N) and dummy columns (j >= M) cost 0.
__device__ __forceinline__ void bid_scan(float px, float py, float pz, bool real, int M, int n, const float *bx, const float *by, const float *bz,
                                         const float *price, int first, int stride, float &b1, int &i1, float &b2) {
    b1 = __builtin_huge_valf(); b2 = __builtin_huge_valf(); i1 = n;
    // (the scan is the auction's whole arithmetic -- bids x n cost evaluations on one CU -- so the real columns run without the
    // dummy tests, and the square root is the hardware's v_sqrt_f32 (1 ulp) rather than the correctly rounded sequence: the
    // assignment's cost is evaluated again in float64 at the end)
    int j = first;
    if (real) {
        for (; j < M; j += stride) {
            const float dx = px - bx[j], dy = py - by[j], dz = pz - bz[j];
            const float v = __builtin_amdgcn_sqrtf((dx * dx + dy * dy) + dz * dz) + price[j];
            if (v < b1) { b2 = b1; b1 = v; i1 = j; }
            else if (v < b2) b2 = v;
        }
    }
    for (; j < n; j += stride) {
        const float v = price[j];
        if (v < b1) { b2 = b1; b1 = v; i1 = j; }
        else if (v < b2) b2 = v;
    }
    wave_best(b1, i1, b2);
}

// person i's bid for its best column i1: the price rises by the value gap to the second best plus eps (> a few ulps of the price);
// the highest (bid, person) of the round wins the column -- one 64-bit LDS atomic max, independent of the order the waves arrive in
__device__ __forceinline__ void place_bid(unsigned long long *slot, const float *price, int i, float b1, int i1, float b2, float eps) {
    const float gap = b2 < __builtin_huge_valf() ? b2 - b1 : 0.f;          // n == 1: no second column
    atomicMax(&slot[i1], pack_bid(price[i1] + gap + eps, i));
}

// person i's coordinates: from the LDS copy when the problem has room for it, else from global memory (0 for a dummy person)
__device__ __forceinline__ bool person_xyz(const float *a, const float *ax, int i, int N, float &px, float &py, float &pz) {
    px = py = pz = 0.f;
    if (i >= N) return false;
    if (ax) { px = ax[i]; py = ax[N + i]; pz = ax[2 * N + i]; }
    else { px = a[3 * i]; py = a[3 * i + 1]; pz = a[3 * i + 2]; }
    return true;
}

// One problem per workgroup.  Persons = rows of a (N), objects = rows of b (M), both padded to n = max(N, M) with dummies whose
// cost to everything is 0 (exact for the rectangular assignment).  Minimises sum c(i, assign[i]) with c = |a_i - b_j| in f32.
__global__ void __launch_bounds__(EMD_THREADS)
emd_auction_kernel(const float *a, int N, const float *b, int M, float eps_final, int max_rounds, int cache_a,
                   int *assign_out, float *prices_out, double *cost_out, int *status_out, EmdStats *stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long emd_lds[];
    __shared__ float red[EMD_WAVES];
    __shared__ float part_b1[EMD_WAVES], part_b2[EMD_WAVES];
    __shared__ int part_i1[EMD_WAVES];
    __shared__ double dred[EMD_WAVES];
    __shared__ int s_count;

    const int n = N > M ? N : M;
    const int prob = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    a += (size_t)prob * N * 3;
    b += (size_t)prob * M * 3;
    unsigned long long *slot = emd_lds;                            // this round's highest bid per object, 0 = none
    float *bx = reinterpret_cast<float *>(slot + n), *by = bx + n, *bz = by + n, *price = bz + n;
    float *ax = cache_a ? price + n : nullptr;                     // [3][N] when cached
    short *owner = reinterpret_cast<short *>(price + n + (cache_a ? 3 * n : 0)), *asg = owner + n, *list = asg + n;

    float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    float finite = 1.f;                                            // 0 once this thread has read a NaN (fminf / fmaxf pass it over)
    for (int j = tid; j < n; j += EMD_THREADS) {
        float x = 0.f, y = 0.f, z = 0.f;
        if (j < M) {
            x = b[3 * j]; y = b[3 * j + 1]; z = b[3 * j + 2];
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
            if (x != x || y != y || z != z) finite = 0.f;
        }
        bx[j] = x; by[j] = y; bz[j] = z;
        price[j] = 0.f;
        slot[j] = 0ull;
    }
    for (int i = tid; i < N; i += EMD_THREADS)
        for (int k = 0; k < 3; ++k) {
            const float v = a[3 * i + k];
            lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v);
            if (v != v) finite = 0.f;
            if (ax) ax[k * N + i] = v;
        }
    // the cost range: no pair is farther apart than the diagonal of the two clouds' common bounding box
    float diag2 = 0.f;
    for (int k = 0; k < 3; ++k) {
        const float l = block_min(lo[k], red), h = -block_min(-hi[k], red);
        diag2 += (h - l) * (h - l);
    }
    const float crange = sqrtf(diag2);
    finite = block_min(finite, red);
    if (!(finite > 0.f) || !(crange < __builtin_huge_valf())) {
        // A NaN or an infinite coordinate (or finite ones whose range overflows f32): every value of such a bidder would be NaN and
        // its best column n, one past the arrays.  Status 2 before the first round; uniform over the workgroup (block_min's result).
        for (int i = tid; i < n; i += EMD_THREADS) {
            assign_out[(size_t)prob * n + i] = -1;
            prices_out[(size_t)prob * n + i] = 0.f;
        }
        if (tid == 0) {
            cost_out[prob] = __builtin_nan("");
            status_out[prob] = 2;
            if (stats) {
                EmdStats st;
                st.rounds = 0; st.bids = 0; st.phases = 0; st.eps_last = 0.f; st.pad = 0;
                stats[prob] = st;
            }
        }
        return;
    }
    // The last epsilon is relative to the cost range's binade, eps_final * 2^floor(log2(crange)): f32 prices grow with the cost range,
    // and an absolute epsilon below half an ulp of a price no longer raises it (two tied bidders then take one object from each other
    // for ever).  Powers of two are exact, so clouds scaled by 2^k give the same rounds and assignment, and prices scaled by 2^k.
    const float eps_end = crange > 0.f ? ldexpf(eps_final, ilogbf(crange)) : eps_final;
    float eps = fmaxf(crange / EMD_THETA, eps_end);

    long long rounds = 0, bids = 0;
    int phases = 0, status = 0;
    for (;;) {
        // a phase: every person unassigned, prices kept (shifted so that the lowest is 0: ties the f32 price magnitude to the cost range)
        float pmin = __builtin_huge_valf();
        for (int j = tid; j < n; j += EMD_THREADS) pmin = fminf(pmin, price[j]);
        pmin = block_min(pmin, red);
        for (int j = tid; j < n; j += EMD_THREADS) { price[j] -= pmin; owner[j] = -1; asg[j] = -1; }
        if (tid == 0) s_count = 0;
        __syncthreads();
        for (;;) {
            for (int i = tid; i < n; i += EMD_THREADS)
                if (asg[i] < 0) list[atomicAdd(&s_count, 1)] = (short)i;
            __syncthreads();
            const int cnt = s_count;                               // uniform: read behind the barrier
            if (cnt == 0) break;
            if (rounds >= max_rounds) { status = 1; break; }
            ++rounds; bids += cnt;
            // Jacobi round: every unassigned person bids, one wave per bidder -- or g waves per bidder (a share of the columns each)
            // when there are fewer bidders than waves: the last rounds of a phase have one or two
            int g = 1;
            while (g * 2 * cnt <= EMD_WAVES) g *= 2;
            if (g == 1) {
                for (int k = wave; k < cnt; k += EMD_WAVES) {
                    const int i = list[k];
                    float px, py, pz, b1, b2;
                    int i1;
                    const bool real = person_xyz(a, ax, i, N, px, py, pz);
                    bid_scan(px, py, pz, real, M, n, bx, by, bz, price, lane, 64, b1, i1, b2);
                    if (lane == 0) place_bid(slot, price, i, b1, i1, b2, eps);
                }
            } else {
                const int k = wave / g, sub = wave % g;
                float b1 = __builtin_huge_valf(), b2 = __builtin_huge_valf();
                int i1 = n;
                if (k < cnt) {
                    float px, py, pz;
                    const bool real = person_xyz(a, ax, list[k], N, px, py, pz);
                    bid_scan(px, py, pz, real, M, n, bx, by, bz, price, sub * 64 + lane, 64 * g, b1, i1, b2);
                }
                if (lane == 0) { part_b1[wave] = b1; part_i1[wave] = i1; part_b2[wave] = b2; }
                __syncthreads();
                if (k < cnt && sub == 0) {                         // lane s of the group's first wave takes partial s: one butterfly
                    b1 = b2 = __builtin_huge_valf();
                    i1 = n;
                    if (lane < g) { b1 = part_b1[wave + lane]; i1 = part_i1[wave + lane]; b2 = part_b2[wave + lane]; }
                    wave_best(b1, i1, b2);
                    if (lane == 0) place_bid(slot, price, list[k], b1, i1, b2, eps);
                }
            }
            __syncthreads();
            // the highest bid takes each object; its previous owner becomes unassigned.  A person bids for one object, so wins at most one.
            if (tid == 0) s_count = 0;
            for (int j = tid; j < n; j += EMD_THREADS) {
                const unsigned long long s = slot[j];
                if (s) {
                    const int w = (int)(unsigned)(s & 0xffffffffull), o = owner[j];
                    if (o >= 0) asg[o] = -1;
                    owner[j] = (short)w;
                    asg[w] = (short)j;
                    price[j] = unpack_bid(s);
                    slot[j] = 0ull;
                }
            }
            __syncthreads();
        }
        if (status) break;
        ++phases;
        if (eps <= eps_end) break;
        eps = fmaxf(eps / EMD_THETA, eps_end);
        __syncthreads();
    }
    __syncthreads();

    // the assignment's cost as cdist evaluates it: float64 differences, squared, summed x, y, z, square root; / N as len(d)
    double sum = 0.0;
    for (int i = tid; i < N; i += EMD_THREADS) {
        const int j = asg[i];
        if (j >= 0 && j < M) {
            const double dx = (double)a[3 * i] - (double)b[3 * j], dy = (double)a[3 * i + 1] - (double)b[3 * j + 1],
                         dz = (double)a[3 * i + 2] - (double)b[3 * j + 2];
            sum += sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);   // fixed butterfly, then the waves in order: deterministic
    if (lane == 0) dred[wave] = sum;
    for (int i = tid; i < n; i += EMD_THREADS) {
        assign_out[(size_t)prob * n + i] = asg[i];
        prices_out[(size_t)prob * n + i] = price[i];
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int w = 0; w < EMD_WAVES; ++w) tot += dred[w];
        cost_out[prob] = tot / (double)N;
        status_out[prob] = status;
        if (stats) {
            EmdStats st;
            st.rounds = rounds; st.bids = bids; st.phases = phases; st.eps_last = eps; st.pad = 0;
            stats[prob] = st;
        }
    }
}

}  // namespace

extern "C" {

int vt_chamfer_nn(const float *a, const float *b, int B, int N, int M, float *d_ab, int *i_ab, float *d_ba, int *i_ba, void *stream) {
    if (B == 0) return 0;
    if (!a || !b || !d_ab || !i_ab || !d_ba || !i_ba || B < 0 || N <= 0 || M <= 0)
        return vt_fail(VT_ERR_INVALID, "vt_chamfer_nn: bad argument (both sets need at least one point)");
    const int nmax = N > M ? N : M;
    hipLaunchKernelGGL(chamfer_nn_kernel, dim3((unsigned)((nmax + NN_THREADS - 1) / NN_THREADS), (unsigned)B, 2u), dim3(NN_THREADS), 0,
                       (hipStream_t)stream, a, b, N, M, d_ab, i_ab, d_ba, i_ba);
    return vt_check(hipGetLastError(), "vt_chamfer_nn");
}

size_t vt_emd_workspace_bytes(int n, int m) {
    if (n <= 0 || m <= 0 || n > VT_EMD_MAX_POINTS || m > VT_EMD_MAX_POINTS) return 0;
    return VT_EMD_WORKSPACE_PER_PROBLEM;
}

int vt_emd_auction(const float *a, int N, const float *b, int M, int B, float eps_final, int max_rounds,
                   int *assign, float *prices, double *cost_f64, int *status, void *ws, size_t ws_bytes, void *stream) {
    if (B == 0) return 0;
    if (!a || !b || !assign || !prices || !cost_f64 || !status || B < 0 || N <= 0 || M <= 0 || max_rounds < 0 || !(eps_final > 0.f))
        return vt_fail(VT_ERR_INVALID, "vt_emd_auction: bad argument");
    if (vt_emd_workspace_bytes(N, M) == 0)
        return vt_fail(VT_ERR_UNSUPPORTED, "vt_emd_auction: more than VT_EMD_MAX_POINTS points on a side (the problem lives in LDS)");
    if (ws && ws_bytes < (size_t)B * VT_EMD_WORKSPACE_PER_PROBLEM)
        return vt_fail(VT_ERR_WORKSPACE, "vt_emd_auction: workspace smaller than B * vt_emd_workspace_bytes(N, M)");
    const int n = N > M ? N : M;
    const bool cache_a = emd_lds_bytes(n, true) <= EMD_LDS_LIMIT;      // up to 3876 points a side
    hipError_t e = vt_max_dyn_lds(reinterpret_cast<const void *>(emd_auction_kernel), EMD_LDS_LIMIT);
    if (e != hipSuccess) return vt_check(e, "vt_emd_auction: hipFuncSetAttribute");
    hipLaunchKernelGGL(emd_auction_kernel, dim3((unsigned)B), dim3(EMD_THREADS), emd_lds_bytes(n, cache_a), (hipStream_t)stream,
                       a, N, b, M, eps_final, max_rounds, (int)cache_a, assign, prices, cost_f64, status, reinterpret_cast<EmdStats *>(ws));
    return vt_check(hipGetLastError(), "vt_emd_auction");
}

}  // extern "C"
