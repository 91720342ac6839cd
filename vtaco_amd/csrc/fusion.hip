// TransformerFusion forward (eval mode) for gfx950: the visual-tactile feature fuser of
// AttentionDecoder.forward_img (reference src/conv_onet/models/decoder.py:237-271 ->
// src/TransformerFusion.py:311-333; RelationUnit :92-113, TransNonlinear :21-25,
// encoder/decoder layers :130-146, :191-219), built with num_layers=1, d_model=32,
// key_feature_dim=64, with_pos_embed=False.
//
// One attention unit, X_q (queries) against X_k (keys/values), all [B,N,32]:
//   Q = l2norm(X_q WQ^T), K = l2norm(X_k WK^T) (64-d), V = X_k WV^T
//   A = softmax_k(Q K^T);  A <- A / (1e-9 + sum_q A)      (the reference's column re-norm)
//   r = relu((X_q - A V) Wt^T);  y = LayerNorm(r + W2 relu(W1 r + b1) + b2);  z = X_q + y
//   out = relu(InstanceNorm_N(z))
// Q and K are unit vectors, so scores lie in [-1,1] and exp() needs no running max; the
// column re-normalisation makes the usual one-pass online softmax impossible, so the N x N
// scores are recomputed three times on the matrix core (bf16 MFMA, split-bf16 operands: see
// below) instead of being stored (N=2048 would need 16 MB per matrix per scene otherwise):
//   rowsum  l_q = sum_k e^{S_qk}          colsum  s_k = sum_q e^{S_qk} / l_q
//   attend  O_q = (1/l_q) sum_k e^{S_qk} V_k / (1e-9 + s_k), chained into the epilogue MLP.
// Score tiles come out of the MFMA with the fixed index on the lane and the streamed index
// in the 16 registers, which is exactly the B operand the next MFMA (E x V') needs.
#include <stdlib.h>
#include <type_traits>

#include "fusion_common.h"

namespace {

// ---- split 16-bit operands ------------------------------------------------------------------
// The N x N products run on the 16-bit matrix core with every f32 operand carried as
// hi + lo (hi = round16(v), lo = round16(v - hi)), f32 accumulation (decode_common.h), instead of
// 32 x v_mfma_f32_32x32x2_f32 (2048 cycles) per 32 x 32 x 64 score tile.  Q, K and V' are split ONCE
// by the kernels that produce them, straight into MFMA fragment order, so the passes do no conversion
// work except for the exponentials E that feed E x V'.
//   scores: HALF pairs (unit vectors, Q times log2 e: |component| <= 1.45, no range issue; the lo halves
//     are half subnormals, hi + lo carries ~22 bits).  Training forward: lo*hi + hi*lo + hi*hi, 12
//     v_mfma_f32_32x32x16_f16 (384 cycles).  Inference: the keys rounded to half, 8 MFMAs (score_tile).
//   E x V': bf16 pairs, three products (V' = V / (1e-9 + s) has no bound).
//
// Q/K row (128 halves = 256 B): [kg 2][part hi|lo 2][k-step t 4][e 8], column = 16t + 8kg + e --
// lane (row, kg) of a 32x32x16 MFMA reads its 4 hi and 4 lo fragments as one 128-B run.
// Q is stored times log2(e), so exp(S) is a bare v_exp_f32 of the MFMA result.
struct FragQK {
    f16x8 hi[4], lo[4];
};
__device__ __forceinline__ void load_fragqk(FragQK &f, const void *rowbase, int kg) {
    const f16x8 *r = reinterpret_cast<const f16x8 *>(reinterpret_cast<const char *>(rowbase) + kg * 128);
#pragma unroll
    for (int t = 0; t < 4; ++t) { f.hi[t] = r[t]; f.lo[t] = r[4 + t]; }
}
__device__ __forceinline__ f32x16 mfma16(const bf16x8 &a, const bf16x8 &b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// D[i][j] = stream_row_i . fixed_row_j over the 64-d keys: lane (j,h) reg r = score of
// streamed row chan_of(r,h) against fixed row j
// STREAM_KEYS: the streamed rows are the keys, otherwise the fixed rows are.  FULL: all three products (queries and keys to ~22
// bits); otherwise the KEYS enter rounded to half precision (q_hi k_hi + q_lo k_hi: 8 MFMAs instead of 12) -- every pass then
// computes the exact attention of the rounded keys, whose rounding errors are independent from key to key and average out over
// the keys a query attends (rounding the queries instead would put one common error on a whole row of scores).
template <bool STREAM_KEYS, bool FULL>
__device__ __forceinline__ f32x16 score_tile(const FragQK &stream, const FragQK &fixed) {
    f32x16 acc;
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (FULL || !STREAM_KEYS) acc = mfma_s(stream.lo[t], fixed.hi[t], acc);
        if (FULL || STREAM_KEYS) acc = mfma_s(stream.hi[t], fixed.lo[t], acc);
        acc = mfma_s(stream.hi[t], fixed.hi[t], acc);
    }
    return acc;
}

// ---- inference: the correction product on ONE fp8 MFMA ("f16f8", as the lattice decode's layers: decode_st3.h) ----------------
// Keys rounded to half as above; the queries' remainder q_lo enters as fp8 (e4m3) against an fp8 copy of k_hi:
//     S = q_hi . k_hi  (4 x v_mfma_f32_32x32x16_f16)  +  2^-18 fp8(q_lo 2^14) . fp8(k_hi 2^4)  (1 x v_mfma_scale_f32_32x32x64_f8f6f4)
// 192 matrix cycles per 32 x 32 x 64 tile instead of 256 and ~30 % less matrix-pipe energy (tools/probe/shape_probe.hip); the
// correction is 2^-11 of the score and carries 4 significant bits -- far below the rounding of the keys.  Both fp8 vectors are
// written ONCE by the projection kernel.  Row (192 B): [kg 2][hi: k-step t 4 x 8 halves | fp8: 32 bytes, byte 8t + e], column
// = 16t + 8kg + e; Q rows carry fp8(q_lo 2^14), K rows fp8(k_hi 2^4).
typedef unsigned u32x8 __attribute__((ext_vector_type(8)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
constexpr int F8_QL = 14, F8_KH = 4;                  // power-of-two shifts of the two fp8 vectors
struct FragQK8 {
    f16x8 hi[4];
    u32x8 q;
};
__device__ __forceinline__ void load_fragqk8(FragQK8 &f, const void *rowbase, int kg) {
    const f16x8 *r = reinterpret_cast<const f16x8 *>(reinterpret_cast<const char *>(rowbase) + kg * 96);
#pragma unroll
    for (int t = 0; t < 4; ++t) f.hi[t] = r[t];
    const u32x4 a = __builtin_bit_cast(u32x4, r[4]), b = __builtin_bit_cast(u32x4, r[5]);
    f.q = u32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
template <int SHIFT>
__device__ __forceinline__ f32x16 mfma_f8(const u32x8 &a, const u32x8 &b, f32x16 c) {       // c += 2^-SHIFT a8 . b8
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(__builtin_bit_cast(i32x8, a), __builtin_bit_cast(i32x8, b), c, 0, 0,
                                                           0, 127 - SHIFT, 0, 127);
}
__device__ __forceinline__ f32x16 score_tile8(const FragQK8 &stream, const FragQK8 &fixed) {
    f32x16 acc;
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = mfma_s(stream.hi[t], fixed.hi[t], acc);
    return mfma_f8<F8_QL + F8_KH>(stream.q, fixed.q, acc);
}
// MODE.FP16_OVFL = 1: the fp8 conversions saturate at +-448 instead of producing NaN (hwreg MODE = 1, bit 23)
// four values / scale as fp8 (e4m3) bytes 0..3 of a dword
__device__ __forceinline__ unsigned fp8x4(float a, float b, float c, float d, float scale) {
    i16x2 w;
    asm volatile("" : "=v"(w));                          // both halves are written below: nothing to initialise
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, a, b, scale, false);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, c, d, scale, true);
    return __builtin_bit_cast(unsigned, w);
}
__device__ __forceinline__ void fp8_saturating_mode() { __builtin_amdgcn_s_setreg((1 - 1) << 11 | 23 << 6 | 1, 1); }

// ---- projections on the f32 matrix core: one wave per 32 points -------------------------------
// D[out][point] += W[out][k] X^T[k][point] for up to five 32-row groups (Q: 2, K: 2, V: 1).  The rows of
// the Q/K groups are permuted so that registers 0..7 / 8..15 of lane-half h hold 8 consecutive
// output columns (16(2g + r/8) + 8h + r%8): exactly one hi and one lo fragment of the split row
// layout above, written with 16-byte stores.  V keeps the natural order (store_acc16).
template <bool DO_Q, bool DO_KV, bool F8>
__global__ void __launch_bounds__(256)
fusion_proj_kernel(const float *Xq, const float *Xk, FusionUnitDev u, float *Qd, float *Kd, float *V, int total, XIds xi, int tiles) {
    __shared__ __attribute__((aligned(16))) float wf[5][16][64];          // [group][k-step][lane] A fragments
    if constexpr (F8) fp8_saturating_mode();
    for (int e = threadIdx.x; e < 5 * 1024; e += 256) {
        const int g = e >> 10, st = (e >> 6) & 15, l = e & 63, i = l & 31, kk = l >> 5, k = 2 * st + kk;
        // output row i of the MFMA <-> accumulator register r of lane-half hh with chan_of(r,hh) == i
        const int hh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3);
        float v = 0.0f;
        if (g < 4) {
            const int gg = g & 1, col = 16 * (2 * gg + (r >> 3)) + 8 * hh + (r & 7);
            if (g < 2 ? DO_Q : DO_KV) v = (g < 2 ? u.WQ : u.WK)[col * 32 + k];
        } else if (DO_KV) {
            v = u.WV[i * 32 + k];
        }
        wf[g][st][l] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    // ``tiles`` 32-point tiles per wave: the staging of the weight fragments above (20 loads per thread) is paid once per
    // 128 * tiles points instead of once per 128
    for (int tile = 0; tile < tiles; ++tile) {
    const int p0 = ((blockIdx.x * tiles + tile) * 4 + wave) * 32;
    if (p0 >= total) return;
    const int p = min(p0 + j, total - 1);
    const bool live = p0 + j < total;
    auto load_x = [&](const float *X, float (&x)[16]) {                       // x[s] = X[p][2s + h]
        const f32x4 *r = reinterpret_cast<const f32x4 *>(X ? X + (size_t)p * 32 : xi.row((size_t)p));      // (null: the rows by finger id)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 t = r[i];
            x[2 * i] = h ? t.y : t.x;
            x[2 * i + 1] = h ? t.w : t.z;
        }
    };
    auto project = [&](const float (&x)[16], int g) {
        f32x16 acc;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[s] = 0.0f;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = mfma(wf[g][s][lane], x[s], acc);
        return acc;
    };
    auto store_unit = [&](const f32x16 &a0, const f32x16 &a1, float *dst, float post, bool is_q) {
        float ss = 0.0f;
#pragma unroll
        for (int s = 0; s < 16; ++s) { ss = fmaf(a0[s], a0[s], ss); ss = fmaf(a1[s], a1[s], ss); }
        ss += __shfl_xor(ss, 32);
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);                     // F.normalize(p=2, eps=1e-12)
        if (!live) return;
        if constexpr (F8) {
            // 192-byte rows: per kg four hi fragments and the 32 fp8 bytes (Q: the remainders, K: a copy of the halves)
            f16x8 *row = reinterpret_cast<f16x8 *>(reinterpret_cast<char *>(dst) + (size_t)p * 192 + h * 96);
            u32x8 q8;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const f32x16 &a = g ? a1 : a0;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int t = 2 * g + half;
                    f16x8 hi;
                    float w[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = (a[8 * half + e] * inv) * post;
                        const _Float16 hb = (_Float16)v;
                        hi[e] = hb;
                        w[e] = is_q ? v - (float)hb : (float)hb;               // what the fp8 vector carries
                    }
                    const float sc = is_q ? 1.0f / (float)(1 << F8_QL) : 1.0f / (float)(1 << F8_KH);
                    q8[2 * t] = fp8x4(w[0], w[1], w[2], w[3], sc);
                    q8[2 * t + 1] = fp8x4(w[4], w[5], w[6], w[7], sc);
                    row[t] = hi;
                }
            }
            reinterpret_cast<u32x4 *>(row)[4] = u32x4{q8[0], q8[1], q8[2], q8[3]};
            reinterpret_cast<u32x4 *>(row)[5] = u32x4{q8[4], q8[5], q8[6], q8[7]};
            return;
        }
        f16x8 *row = reinterpret_cast<f16x8 *>(dst + (size_t)p * 64);            // 16 fragments of 8 halves
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const f32x16 &a = g ? a1 : a0;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f16x8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = (a[8 * half + e] * inv) * post;                // |v| <= log2(e): far inside the half range
                    const _Float16 hb = (_Float16)v;
                    hi[e] = hb;
                    lo[e] = (_Float16)(v - (float)hb);
                }
                const int t = 2 * g + half;
                row[(h * 2 + 0) * 4 + t] = hi;
                row[(h * 2 + 1) * 4 + t] = lo;
            }
        }
    };
    float x[16];
    if (DO_Q) {
        load_x(Xq, x);
        const f32x16 q0 = project(x, 0), q1 = project(x, 1);
        store_unit(q0, q1, Qd, 1.44269504088896341f, true);
    }
    if (DO_KV) {
        if (!DO_Q || Xk != Xq) load_x(Xk, x);
        const f32x16 k0 = project(x, 2), k1 = project(x, 3);
        store_unit(k0, k1, Kd, 1.0f, false);
        const f32x16 v = project(x, 4);
        if (live) store_acc16(V + (size_t)p * 32, v, h);
    }
    }
}

// ---- streamed-tile machinery shared by the three N x N passes ---------------------------------
// A workgroup owns 256 fixed rows (one 32-row tile per wave, 8 waves) and streams ALL rows of the
// other operand through LDS in 32-row tiles, double-buffered: every streamed byte is fetched once
// per 256 fixed rows.
constexpr int FT = 512;                                     // threads per workgroup
constexpr int SROW = 68;                                    // 256-B row + 16 B pad: conflict-free ds_read_b128
constexpr int STILE = 32 * SROW;

// cooperative global -> register -> LDS copy of one 32 x 256-B tile (one 16-B piece per thread)
__device__ __forceinline__ f32x4 tile_fetch(const float *base, int row0, int N) {
    const int i = threadIdx.x;                              // piece: row = i/16, column = i%16
    return *reinterpret_cast<const f32x4 *>(base + (size_t)min(row0 + (i >> 4), N - 1) * 64 + (i & 15) * 4);
}
__device__ __forceinline__ void tile_store(float *tile, const f32x4 &t) {
    const int i = threadIdx.x;
    *reinterpret_cast<f32x4 *>(tile + (i >> 4) * SROW + (i & 15) * 4) = t;
}

// the exponent is already in base 2 (Q carries log2 e)
__device__ __forceinline__ float exp2_unit(float x) { return __builtin_amdgcn_exp2f(x); }

// out[f] = sum over streamed rows i of exp(S_i . F_f) * (w ? w[i] : 1)
//   rowsum: F = Q, S = K, w = null          colsum: F = K, S = Q, w = 1/l
template <bool STREAM_KEYS, bool FULL>
__global__ void __launch_bounds__(FT)
fusion_expsum_kernel(const float *Fd, const float *Sd, const float *w, float *out, int N, int recip_out, int nrb, int B) {
    __shared__ __attribute__((aligned(16))) float tiles[2][STILE];
    __shared__ __attribute__((aligned(16))) float wt[2][32];
    int rb, b;
    chunk_of_workgroup(nrb, B, rb, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int f0 = rb * FROWS + wave * 32;
    Fd += (size_t)b * N * 64; Sd += (size_t)b * N * 64;
    if (w) w += (size_t)b * N;
    FragQK fixed;
    load_fragqk(fixed, Fd + (size_t)min(f0 + j, N - 1) * 64, h);
    const int ntile = (N + 31) / 32;
    f32x4 tr;
    float wreg = 0.0f;
    auto fetch = [&](int t) {
        tr = tile_fetch(Sd, t * 32, N);
        if (threadIdx.x < 32) { const int i = t * 32 + threadIdx.x; wreg = (i < N) ? (w ? w[i] : 1.0f) : 0.0f; }
    };
    fetch(0);
    tile_store(tiles[0], tr);
    if (threadIdx.x < 32) wt[0][threadIdx.x] = wreg;
    __syncthreads();
    float sum = 0.0f;
    for (int t = 0; t < ntile; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntile) fetch(t + 1);
        FragQK stream;
        load_fragqk(stream, tiles[cur] + j * SROW, h);
        const f32x16 sc = score_tile<STREAM_KEYS, FULL>(stream, fixed);
        const f32x16 ww = load_acc16(wt[cur], h);               // w of streamed row chan_of(r,h)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum = fmaf(exp2_unit(sc[r]), ww[r], sum);
        if (t + 1 < ntile) {
            tile_store(tiles[cur ^ 1], tr);
            if (threadIdx.x < 32) wt[cur ^ 1][threadIdx.x] = wreg;
        }
        __syncthreads();
    }
    sum += __shfl_xor(sum, 32);
    if (lane < 32 && f0 + lane < N) out[(size_t)b * N + f0 + lane] = recip_out ? 1.0f / sum : sum;
}

// ---- the same passes on the fp8-corrected tiles (inference) ----
constexpr int SROW8 = 52;                                   // 192-B row + 16 B pad: conflict-free ds_read_b128 (13 slots per row)
constexpr int STILE8 = 32 * SROW8;
// cooperative copy of one 32 x 192-B tile: 384 16-byte pieces, threads 0..383
__device__ __forceinline__ f32x4 tile_fetch8(const float *base, int row0, int N) {
    const int i = threadIdx.x, r = i / 12, c = i - 12 * r;
    return *reinterpret_cast<const f32x4 *>(base + (size_t)min(row0 + r, N - 1) * 48 + c * 4);
}
__device__ __forceinline__ void tile_store8(float *tile, const f32x4 &t) {
    const int i = threadIdx.x, r = i / 12, c = i - 12 * r;
    *reinterpret_cast<f32x4 *>(tile + r * SROW8 + c * 4) = t;
}

// HAS_W = false: the row-sum pass (w == 1 for every streamed row): no weight tile in LDS, no multiply -- the weights were 4 of the
// 10 ds_read_b128 a wave issues per score tile, and the LDS pipe (8 cycles per 16-byte wave read, 16+ waves per CU) is the busiest
// unit of this kernel: 13.15 -> 12.59 ms per 128^3.  (Measured and not kept: two 32-row fixed tiles per wave against every streamed
// fragment -- 3 / 5 reads per score tile instead of 6 / 10 -- needs ~140 registers: at two or three waves per SIMD the per-tile
// barrier is exposed, 13.5 ms with 8-wave and with 4-wave workgroups; forced into 128 registers it spills: 13.6 ms.)
template <bool HAS_W>
__global__ void __launch_bounds__(FT)
fusion_expsum8_kernel(const float *Fd, const float *Sd, const float *w, float *out, int N, int recip_out, int nrb, int B) {
    __shared__ __attribute__((aligned(16))) float tiles[2][STILE8];
    __shared__ __attribute__((aligned(16))) float wt[32];
    int rb, b;
    chunk_of_workgroup(nrb, B, rb, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int f0 = rb * FROWS + wave * 32;
    Fd += (size_t)b * N * 48; Sd += (size_t)b * N * 48;
    if (w) w += (size_t)b * N;
    FragQK8 fixed;
    load_fragqk8(fixed, Fd + (size_t)min(f0 + j, N - 1) * 48, h);
    const int ntile = (N + 31) / 32;
    const bool mover = threadIdx.x < 384;
    f32x4 tr;
    auto fetch = [&](int t) { if (mover) tr = tile_fetch8(Sd, t * 32, N); };
    fetch(0);
    if (mover) tile_store8(tiles[0], tr);
    // a ragged LAST tile needs weights that are zero for the rows beyond N (and w, or 1, for the others): in LDS; every other tile's
    // weights (HAS_W) come straight from global memory -- 16 floats per lane, the same for all lanes of a half wave, requested
    // before the tile's score MFMAs: they were 4 of the 10 ds_read_b128 per tile on the pipe that bounds this kernel
    if (threadIdx.x < 32) { const int i = (ntile - 1) * 32 + threadIdx.x; wt[threadIdx.x] = i < N ? (w ? w[i] : 1.0f) : 0.0f; }
    __syncthreads();
    float sum = 0.0f;
    const bool ragged = (N & 31) != 0;
    for (int t = 0; t < ntile; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntile) fetch(t + 1);
        const bool last_ragged = ragged && t == ntile - 1;
        if constexpr (HAS_W) {
            f32x16 ww;
            if (!last_ragged) ww = load_acc16(w + (size_t)t * 32, h);           // w of streamed row chan_of(r,h)
            FragQK8 stream;
            load_fragqk8(stream, tiles[cur] + j * SROW8, h);
            const f32x16 sc = score_tile8(stream, fixed);
            if (last_ragged) ww = load_acc16(wt, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) sum = fmaf(exp2_unit(sc[r]), ww[r], sum);
        } else {
            FragQK8 stream;
            load_fragqk8(stream, tiles[cur] + j * SROW8, h);
            const f32x16 sc = score_tile8(stream, fixed);
            if (last_ragged) {
                const f32x16 ww = load_acc16(wt, h);
#pragma unroll
                for (int r = 0; r < 16; ++r) sum = fmaf(exp2_unit(sc[r]), ww[r], sum);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += exp2_unit(sc[r]);
            }
        }
        if (t + 1 < ntile && mover) tile_store8(tiles[cur ^ 1], tr);
        __syncthreads();
    }
    sum += __shfl_xor(sum, 32);
    if (lane < 32 && f0 + lane < N) out[(size_t)b * N + f0 + lane] = recip_out ? 1.0f / sum : sum;
}

// V' = V / (1e-9 + s) per key, split and laid out as the A operand of E x V':
// VT[b][tile][c][kg][part][k-step 2][e 8] bf16 with key = 32 tile + chan_of(8 step + e, kg) -- the
// key order of the score accumulator -- and zeros for keys >= N.  One thread per (b, tile, c, kg, step).
__global__ void __launch_bounds__(256)
fusion_scalev_kernel(const float *V, const float *s, float *VT, int N, int ntile, size_t total, int vpitch = 32, int voff = 0) {
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int step = (int)(idx & 1), kg = (int)((idx >> 1) & 1), c = (int)((idx >> 2) & 31);
        const size_t bt = idx >> 7;
        const int tile = (int)(bt % ntile);
        const size_t b = bt / ntile;
        bf16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int key = 32 * tile + chan_of(8 * step + e, kg);
            const float v = (key < N) ? V[(b * N + key) * vpitch + voff + c] / (1e-9f + s[b * N + key]) : 0.0f;
            const __bf16 hb = (__bf16)v;
            hi[e] = hb;
            lo[e] = (__bf16)(v - (float)hb);
        }
        bf16x8 *row = reinterpret_cast<bf16x8 *>(VT) + (bt * 32 + c) * 8 + kg * 4;
        row[step] = hi;
        row[2 + step] = lo;
    }
}

// The same for the fp8-corrected E x V' (inference): V' as half + remainder; per (b, tile, c, kg) 64 bytes = [hi: k-step 0, 1 x 8 halves |
// fp8: bytes j < 16 = V'_lo 2^10 of key chan_of(j, kg), bytes 16 + j = V'_hi of the same key] against E's [E_hi 2^4 | E_lo 2^14]
// (fusion_attend8_kernel), result times 2^-14.  V' beyond the half range saturates (a key no query attends to: s ~ 0).
constexpr int F8_VL = 10, F8_EH = 4, F8_EL = 14;           // V'_lo 2^10 . E_hi 2^4  and  V'_hi 2^0 . E_lo 2^14: both 2^14
__global__ void __launch_bounds__(256)
fusion_scalev8_kernel(const float *V, const float *s, float *VT, int N, int ntile, size_t total) {
    fp8_saturating_mode();
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int kg = (int)(idx & 1), c = (int)((idx >> 1) & 31);
        const size_t bt = idx >> 6;
        const int tile = (int)(bt % ntile);
        const size_t b = bt / ntile;
        float hi[16], lo[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = 32 * tile + chan_of(r, kg);
            float v = (key < N) ? V[(b * N + key) * 32 + c] / (1e-9f + s[b * N + key]) : 0.0f;
            v = fminf(fmaxf(v, -65504.0f), 65504.0f);
            const _Float16 hb = (_Float16)v;
            hi[r] = (float)hb;
            lo[r] = v - (float)hb;
        }
        // piece i of lane (c, kg) at [tile][i][c * 2 + kg]: the 64 lanes of a wave read one contiguous KB per piece (the attend kernel
        // takes its operand straight from here)
        u32x4 *row = reinterpret_cast<u32x4 *>(VT) + bt * 256 + c * 2 + kg;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            f16x8 f;
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (_Float16)hi[8 * st + e];
            row[st * 64] = __builtin_bit_cast(u32x4, f);
        }
        const float sl = 1.0f / (float)(1 << F8_VL);
        row[2 * 64] = u32x4{fp8x4(lo[0], lo[1], lo[2], lo[3], sl), fp8x4(lo[4], lo[5], lo[6], lo[7], sl),
                       fp8x4(lo[8], lo[9], lo[10], lo[11], sl), fp8x4(lo[12], lo[13], lo[14], lo[15], sl)};
        row[3 * 64] = u32x4{fp8x4(hi[0], hi[1], hi[2], hi[3], 1.0f), fp8x4(hi[4], hi[5], hi[6], hi[7], 1.0f),
                       fp8x4(hi[8], hi[9], hi[10], hi[11], 1.0f), fp8x4(hi[12], hi[13], hi[14], hi[15], 1.0f)};
    }
}

// attention output + RelationUnit tail + TransNonlinear + residual: Z = X_q + LN(...)
constexpr int VROW = 36;                                    // V' tile row: 128 B + 16 B pad
// TRAIN: the attention output O is kept for the backward and TransNonlinear's two dropouts are applied (masks: drop_mask).
// FULL: all three products of the scores (see score_tile)
// F8: the inference form on fp8-corrected tiles (score_tile8; E x V' as V'_hi E_hi on two f16 MFMAs + one fp8 MFMA for both
// correction products: fusion_scalev8_kernel)
template <bool TRAIN, bool FULL, bool F8>
__global__ void __launch_bounds__(FT)
fusion_attend_kernel(const float *Qd, const float *Kd, const float *VT, const float *linv, const float *Xq,
                     const float *blob, float *Z, int N, int ntile_, float *Osave, DropCfg dc, int nrb, int B, XIds xi, int o_pitch = 0) {
    static_assert(!(F8 && (TRAIN || FULL)), "the fp8-corrected tiles are the inference form");
    __shared__ __attribute__((aligned(16))) float lds[FU_BLOB];
    __shared__ __attribute__((aligned(16))) float tiles[2][F8 ? STILE8 : STILE];
    // (F8: V' does not go through LDS -- every lane's A operand is 64 contiguous bytes of the tile in global memory, requested a tile
    // ahead: the LDS pipe, which the score tiles' fragments keep as busy as the matrix pipe, loses 4 of its 10 reads per tile)
    __shared__ __attribute__((aligned(16))) float vts[2][F8 ? 4 : 32 * VROW];
    for (int i = threadIdx.x; i < FU_BLOB; i += FT) lds[i] = blob[i];
    if constexpr (F8) fp8_saturating_mode();
    int rb, b;
    chunk_of_workgroup(nrb, B, rb, b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int q0 = rb * FROWS + wave * 32;
    const int ntile = ntile_;
    constexpr int RS = F8 ? 48 : 64;                                     // floats per Q / K row
    Qd += (size_t)b * N * RS; Kd += (size_t)b * N * RS; VT += (size_t)b * ntile * 1024;
    typename std::conditional<F8, FragQK8, FragQK>::type fixed;
    if constexpr (F8) load_fragqk8(fixed, Qd + (size_t)min(q0 + j, N - 1) * RS, h);
    else load_fragqk(fixed, Qd + (size_t)min(q0 + j, N - 1) * RS, h);
    f32x16 o;
#pragma unroll
    for (int s = 0; s < 16; ++s) o[s] = 0.0f;
    f32x4 tr, vreg;
    const int vc = (threadIdx.x & 255) >> 3, vk = (threadIdx.x & 7) * 4;   // V' tile piece: channel row, 16-B column
    const bool mover = !F8 || threadIdx.x < 384;
    auto fetch = [&](int t) {
        if constexpr (F8) { if (mover) tr = tile_fetch8(Kd, t * 32, N); }
        else {
            tr = tile_fetch(Kd, t * 32, N);
            if (threadIdx.x < 256) vreg = *reinterpret_cast<const f32x4 *>(VT + (size_t)t * 1024 + threadIdx.x * 4);
        }
    };
    auto put = [&](int buf) {
        if constexpr (F8) { if (mover) tile_store8(tiles[buf], tr); }
        else {
            tile_store(tiles[buf], tr);
            if (threadIdx.x < 256) *reinterpret_cast<f32x4 *>(vts[buf] + vc * VROW + vk) = vreg;
        }
    };
    // F8: lane (channel j, k-group h)'s V' operand of tile t: [hi k-step 0 | hi k-step 1 | fp8 32 B]
    u32x4 vq[4];
    auto vload = [&](int t) {
        const u32x4 *g = reinterpret_cast<const u32x4 *>(VT + (size_t)t * 1024) + j * 2 + h;
#pragma unroll
        for (int i = 0; i < 4; ++i) vq[i] = g[i * 64];
    };
    fetch(0);
    if constexpr (F8) vload(0);
    put(0);
    __syncthreads();
    const float m1 = opaque_minus_one();
    for (int t = 0; t < ntile; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntile) fetch(t + 1);
        if constexpr (F8) {
            FragQK8 stream;
            load_fragqk8(stream, tiles[cur] + j * SROW8, h);
            f32x16 e = score_tile8(stream, fixed);                          // lane (q,h) reg r: key 32t+chan_of(r,h)
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = exp2_unit(e[r]);
            // E = E_hi (halves, round toward zero) + E_lo; fp8 copies [E_hi 2^4 | E_lo 2^14] for the correction MFMA
            u32x4 eh[2];
            u32x8 eq;
#pragma unroll
            for (int p = 0; p < 8; p += 2) {
                const unsigned ha = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(e[2 * p], e[2 * p + 1]));
                const unsigned hb = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(e[2 * p + 2], e[2 * p + 3]));
                eh[p >> 2][p & 3] = ha;
                eh[p >> 2][(p & 3) + 1] = hb;
                const f16x2 fa = __builtin_bit_cast(f16x2, ha), fb = __builtin_bit_cast(f16x2, hb);
                const float l0 = __builtin_fmaf((float)fa[0], m1, e[2 * p]), l1 = __builtin_fmaf((float)fa[1], m1, e[2 * p + 1]);
                const float l2 = __builtin_fmaf((float)fb[0], m1, e[2 * p + 2]), l3 = __builtin_fmaf((float)fb[1], m1, e[2 * p + 3]);
                i16x2 w;
                asm volatile("" : "=v"(w));
                w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(w, fa, 1.0f / (float)(1 << F8_EH), false);
                w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(w, fb, 1.0f / (float)(1 << F8_EH), true);
                eq[p >> 1] = __builtin_bit_cast(unsigned, w);
                eq[4 + (p >> 1)] = fp8x4(l0, l1, l2, l3, 1.0f / (float)(1 << F8_EL));
            }
            // O^T[c][q] += V'[c][k] E[k][q]: A operand lane (c,kg): [hi k-step 0 | hi k-step 1 | fp8 32 B]
            const u32x4 v2 = vq[2], v3 = vq[3];
            o = mfma_s(__builtin_bit_cast(f16x8, vq[0]), __builtin_bit_cast(f16x8, eh[0]), o);
            o = mfma_s(__builtin_bit_cast(f16x8, vq[1]), __builtin_bit_cast(f16x8, eh[1]), o);
            o = mfma_f8<F8_EL>(u32x8{v2[0], v2[1], v2[2], v2[3], v3[0], v3[1], v3[2], v3[3]}, eq, o);
            if (t + 1 < ntile) vload(t + 1);
        } else {
        FragQK stream;
        load_fragqk(stream, tiles[cur] + j * SROW, h);
        f32x16 e = score_tile<true, FULL>(stream, fixed);                  // lane (q,h) reg r: key 32t+chan_of(r,h)
#pragma unroll
        for (int r = 0; r < 16; ++r) e[r] = exp2_unit(e[r]);
        const Split16 es = split16<false>(e);
        // O^T[c][q] += V'[c][k] E[k][q]: A operand lane (c,kg), step s = keys chan_of(8s+e, kg)
        const bf16x8 *vp = reinterpret_cast<const bf16x8 *>(vts[cur] + j * VROW) + h * 4;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 vh = vp[s], vl = vp[2 + s];
            o = mfma16(vl, es.hi[s], o);
            o = mfma16(vh, es.lo[s], o);
            o = mfma16(vh, es.hi[s], o);
        }
        }
        if (t + 1 < ntile) put(cur ^ 1);
        __syncthreads();
    }
    const int q = min(q0 + j, N - 1);
    const float li = linv[(size_t)b * N + q];
#pragma unroll
    for (int s = 0; s < 16; ++s) o[s] *= li;
    if (o_pitch > 0) {          // d_model beyond 32: this launch is one 32-channel slice of V'; leave the attention output, no epilogue
        if (q0 + j < N) store_acc16(Osave + ((size_t)b * N + q0 + j) * o_pitch, o, h);
        return;
    }
    // lane (q,h) reg r = channel chan_of(r,h) of the attention output: the accumulator layout
    const float *xrow = Xq ? Xq + ((size_t)b * N + q) * 32 : xi.row((size_t)b * N + q);
    const f32x16 x = load_acc16(xrow, h);
    const uint32_t pt = (uint32_t)((size_t)b * N + q);
    if (TRAIN && q0 + j < N) store_acc16(Osave + (size_t)pt * 32, o, h);
    f32x16 d = x - o;
    f32x16 r;
#pragma unroll
    for (int s = 0; s < 16; ++s) r[s] = 0.0f;
    r = dense32<false>(r, lds + FU_WT, d, lane);
    r = relu16(r);                                               // relu(trans_conv(q - out))
    f32x16 ha = load_frag16(lds + FU_BIAS + 0 * 32 + h * 16), hb = load_frag16(lds + FU_BIAS + 1 * 32 + h * 16);
    ha = dense32<false>(ha, lds + FU_W1A, r, lane);
    hb = dense32<false>(hb, lds + FU_W1B, r, lane);
    f32x16 t2 = load_frag16(lds + FU_BIAS + 2 * 32 + h * 16);
    if (TRAIN) {
        ha = drop16(relu16(ha), dc, 0, pt, h, 0);
        hb = drop16(relu16(hb), dc, 0, pt, h, 32);
        t2 = dense32<false>(t2, lds + FU_W2A, ha, lane);
        t2 = dense32<false>(t2, lds + FU_W2B, hb, lane);
        t2 = drop16(t2, dc, 1, pt, h, 0);
    } else {
        t2 = dense32<true>(t2, lds + FU_W2A, ha, lane);
        t2 = dense32<true>(t2, lds + FU_W2B, hb, lane);
    }
    t2 = t2 + r;
    // LayerNorm over the 32 channels of this point (16 registers x 2 lane halves)
    float m = 0.0f;
#pragma unroll
    for (int s = 0; s < 16; ++s) m += t2[s];
    m += __shfl_xor(m, 32);
    m *= (1.0f / 32.0f);
    float var = 0.0f;
#pragma unroll
    for (int s = 0; s < 16; ++s) { const float c = t2[s] - m; var = fmaf(c, c, var); }
    var += __shfl_xor(var, 32);
    const float rstd = 1.0f / sqrtf(var * (1.0f / 32.0f) + 1e-5f);
    const f32x16 ga = load_frag16(lds + FU_BIAS + 3 * 32 + h * 16), be = load_frag16(lds + FU_BIAS + 4 * 32 + h * 16);
    f32x16 z;
#pragma unroll
    for (int s = 0; s < 16; ++s) z[s] = x[s] + ((t2[s] - m) * rstd * ga[s] + be[s]);
    if (q0 + j < N) store_acc16(Z + ((size_t)b * N + q0 + j) * 32, z, h);
}

// out = relu((z - mean_N) / sqrt(var_N + 1e-5)) per (scene, channel); one block per scene
__global__ void __launch_bounds__(1024)
fusion_inorm_relu_kernel(const float *Z, float *out, int N, int pitch = 32) {
    __shared__ float red[32][33];
    __shared__ float mean[32], rstd[32];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;        // 32 row groups; blockIdx.y: the 32-channel slice of a wider row
    const float *z = Z + (size_t)blockIdx.x * N * pitch + blockIdx.y * 32;
    float *o = out + (size_t)blockIdx.x * N * pitch + blockIdx.y * 32;
    // mean = z_0 + mean(z - z_0): a channel that is constant over the chunk (an untouched chunk's tactile branch: all-zero
    // inputs give every point the same vector) then has residuals of exactly 0 instead of the rounding noise of a 2048-term
    // sum, which 1/sqrt(0 + 1e-5) would multiply by 316
    const float shift = z[c];
    float s = 0.0f;
    for (int n = g; n < N; n += 32) s += z[(size_t)n * pitch + c] - shift;
    red[g][c] = s;
    __syncthreads();
    if (threadIdx.x < 32) {
        float t = 0.0f;
        for (int i = 0; i < 32; ++i) t += red[i][threadIdx.x];
        mean[threadIdx.x] = z[threadIdx.x] + t / (float)N;
    }
    __syncthreads();
    const float m = mean[c];
    s = 0.0f;
    for (int n = g; n < N; n += 32) { const float d = z[(size_t)n * pitch + c] - m; s = fmaf(d, d, s); }
    __syncthreads();
    red[g][c] = s;
    __syncthreads();
    if (threadIdx.x < 32) {
        float t = 0.0f;
        for (int i = 0; i < 32; ++i) t += red[i][threadIdx.x];
        rstd[threadIdx.x] = 1.0f / sqrtf(t / (float)N + 1e-5f);
    }
    __syncthreads();
    const float rs = rstd[c];
    for (int n = g; n < N; n += 32) o[(size_t)n * pitch + c] = fmaxf((z[(size_t)n * pitch + c] - m) * rs, 0.0f);
}

// The same for chunks of at most 2048 points (the reference's chunk size): a thread keeps its 16 x 4 values in registers --
// one read of z instead of three; thread = (row group of 128, channel quad), 16-byte accesses.
__global__ void __launch_bounds__(1024)
fusion_inorm_relu_cached_kernel(const float *Z, float *out, int N) {
    __shared__ float red[16][32];
    __shared__ float stat[32];
    const int q = threadIdx.x & 7, g = threadIdx.x >> 3, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *z = Z + (size_t)blockIdx.x * N * 32 + q * 4;
    float *o = out + (size_t)blockIdx.x * N * 32 + q * 4;
    f32x4 v[IN_ROWS];
#pragma unroll
    for (int k = 0; k < IN_ROWS; ++k) {
        const int n = g + 128 * k;
        v[k] = n < N ? *reinterpret_cast<const f32x4 *>(z + (size_t)n * 32) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const f32x4 shift = *reinterpret_cast<const f32x4 *>(z);                 // row 0 (see the kernel above)
    // sum over the chunk of one f32x4 per thread: lanes q, q+8, .. of a wave, then the 16 waves
    auto chunk_sum = [&](f32x4 t) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { t[e] += __shfl_xor(t[e], 8); t[e] += __shfl_xor(t[e], 16); t[e] += __shfl_xor(t[e], 32); }
        __syncthreads();                                                     // (the previous round's readers are done)
        if (lane < 8) *reinterpret_cast<f32x4 *>(&red[wave][lane * 4]) = t;
        __syncthreads();
        if (threadIdx.x < 32) {
            float a = 0.0f;
            for (int w = 0; w < 16; ++w) a += red[w][threadIdx.x];
            stat[threadIdx.x] = a;
        }
        __syncthreads();
        return *reinterpret_cast<const f32x4 *>(&stat[q * 4]);
    };
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < IN_ROWS; ++k) if (g + 128 * k < N) acc += v[k] - shift;
    const f32x4 m = shift + chunk_sum(acc) / (float)N;
    acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < IN_ROWS; ++k)
        if (g + 128 * k < N) { const f32x4 d = v[k] - m; for (int e = 0; e < 4; ++e) acc[e] = fmaf(d[e], d[e], acc[e]); }
    const f32x4 var = chunk_sum(acc) / (float)N;
    f32x4 rs;
#pragma unroll
    for (int e = 0; e < 4; ++e) rs[e] = 1.0f / sqrtf(var[e] + 1e-5f);
#pragma unroll
    for (int k = 0; k < IN_ROWS; ++k) {
        const int n = g + 128 * k;
        if (n < N) {
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = fmaxf((v[k][e] - m[e]) * rs[e], 0.0f);
            *reinterpret_cast<f32x4 *>(o + (size_t)n * 32) = r;
        }
    }
}

struct FusionWs {
    float *Qd, *Kd, *V, *VT, *l, *s, *Z, *M, *T, *blob_s, *blob_x;
};

size_t fusion_layout(int B, int N, FusionWs *ws, char *base) {
    const size_t P = (size_t)B * N, Npad = (size_t)(N + 31) / 32 * 32;
    size_t off = 0;
    auto take = [&](size_t floats) { float *p = base ? (float *)(base + off) : nullptr; off += (floats * 4 + 255) / 256 * 256; return p; };
    float *Qd = take(P * 64), *Kd = take(P * 64), *V = take(P * 32), *VT = take((size_t)B * 32 * Npad);
    float *l = take(P), *s = take(P), *Z = take(P * 32), *M = take(P * 32), *T = take(P * 32);
    float *bs = take(FU_BLOB), *bx = take(FU_BLOB);
    if (ws) *ws = FusionWs{Qd, Kd, V, VT, l, s, Z, M, T, bs, bx};
    return off;
}

// one attention unit: Xq against Xk -> out = relu(IN(Xq + MHA(Xq, Xk, Xk))).  ``Osave`` != null: training forward (w.l / w.s /
// w.V / w.Z then point into the caller's saved state instead of the scratch workspace, and the dropouts of ``dc`` are applied)
void run_unit(const float *Xq, const float *Xk, const FusionUnitDev &u, const float *blob, const FusionWs &w,
              float *out, int B, int N, hipStream_t s, float *Osave = nullptr, DropCfg dc = DropCfg{0, 0, 1.0f, 0, 6}, XIds xi = XIds{}) {
    const int P = B * N;
    // the score form and every launch shape: fusion_plan (fusion_common.h), the rule vt_fusion_plan reports
    const FusionPlan f = fusion_plan(B, N, 32, Osave != nullptr);
    const int ntile = f.ntile, nrb = f.nrb, tiles = f.proj_tiles;
    const dim3 pg(f.proj_grid), tg((unsigned)nrb * (unsigned)B);   // see chunk_of_workgroup
    const bool full = f.form == VT_FUSION_FORM_FULL, f8 = f.form == VT_FUSION_FORM_F8;
    if (Xq == Xk) {
        if (f8) hipLaunchKernelGGL((fusion_proj_kernel<true, true, true>), pg, dim3(256), 0, s, Xq, Xk, u, w.Qd, w.Kd, w.V, P, xi, tiles);
        else hipLaunchKernelGGL((fusion_proj_kernel<true, true, false>), pg, dim3(256), 0, s, Xq, Xk, u, w.Qd, w.Kd, w.V, P, xi, tiles);
    } else if (f8) {
        hipLaunchKernelGGL((fusion_proj_kernel<true, false, true>), pg, dim3(256), 0, s, Xq, Xk, u, w.Qd, w.Kd, w.V, P, xi, tiles);
        hipLaunchKernelGGL((fusion_proj_kernel<false, true, true>), pg, dim3(256), 0, s, Xq, Xk, u, w.Qd, w.Kd, w.V, P, xi, tiles);
    } else {
        hipLaunchKernelGGL((fusion_proj_kernel<true, false, false>), pg, dim3(256), 0, s, Xq, Xk, u, w.Qd, w.Kd, w.V, P, xi, tiles);
        hipLaunchKernelGGL((fusion_proj_kernel<false, true, false>), pg, dim3(256), 0, s, Xq, Xk, u, w.Qd, w.Kd, w.V, P, xi, tiles);
    }
    if (f8) {
        hipLaunchKernelGGL(fusion_expsum8_kernel<false>, tg, dim3(FT), 0, s, w.Qd, w.Kd, (const float *)nullptr, w.l, N, 1, nrb, B);                // 1/l_q
        hipLaunchKernelGGL(fusion_expsum8_kernel<true>, tg, dim3(FT), 0, s, w.Kd, w.Qd, (const float *)w.l, w.s, N, 0, nrb, B);                    // s_k
    } else if (full) {
        hipLaunchKernelGGL((fusion_expsum_kernel<true, true>), tg, dim3(FT), 0, s, w.Qd, w.Kd, (const float *)nullptr, w.l, N, 1, nrb, B);
        hipLaunchKernelGGL((fusion_expsum_kernel<false, true>), tg, dim3(FT), 0, s, w.Kd, w.Qd, (const float *)w.l, w.s, N, 0, nrb, B);
    } else {
        hipLaunchKernelGGL((fusion_expsum_kernel<true, false>), tg, dim3(FT), 0, s, w.Qd, w.Kd, (const float *)nullptr, w.l, N, 1, nrb, B);
        hipLaunchKernelGGL((fusion_expsum_kernel<false, false>), tg, dim3(FT), 0, s, w.Kd, w.Qd, (const float *)w.l, w.s, N, 0, nrb, B);
    }
    if (f8) hipLaunchKernelGGL(fusion_scalev8_kernel, dim3(f.scalev_grid), dim3(256), 0, s, w.V, w.s, w.VT, N, ntile, f.scalev_items);
    else hipLaunchKernelGGL(fusion_scalev_kernel, dim3(f.scalev_grid), dim3(256), 0, s, w.V, w.s, w.VT, N, ntile, f.scalev_items);
    if (Osave)
        hipLaunchKernelGGL((fusion_attend_kernel<true, true, false>), tg, dim3(FT), 0, s, w.Qd, w.Kd, w.VT, w.l, Xq, blob, w.Z, N, ntile, Osave, dc, nrb, B, xi);
    else if (full)
        hipLaunchKernelGGL((fusion_attend_kernel<false, true, false>), tg, dim3(FT), 0, s, w.Qd, w.Kd, w.VT, w.l, Xq, blob, w.Z, N, ntile, Osave, dc, nrb, B, xi);
    else if (f8)
        hipLaunchKernelGGL((fusion_attend_kernel<false, false, true>), tg, dim3(FT), 0, s, w.Qd, w.Kd, w.VT, w.l, Xq, blob, w.Z, N, ntile, Osave, dc, nrb, B, xi);
    else
        hipLaunchKernelGGL((fusion_attend_kernel<false, false, false>), tg, dim3(FT), 0, s, w.Qd, w.Kd, w.VT, w.l, Xq, blob, w.Z, N, ntile, Osave, dc, nrb, B, xi);
    if (!f.inorm_streamed) hipLaunchKernelGGL(fusion_inorm_relu_cached_kernel, dim3(B), dim3(1024), 0, s, w.Z, out, N);
    else hipLaunchKernelGGL(fusion_inorm_relu_kernel, dim3(B), dim3(1024), 0, s, w.Z, out, N);
}


// ---- TransformerFusion at d_model = C beyond 32 (64, 96, 128: the reference's AttentionDecoder defaults to c_dim 128, ----------------
// decoder.py:176-207).  The N x N passes depend on d_model only through V: the scores take the same 64-dim split Q / K rows, so the
// exp-sum kernels run unchanged (all three half products: the form the training forward uses), and the attend kernel runs once per
// 32-channel slice of V' and leaves the attention output (o_pitch) instead of chaining into the 32-wide epilogue.  Around them:
//   fusionw_proj_kernel      Q, K rows in the passes' split format, V [P][C]: f32 MFMA, the weights staged in LDS in fragment order
//   fusionw_epilogue_kernel  z = x + LN(r + linear2(relu(linear1(r)))), r = relu(trans_conv(x - o)): f32 MFMA, 32 points per workgroup
//   fusion_inorm_relu_kernel InstanceNorm over the chunk + ReLU per (chunk, 32-channel slice)
// Eval mode only (the generator's path); exact f32 outside the score / E x V' products.
constexpr int FW_MAX = 128;

template <int C>
__global__ void __launch_bounds__(256)
fusionw_proj_kernel(const float *Xq, const float *Xk, FusionUnitDev u, float *Qd, float *Kd, float *V, int total, int do_q, int do_kv) {
    constexpr int KS = C / 2, NV = C / 32;                           // k-steps of the 32x32x2 MFMA; 32-row blocks of V
    extern __shared__ __attribute__((aligned(16))) float fw_wf[];   // [4 + NV groups][KS][64 lanes] A fragments
    for (int e = threadIdx.x; e < (4 + NV) * KS * 64; e += 256) {
        const int l = e & 63, st = (e >> 6) % KS, g = e / (64 * KS), i = l & 31, kk = l >> 5, k = 2 * st + kk;
        const int hh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3);    // output row i <-> accumulator register r of lane half hh
        float v = 0.0f;
        if (g < 4) {
            const int gg = g & 1, col = 16 * (2 * gg + (r >> 3)) + 8 * hh + (r & 7);
            if (g < 2 ? do_q : do_kv) v = (g < 2 ? u.WQ : u.WK)[col * C + k];
        } else if (do_kv) {
            v = u.WV[(32 * (g - 4) + i) * C + k];
        }
        fw_wf[e] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    for (int tile = 0; tile < PROJ_TILES; ++tile) {
        const int p0 = ((blockIdx.x * PROJ_TILES + tile) * 4 + wave) * 32;
        if (p0 >= total) return;
        const int p = min(p0 + j, total - 1);
        const bool live = p0 + j < total;
        float x[KS];
        auto load_x = [&](const float *X) {                          // x[s] = X[p][2 s + h]
            const f32x4 *r = reinterpret_cast<const f32x4 *>(X + (size_t)p * C);
#pragma unroll
            for (int i = 0; i < C / 4; ++i) {
                const f32x4 t = r[i];
                x[2 * i] = h ? t.y : t.x;
                x[2 * i + 1] = h ? t.w : t.z;
            }
        };
        auto project = [&](int g) {
            f32x16 acc;
#pragma unroll
            for (int s = 0; s < 16; ++s) acc[s] = 0.0f;
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = mfma(fw_wf[(g * KS + s) * 64 + lane], x[s], acc);
            return acc;
        };
        auto store_unit = [&](const f32x16 &a0, const f32x16 &a1, float *dst, float post) {
            float ss = 0.0f;
#pragma unroll
            for (int s = 0; s < 16; ++s) { ss = fmaf(a0[s], a0[s], ss); ss = fmaf(a1[s], a1[s], ss); }
            ss += __shfl_xor(ss, 32);
            const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);                     // F.normalize(p=2, eps=1e-12)
            if (!live) return;
            f16x8 *row = reinterpret_cast<f16x8 *>(dst + (size_t)p * 64);            // 16 fragments of 8 halves (fusion_proj_kernel's rows)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const f32x16 &a = g ? a1 : a0;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    f16x8 hi, lo;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = (a[8 * half + e] * inv) * post;
                        const _Float16 hb = (_Float16)v;
                        hi[e] = hb;
                        lo[e] = (_Float16)(v - (float)hb);
                    }
                    const int t = 2 * g + half;
                    row[(h * 2 + 0) * 4 + t] = hi;
                    row[(h * 2 + 1) * 4 + t] = lo;
                }
            }
        };
        if (do_q) {
            load_x(Xq);
            const f32x16 q0 = project(0), q1 = project(1);
            store_unit(q0, q1, Qd, 1.44269504088896341f);
        }
        if (do_kv) {
            if (!do_q || Xk != Xq) load_x(Xk);
            const f32x16 k0 = project(2), k1 = project(3);
            store_unit(k0, k1, Kd, 1.0f);
#pragma unroll
            for (int vb = 0; vb < NV; ++vb) {
                const f32x16 v = project(4 + vb);
                if (live) store_acc16(V + (size_t)p * C + 32 * vb, v, h);
            }
        }
    }
}

// W [H][K] -> fragments [H/32][K/8][64 lanes][4]: lane (row r = l & 31, kg = l >> 5), element e = W[32 ob + r][8 kq + 2 e + kg] -- the A
// operands of four consecutive 32x32x2 k-steps (the layout of decode_wide.hip's weight stream)
__global__ void fusionw_pack_kernel(const float *w, int H, int K, float *dst) {
    const size_t total = (size_t)H * K;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < total; f += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(f & 3), l = (int)((f >> 2) & 63);
        const size_t q = f >> 8;
        const int kq = (int)(q % (K / 8)), ob = (int)(q / (K / 8));
        dst[f] = w[(size_t)(32 * ob + (l & 31)) * K + 8 * kq + 2 * e + (l >> 5)];
    }
}
constexpr int FW_PITCH = 33;
// acc += W[32 rows of block ob][K] . X[K][32 points]; wf: the layer's fragments, x: LDS [K][FW_PITCH]
__device__ __forceinline__ f32x16 fusionw_gemm(f32x16 acc, const float *wf, int ob, int K, const float *x, int lane) {
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(wf) + (size_t)ob * (K / 8) * 64 + lane;
    const float *xb = x + (lane >> 5) * FW_PITCH + (lane & 31);
    for (int kq = 0; kq < K / 8; ++kq) {
        const f32x4 a = w4[(size_t)kq * 64];
        const float *xr = xb + kq * 8 * FW_PITCH;
        acc = mfma(a.x, xr[0], acc);
        acc = mfma(a.y, xr[2 * FW_PITCH], acc);
        acc = mfma(a.z, xr[4 * FW_PITCH], acc);
        acc = mfma(a.w, xr[6 * FW_PITCH], acc);
    }
    return acc;
}
struct FusionwEpi { const float *wt, *w1, *w2, *b1, *b2, *lnw, *lnb; };     // packed fragments (wt [C][C], w1 [64][C], w2 [C][64]) and f32 vectors
// z[p] = x[p] + LayerNorm(r + linear2(relu(linear1(r))))  with  r = relu(trans_conv(x[p] - o[p]))   (TransformerFusion.py:21-25, 110-113)
// C / 32 waves, 32 points per tile; wave ob owns the output rows 32 ob .. 32 ob + 31, waves 0 and 1 the 64 hidden rows of linear1
template <int C>
__global__ void __launch_bounds__(C * 2)
fusionw_epilogue_kernel(const float *X, const float *O, FusionwEpi e, float *Z, int total, DropCfg dc) {
    constexpr int NW = C / 32;
    __shared__ float bufD[C * FW_PITCH], bufR[C * FW_PITCH], bufH[64 * FW_PITCH], red[2][NW][32];
    const int tid = threadIdx.x, lane = tid & 63, ob = tid >> 6, j = lane & 31, kg = lane >> 5;
    const int ntiles = (total + 31) / 32;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int i = tid; i < 32 * C; i += C * 2) {                  // d = x - o, channel-major [c][pt]
            const int pt = i / C, c = i - pt * C;
            const int p = min(tile * 32 + pt, total - 1);
            bufD[c * FW_PITCH + pt] = X[(size_t)p * C + c] - O[(size_t)p * C + c];
        }
        __syncthreads();
        f32x16 r;
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = 0.0f;
        r = relu16(fusionw_gemm(r, e.wt, ob, C, bufD, lane));
#pragma unroll
        for (int i = 0; i < 16; ++i) bufR[(32 * ob + chan_of(i, kg)) * FW_PITCH + j] = r[i];
        __syncthreads();
        if (ob < 2) {
            f32x16 hd;
#pragma unroll
            for (int i = 0; i < 16; ++i) hd[i] = e.b1[32 * ob + chan_of(i, kg)];
            hd = relu16(fusionw_gemm(hd, e.w1, ob, C, bufR, lane));
            const uint32_t pd = (uint32_t)min(tile * 32 + j, total - 1);           // TransNonlinear's dropout on relu(linear1), train mode
#pragma unroll
            for (int i = 0; i < 16; ++i) bufH[(32 * ob + chan_of(i, kg)) * FW_PITCH + j] = hd[i] * drop_mask(dc, 0, pd, (uint32_t)(32 * ob + chan_of(i, kg)));
        }
        __syncthreads();
        f32x16 t;
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = e.b2[32 * ob + chan_of(i, kg)];
        t = fusionw_gemm(t, e.w2, ob, 64, bufH, lane);
        {
            const uint32_t pd = (uint32_t)min(tile * 32 + j, total - 1);           // ... and dropout2 on linear2's output
#pragma unroll
            for (int i = 0; i < 16; ++i) t[i] = fmaf(t[i], drop_mask(dc, 1, pd, (uint32_t)(32 * ob + chan_of(i, kg))), r[i]);
        }
        // LayerNorm over the C channels of a point: this wave's 32 (16 registers x 2 lane halves), then the waves' sums through LDS
        float m = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) m += t[i];
        m += __shfl_xor(m, 32);
        if (kg == 0) red[0][ob][j] = m;
        __syncthreads();
        m = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) m += red[0][w][j];
        m *= 1.0f / (float)C;
        float var = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { const float c = t[i] - m; var = fmaf(c, c, var); }
        var += __shfl_xor(var, 32);
        if (kg == 0) red[1][ob][j] = var;
        __syncthreads();
        var = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) var += red[1][w][j];
        const float rstd = 1.0f / sqrtf(var * (1.0f / (float)C) + 1e-5f);
        const int p = tile * 32 + j;
        if (p < total) {
            const f32x16 x = load_acc16(X + (size_t)p * C + 32 * ob, kg);
            f32x16 z;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ch = 32 * ob + chan_of(i, kg);
                z[i] = x[i] + ((t[i] - m) * rstd * e.lnw[ch] + e.lnb[ch]);
            }
            store_acc16(Z + (size_t)p * C + 32 * ob, z, kg);
        }
        __syncthreads();                                              // the buffers and `red` are free again
    }
}

struct FusionwWs {
    float *Qd, *Kd, *V, *VT, *l, *s, *O, *Z, *M, *T, *blob;        // blob: the 32-wide attend kernel's (unused) epilogue image
    float *pk[2];                                                   // per unit: packed wt | w1 | w2
};
size_t fusionw_layout(int B, int N, int C, FusionwWs *ws, char *base) {
    const size_t P = (size_t)B * N, Npad = (size_t)(N + 31) / 32 * 32;
    size_t off = 0;
    auto take = [&](size_t floats) { float *p = base ? (float *)(base + off) : nullptr; off += (floats * 4 + 255) / 256 * 256; return p; };
    FusionwWs w;
    w.Qd = take(P * 64); w.Kd = take(P * 64); w.V = take(P * C); w.VT = take((size_t)B * 32 * Npad);
    w.l = take(P); w.s = take(P); w.O = take(P * C); w.Z = take(P * C); w.M = take(P * C); w.T = take(P * C);
    w.blob = take(FU_BLOB);
    for (int k = 0; k < 2; ++k) w.pk[k] = take((size_t)C * C + 2 * 64 * (size_t)C);
    if (ws) *ws = w;
    return off;
}

template <int C>
void run_unit_wide(const float *Xq, const float *Xk, const FusionUnitDev &u, const float *pk, const FusionwWs &w, float *out, int B, int N, hipStream_t s,
                   DropCfg dc = DropCfg{0, 0, 1.0f, 0, 8}) {
    const int P = B * N;
    const FusionPlan f = fusion_plan(B, N, C, false);               // (all three half products whether a backward follows or not)
    const int ntile = f.ntile, nrb = f.nrb;
    const dim3 pg(f.proj_grid), tg((unsigned)nrb * (unsigned)B);
    const size_t plds = (size_t)(4 + C / 32) * (C / 2) * 64 * sizeof(float);
    hipLaunchKernelGGL(fusionw_proj_kernel<C>, pg, dim3(256), plds, s, Xq, Xk, u, w.Qd, w.Kd, w.V, P, 1, 1);
    hipLaunchKernelGGL((fusion_expsum_kernel<true, true>), tg, dim3(FT), 0, s, w.Qd, w.Kd, (const float *)nullptr, w.l, N, 1, nrb, B);
    hipLaunchKernelGGL((fusion_expsum_kernel<false, true>), tg, dim3(FT), 0, s, w.Kd, w.Qd, (const float *)w.l, w.s, N, 0, nrb, B);
    for (int sl = 0; sl < C / 32; ++sl) {                            // the attention output, one 32-channel slice of V' at a time
        hipLaunchKernelGGL(fusion_scalev_kernel, dim3(f.scalev_grid), dim3(256), 0, s, w.V, w.s, w.VT, N, ntile, f.scalev_items, C, 32 * sl);
        hipLaunchKernelGGL((fusion_attend_kernel<false, true, false>), tg, dim3(FT), 0, s, w.Qd, w.Kd, w.VT, w.l, Xq, w.blob, w.Z, N, ntile,
                           w.O + 32 * sl, DropCfg{0, 0, 1.0f, 0, 6}, nrb, B, XIds{}, C);
    }
    FusionwEpi e{pk, pk + (size_t)C * C, pk + (size_t)C * C + 64 * (size_t)C, u.l1b, u.l2b, u.lnw, u.lnb};
    hipLaunchKernelGGL(fusionw_epilogue_kernel<C>, dim3(f.epilogue_grid), dim3(C * 2), 0, s, Xq, w.O, e, w.Z, P, dc);
    hipLaunchKernelGGL(fusion_inorm_relu_kernel, dim3(B, C / 32), dim3(1024), 0, s, w.Z, out, N, C);
}

template <int C>
int fusion_fwd_wide(const float *c_img, const float *c, int B, int N, const vt_fusion_params *p, void *workspace, size_t workspace_bytes,
                    float *out, hipStream_t s) {
    FusionwWs w;
    if (workspace_bytes < fusionw_layout(B, N, C, &w, (char *)workspace)) return vt_fail(VT_ERR_WORKSPACE, "vt_fusion_fwd: workspace too small");
    hipError_t e = vt_max_dyn_lds(reinterpret_cast<const void *>(&fusionw_proj_kernel<C>), 160 * 1024);
    if (e != hipSuccess) return vt_check(e, "vt_fusion_fwd: hipFuncSetAttribute");
    const FusionUnitDev us = unit_of(p->self_attn), ux = unit_of(p->cross_attn);
    hipLaunchKernelGGL(fusion_pack_kernel, dim3(6), dim3(1024), 0, s, us, w.blob);          // (any valid image: the slices return before using it)
    for (int k = 0; k < 2; ++k) {
        const FusionUnitDev &u = k ? ux : us;
        hipLaunchKernelGGL(fusionw_pack_kernel, dim3(64), dim3(256), 0, s, u.Wt, C, C, w.pk[k]);
        hipLaunchKernelGGL(fusionw_pack_kernel, dim3(32), dim3(256), 0, s, u.l1w, 64, C, w.pk[k] + (size_t)C * C);
        hipLaunchKernelGGL(fusionw_pack_kernel, dim3(32), dim3(256), 0, s, u.l2w, C, 64, w.pk[k] + (size_t)C * C + 64 * (size_t)C);
    }
    run_unit_wide<C>(c, c, us, w.pk[0], w, w.M, B, N, s);              // encoder: memory from the grid features
    run_unit_wide<C>(c_img, c_img, us, w.pk[0], w, w.T, B, N, s);      // decoder self-attention (SAME weights)
    run_unit_wide<C>(w.T, w.M, ux, w.pk[1], w, out, B, N, s);          // decoder cross-attention
    return vt_check(hipGetLastError(), "vt_fusion_fwd");
}

// the training forward at d_model C > 32: the same launches with TransNonlinear's dropouts and with the O(N) state the backward needs
// (1 / l, s, V, O, Z per attention call; the two inner results) written into the caller's saved buffer instead of the scratch workspace
template <int C>
int fusion_fwd_train_wide(const float *c_img, const float *c, int B, int N, const vt_fusion_params *p, float p_drop, unsigned long long seed,
                          void *workspace, size_t workspace_bytes, void *saved, size_t saved_bytes, float *out, hipStream_t s) {
    FusionwWs w;
    FusionSaved sv;
    if (workspace_bytes < fusionw_layout(B, N, C, &w, (char *)workspace)) return vt_fail(VT_ERR_WORKSPACE, "vt_fusion_fwd_train: workspace too small");
    if (saved_bytes < fusion_saved_layout(B, N, &sv, (char *)saved, C)) return vt_fail(VT_ERR_WORKSPACE, "vt_fusion_fwd_train: saved-state buffer too small");
    hipError_t e = vt_max_dyn_lds(reinterpret_cast<const void *>(&fusionw_proj_kernel<C>), 160 * 1024);
    if (e != hipSuccess) return vt_check(e, "vt_fusion_fwd_train: hipFuncSetAttribute");
    const FusionUnitDev us = unit_of(p->self_attn), ux = unit_of(p->cross_attn);
    hipLaunchKernelGGL(fusion_pack_kernel, dim3(6), dim3(1024), 0, s, us, w.blob);
    for (int k = 0; k < 2; ++k) {
        const FusionUnitDev &u = k ? ux : us;
        hipLaunchKernelGGL(fusionw_pack_kernel, dim3(64), dim3(256), 0, s, u.Wt, C, C, w.pk[k]);
        hipLaunchKernelGGL(fusionw_pack_kernel, dim3(32), dim3(256), 0, s, u.l1w, 64, C, w.pk[k] + (size_t)C * C);
        hipLaunchKernelGGL(fusionw_pack_kernel, dim3(32), dim3(256), 0, s, u.l2w, C, 64, w.pk[k] + (size_t)C * C + 64 * (size_t)C);
    }
    auto call = [&](int k, const float *Xq, const float *Xk, const FusionUnitDev &u, const float *pk, float *dst) {
        FusionwWs wk = w;
        wk.l = sv.linv[k]; wk.s = sv.s[k]; wk.V = sv.V[k]; wk.O = sv.O[k]; wk.Z = sv.Z[k];
        run_unit_wide<C>(Xq, Xk, u, pk, wk, dst, B, N, s, drop_cfg(p_drop, seed, (uint32_t)k, 8));
    };
    call(0, c, c, us, w.pk[0], sv.M);
    call(1, c_img, c_img, us, w.pk[0], sv.T);
    call(2, sv.T, sv.M, ux, w.pk[1], out);
    return vt_check(hipGetLastError(), "vt_fusion_fwd_train");
}

}  // namespace

extern "C" {

size_t vt_fusion_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return fusion_layout(B, N, nullptr, nullptr);
}

// what a fuser call of this shape launches (fusion_plan: the launchers' own rule); nothing is launched
int vt_fusion_plan(int B, int N, int d_model, int train, int *form, int *proj_tiles, int *inorm_streamed, int *fwd_row_blocks,
                   int *bwd_row_blocks, int *scalev_strided, int *epilogue_strided, int *add_strided, int *bwd_point_strided) {
    if (B <= 0 || N <= 0 || (int64_t)B * N * FW_MAX >= 0x7fffffffll) return VT_ERR_INVALID;
    if (d_model < 32 || (d_model & 31) || d_model > FW_MAX) return VT_ERR_UNSUPPORTED;
    const FusionPlan f = fusion_plan(B, N, d_model, train != 0);
    if (form) *form = f.form;
    if (proj_tiles) *proj_tiles = f.proj_tiles;
    if (inorm_streamed) *inorm_streamed = f.inorm_streamed;
    if (fwd_row_blocks) *fwd_row_blocks = f.nrb;
    if (bwd_row_blocks) *bwd_row_blocks = f.bwd_nrb;
    if (scalev_strided) *scalev_strided = f.scalev_strided;
    if (epilogue_strided) *epilogue_strided = f.epilogue_strided;
    if (add_strided) *add_strided = f.add_strided;
    if (bwd_point_strided) *bwd_point_strided = f.bwd_point_strided;
    return 0;
}

size_t vt_fusion_workspace_bytes_wide(int B, int N, int d_model) {
    if (B <= 0 || N <= 0 || d_model <= 0 || (d_model & 31) || d_model > FW_MAX) return 0;
    return d_model == 32 ? fusion_layout(B, N, nullptr, nullptr) : fusionw_layout(B, N, d_model, nullptr, nullptr);
}

int vt_fusion_fwd(const float *c_img, const float *c, int B, int N, const vt_fusion_params *p,
                  void *workspace, size_t workspace_bytes, float *out, void *stream) {
    if (!c_img || !c || !p || !workspace || !out) return vt_fail(VT_ERR_INVALID, "vt_fusion_fwd: null argument");
    if (B <= 0 || N <= 0) return vt_fail(VT_ERR_INVALID, "vt_fusion_fwd: bad size");
    if (p->key_dim == 64 && p->d_model == 64) return fusion_fwd_wide<64>(c_img, c, B, N, p, workspace, workspace_bytes, out, (hipStream_t)stream);
    if (p->key_dim == 64 && p->d_model == 96) return fusion_fwd_wide<96>(c_img, c, B, N, p, workspace, workspace_bytes, out, (hipStream_t)stream);
    if (p->key_dim == 64 && p->d_model == 128) return fusion_fwd_wide<128>(c_img, c, B, N, p, workspace, workspace_bytes, out, (hipStream_t)stream);
    if (p->d_model != 32 || p->key_dim != 64)
        return vt_fail(VT_ERR_UNSUPPORTED, "vt_fusion_fwd: d_model in {32, 64, 96, 128} with key_feature_dim = 64 (workspace: vt_fusion_workspace_bytes_wide)");
    FusionWs w;
    if (workspace_bytes < fusion_layout(B, N, &w, (char *)workspace)) return vt_fail(VT_ERR_WORKSPACE, "vt_fusion_fwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const FusionUnitDev us = unit_of(p->self_attn), ux = unit_of(p->cross_attn);
    hipLaunchKernelGGL(fusion_pack_kernel, dim3(6), dim3(1024), 0, s, us, w.blob_s);
    hipLaunchKernelGGL(fusion_pack_kernel, dim3(6), dim3(1024), 0, s, ux, w.blob_x);
    run_unit(c, c, us, w.blob_s, w, w.M, B, N, s);                 // encoder: memory from the grid features
    run_unit(c_img, c_img, us, w.blob_s, w, w.T, B, N, s);         // decoder self-attention (SAME weights)
    run_unit(w.T, w.M, ux, w.blob_x, w, out, B, N, s);             // decoder cross-attention
    return vt_check(hipGetLastError(), "vt_fusion_fwd");
}

// vt_fusion_fwd with the tactile rows by finger id: finger_ids [rows][N] (255 = no feature), finger_feats [n_fingers][32]; batch
// element b reads ids row chunk_index[b] (device ints; NULL: row b)
int vt_fusion_fwd_ids(const unsigned char *finger_ids, const float *finger_feats, int n_fingers, const int *chunk_index,
                      const float *c, int B, int N, const vt_fusion_params *p,
                      void *workspace, size_t workspace_bytes, float *out, void *stream) {
    if (!finger_ids || !finger_feats || !c || !p || !workspace || !out) return vt_fail(VT_ERR_INVALID, "vt_fusion_fwd_ids: null argument");
    if (B <= 0 || N <= 0 || n_fingers <= 0 || n_fingers > 255) return vt_fail(VT_ERR_INVALID, "vt_fusion_fwd_ids: bad size");
    if (p->d_model != 32 || p->key_dim != 64) return vt_fail(VT_ERR_UNSUPPORTED, "vt_fusion_fwd_ids: d_model=32, key_feature_dim=64 only");
    FusionWs w;
    if (workspace_bytes < fusion_layout(B, N, &w, (char *)workspace)) return vt_fail(VT_ERR_WORKSPACE, "vt_fusion_fwd_ids: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const FusionUnitDev us = unit_of(p->self_attn), ux = unit_of(p->cross_attn);
    hipLaunchKernelGGL(fusion_pack_kernel, dim3(6), dim3(1024), 0, s, us, w.blob_s);
    hipLaunchKernelGGL(fusion_pack_kernel, dim3(6), dim3(1024), 0, s, ux, w.blob_x);
    XIds xi;
    xi.ids = finger_ids; xi.table = finger_feats; xi.chunk = chunk_index; xi.N = N; xi.F = (unsigned)n_fingers;
    run_unit(c, c, us, w.blob_s, w, w.M, B, N, s);                 // encoder: memory from the grid features
    run_unit(nullptr, nullptr, us, w.blob_s, w, w.T, B, N, s, nullptr, DropCfg{0, 0, 1.0f, 0, 6}, xi);   // decoder self-attention on the rows by id
    run_unit(w.T, w.M, ux, w.blob_x, w, out, B, N, s);             // decoder cross-attention
    return vt_check(hipGetLastError(), "vt_fusion_fwd_ids");
}

size_t vt_fusion_saved_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return fusion_saved_layout(B, N, nullptr, nullptr);
}

size_t vt_fusion_saved_bytes_wide(int B, int N, int d_model) {
    if (B <= 0 || N <= 0 || d_model <= 0 || (d_model & 31) || d_model > FW_MAX) return 0;
    return fusion_saved_layout(B, N, nullptr, nullptr, d_model);
}

int vt_fusion_fwd_train(const float *c_img, const float *c, int B, int N, const vt_fusion_params *p, float p_drop,
                        unsigned long long seed, void *workspace, size_t workspace_bytes, void *saved, size_t saved_bytes,
                        float *out, void *stream) {
    if (!c_img || !c || !p || !workspace || !saved || !out) return vt_fail(VT_ERR_INVALID, "vt_fusion_fwd_train: null argument");
    if (B <= 0 || N <= 0) return vt_fail(VT_ERR_INVALID, "vt_fusion_fwd_train: bad size");
    if (!(p_drop >= 0.0f && p_drop < 1.0f)) return vt_fail(VT_ERR_INVALID, "vt_fusion_fwd_train: p_drop must be in [0, 1)");
    if (p->key_dim == 64 && p->d_model == 64) return fusion_fwd_train_wide<64>(c_img, c, B, N, p, p_drop, seed, workspace, workspace_bytes, saved, saved_bytes, out, (hipStream_t)stream);
    if (p->key_dim == 64 && p->d_model == 96) return fusion_fwd_train_wide<96>(c_img, c, B, N, p, p_drop, seed, workspace, workspace_bytes, saved, saved_bytes, out, (hipStream_t)stream);
    if (p->key_dim == 64 && p->d_model == 128) return fusion_fwd_train_wide<128>(c_img, c, B, N, p, p_drop, seed, workspace, workspace_bytes, saved, saved_bytes, out, (hipStream_t)stream);
    if (p->d_model != 32 || p->key_dim != 64) return vt_fail(VT_ERR_UNSUPPORTED, "vt_fusion_fwd_train: d_model in {32, 64, 96, 128} with key_feature_dim = 64");
    FusionWs w;
    FusionSaved sv;
    if (workspace_bytes < fusion_layout(B, N, &w, (char *)workspace)) return vt_fail(VT_ERR_WORKSPACE, "vt_fusion_fwd_train: workspace too small");
    if (saved_bytes < fusion_saved_layout(B, N, &sv, (char *)saved)) return vt_fail(VT_ERR_WORKSPACE, "vt_fusion_fwd_train: saved-state buffer too small");
    hipStream_t s = (hipStream_t)stream;
    const FusionUnitDev us = unit_of(p->self_attn), ux = unit_of(p->cross_attn);
    hipLaunchKernelGGL(fusion_pack_kernel, dim3(6), dim3(1024), 0, s, us, w.blob_s);
    hipLaunchKernelGGL(fusion_pack_kernel, dim3(6), dim3(1024), 0, s, ux, w.blob_x);
    auto call = [&](int k, const float *Xq, const float *Xk, const FusionUnitDev &u, const float *blob, float *dst) {
        FusionWs wk = w;
        wk.l = sv.linv[k]; wk.s = sv.s[k]; wk.V = sv.V[k]; wk.Z = sv.Z[k];
        run_unit(Xq, Xk, u, blob, wk, dst, B, N, s, sv.O[k], drop_cfg(p_drop, seed, (uint32_t)k));
    };
    call(0, c, c, us, w.blob_s, sv.M);                             // encoder: memory from the grid features
    call(1, c_img, c_img, us, w.blob_s, sv.T);                     // decoder self-attention (SAME weights)
    call(2, sv.T, sv.M, ux, w.blob_x, out);                        // decoder cross-attention
    return vt_check(hipGetLastError(), "vt_fusion_fwd_train");
}

}  // extern "C"
