// The second-order jet of the 32/32/5 LocalDecoder's field at query points (DESIGN.md, section "field_jet / refine";
// tests/refine_ref.py states it in float64 autograd):  jet[g] = (f, f_x, f_y, f_z, f_xy, f_xz, f_yz, 0).
//
// f(p) = MLP(p, c(p)), c the trilinear sample of the feature grid.  The MLP is piecewise linear in (p, c) jointly, so inside a grid
// cell and away from ReLU kinks a = df/dc [32] and b = df/dp along fc_p [3] are constant around p, and with
// phi_k = a . (corner row k) at the cell's 8 corners
//     grad f = b + s (.) grad(trilinear phi),    f_uv = s_u s_v d2(trilinear phi)/du dv  (u != v),    f_uu = 0,
// s_u = (R - 1) / divisor per axis, 0 on an axis whose coordinate grid_coord clamps (q >= 1 -> 0.999, q < 0 -> 0: autograd's answer for
// the reference's in-place clamp).  a and b come from one walk back through the MLP with cotangent 1 on the TRANSPOSED weights, with
// the ReLU masks of this very forward: exact-f32 matrix core both ways (a mask from other arithmetic belongs to no function).
//
// Two forms, the same arithmetic in the same order (equal bits; tests/test_field_jet_gpu.py):
//   vt_decode_jet_composed   vt_decode_fwd with its save buffer, vt_decode_bwd_dc with grad_out = 1, then jet_gather_kernel on
//                            d c, d x_0 (gws slot 0) and the corner rows.  2.9 KB of workspace traffic per point.
//   vt_decode_jet            one kernel, one wave per 32 points: forward with the 11 ReLU masks kept as 16-bit words in registers, the
//                            transposed walk, the corner dot products.  Forward and transposed blobs both live in LDS (122.4 KB of the
//                            CU's 160 KB: one workgroup of 8 waves per CU).  The 8 corner rows are read twice (gather, then phi):
//                            holding them would take 128 registers through 480 MFMAs; the second read hits the L1 / L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_common.h"

namespace {

constexpr int JET_FWD_FLOATS = VT_OFF_WPI;                          // biases, heads, fc_p and the 15 dense layers of the forward blob
constexpr int JET_T_FLOATS = 15 * 1024 + 32;                        // the 15 transposed layers the plain decoder has, then fc_out's fragment
constexpr int JET_T_OUT = 15 * 1024;
constexpr int JET_LDS_FLOATS = JET_FWD_FLOATS + JET_T_FLOATS;
constexpr int JET_THREADS = 512;
constexpr int64_t JET_CHUNK = (int64_t)1 << 17;                     // points per pass of the composed form (B = 1): 400 MB of workspace
static_assert(JET_FWD_FLOATS % 4 == 0 && JET_T_OUT % 4 == 0 && VT_OFFT_OUT % 4 == 0, "the images are copied as float4");
static_assert(JET_FWD_FLOATS * 4 < 65536 && JET_T_FLOATS * 4 < 65536, "each image is read through 16-bit ds_read offsets from its own base");
static_assert(JET_LDS_FLOATS * 4 <= 160 * 1024, "both blobs must fit the CU's LDS");

struct JetArgs {
    DecodeArgs d;            // grid, pts, blob, N, total, R, divisor
    const float *blobT;
    const float *out;        // composed: logits [total]
    const float *grad_c;     // composed: d c [total][32]
    const float *gx0;        // composed: d x_0 [total][32] (gws slot 0)
    float *jet;              // [total][8]
};

// 1 where grid_coord leaves the coordinate free, 0 where it pins it (q >= 1 -> 0.999, q < 0 -> 0)
__device__ __forceinline__ float axis_free(float v, float divisor) {
    const float q = v / divisor + 0.5f;
    return (q >= 1.0f || q < 0.0f) ? 0.0f : 1.0f;
}

// Everything behind the two vector-Jacobian products, shared by both forms.  a: d f / d c in gather layout (register s of lane-half h =
// channel 16h+s); G0: d f / d x_0 in accumulator layout; wp: fc_p's A fragments [2 k-steps][64 lanes] (LDS or global).
// Both lane halves of a point call it; half 0 writes the row.
__device__ __forceinline__ void jet_tail(const DecodeArgs &d, const float *wp, const f32x16 &a, const f32x16 &G0, float f,
                                         float px, float py, float pz, uint32_t b, int h, bool live, float *row) {
    const int R = d.R;
    const Tri t = tri_setup(px, py, pz, d.divisor, R);
    const float *gb = d.grid + (size_t)b * R * R * R * 32 + 16 * h;
    float phi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int zz = (k & 4) ? t.z1 : t.z0, yy = (k & 2) ? t.y1 : t.y0, xx = (k & 1) ? t.x1 : t.x0;
        const f32x16 v = load_frag16(gb + (((size_t)zz * R + yy) * R + xx) * 32);
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) s = fmaf(a[j], v[j], s);
        phi[k] = s;
    }
    // b_j = sum_o fc_p.weight[o][j] d x_0[o]: column j of fc_p sits at wp[(j >> 1) * 64 + (j & 1) * 32 + o]
    float bx = 0.0f, by = 0.0f, bz = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = chan_of(r, h);
        bx = fmaf(G0[r], wp[o], bx);
        by = fmaf(G0[r], wp[32 + o], by);
        bz = fmaf(G0[r], wp[64 + o], bz);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) phi[k] += __shfl_xor(phi[k], 32);
    bx += __shfl_xor(bx, 32); by += __shfl_xor(by, 32); bz += __shfl_xor(bz, 32);
    if (h != 0 || !live) return;
    // corner k: bit 0 = x + 1, bit 1 = y + 1, bit 2 = z + 1.  Differences along one axis, then the other weights.
    const float x00 = phi[1] - phi[0], x10 = phi[3] - phi[2], x01 = phi[5] - phi[4], x11 = phi[7] - phi[6];   // d/dx at (y, z)
    const float y00 = phi[2] - phi[0], y10 = phi[3] - phi[1], y01 = phi[6] - phi[4], y11 = phi[7] - phi[5];   // d/dy at (x, z)
    const float z00 = phi[4] - phi[0], z10 = phi[5] - phi[1], z01 = phi[6] - phi[2], z11 = phi[7] - phi[3];   // d/dz at (x, y)
    const float tx = (x00 * t.wy0 + x10 * t.wy1) * t.wz0 + (x01 * t.wy0 + x11 * t.wy1) * t.wz1;
    const float ty = (y00 * t.wx0 + y10 * t.wx1) * t.wz0 + (y01 * t.wx0 + y11 * t.wx1) * t.wz1;
    const float tz = (z00 * t.wx0 + z10 * t.wx1) * t.wy0 + (z01 * t.wx0 + z11 * t.wx1) * t.wy1;
    const float txy = (x10 - x00) * t.wz0 + (x11 - x01) * t.wz1;
    const float txz = (x01 - x00) * t.wy0 + (x11 - x10) * t.wy1;
    const float tyz = (y01 - y00) * t.wx0 + (y11 - y10) * t.wx1;
    const float sc = (float)(R - 1) / d.divisor;
    const float sx = sc * axis_free(px, d.divisor), sy = sc * axis_free(py, d.divisor), sz = sc * axis_free(pz, d.divisor);
    f32x4 *q = reinterpret_cast<f32x4 *>(row);
    q[0] = f32x4{f, bx + sx * tx, by + sy * ty, bz + sz * tz};
    q[1] = f32x4{(sx * sy) * txy, (sx * sz) * txz, (sy * sz) * tyz, 0.0f};
}

// ---- composed form: the last of its three launches ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) jet_gather_kernel(JetArgs a) {
    const int lane = threadIdx.x & 63, pl = lane & 31, h = lane >> 5;
    const uint32_t ntiles = (a.d.total + 31u) >> 5;
    for (uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6); tile < ntiles; tile += gridDim.x * 4) {
        uint32_t g = tile * 32u + pl;
        const bool live = g < a.d.total;
        if (!live) g = a.d.total - 1u;
        const uint32_t b = g / a.d.N;
        float px, py, pz;
        point_of(a.d, g, g - b * a.d.N, px, py, pz);
        const f32x16 dc = load_frag16(a.grad_c + (size_t)g * 32 + 16 * h);
        const f32x16 G0 = load_acc16(a.gx0 + (size_t)g * 32, h);
        jet_tail(a.d, a.d.blob + VT_OFF_WP, dc, G0, a.out[g], px, py, pz, b, h, live, a.jet + (size_t)g * 8);
    }
}

// ---- fused form ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned mask16(const f32x16 &v) {
    unsigned m = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) m |= (v[s] > 0.0f) ? (1u << s) : 0u;
    asm volatile("" : "+v"(m));          // one VGPR of bits; left visible, the compares stay alive as 16 lane masks in SGPR pairs
    return m;
}
__device__ __forceinline__ f32x16 masked16(const f32x16 &v, unsigned m) {
    f32x16 r;
#pragma unroll
    for (int s = 0; s < 16; ++s) {      // bit s spread over the word (one v_bfe_i32), then an AND: x or +0.0
        const float x = v[s];           // (a copy: __builtin_bit_cast of the vector element itself read element 0 for every s)
        r[s] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & (unsigned)((int)(m << (31 - s)) >> 31));
    }
    return r;
}
__device__ __forceinline__ f32x16 zero16() {
    f32x16 r;
#pragma unroll
    for (int s = 0; s < 16; ++s) r[s] = 0.0f;
    return r;
}

__global__ void __launch_bounds__(JET_THREADS, 1)
decode_jet_kernel(JetArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(a.d.blob);
        const f32x4 *srcT = reinterpret_cast<const f32x4 *>(a.blobT);
        f32x4 *dst = reinterpret_cast<f32x4 *>(lds);
        for (int i = threadIdx.x; i < JET_FWD_FLOATS / 4; i += JET_THREADS) dst[i] = src[i];
        for (int i = threadIdx.x; i < JET_T_OUT / 4; i += JET_THREADS) dst[JET_FWD_FLOATS / 4 + i] = srcT[i];
        if (threadIdx.x < 8) dst[(JET_FWD_FLOATS + JET_T_OUT) / 4 + threadIdx.x] = srcT[VT_OFFT_OUT / 4 + threadIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, pl = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int WPB = JET_THREADS / 64;
    const uint32_t total = a.d.total;
    const uint32_t ntiles = (total + 31u) >> 5;
    const int R = a.d.R;

    for (uint32_t tile = blockIdx.x * WPB + wave; tile < ntiles; tile += gridDim.x * WPB) {
        unsigned lds_off = 0;                                        // (keeps the weight reads inside the tile loop: decode.hip)
        asm volatile("" : "+v"(lds_off));
        const float *L = lds + lds_off;
        unsigned lds_off_t = JET_FWD_FLOATS;                         // (its own opaque base: both images within a ds_read's immediate)
        asm volatile("" : "+v"(lds_off_t));
        const float *LT = lds + lds_off_t;
        uint32_t g = tile * 32u + pl;
        const bool live = g < total;
        if (!live) g = total - 1u;
        const uint32_t b = g / a.d.N;
        float px, py, pz;
        point_of(a.d, g, g - b * a.d.N, px, py, pz);

        // ---- trilinear gather, as decode_fwd_kernel's direct path: the same FMA order ----
        f32x16 c = zero16();
        {
            const Tri t = tri_setup(px, py, pz, a.d.divisor, R);
            const float *gb = a.d.grid + (size_t)b * R * R * R * 32 + 16 * h;
            auto plane = [&](int zz, float wz) {
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const int yy = dy ? t.y1 : t.y0;
                    const float wy = dy ? t.wy1 : t.wy0;
                    const size_t row = ((size_t)zz * R + yy) * R;
                    const f32x16 v0 = load_frag16(gb + (row + t.x0) * 32);
                    const f32x16 v1 = load_frag16(gb + (row + t.x1) * 32);
                    const float w0 = (t.wx0 * wy) * wz;
                    const float w1 = (t.wx1 * wy) * wz;
#pragma unroll
                    for (int s = 0; s < 16; ++s) c[s] = fmaf(v0[s], w0, c[s]);
#pragma unroll
                    for (int s = 0; s < 16; ++s) c[s] = fmaf(v1[s], w1, c[s]);
                }
            };
            plane(t.z0, t.wz0);
            pin16(c);
            __builtin_amdgcn_sched_barrier(0);
            plane(t.z1, t.wz1);
            pin16(c);
            __builtin_amdgcn_sched_barrier(0);
        }

        // ---- forward, as decode.hip's exact-f32 mlp_and_heads; the ReLU masks stay in registers ----
        unsigned mx[5], mh[5];
        f32x16 net = load_frag16(L + VT_OFF_BIAS + h * 16);
        net = mfma(L[VT_OFF_WP + lane], h ? py : px, net);
        net = mfma(L[VT_OFF_WP + 64 + lane], h ? 0.0f : pz, net);
        net = dense32<false>(net, L + VT_OFF_WL, c, lane);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float *wl = L + VT_OFF_WL + (1 + 3 * i) * 1024;
            f32x16 hid = load_frag16(L + VT_OFF_BIAS + (1 + 2 * i) * 32 + h * 16);
            mx[i] = mask16(net);
            hid = dense32<true>(hid, wl, net, lane);
            mh[i] = mask16(hid);
            net = dense32<true>(net, wl + 1024, hid, lane);
            if (i < 4) net = dense32<false>(net, wl + 2048, c, lane);
            const f32x16 bb = load_frag16(L + VT_OFF_BIAS + (2 + 2 * i) * 32 + h * 16);
            net = net + bb;
        }
        float f = 0.0f;
        {
            const f32x16 wo = load_frag16(L + VT_OFF_OUT + h * 16);
#pragma unroll
            for (int s = 0; s < 16; ++s) f = fmaf(relu1(net[s]), wo[s], f);
            f += __shfl_xor(f, 32);
            f += L[VT_OFF_OUT + 64];
        }

        // ---- the walk back with cotangent 1, as decode_bwd_data_kernel ----
        f32x16 G = masked16(load_frag16(LT + JET_T_OUT + h * 16), mask16(net));      // d net_5
        f32x16 dc = zero16();
#pragma unroll
        for (int i = 4; i >= 0; --i) {
            if (i < 4) dc = dense32<false>(dc, LT + (i + 1) * 1024, G, lane);          // += fc_c{i+1}^T G
            f32x16 t = dense32<false>(zero16(), LT + (5 + i) * 1024, G, lane);         // fc_1^T G
            t = masked16(t, mh[i]);                                                    // d h_i
            const f32x16 u = masked16(dense32<false>(zero16(), LT + (10 + i) * 1024, t, lane), mx[i]);
            G = G + u;                                                                 // d x_i
        }
        dc = dense32<false>(dc, LT, G, lane);                                          // += fc_c0^T d x_0

        jet_tail(a.d, L + VT_OFF_WP, dc, G, f, px, py, pz, b, h, live, a.jet + (size_t)g * 8);
    }
}

bool jet_args(JetArgs &a, const float *grid_cl, int B, int R, int C, const float *pts, int64_t N, const float *blob, const float *blob_t,
              double padding, float *jet, const char *who, int &rc) {
    rc = 0;
    if (!grid_cl || !pts || !blob || !blob_t || !jet || B <= 0 || R < 2 || N <= 0) { rc = vt_fail(VT_ERR_INVALID, who); return false; }
    if (C != 32) { rc = vt_fail(VT_ERR_UNSUPPORTED, "the field jet is built for hidden 32, c_dim 32, 5 blocks"); return false; }
    if ((int64_t)B * N >= (int64_t)1 << 31) { rc = vt_fail(VT_ERR_UNSUPPORTED, "B*N must be < 2^31"); return false; }
    DecodeArgs &d = a.d;
    d.c_direct = nullptr; d.brick = 0; d.cimg_ids = nullptr; d.cimg_table = nullptr; d.cimg_nf = 0; d.grid = grid_cl; d.pts = pts; d.c_img = nullptr;
    d.blob = blob; d.out = nullptr; d.out2 = nullptr; d.save = nullptr; d.status = nullptr; d.clk = nullptr; d.claim = 0;
    d.N = (uint32_t)N; d.total = (uint32_t)((int64_t)B * N); d.lattice_first = 0;
    d.R = R; d.nx = 0; d.box = 0.0f; d.divisor = (float)(1.0 + padding + 10e-4);
    a.blobT = blob_t; a.out = nullptr; a.grad_c = nullptr; a.gx0 = nullptr; a.jet = jet;
    return true;
}

size_t up256(size_t x) { return (x + 255) / 256 * 256; }

struct ComposedWs {
    size_t save, gws, grad_c, out, ones, bytes;
};
ComposedWs composed_layout(int B, int64_t N) {
    const int64_t n = (B == 1 && N > JET_CHUNK) ? JET_CHUNK : (int64_t)B * N;
    ComposedWs w;
    size_t at = 0;
    w.save = at; at += up256(vt_decode_save_bytes(n));
    w.gws = at; at += up256(vt_decode_gws_bytes(n));
    w.grad_c = at; at += up256((size_t)n * 32 * sizeof(float));
    w.out = at; at += up256((size_t)n * sizeof(float));
    w.ones = at; at += up256((size_t)n * sizeof(float));
    w.bytes = at;
    return w;
}

}  // namespace

extern "C" {

int vt_decode_jet(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N, const float *blob, const float *blob_t,
                  double padding, float *jet, void *stream) {
    JetArgs a;
    int rc;
    if (!jet_args(a, grid_cl, B, R, C, pts, N, blob, blob_t, padding, jet, "vt_decode_jet: bad argument", rc)) return rc;
    const size_t lds_bytes = (size_t)JET_LDS_FLOATS * sizeof(float);
    hipError_t e = vt_max_dyn_lds(reinterpret_cast<const void *>(&decode_jet_kernel), (int)lds_bytes);
    if (e != hipSuccess) return vt_check(e, "vt_decode_jet: hipFuncSetAttribute");
    const int64_t ntiles = ((int64_t)a.d.total + 31) / 32;
    int64_t blocks = (ntiles + JET_THREADS / 64 - 1) / (JET_THREADS / 64);
    const int64_t cap = vt_num_cus();                                // one workgroup per CU: the LDS holds one pair of blobs
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(decode_jet_kernel, dim3((unsigned)blocks), dim3(JET_THREADS), lds_bytes, (hipStream_t)stream, a);
    return vt_check(hipGetLastError(), "vt_decode_jet");
}

size_t vt_decode_jet_composed_workspace_bytes(int B, int64_t N) {
    if (B <= 0 || N <= 0) return 0;
    return composed_layout(B, N).bytes;
}

int vt_decode_jet_composed(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N, const float *blob, const float *blob_t,
                           double padding, float *jet, void *workspace, size_t workspace_bytes, void *stream) {
    JetArgs a;
    int rc;
    if (!jet_args(a, grid_cl, B, R, C, pts, N, blob, blob_t, padding, jet, "vt_decode_jet_composed: bad argument", rc)) return rc;
    const ComposedWs w = composed_layout(B, N);
    if (!workspace || workspace_bytes < w.bytes) return vt_fail(VT_ERR_WORKSPACE, "vt_decode_jet_composed: workspace too small");
    char *ws = static_cast<char *>(workspace);
    float *save = reinterpret_cast<float *>(ws + w.save), *gws = reinterpret_cast<float *>(ws + w.gws);
    float *grad_c = reinterpret_cast<float *>(ws + w.grad_c), *out = reinterpret_cast<float *>(ws + w.out);
    float *ones = reinterpret_cast<float *>(ws + w.ones);
    hipStream_t st = (hipStream_t)stream;
    const int64_t step = (B == 1 && N > JET_CHUNK) ? JET_CHUNK : N;  // (B > 1 runs whole: a scene's points are one call's N)
    rc = vt_fill32(ones, 0x3f800000u, (size_t)(B == 1 ? step : (int64_t)B * N) * sizeof(float), st);
    if (rc) return rc;
    for (int64_t lo = 0; lo < N; lo += step) {
        const int64_t n = (N - lo < step) ? N - lo : step;
        const float *p = pts + (size_t)lo * 3;
        rc = vt_decode_fwd(grid_cl, B, R, C, p, n, 0, 0.0f, 0, nullptr, blob, padding, out, nullptr, save, stream);
        if (rc) return rc;
        rc = vt_decode_bwd_dc(B, R, C, p, n, padding, blob_t, ones, nullptr, save, gws, grad_c, nullptr, stream);
        if (rc) return rc;
        JetArgs c = a;
        c.d.pts = p; c.d.N = (uint32_t)n; c.d.total = (uint32_t)((int64_t)B * n);
        c.out = out; c.grad_c = grad_c; c.gx0 = gws; c.jet = jet + (size_t)lo * 8;
        int64_t blocks = (((int64_t)c.d.total + 31) / 32 + 3) / 4;
        const int64_t cap = 8 * vt_num_cus();
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(jet_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, st, c);
        rc = vt_check(hipGetLastError(), "vt_decode_jet_composed");
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
