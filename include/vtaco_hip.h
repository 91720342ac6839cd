/*
 * vtaco_hip.h -- C ABI of libvtaco_hip.so, the MI355X (gfx950) implementation
 * of VTacO's occupancy hot path.
 *
 * The reference (jeffsonyu/VTacO) is pure Python: its "plugin API" for this path
 * is the nn.Module registry (decoder_dict / encoder_dict).  There is no FFI in
 * the reference, so each entry point below names the reference *call site* whose
 * third-party native op it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - no allocation, no synchronisation, no host<->device copy inside any call
 *     (graph-capture safe) unless stated;
 *   - return value: 0 = ok, >0 = a hipError_t from the runtime, <0 = VT_ERR_*;
 *     vt_last_error() returns a static, thread-local description;
 *   - all float data is IEEE float32, all layouts are dense row-major in the
 *     stated dimension order.
 */
#ifndef VTACO_HIP_H
#define VTACO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VT_ABI_VERSION 1

#define VT_ERR_INVALID      (-1)  /* bad argument (NULL, negative size, ...)        */
#define VT_ERR_UNSUPPORTED  (-2)  /* shape outside what the gfx950 kernels cover    */
#define VT_ERR_WORKSPACE    (-3)  /* caller-provided workspace too small            */

#define VT_MAX_BLOCKS 8

int         vt_abi_version(void);
const char *vt_last_error(void);

/* ------------------------------------------------------------------------- */
/* Decoder weights.                                                            */
/* Replaces: nothing in the reference; it is the one-off repack of the          */
/* nn.Linear parameters of LocalDecoder (src/conv_onet/models/decoder.py:27-44) */
/* into the MFMA-fragment order vt_decode_fwd reads from LDS.                   */
/* ------------------------------------------------------------------------- */
typedef struct vt_decoder_params {
    int32_t hidden;      /* hidden_size: 32 (vt_decoder_pack*), 32..256 (_pack_wide)  */
    int32_t c_dim;       /* c_dim: 32 (vt_decoder_pack*), 32..256 (_pack_wide)        */
    int32_t n_blocks;    /* n_blocks: 5 (vt_decoder_pack*), 1..8 (_pack_wide)         */
    int32_t p_in;        /* columns of fc_p_w: 3 (fc_p) or 3+c_dim (fc_p_img)        */
    const float *fc_p_w; /* [hidden, p_in]  fc_p.weight or fc_p_img.weight           */
    const float *fc_p_b; /* [hidden]                                                 */
    const float *fc_c_w[VT_MAX_BLOCKS]; /* [hidden, c_dim] fc_c.{i}.weight           */
    const float *fc_c_b[VT_MAX_BLOCKS]; /* [hidden]                                  */
    const float *fc0_w[VT_MAX_BLOCKS];  /* [hidden, hidden] blocks.{i}.fc_0.weight   */
    const float *fc0_b[VT_MAX_BLOCKS];
    const float *fc1_w[VT_MAX_BLOCKS];  /* [hidden, hidden] blocks.{i}.fc_1.weight   */
    const float *fc1_b[VT_MAX_BLOCKS];
    const float *fc_out_w;  /* [1, hidden] fc_out.weight                             */
    const float *fc_out_b;  /* [1]                                                   */
    const float *fc_out2_w; /* fc_out_contact.weight or NULL                         */
    const float *fc_out2_b; /* fc_out_contact.bias   or NULL                         */
} vt_decoder_params;

/* Size in bytes of the packed blob for a given (hidden, c_dim, n_blocks). */
size_t vt_decoder_blob_bytes(int hidden, int c_dim, int n_blocks);

/* params_host: HOST pointer to the struct (its members are device pointers). */
int vt_decoder_pack(const vt_decoder_params *params_host, float *blob, size_t blob_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* Feature grid layout.                                                        */
/* vt_decode_* read the grid channels-last: grid_cl[b][z][y][x][c].            */
/* Replaces: the implicit NCDHW read of F.grid_sample (decoder.py:62-68).      */
/* ------------------------------------------------------------------------- */
int vt_grid_to_channels_last(const float *grid_ncdhw, float *grid_cl,
                             int B, int C, int D, int H, int W, void *stream);
int vt_grid_from_channels_last(const float *grid_cl, float *grid_ncdhw,
                               int B, int C, int D, int H, int W, void *stream);

/* ------------------------------------------------------------------------- */
/* Fused trilinear gather + conditioned ResNet MLP, forward.                    */
/* Replaces: LocalDecoder.forward / forward_img / forward_contact               */
/*   (decoder.py:135-161, 71-103, 105-133) = normalize_3d_coordinate            */
/*   (src/common.py:293-309) + F.grid_sample (decoder.py:62-68) + fc_p +        */
/*   5 x (fc_c[i] add, ResnetBlockFC src/layers.py:41-50) + fc_out.             */
/*                                                                             */
/*   pts      [B,N,3] query points, or NULL for lattice mode;                   */
/*   lattice mode: the n-th point of every batch element is the                 */
/*     (lattice_first + n)-th point of box * make_3d_grid((-.5,)*3,(.5,)*3,     */
/*     (nx,)*3) (src/common.py:178-197, generation.py:155-157): axis 0 slowest; */
/*   c_img    [B,N,c_dim] tactile features (forward_img) or NULL;               */
/*   blob     from vt_decoder_pack (packed with p_in = 3+c_dim iff c_img);      */
/*   out      [B,N] logits; out2 [B,N] contact logits or NULL;                  */
/*   save     NULL (inference) or vt_decode_save_bytes(B*N) bytes: the training  */
/*            forward leaves the activations vt_decode_bwd needs there.          */
/* ------------------------------------------------------------------------- */
int vt_decode_fwd(const float *grid_cl, int B, int R, int C,
                  const float *pts, int64_t N,
                  int lattice_nx, float lattice_box, int64_t lattice_first,
                  const float *c_img, const float *blob, double padding,
                  float *out, float *out2, float *save, void *stream);

/* Split-bf16 ("bf16x3") inference variant of vt_decode_fwd / vt_decode_fwd_ids for the same   */
/* reference functions.  Every f32 operand v of the 16 dense 32x32 layers is carried as           */
/* bf16(v) + bf16(v - bf16(v)) and every product as W_lo*x_hi + W_hi*x_lo + W_hi*x_hi on the       */
/* bf16 matrix core with f32 accumulation (error ~2^-16 relative per product: 2e-5 abs on the      */
/* O(1) logits of the golden vectors, inside the 1e-4 parity bar; plain bf16 is ~1e-2).  The        */
/* gather, fc_p, biases, residuals and the output heads stay f32.  blob_bf16x3 comes from           */
/* vt_decoder_pack_bf16x3 (same size as the f32 blob).  c_img and finger_ids are alternatives         */
/* (both NULL = visual-only); no `save`: the training forward is the exact-f32 vt_decode_fwd.          */
int vt_decoder_pack_bf16x3(const vt_decoder_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_decode_fwd_bf16x3(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                         int lattice_nx, float lattice_box, int64_t lattice_first,
                         const float *c_img, const unsigned char *finger_ids, const float *finger_feats, int F,
                         const float *blob_bf16x3, double padding, float *out, float *out2, void *stream);

/* Split-f16 ("f16x3") variant: the same three-product scheme with IEEE half hi / lo parts on      */
/* v_mfma_f32_32x32x16_f16 (the same matrix rate as bf16).  hi + lo carries 21-22 mantissa bits     */
/* (logit error ~1e-6 on the goldens against ~1.6e-5 for bf16x3) for operand magnitudes below       */
/* 65504 -- activations beyond that saturate, so networks with huge hidden activations belong on     */
/* bf16x3 or f32 -- and relu + split costs two VALU instructions per value instead of four            */
/* (v_cvt_pkrtz_f16_f32, v_pk_max_f16, v_fma_mix{lo,hi}_f16 with clamp): the lattice decode's       */
/* fastest form.  Same arguments and blob size as the bf16x3 pair; blob from vt_decoder_pack_f16x3.  */
/* Replaces the same reference functions (decoder.py:135-161, 71-103 on no-grad paths).              */
int vt_decoder_pack_f16x3(const vt_decoder_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_decode_fwd_f16x3(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                        int lattice_nx, float lattice_box, int64_t lattice_first,
                        const float *c_img, const unsigned char *finger_ids, const float *finger_feats, int F,
                        const float *blob_f16x3, double padding, float *out, float *out2, void *stream);

/* "f16f8": the dense lattice decode with the two correction products of every layer on ONE fp8   */
/* (e4m3) 32x32x64 MFMA: W x = W_hi x_hi (two f16 MFMAs, as f16x3) + [W_lo 2^15 | W_hi 2^4] .       */
/* [x_hi 2^-2 | x_lo 2^9] with the MFMA's block scales undoing the shifts -- 128 matrix cycles per   */
/* layer instead of 192 and ~40 % less matrix-pipe energy (the kernel is power-limited).  The        */
/* corrections carry 4 significant bits per operand: logits within ~4e-5 of the f32 reference on    */
/* the golden decoder (inside the 1e-4 parity bar; f16x3: ~1e-6); activations beyond 448 * 4          */
/* saturate in the correction (never NaN).  Lattice mode only, for slabs the slot-pipelined kernel   */
/* covers (vt_decode_f16f8_covers: whole x-plane pairs, nx % 8 == 0, < 0.55 voxels per lattice       */
/* step, c_dim 32); everything else is vt_decode_fwd_f16x3's.  blob from vt_decoder_pack_f16f8       */
/* (same size).  Replaces the same reference functions on the generator's no-grad path               */
/* (decoder.py:135-161, 71-103 via generation.py:338-383).                                            */
int vt_decoder_pack_f16f8(const vt_decoder_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_decode_f16f8_covers(int R, int C, int lattice_nx, float lattice_box, int64_t lattice_first, int64_t N, double padding);
int vt_decode_fwd_f16f8(const float *grid_cl, int B, int R, int C, int64_t N,
                        int lattice_nx, float lattice_box, int64_t lattice_first,
                        const float *c_img, const unsigned char *finger_ids, const float *finger_feats, int F,
                        const float *blob_f16f8, double padding, float *out, void *stream);

/* Which kernel form a lattice decode of this shape takes (host only: nothing is launched, no GPU   */
/* call is made; no reference counterpart).  The same rule vt_decode_fwd, vt_decode_fwd_ids,          */
/* vt_decode_fwd_bf16x3, vt_decode_fwd_f16x3 and vt_decode_fwd_f16f8 dispatch by, the environment's   */
/* A/B knobs included, so a test can confirm that a case runs the kernel it means to:                 */
/*   VT_LATTICE_LINEAR   tiles of 32 consecutive lattice indices, direct gather (any nx, any range)  */
/*   VT_LATTICE_BRICK    2 x 4 x 4 point bricks, direct gather: nx % 4 == 0, first and N multiples    */
/*                       of 2 nx^2 (a slab of whole x-plane pairs)                                     */
/*   VT_LATTICE_STAGED   bricks with the 3 x 4 x 4 voxel footprint staged in LDS: R >= 4, nx <= 512,  */
/*                       s = (R-1) box / ((nx-1) divisor) < 0.66 voxels per lattice step, LDS fits    */
/*   VT_LATTICE_STAGED2  2 x 4 x 8 double bricks, 3 x 4 x 6 footprint: nx % 8 == 0, R >= 6, s < 0.55, */
/*                       no contact head                                                               */
/*   VT_LATTICE_STAGED3  the slot-pipelined double-brick kernel of the half-precision forms            */
/* precision: VT_PRECISION_F32 / _BF16X3 / _F16X3 / _F16F8; want_contact: the call gives out2;        */
/* have_c_direct: the features are given (vt_decode_mlp_fwd*), no grid is sampled.  Returns the form, */
/* or VT_ERR_INVALID / VT_ERR_UNSUPPORTED where the launcher would refuse the call (C != 32, nx < 2,  */
/* a range outside the lattice, an f16f8 slab vt_decode_f16f8_covers does not cover).                  */
#define VT_LATTICE_LINEAR  0
#define VT_LATTICE_BRICK   1
#define VT_LATTICE_STAGED  2
#define VT_LATTICE_STAGED2 3
#define VT_LATTICE_STAGED3 4
#define VT_PRECISION_F32    0
#define VT_PRECISION_BF16X3 1
#define VT_PRECISION_F16X3  2
#define VT_PRECISION_F16F8  3
int vt_decode_lattice_form(int R, int C, int lattice_nx, float lattice_box, int64_t lattice_first, int64_t N, double padding,
                           int precision, int want_contact, int have_c_direct);

/* Range guard of the half-precision decodes (vt_decode_fwd_f16x3 / _f16f8): their hi operand     */
/* saturates at 65504 (round toward zero: never an infinity), after which the logits silently lose  */
/* parity.  Every launch samples its relu'd hi operands (two of a lane's sixteen channels, every     */
/* point and layer) and sets bits of a per-DEVICE status word (the current device's):                 */
/*   bit 0: a sampled half reached 65504 -- re-run with vt_decode_fwd_bf16x3 or the exact-f32 kernel; */
/*   bit 1 (vt_decode_fwd_f16f8 only): a sampled half reached 1024, where the fp8 copies of the       */
/*          correction products begin to clip and the 1e-4 contract of that kernel ends -- re-run     */
/*          with vt_decode_fwd_f16x3;                                                                  */
/*   bit 2 (vt_decode_fwd_f16f8 only): a logit beyond 2.5 in magnitude was written -- that kernel's    */
/*          error is relative (~3e-5 |logit|), its 1e-4 absolute contract ends there: re-run likewise.  */
/* vt_decode_range_status copies that word to the host (synchronises `stream`) and, with `reset`,    */
/* clears it (the host mirror's Generator3D does the re-runs); host_status NULL with `reset`: clear    */
/* only, asynchronously on `stream` (the start of a scene).  No reference counterpart: the             */
/* reference is f32 (decoder.py:135-161).                                                              */
int vt_decode_range_status(unsigned *host_status, int reset, void *stream);

/* Measurement aid (bench.py's clock evidence; no reference counterpart): the lattice kernels of      */
/* vt_decode_fwd* stamp every workgroup's lifetime with the constant-rate counter and workgroup 0's     */
/* also with the shader-clock counter; this returns the last launch's differences of workgroup 0 on     */
/* the current device and the constant counter's rate in kHz (synchronises `stream`):                   */
/* shader MHz = cycles / ticks * ref_khz / 1000; and, with max_wgs > 0, the (start, end) ticks of the   */
/* first min(max_wgs, workgroups, 512) workgroups -- the launch's ramp and tail.                         */
int vt_decode_last_clock(unsigned long long *shader_cycles, unsigned long long *ref_ticks, int *ref_khz,
                         unsigned long long *wg_ticks, int max_wgs, int *n_wgs, void *stream);

/* LocalDecoder beyond the shipped shape.  Replaces the same reference functions (decoder.py:135-161, */
/* 71-103, 105-133) for hidden_size and c_dim any multiples of 32 up to 256 (the class defaults are      */
/* 256 / 128, decoder.py:24), n_blocks <= VT_MAX_BLOCKS, and `leaky`: leaky_relu(0.2) in front of the       */
/* output heads (decoder.py:46-49, 157; the ResnetBlockFC activations are ReLU regardless, layers.py:33).    */
/* Exact f32 (v_mfma_f32_32x32x2_f32); training: below.  The weights stream from L2 in the fragment order      */
/* vt_decoder_pack_wide writes (params_host->hidden / c_dim / n_blocks / p_in describe the shape; p_in = 3,    */
/* or 3 + c_dim for forward_img); blob_bytes from vt_decoder_wide_blob_bytes (0: shape not covered).           */
/* vt_decode_fwd_wide: the arguments of vt_decode_fwd (pts or lattice, optional c_img [B,N,c_dim], out2 for     */
/* the contact head) plus the shape the blob was packed for; C = c_dim = the grid's channel count; flags:        */
/* VT_WIDE_LEAKY (leaky=True), VT_WIDE_NEAREST (sample_mode='nearest': F.grid_sample mode 'nearest', i.e. the     */
/* voxel at the half-to-even rounded coordinate, decoder.py:62-68).                                               */
#define VT_WIDE_LEAKY 1
#define VT_WIDE_NEAREST 2
size_t vt_decoder_wide_blob_bytes(int hidden, int c_dim, int n_blocks, int p_in);
int vt_decoder_pack_wide(const vt_decoder_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_decode_fwd_wide(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                       int lattice_nx, float lattice_box, int64_t lattice_first,
                       const float *c_img, const float *blob_wide, int hidden, int n_blocks, int flags, double padding,
                       float *out, float *out2, void *stream);
/* Split-f16 form of the same forward (inference): W x = W_lo x_hi + W_hi x_lo + W_hi x_hi on v_mfma_f32_32x32x16_f16 with f32     */
/* accumulation, operands as IEEE-half hi + lo pairs (21-22 mantissa bits: f32-level logits while the hidden activations stay      */
/* inside the half range -- watched like the shipped-shape kernels': vt_decode_range_status).  A workgroup owns 64 points as two   */
/* groups that share every streamed weight fragment.  Blob: vt_decoder_pack_wide_f16x3 (its own fragment format and size).         */
/* Same arguments and coverage as vt_decode_fwd_wide.  256 / 128 / 5 at 128^3: see profiles/ (exact f32: 36 ms).                   */
size_t vt_decoder_wide_blob_f16x3_bytes(int hidden, int c_dim, int n_blocks, int p_in);
int vt_decoder_pack_wide_f16x3(const vt_decoder_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_decode_fwd_wide_f16x3(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                             int lattice_nx, float lattice_box, int64_t lattice_first,
                             const float *c_img, const float *blob_wide_f16x3, int hidden, int n_blocks, int flags, double padding,
                             float *out, float *out2, void *stream);
/* The two forwards above with the tactile feature given per point as a finger id (255 = none) and the [n_fingers][C] table of   */
/* finger features instead of the dense c_img tensor (reference generation.py:159-255 builds c_img_all [1, nx^3, C] on the host:   */
/* 8.6 GB at 256^3 / c_dim 128); the blob is the one packed with fc_p_img (p_in = 3 + C).  Equal to the dense form bit for bit.   */
int vt_decode_fwd_wide_ids(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                           int lattice_nx, float lattice_box, int64_t lattice_first,
                           const unsigned char *finger_ids, const float *finger_feats, int n_fingers,
                           const float *blob_wide, int hidden, int n_blocks, int flags, double padding,
                           float *out, float *out2, void *stream);
/* vt_decode_fwd_wide_f16x3 with a workspace.  At hidden 64 / c_dim 32 / n_blocks <= 5 without tactile input columns (c_img NULL)   */
/* the whole network fits the registers of one workgroup: 2 n_blocks waves each keep 32 rows of one block's three layers as MFMA    */
/* operands for the whole launch and the 32-point tiles move through them as a pipeline (three barriers per tick, no weight         */
/* traffic; decode_wide_pipe.inc), fed with per-point features.  With `workspace` of vt_decode_wide_f16x3_workspace_bytes(B N,      */
/* ...) bytes (0: the shape does not use one) a pre-pass leaves the grid's samples there (same sums, same order) and the pipeline   */
/* runs on them; without it (or through vt_decode_fwd_wide_f16x3) the streaming kernel runs.  vt_decode_mlp_fwd_wide_f16x3, whose    */
/* features are given, takes the pipeline by itself.  decoder.py:24-51, 71-103.                                                     */
size_t vt_decode_wide_f16x3_workspace_bytes(int64_t total_points, int hidden, int c_dim, int n_blocks, int tactile);
int vt_decode_fwd_wide_f16x3_ws(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                                int lattice_nx, float lattice_box, int64_t lattice_first,
                                const float *c_img, const float *blob, int hidden, int n_blocks, int flags, double padding,
                                float *out, float *out2, void *workspace, size_t workspace_bytes, void *stream);
int vt_decode_fwd_wide_f16x3_ids(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                                 int lattice_nx, float lattice_box, int64_t lattice_first,
                                 const unsigned char *finger_ids, const float *finger_feats, int n_fingers,
                                 const float *blob_wide_f16x3, int hidden, int n_blocks, int flags, double padding,
                                 float *out, float *out2, void *stream);
/* The conditioned MLP of the wide shapes on features given per point, c [B][N][C], instead of the grid gather: what runs behind the  */
/* fuser in AttentionDecoder.forward_img (decoder.py:259-271) at the reference's default widths; blob packed with fc_p (p_in = 3).  */
int vt_decode_mlp_fwd_wide(const float *c, int B, int C, const float *pts, int64_t N,
                           int lattice_nx, float lattice_box, int64_t lattice_first,
                           const float *blob_wide, int hidden, int n_blocks, int flags, float *out, float *out2, void *stream);
int vt_decode_mlp_fwd_wide_f16x3(const float *c, int B, int C, const float *pts, int64_t N,
                                 int lattice_nx, float lattice_box, int64_t lattice_first,
                                 const float *blob_wide_f16x3, int hidden, int n_blocks, int flags, float *out, float *out2, void *stream);

/* The same shapes under autograd (the reference trains them through torch autograd: decoder.py:24-51,     */
/* 135-161 called from training.py:476-489, 734-740, 879).                                                   */
/*   vt_decode_fwd_wide_train  vt_decode_fwd_wide on query points that also keeps, point-major, the inputs     */
/*                       of every layer: save = vt_decode_wide_save_floats floats laid out as                    */
/*                       c [P][c_dim] | per block relu(net + fc_c(c)) [P][H], relu(fc_0(.)) [P][H] | actvn(net) [P][H]. */
/*   vt_decoder_pack_wide_t    the transposed weight fragments the backward streams (W1^T, W0^T, Wc^T per block,    */
/*                       fc_p_img's c_img columns transposed, the two head vectors).                               */
/*   vt_decode_bwd_wide  grad_out [P] (and grad_out2 for the contact head, or NULL) -> d grid (channels-last, f32     */
/*                       atomics into a ZEROED buffer; NULL: not wanted), d c_img [P][c_dim] (NULL: not wanted), and  */
/*                       gws = vt_decode_wide_gws_floats floats: dN_i [P][H] for i = 0..n_blocks (gradient of the     */
/*                       residual stream in front of block i; dN_nb: behind the last block) then dH_i [P][H]          */
/*                       (gradient of fc_0_i's output).  The weight gradients are vt_rows_wgrad over these rows:       */
/*                       fc_p <- (dN_0, [p | c_img]); fc_c_i <- (dN_i, c); fc_0_i <- (dH_i, save a0_i);                */
/*                       fc_1_i <- (dN_{i+1}, save a1_i); fc_out <- (grad_out, save actvn(net)).  No gradient with     */
/*                       respect to the query points (the reference never reads it: SURVEY.md 8a row A14).             */
size_t vt_decode_wide_save_floats(int64_t total_points, int hidden, int c_dim, int n_blocks);
size_t vt_decode_wide_gws_floats(int64_t total_points, int hidden, int c_dim, int n_blocks);
/* Which kernel a wide decode takes and how it is launched, without launching anything (host code: the rule the launchers themselves */
/* call).  kind: VT_WIDE_KIND_FWD (vt_decode_fwd_wide / _train / vt_decode_mlp_fwd_wide*), VT_WIDE_KIND_BWD (vt_decode_bwd_wide /      */
/* vt_decode_mlp_bwd_wide), VT_WIDE_KIND_F16X3 (vt_decode_fwd_wide_f16x3*); tactile: the call gives c_img or finger ids;               */
/* have_workspace (F16X3 only): the call has 16-byte aligned features for the 64 / 32 pipeline -- a workspace of                       */
/* vt_decode_wide_f16x3_workspace_bytes, or the features themselves (vt_decode_mlp_fwd_wide_f16x3).  Any result pointer may be NULL:   */
/*   waves        64-lane waves per workgroup               groups       32-point groups per wave that share a weight fragment         */
/*   pairs        sets of `groups` groups per tile, after the LDS cap     heads_on_c   the heads' partial sums lie over the c planes   */
/*   tile_points  points per workgroup tile                 grid_cap     the most workgroups a launch takes: tiles beyond it are       */
/*   pipeline     1: the register-resident 64 / 32 pipeline              walked by the workgroups in a loop (tile += grid)             */
/* Returns 0, or VT_ERR_INVALID / VT_ERR_UNSUPPORTED where the launcher would refuse the shape.                                        */
#define VT_WIDE_KIND_FWD   0
#define VT_WIDE_KIND_BWD   1
#define VT_WIDE_KIND_F16X3 2
int vt_decode_wide_form(int hidden, int c_dim, int n_blocks, int tactile, int kind, int64_t total_points, int have_workspace,
                        int *waves, int *groups, int *pairs, int *heads_on_c, int *tile_points, int *grid_cap, int *pipeline);
int vt_decode_fwd_wide_train(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                             const float *c_img, const float *blob_wide, int hidden, int n_blocks, int flags, double padding,
                             float *out, float *out2, float *save, void *stream);
size_t vt_decoder_wide_blob_t_bytes(int hidden, int c_dim, int n_blocks);
int vt_decoder_pack_wide_t(const vt_decoder_params *params_host, float *blob_t, size_t blob_bytes, void *stream);
int vt_decode_bwd_wide(int B, int R, int C, const float *pts, int64_t N, const float *blob_wide_t, int hidden, int n_blocks, int flags,
                       double padding, const float *grad_out, const float *grad_out2, const float *save, float *gws,
                       float *grad_grid_cl, float *grad_c_img, void *stream);
/* The conditioned MLP alone under autograd at these widths (AttentionDecoder.forward_img behind its fuser, decoder.py:259-271 with  */
/* c_dim 64 / 96 / 128): vt_decode_mlp_fwd_wide on query points that also fills `save` (same layout; its c slot is left unwritten --   */
/* the caller holds c), and the data pass that returns d c per point [B][N][C] instead of a grid scatter.  gws and the weight          */
/* gradients as vt_decode_bwd_wide's, with fc_c_i <- (dN_i, the caller's c).  vt_sample_grid_bwd[_sorted] take any c_dim % 32 == 0.    */
int vt_decode_mlp_fwd_wide_train(const float *c, int B, int C, const float *pts, int64_t N, const float *blob_wide, int hidden, int n_blocks,
                                 int flags, float *out, float *out2, float *save, void *stream);
int vt_decode_mlp_bwd_wide(int B, int C, const float *pts, int64_t N, const float *blob_wide_t, int hidden, int n_blocks, int flags,
                           const float *grad_out, const float *grad_out2, const float *save, float *gws, float *grad_c, void *stream);

/* Tactile feature assignment and decode by finger id (SURVEY.md section 8f "next" row 2).        */
/* Replaces: the scipy cdist + np.where glue that fills the dense c_img_all [1,N,32] at            */
/*   src/conv_onet/generation.py:186-200 (mode 0: nearest fingertip, radius 0.05, only if that      */
/*   finger's touch succeeded) and :245-255 (mode 1: within radius 0.015 of any of the finger's      */
/*   contact points; fingers in ascending order, later ones overwrite).                              */
/*   anchors [F,K,3], count [F] (valid anchors per finger), success [F] (u8); ids [B,N] u8, 255=none. */
/* vt_decode_fwd_ids = vt_decode_fwd with c_img[b,n,:] = finger_feats[ids[b,n]] (0 where 255).        */
/* In every *_ids entry an id >= n_fingers (F) reads as 255 does -- a zero feature -- never as a row  */
/* past the table (the host gather this replaces, table[row], raised on such an index).              */
int vt_tactile_assign(const float *pts, int B, int64_t N, int lattice_nx, float lattice_box, int64_t lattice_first,
                      const float *anchors, const int *count, const unsigned char *success, int F, int K,
                      int mode, double radius, unsigned char *ids, void *stream);
int vt_decode_fwd_ids(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                      int lattice_nx, float lattice_box, int64_t lattice_first,
                      const unsigned char *finger_ids, const float *finger_feats, int F,
                      const float *blob, double padding, float *out, void *stream);

/* The two halves of vt_decode_fwd on their own, for AttentionDecoder.forward_img      */
/* (decoder.py:237-271), which transforms the sampled features before the MLP:         */
/*   vt_sample_grid    feat[B,N,C] = trilinear sample only (decoder.py:62-68);          */
/*   vt_decode_mlp_fwd the MLP on given features c[B,N,C] (decoder.py:255-269).         */
int vt_sample_grid(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N,
                   int lattice_nx, float lattice_box, int64_t lattice_first, double padding,
                   float *feat, void *stream);
int vt_decode_mlp_fwd(const float *c, int B, int C, const float *pts, int64_t N,
                      int lattice_nx, float lattice_box, int64_t lattice_first,
                      const float *blob, float *out, void *stream);
/* the same with split-f16 layers (blob from vt_decoder_pack_f16x3; inference: 2.6x the f32 form's rate at f32-level logits) */
int vt_decode_mlp_fwd_f16x3(const float *c, int B, int C, const float *pts, int64_t N,
                            int lattice_nx, float lattice_box, int64_t lattice_first,
                            const float *blob_f16x3, float *out, void *stream);
/* ... and their training forms (autograd of decoder.py:237-271 around the fuser): the MLP forward   */
/* that saves activations (save: vt_decode_save_bytes), its backward to the features it was given      */
/* (grad_c [B,N,C]; parameter gradients: vt_decode_wgrad on the same save/gws), and the backward of     */
/* vt_sample_grid (scatter-add of grad_feat into grad_grid_cl, which the caller zeroes).                 */
int vt_decode_mlp_fwd_train(const float *c, int B, int C, const float *pts, int64_t N,
                            int lattice_nx, float lattice_box, int64_t lattice_first,
                            const float *blob, float *out, float *save, void *stream);
int vt_decode_mlp_bwd(int B, int C, const float *pts, int64_t N,
                      int lattice_nx, float lattice_box, int64_t lattice_first,
                      const float *blob_t, const float *grad_out, const float *save, float *gws,
                      float *grad_c, void *stream);
int vt_sample_grid_bwd(int B, int R, int C, const float *pts, int64_t N,
                       int lattice_nx, float lattice_box, int64_t lattice_first, double padding,
                       const float *grad_feat, float *grad_grid_cl, void *stream);
/* vt_sample_grid_bwd with the points grouped by trilinear cell: order / seg_lo / seg_hi from vt_voxel_build(pts, B, N, R - 1,       */
/* padding, ...) (a point's bin at resolution R - 1 is the cell whose eight corners it touches).  One wave per cell sums its points'    */
/* contributions in ascending point order and issues its atomics once per cell: the form for clustered query points (the contact        */
/* clouds of training.py:817-866 put up to 128 points of a scene into a few cells, whose per-point atomics collide).  Same sums.         */
/* The cells go in eight launches, one per parity of the cell's base node: cells of one parity share no node, so the (up to eight)       */
/* cell sums that meet at a node are added in a fixed order and the gradient is the same bit for bit in every run.                      */
int vt_sample_grid_bwd_sorted(int B, int R, int C, const float *pts, int64_t N, double padding, const float *grad_feat,
                              const int *order, const int *seg_lo, const int *seg_hi, float *grad_grid_cl, void *stream);
/* vt_decode_bwd_contact that leaves d c (the gradient of the sampled features, [B*N][32]) in `grad_c` instead of scattering it:  */
/* the caller scatters with vt_sample_grid_bwd_sorted (query points given explicitly; grad_out2 / grad_c_img may be NULL).            */
int vt_decode_bwd_dc(int B, int R, int C, const float *pts, int64_t N, double padding,
                     const float *blob_t, const float *grad_out, const float *grad_out2, const float *save, float *gws,
                     float *grad_c, float *grad_c_img, void *stream);

/* ------------------------------------------------------------------------- */
/* Plane features: the bilinear samples of the canonical planes (sample_planes.hip). */
/* Replaces: sample_plane_feature and the key walk around it at decoder.py:55-60, 135-147 */
/* (normalize_coordinate, src/common.py:268-291: divisor 1 + padding + 10e-6, values >= 1 become 1 - 10e-6, values < 0 */
/* become 0 -- not the 3-D constants; F.grid_sample with align_corners=True and border padding).                        */
/*   feat[B,N,C] = base? + xz? + xy? + yz?   summed in exactly that order.                                              */
/* xz / xy / yz: [B,C,R,R] float32 contiguous, NULL = absent, at least one present; all share one square R in [2, 1024];  */
/* C % 32 == 0, C <= 256.  The projected axes are vt_plane_build's (xz: x, z; xy: x, y; yz: y, z); the first indexes the   */
/* last (W) dimension.  base: optional [B,N,C] to add onto (the result of vt_sample_grid: the grid is the reference's first */
/* term), may alias feat.  Query points: pts [B,N,3], or NULL with the lattice (lattice_nx, lattice_box, lattice_first, N)  */
/* in vt_sample_grid's arithmetic (nx <= 1625: nx^3 below 2^32).  flags: VT_PLANES_NEAREST = mode 'nearest' (half to even) instead of 'bilinear';         */
/* VT_PLANES_LATTICE_POINTS = the lattice through the point kernel on generated coordinates instead of the per-plane tables */
/* of the nx^2 distinct samples (the same bits either way, and the same bits as the point form on the materialised lattice). */
/* workspace: vt_sample_planes_workspace_bytes(B, R, C, number of planes present, lattice_nx or 0) bytes, 16-byte aligned   */
/* like base and feat.  Bad arguments return VT_ERR_INVALID / VT_ERR_UNSUPPORTED / VT_ERR_WORKSPACE before any GPU call.    */
#define VT_PLANES_NEAREST 1
#define VT_PLANES_LATTICE_POINTS 2
/* VT_PLANES_PREPARED: the workspace still holds the channels-last copies (and, in table form, the tables) an earlier call left  */
/* there for the same planes, R, C, flags and lattice nx / box: the call skips that preparation (the slabs of one lattice, the     */
/* levels of one MISE extraction).  The caller vouches for it; a different lattice_first / N / pts / base is what may change.    */
#define VT_PLANES_PREPARED 4
size_t vt_sample_planes_workspace_bytes(int B, int R, int C, int n_planes, int lattice_nx);
int vt_sample_planes(const float *xz, const float *xy, const float *yz, int B, int R, int C,
                     const float *pts, int64_t N, int lattice_nx, float lattice_box, int64_t lattice_first,
                     double padding, int flags, const float *base, float *feat,
                     void *workspace, size_t workspace_bytes, void *stream);
/* Its backward (the autograd of decoder.py:55-60): grad_feat [B,N,C] -> grad_xz / grad_xy / grad_yz [B,C,R,R] for the     */
/* non-NULL outputs (at least one).  The outputs are WRITTEN, every element, not accumulated into: no pre-zeroed memory is  */
/* asked of the caller; a NULL output's plane is skipped.  Bilinear: four pixels with the forward's weights; nearest: one.   */
/* The gradient to base is grad_feat itself.  The points are grouped by bilinear cell (vt_plane_build_multi at R - 1) and    */
/* one wave per cell sums in ascending point order before its f32 atomics, so clustered points cost one atomic set per cell. */
/* Query points only (pts [B,N,3], not a lattice).  workspace: vt_sample_planes_bwd_workspace_bytes(B, N, R, C, number of    */
/* outputs) bytes, 16-byte aligned.                                                                                          */
size_t vt_sample_planes_bwd_workspace_bytes(int B, int64_t N, int R, int C, int n_planes);
int vt_sample_planes_bwd(int B, int R, int C, const float *pts, int64_t N, double padding, int flags,
                         const float *grad_feat, float *grad_xz, float *grad_xy, float *grad_yz,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* TransformerFusion forward (eval mode).                                       */
/* Replaces: self.fuser(c_img, 1, c, 1) at decoder.py:258, i.e.                  */
/*   TransformerFusion.forward (src/TransformerFusion.py:311-333) with           */
/*   num_layers=1, d_model=32, key_feature_dim=64, with_pos_embed=False:          */
/*   RelationUnit (:92-113, incl. the column re-normalisation :104),              */
/*   TransNonlinear (:21-25), InstanceNorm1d over the N points of the chunk.       */
/* self_attn is shared by the encoder layer and the decoder layer's               */
/* self-attention (the reference builds both from ONE module, :291-309).           */
/* c_img, c, out: [B,N,32].  Attention couples the N points of a chunk: N is part   */
/* of the function's definition.                             */
/* ------------------------------------------------------------------------- */
typedef struct vt_fusion_unit {
    const float *WK;         /* [64,32] head.0.WK.weight                              */
    const float *WQ;         /* [64,32] head.0.WQ.weight                              */
    const float *WV;         /* [32,32] head.0.WV.weight                              */
    const float *trans_conv; /* [32,32] head.0.trans_conv.weight                      */
    const float *linear1_w;  /* [64,32] extra_nonlinear.0.linear1.weight              */
    const float *linear1_b;  /* [64]                                                  */
    const float *linear2_w;  /* [32,64] extra_nonlinear.0.linear2.weight              */
    const float *linear2_b;  /* [32]                                                  */
    const float *norm2_w;    /* [32] extra_nonlinear.0.norm2.weight                   */
    const float *norm2_b;    /* [32]                                                  */
} vt_fusion_unit;

typedef struct vt_fusion_params {
    int32_t d_model;         /* 32 (every entry point) or 64 / 96 / 128 (vt_fusion_fwd only) */
    int32_t key_dim;         /* must be 64 */
    vt_fusion_unit self_attn;   /* fuser.encoder.layers.0.self_attn (== decoder.layers.0.self_attn) */
    vt_fusion_unit cross_attn;  /* fuser.decoder.layers.0.cross_attn                                 */
} vt_fusion_params;

size_t vt_fusion_workspace_bytes(int B, int N);
/* d_model beyond 32 (the reference's AttentionDecoder defaults to c_dim = d_model = 128, decoder.py:176-207; key_feature_dim stays 64):  */
/* vt_fusion_fwd takes d_model in {32, 64, 96, 128} (c_img, c, out: [B][N][d_model]; vt_fusion_unit's shapes with 32 -> d_model: WK / WQ  */
/* [64][d], WV / trans_conv [d][d], linear1 [64][d], linear2 [d][64], norm2 [d]) with a workspace of vt_fusion_workspace_bytes_wide.      */
/* Eval mode; the wider rows run generic-width projection / epilogue kernels around the same N x N passes.                                */
size_t vt_fusion_workspace_bytes_wide(int B, int N, int d_model);
int vt_fusion_fwd(const float *c_img, const float *c, int B, int N, const vt_fusion_params *params_host,
                  void *workspace, size_t workspace_bytes, float *out, void *stream);
/* The same forward with the tactile features of the decoder's self-attention given per point as a finger id (255 = none: a zero  */
/* row) and the [n_fingers][32] table -- what the reference gathers into c_img_all on the host (generation.py:159-255, consumed by */
/* AttentionDecoder.forward_img, decoder.py:237-271).  finger_ids [rows][N]; batch element b reads row chunk_index[b] (device      */
/* int32 [B]: the chunks a generator picked out of a lattice) or row b when chunk_index is NULL.  Equal to vt_fusion_fwd on the    */
/* gathered tensor bit for bit.                                                                                                    */
int vt_fusion_fwd_ids(const unsigned char *finger_ids, const float *finger_feats, int n_fingers, const int *chunk_index,
                      const float *c, int B, int N, const vt_fusion_params *params_host,
                      void *workspace, size_t workspace_bytes, float *out, void *stream);

/* ------------------------------------------------------------------------- */
/* TransformerFusion under autograd (training).                                  */
/* Replaces: PyTorch autograd of self.fuser(c_img, 1, c, 1) (decoder.py:258)      */
/*   triggered by loss.backward() at src/conv_onet/training.py:79,89,96:          */
/*   RelationUnit.forward (src/TransformerFusion.py:92-113: l2-normalised WK/WQ,  */
/*   softmax over keys, the column re-normalisation :104, WV, trans_conv, relu),  */
/*   TransNonlinear.forward (:21-25, with its two train-mode dropouts :13-19),     */
/*   the encoder / decoder layers' InstanceNorm1d + relu (:144-145, :209-218).      */
/* vt_fusion_fwd_train = vt_fusion_fwd that (a) applies the dropouts with          */
/*   probability p_drop (0 = eval), masks a pure function of `seed`, and            */
/*   (b) leaves, in `saved` (vt_fusion_saved_bytes, caller-owned, kept until the     */
/*   backward), per attention call the softmax row sums, column sums, value rows,     */
/*   attention outputs and pre-InstanceNorm sums -- O(N) state, never N x N.          */
/* vt_fusion_bwd: d_out [B,N,32] -> d_c_img, d_c [B,N,32] (overwritten) and the     */
/*   gradient of every parameter, written to the buffers of `grads` (overwritten;   */
/*   the self-attention unit is ONE module used twice, :291-309: its gradient is     */
/*   the sum of both uses).  The N x N scores are recomputed tile by tile on the      */
/*   matrix core; reductions are in a fixed order (bit-reproducible).                 */
/* vt_fusion_dropout_mask: the factors (0 or 1/(1-p)) the kernels apply for           */
/*   (call 0 = encoder self-attention, 1 = decoder self-attention, 2 = cross;          */
/*   which 0 = TransNonlinear.dropout [points,64], 1 = dropout2 [points,32]) --         */
/*   lets a test feed the same masks to a reference implementation.                     */
/* ------------------------------------------------------------------------- */
typedef struct vt_fusion_unit_grads {
    float *WK, *WQ, *WV, *trans_conv, *linear1_w, *linear1_b, *linear2_w, *linear2_b, *norm2_w, *norm2_b;
} vt_fusion_unit_grads;

typedef struct vt_fusion_grads {
    vt_fusion_unit_grads self_attn;
    vt_fusion_unit_grads cross_attn;
} vt_fusion_grads;

size_t vt_fusion_saved_bytes(int B, int N);
size_t vt_fusion_bwd_workspace_bytes(int B, int N);
int vt_fusion_fwd_train(const float *c_img, const float *c, int B, int N, const vt_fusion_params *params_host, float p_drop,
                        unsigned long long seed, void *workspace, size_t workspace_bytes, void *saved, size_t saved_bytes,
                        float *out, void *stream);
int vt_fusion_bwd(const float *d_out, const float *c_img, const float *c, int B, int N, const vt_fusion_params *params_host,
                  float p_drop, unsigned long long seed, const void *saved, size_t saved_bytes, void *workspace,
                  size_t workspace_bytes, float *d_c_img, float *d_c, const vt_fusion_grads *grads_host, void *stream);
int vt_fusion_dropout_mask(float p_drop, unsigned long long seed, int call, int which, int points, float *mask, void *stream);
/* d_model 64 / 96 / 128 under autograd (the reference trains AttentionDecoder at its defaults c_dim 128 / hidden 256 like any module,   */
/* decoder.py:176-207): vt_fusion_fwd_train / vt_fusion_bwd take those widths too (tensors [B][N][d_model], the unit's shapes with 32 ->   */
/* d_model), with `saved` of vt_fusion_saved_bytes_wide, workspaces of vt_fusion_workspace_bytes_wide / vt_fusion_bwd_workspace_bytes_wide.  */
/* The backward's three N x N passes are linear in their payload and run once per 32-channel slice of it (per-key / per-query scalars    */
/* enter with the first slice); the per-point parts are one-wave-per-point kernels with the weights in LDS; the weight gradients are        */
/* vt_rows_wgrad products.  Dropout masks of these widths: vt_fusion_dropout_mask_wide (which 1: [points][d_model]).                        */
size_t vt_fusion_saved_bytes_wide(int B, int N, int d_model);
size_t vt_fusion_bwd_workspace_bytes_wide(int B, int N, int d_model);
int vt_fusion_dropout_mask_wide(float p_drop, unsigned long long seed, int call, int which, int points, int d_model, float *mask, void *stream);
/* What a fuser call of B chunks of N points at d_model launches: the rule the vt_fusion_fwd* / vt_fusion_bwd launchers themselves take   */
/* their decisions from, asked without launching anything (host code; at d_model > 32 it reads the device's compute-unit count).  train:  */
/* vt_fusion_fwd_train / vt_fusion_bwd, otherwise vt_fusion_fwd / vt_fusion_fwd_ids.  Honours VTACO_FUSION_SCORE_TERMS as the launchers    */
/* do.  Any result pointer may be NULL:                                                                                                 */
/*   form              VT_FUSION_FORM_*: FULL all three half products of the scores (training forward, every d_model > 32), HALF_PAIR     */
/*                     the keys rounded to half (inference, N < 512), F8 rounded keys with the fp8 corrections (inference, N >= 512)      */
/*   proj_tiles        32-point tiles per wave of the forward projection kernel                                                         */
/*   inorm_streamed    1: the InstanceNorm kernel that re-reads its chunk (N > 2048, every d_model > 32), 0: the register-cached one      */
/*   fwd_row_blocks / bwd_row_blocks   workgroups per chunk of the forward (256 rows) / backward (128 rows) N x N passes                 */
/*   scalev_strided, epilogue_strided (d_model > 32), add_strided (backward), bwd_point_strided (backward, d_model > 32)                 */
/*                     1: that kernel's grid is at its cap and its workgroups walk the rest in a loop (the backward's: with train)      */
/* Returns 0, VT_ERR_INVALID (sizes) or VT_ERR_UNSUPPORTED (d_model).                                                                   */
#define VT_FUSION_FORM_FULL      0
#define VT_FUSION_FORM_HALF_PAIR 1
#define VT_FUSION_FORM_F8        2
int vt_fusion_plan(int B, int N, int d_model, int train, int *form, int *proj_tiles, int *inorm_streamed, int *fwd_row_blocks,
                   int *bwd_row_blocks, int *scalev_strided, int *epilogue_strided, int *add_strided, int *bwd_point_strided);

/* ------------------------------------------------------------------------- */
/* Backward of vt_decode_fwd (training).                                        */
/* Replaces: PyTorch autograd of LocalDecoder.forward / forward_img, triggered   */
/*   by loss.backward() at src/conv_onet/training.py:79,89,96 (grid_sampler_3d   */
/*   backward, addmm backward, relu backward).                                   */
/*   vt_decoder_pack_t : transposed-weight blob for the data gradient;           */
/*   vt_decode_bwd     : grad_out [B,N] -> grad_grid_cl [B,R,R,R,C] (ACCUMULATED  */
/*                       with f32 atomics: zero it first; may be NULL),           */
/*                       grad_c_img [B,N,C] (or NULL), and per-layer output       */
/*                       gradients in `gws` (vt_decode_gws_bytes);                */
/*   vt_decode_wgrad   : all parameter gradients into `grads`                     */
/*                       (vt_decode_wgrad_floats(p_in) floats, nn.Linear layout): */
/*                       fc_p.w[32*p_in] fc_p.b[32] fc_c.w[5][32*32] fc_c.b[5][32] */
/*                       fc_0.w[5][..] fc_0.b[5][32] fc_1.w[5][..] fc_1.b[5][32]   */
/*                       fc_out.w[32] fc_out.b[1]; p_in = 35 iff c_img != NULL.   */
/*                       Partials are summed in a fixed order: bit-reproducible.  */
/* Buffer layouts (P = B*N points, each slot P rows of 32 floats, row = point):  */
/*   save [12][P][32], written by vt_decode_fwd / vt_decode_mlp_fwd_train:        */
/*     slot 0       c, the sampled (or given) features                            */
/*     slots 1..5   relu(x_i), x_i the input of block i (fc_c_i(c) included)      */
/*     slots 6..10  relu(h_i), h_i = fc_0_i(relu(x_i))                            */
/*     slot 11      relu(net_5), the input of both output heads                   */
/*     (the values are the layer inputs of the weight gradients, their signs the  */
/*      ReLU masks of the data pass)                                              */
/*   gws [11][P][32], written by vt_decode_bwd / _dc / vt_decode_mlp_bwd, read by */
/*   vt_decode_wgrad:                                                             */
/*     slot 0       d x_0   (-> fc_p / fc_p_img and fc_c_0)                       */
/*     slots 1..5   d h_i   (-> fc_0_i, with save slot 1+i)                       */
/*     slots 6..10  d (output of block i) = d x_i+1, slot 10 = d net_5            */
/*                  (-> fc_1_i with save slot 6+i, and fc_c_i+1 with save slot 0) */
/* ------------------------------------------------------------------------- */
size_t vt_decoder_blob_t_bytes(int hidden, int c_dim, int n_blocks);
int vt_decoder_pack_t(const vt_decoder_params *params_host, float *blob_t, size_t blob_bytes, void *stream);
size_t vt_decode_save_bytes(int64_t total_points);
size_t vt_decode_gws_bytes(int64_t total_points);
int vt_decode_bwd(int B, int R, int C, const float *pts, int64_t N,
                  int lattice_nx, float lattice_box, int64_t lattice_first, double padding,
                  const float *blob_t, const float *grad_out, const float *save, float *gws,
                  float *grad_grid_cl, float *grad_c_img, void *stream);
size_t vt_decode_wgrad_workspace_bytes(int64_t total_points);
size_t vt_decode_wgrad_floats(int p_in);
int vt_decode_wgrad(int B, const float *pts, int64_t N, int lattice_nx, float lattice_box, int64_t lattice_first,
                    const float *c_img, const float *grad_out, const float *save, const float *gws,
                    void *workspace, size_t workspace_bytes, float *grads, void *stream);

/* The same two calls with the contact head (LocalDecoder.forward_contact under autograd,  */
/* decoder.py:105-133 -> training.py:896-948): grad_out2 [B,N] is the gradient of the      */
/* contact logits; `grads` has vt_decode_wgrad_floats_contact(p_in) floats: the layout     */
/* above followed by fc_out_contact.w[32] fc_out_contact.b[1].  blob_t must come from a    */
/* vt_decoder_pack_t call whose params carry fc_out2_w.  grad_out2 NULL = the plain calls. */
int vt_decode_bwd_contact(int B, int R, int C, const float *pts, int64_t N,
                          int lattice_nx, float lattice_box, int64_t lattice_first, double padding,
                          const float *blob_t, const float *grad_out, const float *grad_out2, const float *save, float *gws,
                          float *grad_grid_cl, float *grad_c_img, void *stream);
size_t vt_decode_wgrad_floats_contact(int p_in);
int vt_decode_wgrad_contact(int B, const float *pts, int64_t N, int lattice_nx, float lattice_box, int64_t lattice_first,
                            const float *c_img, const float *grad_out, const float *grad_out2, const float *save, const float *gws,
                            void *workspace, size_t workspace_bytes, float *grads, void *stream);

/* ------------------------------------------------------------------------- */
/* Marching cubes (Lewiner), vertex numbering identical to scikit-image's.      */
/* Replaces: skimage.measure.marching_cubes(value_grid,                         */
/*   gradient_direction='ascent') + the rescale `v -= nx/2; v *= 1.1/nx`        */
/*   (src/conv_onet/generation.py:268-272; src/conv_onet/inferencing.py:172-179).*/
/*                                                                             */
/* Two phases, because the output size is data dependent:                       */
/*   vt_mc_count  classifies the cells and scans the counts into `workspace`;   */
/*   vt_mc_read_counts copies {nverts, nfaces, level} to the host (this one      */
/*                SYNCHRONISES the stream -- skip it when capacities are known); */
/*   vt_mc_emit   writes verts [nverts,3] f32 (array-axis order, like skimage)   */
/*                and faces [nfaces,3] i32; entries beyond the capacities are    */
/*                dropped.  rescale != 0 applies (v - shift) * scale in f32.     */
/* vol is [n0,n1,n2] f32; auto_level != 0 uses skimage's default                */
/* 0.5*(min+max) instead of `level`.  workspace: vt_mc_workspace_bytes().       */
/* ------------------------------------------------------------------------- */
size_t vt_mc_workspace_bytes(int n0, int n1, int n2);
int vt_mc_count(const float *vol, int n0, int n1, int n2, double level, int auto_level,
                void *workspace, size_t workspace_bytes, void *stream);
int vt_mc_read_counts(const void *workspace, int *nverts_host, int *nfaces_host, double *level_host, void *stream);
/* the same read in two halves: _begin queues the copy (page-locked slot, an event right behind it) and returns a token; _end      */
/* waits for that event only -- launches made between the two (the speculative vt_mc_emit) run under the wait instead of in front  */
/* of it.  Sixteen tokens may be outstanding; a seventeenth _begin fails (VT_ERR_INVALID), _end spends its token.                 */
int vt_mc_read_counts_begin(const void *workspace, void *stream, int *token);
int vt_mc_read_counts_end(int token, int *nverts_host, int *nfaces_host, double *level_host);
/* vt_mc_count whose last kernel also writes the counts, the level and then a sequence number into a page-locked host slot: no copy */
/* command and no event in the stream (the emit kernels queued behind it start when the scan ends); returns the token               */
/* vt_mc_read_counts_end takes, which then polls the slot for that sequence number instead of waiting for an event.                 */
int vt_mc_count_notify(const float *vol, int n0, int n1, int n2, double level, int auto_level,
                       void *workspace, size_t workspace_bytes, void *stream, int *token);
/* The same for a scene whose launches are CAPTURED in a hipGraph (a kernel argument -- vt_mc_count_notify's sequence number -- would  */
/* be frozen into the graph): vt_mc_echo_slot makes a page-locked slot (outside the capture; it lives as long as the graph),            */
/* vt_mc_count_echo is vt_mc_count whose scan kernel reads the number to echo from that slot, vt_mc_echo_arm sets a fresh number        */
/* before every replay and vt_mc_echo_wait spins until the slot's header carries it, then returns the counts.  One replay in flight     */
/* per slot.  (No copy command and no event between the scan and the emit kernels: 19 us of a 0.9 ms scene.)                             */
int vt_mc_echo_slot(int *token);
/* vt_mc_echo_release hands a slot back once the graph that echoes into it has been destroyed (no replay in flight): the next   */
/* vt_mc_echo_slot reuses its page-locked block.                                                                                */
int vt_mc_echo_release(int token);
int vt_mc_count_echo(const float *vol, int n0, int n1, int n2, double level, int auto_level,
                     void *workspace, size_t workspace_bytes, void *stream, int token);
int vt_mc_echo_arm(int token);
int vt_mc_echo_wait(int token, void *stream, int *nverts_host, int *nfaces_host, double *level_host);
int vt_mc_emit(const float *vol, int n0, int n1, int n2, void *workspace,
               float *verts, int max_verts, int *faces, int max_faces,
               int rescale, float shift, float scale, void *stream);
/* vt_mc_emit_normals: the other half of `vertices, faces, normals, values = measure.marching_cubes(value_grid,                    */
/*   gradient_direction='ascent')` (src/conv_onet/generation.py:270; src/conv_onet/inferencing.py:174,316; Generator3D's            */
/*   with_normals, generation.py:34,46): normals [nverts,3] f32, unit, array-axis order, and values [nverts] f32, rows in the       */
/*   numbering of vt_mc_emit's vertices; rows beyond max_verts are dropped.  Runs behind vt_mc_count and vt_mc_emit on the same     */
/*   vol and workspace (it reads the triangle lists, ranks and vertex bases they left there); asynchronous, one launch, no atomics, */
/*   equal bits from run to run.  The rule is scikit-image 0.18.3's (tests/mc_normals_ref.py restates it): a normal that is zero    */
/*   or not finite is (0,0,0).  A uniform rescale of the vertices leaves the normals as they are.                                   */
int vt_mc_emit_normals(const float *vol, int n0, int n1, int n2, void *workspace, float *normals, float *values, int max_verts, void *stream);

/* ------------------------------------------------------------------------- */
/* Multiresolution isosurface extraction (MISE): one refinement step on the device.                                          */
/* Replaces: MultiGridExtractor (src/utils/mesh.py:7-84, with check_voxel_boundary, src/utils/voxels.py:222-257), which the   */
/*   reference keeps but never calls.  Grids are x-major [n][n][n] f32 (marching cubes' layout), lattice ids g = (x n + y) n + z, */
/*   coordinates box * linspace(-0.5, 0.5, n) computed as the decode kernels' lattice does.  n <= VT_MISE_MAX_N.                */
/* vt_mise_lattice: ids[g] = g (ids may be NULL) and pts[g] = the coordinates of lattice point g, for all n^3 points.          */
/* vt_mise_refine: from the coarse grid [nc]^3 to the fine grid [nf]^3, nf = 2 nc - 1.  active [(nc-1)^3] u8 (workspace, left  */
/*   holding the classification): a coarse voxel is active when its 8 corners are not all on one side of `level`, the side     */
/*   being marching cubes' own (double)v - level > 0 (the reference: v < threshold; they differ only where v equals the level). */
/*   fine[(x,y,z)] = coarse[(x/2, y/2, z/2)]; fine point (2i,2j,2l) is known where coarse_known [nc^3] u8 says (NULL: every    */
/*   coarse point known), the others are not.  An unknown fine point that is a corner of a fine voxel whose parent coarse voxel */
/*   is active is appended to the query list (qids [capacity] i32, qpts                                                         */
/*   [capacity][3] f32) in an order that varies from run to run.  *count (a device word, zeroed by the call) receives the      */
/*   number of query points; only the first `capacity` are written -- a count above it asks for a larger list and another     */
/*   call.  known [nf^3] u8 (the fine known mask before the query list is decoded) may be NULL.                                */
/* vt_mise_scatter: fine[ids[i]] = vals[i] (and known[ids[i]] = 1 when known is not NULL) for i < m; ids outside [0, total)    */
/*   are skipped.                                                                                                                */
#define VT_MISE_MAX_N 513
int vt_mise_lattice(int n, float box, int *ids, float *pts, void *stream);
int vt_mise_refine(const float *coarse, const unsigned char *coarse_known, int nc, double level, float box, unsigned char *active, float *fine,
                   unsigned char *known, int *qids, float *qpts, int64_t capacity, int *count, void *stream);
int vt_mise_scatter(const int *ids, const float *vals, int64_t m, float *fine, int64_t total, unsigned char *known,
                    void *stream);

/* ------------------------------------------------------------------------- */
/* Touch session: one touch merged into the id lattice an object keeps across touches.                                          */
/* Replaces: the carried-over c_img_all of Inferencer.inference_img / inference_img_t2d (src/conv_onet/inferencing.py:155-170,     */
/*   274-313): created at the first touch, every later touch writes its fingers' features where its fingers are.                 */
/* ids [nx^3] u8 holds per lattice point the ROW of the session's feature table, 255 = no row.  vt_touch_merge evaluates         */
/*   vt_tactile_assign's rule (same arguments, same arithmetic, lattice mode, first = 0) at every lattice point; where it names   */
/*   finger f, ids[g] = row_base + f and g is appended to the list (changed_ids [capacity] i32, changed_pts [capacity][3] f32: the */
/*   lattice's coordinates); every other ids[g] is left alone.  The list is in ASCENDING lattice order on every run.              */
/*   *n_changed (a device word) receives its length; only the first `capacity` entries are written -- a length above it asks for  */
/*   a larger list (the ids are merged either way, so a second call with the same arguments lists the same points).               */
/*   Only the part of the lattice the successful fingers' anchors (grown by the radius) can reach is visited.                     */
/*   row_base + F > 254 is VT_ERR_UNSUPPORTED, before any launch.  workspace: vt_touch_workspace_bytes(nx) bytes.                  */
/*   The decoded logits of the list go into the value lattice with vt_mise_scatter(changed_ids, logits, m, values, nx^3, NULL).   */
size_t vt_touch_workspace_bytes(int nx);
int vt_touch_merge(const float *anchors, const int *count, const unsigned char *success, int F, int K, int mode, double radius,
                   int nx, float box, int row_base, unsigned char *ids, int *changed_ids, float *changed_pts, int64_t capacity,
                   int *n_changed, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* PointNet local-pool voxeliser.                                              */
/* Replaces: normalize_3d_coordinate + coordinate2index (src/common.py:293-309, */
/*   333-348; call site src/encoder/pointnet.py:151-152), torch_scatter          */
/*   scatter_max + gather in pool_local (pointnet.py:116-132) and scatter_mean   */
/*   in generate_grid_features (pointnet.py:102-110), and their autograd.        */
/*                                                                             */
/* vt_voxel_build runs once per forward: idx[b,t] = ix + R*(iy + R*iz) (bit-exact */
/* with the reference's f32 maths), order[b,j] = point ids sorted by (voxel,      */
/* point), seg_lo/seg_hi[b,t] = the sorted range of t's voxel.  Up to 8192 points  */
/* per scene sort inside one workgroup's LDS (one launch); larger clouds take the  */
/* same stable radix sort through global memory (2 + 3 launches per five id bits). */
/* pool_max: out[b,t,c] = max_{t' in voxel(t)} feat[b,t',c], argmax = winning t'.  */
/* scatter_mean: grid[b,c,z,y,x] (NCDHW, zero-filled inside) = per-voxel mean.     */
/* All reductions run in ascending point order: bit-reproducible.                 */
/* ------------------------------------------------------------------------- */
int vt_voxel_build(const float *pts, int B, int T, int R, double padding,
                   int *idx, int *order, int *seg_lo, int *seg_hi, void *stream);
/* vt_voxel_build that also zero-fills `clear` (clear_bytes, both multiples of 16; e.g. the grid the scatter-mean fills next) with */
/* the workgroups the sort leaves idle: the torch.zeros of generate_grid_features (pointnet.py:102-110) without a launch of its own. */
int vt_voxel_build_clear(const float *pts, int B, int T, int R, double padding,
                         int *idx, int *order, int *seg_lo, int *seg_hi, void *clear, size_t clear_bytes, void *stream);
/* flags [B][(R/8)^3] bytes: bit 0 where no point of the scene lies in the 10^3 halo of that 8^3 voxel block, i.e. the mean grid  */
/* of generate_grid_features (pointnet.py:102-110) is zero over everything a 3x3x3 conv of the block reads; bit 1 where none lies */
/* in its 12^3 halo either (what a second 3x3x3 conv behind the first depends on): values 0, 1 and 3 (idx from vt_voxel_build;    */
/* R a multiple of 8, at most 128).  Consumed by vt_unet3d_fwd_skip / vt_conv3d_gcr_f16x3_skip (any non-zero flag skips there).  */
int vt_voxel_tile_flags(const int *idx, int B, int T, int R, unsigned char *flags, void *stream);
/* vt_voxel_build_clear (clear may be NULL with clear_bytes 0) that leaves those flags as well: the sorting workgroup marks the blocks */
/* while it computes the voxel ids (no launch of its own, no second pass over the points).                                       */
int vt_voxel_build_clear_flags(const float *pts, int B, int T, int R, double padding, int *idx, int *order, int *seg_lo, int *seg_hi,
                               void *clear, size_t clear_bytes, unsigned char *tile_flags, void *stream);
int vt_voxel_pool_max_fwd(const float *feat, const int *order, const int *seg_lo, const int *seg_hi,
                          int B, int T, int C, float *out, int *argmax, void *stream);
/* pool_local over K <= 4 cell partitions of the same points, summed in the order k = 0, 1, ... (the hand encoder's xz + xy + yz planes,    */
/* pointnet.py:116-132: `c += pooled`): out[b][t][c] = sum_k max of feat over t's cell in partition k; order / seg_lo / seg_hi / argmax:    */
/* host arrays of K device pointers (argmax, or its entries, may be NULL in the forward).  Same maxima and first arg-maxima as K calls of   */
/* vt_voxel_pool_max_fwd + K - 1 adds; one launch.  The backward sums, per partition in order, the cell's grad_out at its arg-max point.     */
int vt_voxel_pool_max_sum_fwd(const float *feat, int K, const int *const *order, const int *const *seg_lo, const int *const *seg_hi,
                              int B, int T, int C, float *out, int *const *argmax, void *stream);
int vt_voxel_pool_max_sum_bwd(const float *grad_out, int K, int *const *argmax, const int *const *order, const int *const *seg_lo,
                              const int *const *seg_hi, int B, int T, int C, float *grad_feat, void *stream);
/* pool_local with scatter_type = 'mean' (pointnet.py:64-69, 116-132: scatter_mean over the cells, gathered back to the points):  */
/* out[b][t][c] = mean of feat over the points of t's cell (cells of a volume or a plane: the segments of vt_voxel_build /          */
/* vt_plane_build).  Its backward is the same call on the gradient.                                                              */
int vt_voxel_pool_mean(const float *feat, const int *order, const int *seg_lo, const int *seg_hi, int B, int T, int C, float *out, void *stream);
int vt_voxel_pool_max_bwd(const float *grad_out, const int *argmax, const int *order,
                          const int *seg_lo, const int *seg_hi,
                          int B, int T, int C, float *grad_feat, void *stream);
int vt_voxel_scatter_mean_fwd(const float *feat, const int *idx, const int *order,
                              const int *seg_lo, const int *seg_hi,
                              int B, int T, int C, int R, float *grid, void *stream);
int vt_voxel_scatter_mean_bwd(const float *grad_grid, const int *idx, const int *seg_lo, const int *seg_hi,
                              int B, int T, int C, int R, float *grad_feat, void *stream);

/* ------------------------------------------------------------------------- */
/* UNet3D forward (inference), channels-last.                                   */
/* Replaces (SURVEY.md section 8f "next" row 1): the SingleConv 'gcr' blocks     */
/*   GroupNorm -> Conv3d(3,pad 1,no bias) -> ReLU (src/encoder/unet3d.py:20-72),  */
/*   MaxPool3d(2) (:219-238), nearest upsample + concat (:283-293, 321-323) and   */
/*   the final 1x1x1 conv (:440-441) of UNet3D.forward (:449-474).                */
/* All activations are [B,D,H,W,C] f32; channel counts multiples of 32.           */
/*   vt_conv3d_pack      Conv3d weight [Cout,Cin,3,3,3] -> MFMA fragment order;    */
/*   vt_gn_scale_shift   GroupNorm statistics of the (virtually concatenated)      */
/*                       input -> scale_shift[B][Cin][2];                          */
/*   vt_conv3d_gcr       out = relu?(conv3x3x3(x * scale + shift)), zero padding   */
/*                       applied after the normalisation; input = skip [..,C1],    */
/*                       optionally followed by `low` [B,D/2,H/2,W/2,C2]            */
/*                       nearest-upsampled (neither is materialised);               */
/*   vt_maxpool3d_cl, vt_conv1x1_cl: the remaining two layer types;                 */
/*   vt_voxel_scatter_mean_cl_fwd: scatter-mean writing the channels-last grid.     */
/* ------------------------------------------------------------------------- */
size_t vt_conv3d_packed_floats(int Cout, int Cin);
int vt_conv3d_pack(const float *w, int Cout, int Cin, float *packed, void *stream);
/* GroupNorm statistics travel as per-block partial sums part[B][nblk][C][2] = (sum, sumsq)   */
/* written by the PRODUCER of a tensor: vt_conv3d_gcr's epilogue (nblk =                       */
/* vt_conv3d_stat_blocks) or vt_channel_stats (any nblk) for pooled tensors / the input.       */
/* vt_gn_scale_shift reduces them in a fixed order into scale_shift[B][C1+C2][2]; part2 (may   */
/* be NULL) is the nearest-upsampled `low` source, whose sums count 8 times.                    */
size_t vt_stats_floats(int B, int D, int H, int W, int C);
int vt_conv3d_stat_blocks(int B, int D, int H, int W, int Cin, int Cout);
int vt_channel_stats(const float *x, int B, int64_t V, int C, int nblk, float *part, void *stream);
int vt_gn_scale_shift(const float *part1, int nblk1, int C1, const float *part2, int nblk2, int C2,
                      int B, int64_t voxels, int groups, const float *gamma, const float *beta, double eps,
                      float *scale_shift, void *stream);
int vt_conv3d_gcr(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                  const float *scale_shift, const float *packed_w, int Cout, int relu, float *out,
                  float *out_part, void *stream);
/* The whole UNet3D.forward (unet3d.py:449-474) in one call: encoder levels (max-pool from level 1  */
/* on, two gcr convs each), decoder levels (virtual upsample+concat, two gcr convs), final 1x1x1     */
/* conv.  `packed` = vt_conv3d_pack of the level's Conv3d weight.  x_cl [B,R,R,R,enc[0][0].cin].      */
#define VT_UNET_MAX_LEVELS 6
typedef struct vt_unet3d_conv {
    const float *gn_w;    /* groupnorm.weight [cin] */
    const float *gn_b;    /* groupnorm.bias   [cin] */
    const float *packed;  /* vt_conv3d_pack(conv.weight [cout,cin,3,3,3]) */
    int32_t cin, cout;
    const float *packed_bf16x3;  /* vt_conv3d_pack_bf16x3(conv.weight) or NULL: run this conv on the bf16 matrix core with */
                                 /* split-bf16 operands where vt_conv3d_stat_blocks_bf16x3(...) != 0, exact f32 elsewhere */
    const float *packed_f16x3;   /* vt_conv3d_pack_f16x3(conv.weight) or NULL: where vt_conv3d_stat_blocks_f16x3(...) != 0 this conv runs */
                                 /* the persistent split-f16 kernel (takes precedence over packed_bf16x3)                              */
    const float *packed_f16x3_thin; /* vt_conv3d_pack_f16x3_thin(conv.weight) or NULL: the shapes of packed_bf16x3 (the thin-tile and */
                                 /* K-split kernels) on IEEE-half pairs instead of bf16 pairs; takes precedence over packed_bf16x3     */
    const float *packed_f16x3_up;   /* decoder-entry layers (dec[k][0]) only, or NULL: vt_conv3d_pack_f16x3_up(conv.weight, C1 = the skip's */
                                 /* channels); where vt_conv3d_up_covers(...) the layer runs in per-parity form (vt_conv3d_gcr_f16x3_up)  */
} vt_unet3d_conv;
typedef struct vt_unet3d_params {
    int32_t n_levels;     /* len(f_maps) */
    int32_t groups;       /* num_groups (1 is used when a layer has fewer channels) */
    double eps;           /* GroupNorm eps */
    vt_unet3d_conv enc[VT_UNET_MAX_LEVELS][2];   /* encoders.{i}.basic_module.SingleConv{1,2} */
    vt_unet3d_conv dec[VT_UNET_MAX_LEVELS][2];   /* decoders.{k}.basic_module.SingleConv{1,2} */
    const float *final_w; /* final_conv.weight [out_channels, f_maps[0]] */
    const float *final_b; /* final_conv.bias or NULL */
    int32_t out_channels;
    const float *final_packed_f16x3; /* vt_conv1x1_pack_f16x3(final_w) or NULL: the final conv runs in the last layer's epilogue */
                                     /* where that layer is on the specialised-wave split-f16 kernel and both are 32 channels wide */
} vt_unet3d_params;
/* Split-bf16 form of vt_conv3d_pack / vt_conv3d_stat_blocks / vt_conv3d_gcr (same arguments): the 3x3x3 convolution  */
/* as W_lo*x_hi + W_hi*x_lo + W_hi*x_hi on the bf16 matrix core with f32 accumulation (hi = bf16(v), lo = bf16(v - hi));  */
/* GroupNorm, ReLU and the output statistics stay f32.  Covers volumes whose sides are multiples of 8 and that give at     */
/* least 64 workgroups of 8x8x8 / 8x8x4 (large levels) or 8x8x2 (16^3-class levels) tiles per cout block                   */
/* (stat_blocks returns 0 and gcr VT_ERR_UNSUPPORTED otherwise: use the f32 form).  6.6e-5 abs on the UNet3D golden       */
/* (scale 2.4), 4e-5 on the logits decoded from the resulting grid.                                                       */
int vt_conv3d_pack_bf16x3(const float *w, int Cout, int Cin, float *packed, void *stream);
int vt_conv3d_stat_blocks_bf16x3(int B, int D, int H, int W, int Cin, int Cout);
int vt_conv3d_gcr_bf16x3(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                         const float *scale_shift, const float *packed_w_bf16x3, int Cout, int relu, float *out,
                         float *out_part, void *stream);
/* K-split form of vt_conv3d_gcr_bf16x3 for the levels whose output tiles cannot fill the chip (the 16^3 and 8^3 levels of  */
/* ONE scene, unet3d.py:449-474 at num_levels 4): the 16-channel blocks of the input are dealt over 2-8 workgroups per     */
/* output tile, the raw partial sums go through `workspace` and a second launch adds them in slice order (bit-reproducible), */
/* applies the ReLU and writes the GroupNorm partial sums of every 128-voxel block (stat_blocks = D*H*W/128).  Same packed   */
/* weights as vt_conv3d_gcr_bf16x3.  workspace_bytes / stat_blocks return 0 where the plain kernels already fill the chip   */
/* (fewer than eight 16-channel blocks, or VTACO_CONV_KSPLIT=0): use them there.  One scene, both launches: 384->128 at   */
/* 16^3 77 -> 40 us, 128->128 at 16^3 29 -> 22 us, 128->128 / 128->256 at 8^3 33 -> 13 us (f32 K-split kernel before).          */
/* The same two kernels on IEEE-half hi + lo pairs (21-22 mantissa bits instead of 16; same fragment layout, sizes, coverage and    */
/* arguments): for the thin levels of a network whose large levels run the split-f16 kernels -- with bf16 pairs there they were  */
/* most of the encoder's remaining drift against the f32 reference.  Inputs are GroupNorm outputs: inside the half range.        */
int vt_conv3d_pack_f16x3_thin(const float *w, int Cout, int Cin, float *packed, void *stream);
int vt_conv3d_gcr_f16x3_thin(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                             const float *scale_shift, const float *packed_w_f16x3_thin, int Cout, int relu, float *out,
                             float *out_part, void *stream);
int vt_conv3d_gcr_f16x3_thin_ksplit(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                                    const float *scale_shift, const float *packed_w_f16x3_thin, int Cout, int relu, float *out,
                                    float *out_part, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_conv3d_ksplit_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout);
int vt_conv3d_stat_blocks_ksplit(int B, int D, int H, int W, int Cin, int Cout);
int vt_conv3d_gcr_bf16x3_ksplit(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                                const float *scale_shift, const float *packed_w_bf16x3, int Cout, int relu, float *out,
                                float *out_part, void *workspace, size_t workspace_bytes, void *stream);
/* Split-f16 form ("f16x3") for the large volumes (same reference layer: unet3d.py:20-72 SingleConv 'gcr'): operands as */
/* IEEE-half hi + lo pairs (21-22 mantissa bits: f32-rounding-level error on GroupNorm outputs and conv weights) on      */
/* v_mfma_f32_32x32x16_f16, in a persistent, double-buffered kernel: input channels in chunks of eight with a PAIR of     */
/* taps per MFMA k-step, the next chunk's image and weight fragments written to the other LDS buffer while the current    */
/* chunk's taps run, one barrier per chunk, workgroups walking their tiles of a scene without per-tile prologues; the       */
/* output's GroupNorm partial sums are per workgroup (stat_blocks = workgroups per scene).  Covers side lengths that are     */
/* multiples of 8 with >= 256 tiles of 8x8x8 or >= 128 tiles of 8x8x4 per launch (stat_blocks returns 0 otherwise).          */
/* The packed blob has its own size (28 instead of 27 tap slots per channel pair): vt_conv3d_packed_floats_f16x3.            */
/* vt_conv3d_gcr_f16x3 on a plain layer (no `low`) whose input is ZERO before the normalisation over the halo of the flagged 8^3    */
/* blocks (tile_flags [B][(D/8)(H/8)(W/8)], vt_voxel_tile_flags): the normalised input there is the per-channel shift, so a block's */
/* output is, per voxel, the sum over the taps inside the volume of T[tap][cout] = sum_cin W[cout][cin][tap] shift[cin] -- the     */
/* workgroups of a scene deal the blocks that need their taps among themselves and fill the others from T (the UNet3D's first      */
/* layer, unet3d.py:449-474 on the grid of pointnet.py:102-110: a 3000-point cloud leaves 3/4 of the 512 blocks of a 64^3 grid     */
/* empty).  Equal to the dense kernel to f32 rounding of T (the dense kernel sums the same products in another order).  Shapes    */
/* the specialised-wave kernel does not run, or lists of more than 64 blocks per workgroup, fall back to the dense walk.           */
int vt_conv3d_gcr_f16x3_skip(const float *x, int C, int B, int D, int H, int W, const float *scale_shift, const float *packed_w_f16x3,
                             int Cout, int relu, const unsigned char *tile_flags, float *out, float *out_part, void *stream);
size_t vt_conv3d_packed_floats_f16x3(int Cout, int Cin);
int vt_conv3d_pack_f16x3(const float *w, int Cout, int Cin, float *packed, void *stream);
/* the fragments of the conv that computes this layer's DATA GRADIENT (autograd of unet3d.py:20-72: conv_transpose = the forward    */
/* kernels on W with channels swapped and taps flipped) straight from w [Cout][Cin][27]: vt_conv3d_packed_floats_f16x3(Cin, Cout)   */
/* floats, equal to vt_conv3d_pack_f16x3 of w.flip(2,3,4).transpose(0,1) without that copy.                                         */
int vt_conv3d_pack_f16x3_t(const float *w, int Cout, int Cin, float *packed, void *stream);
int vt_conv3d_stat_blocks_f16x3(int B, int D, int H, int W, int Cin, int Cout);
int vt_conv3d_gcr_f16x3(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                        const float *scale_shift, const float *packed_w_f16x3, int Cout, int relu, float *out,
                        float *out_part, void *stream);
/* The same kernel for inputs far below the half range (the data-gradient convolution of the backward: dxn =           */
/* conv(g, W^T flipped) with g = dy * [y > 0], autograd of unet3d.py:20-72): `in_absmax` is a device scalar holding         */
/* max |input|; the kernel multiplies the input by the power of two that brings it to ~2^10 before the split and            */
/* divides the result by it (both exact), so the split keeps ~21 bits relative to the tensor's largest element.             */
int vt_conv3d_gcr_f16x3_scaled(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                               const float *scale_shift, const float *packed_w_f16x3, int Cout, int relu, float *out,
                               float *out_part, const float *in_absmax, void *stream);
/* Decoder-entry layers in per-parity form (reference unet3d.py:195-293: Decoder.forward = nearest upsample of the lower level,   */
/* torch.cat((encoder_features, x)), DoubleConv; :449-474 the call order).  The layer reads the virtual [skip | upsample(low)]; over   */
/* the upsampled channels a 3x3x3 conv is, per output parity class (x&1, y&1, z&1), a 2x2x2 conv over `low` itself with the taps that  */
/* share a low voxel summed in the weights -- 8 instead of 27 taps and a 6^3 instead of a 10^3 halo for those channels.  `packed_up`   */
/* = vt_conv3d_pack_f16x3_up(w [Cout][C1+C2][3][3][3], C1): the eight classes' merged taps of the low channels as half pairs           */
/* (vt_conv3d_up_packed_floats(Cout, C2) floats); the skip channels keep vt_conv3d_pack_f16x3's fragments (`packed_w_f16x3`, the       */
/* whole layer's blob).  Same arguments, statistics blocks and output as vt_conv3d_gcr_f16x3, equal to it to f32 rounding of the merged */
/* weights.  Covers what vt_conv3d_up_covers reports: a shape of the specialised-wave kernel with C1, C2 multiples of 16.              */
size_t vt_conv3d_up_packed_floats(int Cout, int C2);
int vt_conv3d_pack_f16x3_up(const float *w, int Cout, int Cin, int C1, float *packed, void *stream);
int vt_conv3d_up_covers(int C1, int C2, int B, int D, int H, int W, int Cout);
int vt_conv3d_gcr_f16x3_up(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                           const float *scale_shift, const float *packed_w_f16x3, const float *packed_up, int Cout, int relu, float *out,
                           float *out_part, void *stream);
/* The last 'gcr' layer of the UNet3D together with final_conv (unet3d.py:470-474, a 1x1x1 conv 32 -> 32): relu(conv) stays in      */
/* registers, is split into half pairs and multiplied by the packed final weight in the epilogue -- no intermediate tensor, no     */
/* second launch.  Cout must be 32 and the shape one the specialised-wave kernel covers (VT_ERR_UNSUPPORTED otherwise).            */
int vt_conv3d_final_fusable(int B, int D, int H, int W, int Cin, int Cout);   /* 1 where _final covers the layer */
int vt_conv1x1_pack_f16x3(const float *w, int Cout, int Cin, float *packed /* 1024 floats */, void *stream);
int vt_conv3d_gcr_f16x3_final(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                              const float *scale_shift, const float *packed_w_f16x3, int Cout,
                              const float *final_packed_f16x3, const float *final_b, float *out, void *stream);
/* the same launch, and relu(conv(...)) itself to `y_keep` [B,D,H,W,32]: the training forward keeps the last layer's output for its     */
/* backward and for vt_conv1x1_bwd_masked (reference: the same two modules under autograd, src/conv_onet/training.py:757-894)            */
int vt_conv3d_gcr_f16x3_final_keep(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                                   const float *scale_shift, const float *packed_w_f16x3, int Cout,
                                   const float *final_packed_f16x3, const float *final_b, float *out, float *y_keep, void *stream);
size_t vt_unet3d_workspace_bytes(int B, int R, const vt_unet3d_params *params_host);
int vt_unet3d_fwd(const float *x_cl, int B, int R, const vt_unet3d_params *params_host,
                  void *workspace, size_t workspace_bytes, float *out, void *stream);
/* the same with the input's GroupNorm partial sums supplied by its producer (in_part [B][in_nblk][C][2], e.g. from                 */
/* vt_pointnet_mlp_fused): no statistics pass over the input grid.                                                              */
int vt_unet3d_fwd_stats(const float *x_cl, const float *in_part, int in_nblk, int B, int R, const vt_unet3d_params *params_host,
                        void *workspace, size_t workspace_bytes, float *out, void *stream);
/* vt_unet3d_fwd / vt_unet3d_fwd_stats (in_part may be NULL: statistics pass over x) with the first layer's empty blocks skipped:   */
/* tile_flags [B][(R/8)^3] from vt_voxel_tile_flags on the cloud that x was scattered from (vt_conv3d_gcr_f16x3_skip).  Where the    */
/* first DoubleConv is 32 -> 32 -> 32 channels with 8 groups (unet3d.py:96-127, the shipped f_maps) the SECOND layer skips the       */
/* blocks whose 12^3 halo is empty (flag bit 1) as well: the first layer's output is a constant per border class around them, so    */
/* the second's is one per class of a two-voxel rim (125 classes) -- sums over taps of W2 gamma2 relu(K1), W2 gamma2 and W2 beta2     */
/* that the first launch leaves per GroupNorm group, combined with the second GroupNorm's statistics by the second launch.          */
/* vt_unet3d_skip_layers: how many layers of this network take the flags at this batch and resolution (0, 1 or 2).                 */
int vt_unet3d_skip_layers(int B, int R, const vt_unet3d_params *params_host);
int vt_unet3d_fwd_skip(const float *x_cl, const float *in_part, int in_nblk, const unsigned char *tile_flags, int B, int R,
                       const vt_unet3d_params *params_host, void *workspace, size_t workspace_bytes, float *out, void *stream);
int vt_maxpool3d_cl(const float *x, int B, int D, int H, int W, int C, float *out, void *stream);
/* the same max-pool and, from the same pass, the pooled tensor's GroupNorm partial sums as vt_channel_stats would leave them   */
/* (bit-identical: same blocks, same order): part [B][nblk][C][2].                                                          */
int vt_maxpool3d_cl_stats(const float *x, int B, int D, int H, int W, int C, float *out, int nblk, float *part, void *stream);
int vt_conv1x1_cl(const float *x, int64_t V, int Cin, const float *w, const float *bias, int Cout, float *out, void *stream);
int vt_voxel_scatter_mean_cl_fwd(const float *feat, const int *idx, const int *order,
                                 const int *seg_lo, const int *seg_hi,
                                 int B, int T, int C, int R, float *grid_cl, void *stream);
int vt_voxel_scatter_mean_cl_bwd(const float *grad_grid_cl, const int *idx, const int *seg_lo, const int *seg_hi,
                                 int B, int T, int C, int R, float *grad_feat, void *stream);


/* ------------------------------------------------------------------------- */
/* UNet3D backward (training), channels-last.                                   */
/* Replaces: PyTorch autograd of the 'gcr' SingleConv, MaxPool3d and the        */
/*   upsample+concat of src/encoder/unet3d.py:20-72, 219-238, 283-293, run by    */
/*   loss.backward() (src/conv_onet/training.py:79,89,96).  For one block         */
/*   y = relu(conv(xn)), xn = GroupNorm([skip | upsample(low)]) and a gradient dy: */
/*   vt_relu_mask      g = dy where y > 0, else 0;                                 */
/*   (data gradient)   dxn = vt_conv3d_gcr[_bf16x3](g, pack(W^T flipped), no norm, */
/*                     no relu): the forward kernels on repacked weights;           */
/*   vt_conv3d_wgrad   dW[Cout][Cin][3][3][3] = sum_v g[v] (x) xn[v+tap] (xn is      */
/*                     re-normalised from skip/low with the forward scale_shift);     */
/*   vt_gn_bwd         GroupNorm backward from dxn: dskip [B,D,H,W,C1], dlow           */
/*                     [B,D/2,H/2,W/2,C2] (children summed; either may be NULL),        */
/*                     dgb[B][C][2] = per-scene (dgamma, dbeta); part1/part2 are the     */
/*                     FORWARD statistics of skip/low; bpart [B][nblkb][C][2] and coef    */
/*                     [B][C][3] are scratch;                                              */
/*   vt_maxpool3d_cl_bwd  routes dy to the first maximum of each 2x2x2 window.             */
/* ------------------------------------------------------------------------- */
int vt_relu_mask(const float *dy, const float *y, float *g, int64_t n, void *stream);
/* the same, and *absmax = max |g| (device scalar; feeds the power-of-two rescale of the split-half data / weight gradient kernels) */
int vt_relu_mask_absmax(const float *dy, const float *y, float *g, int64_t n, float *absmax, void *stream);
/* Backward of the UNet3D's final 1x1x1 conv (32 -> 32 channels; reference: src/encoder/unet3d.py final_conv under autograd,           */
/* src/conv_onet/training.py:757-894) fused with the ReLU mask of the layer in front of it: dout, y [n,32] (y = that layer's ReLU        */
/* output = the conv's input), w [32,32] (out, in).  g[v] = (y[v] > 0) * (dout[v] W), *absmax = max |g| (device scalar, or NULL),         */
/* dw [32,32] = dout^T y, db [32] = column sums of dout (either may be NULL).  Exact f32 (v_mfma_f32_32x32x2_f32), fixed summation        */
/* order.  One pass over dout and y instead of the framework's GEMM + vt_relu_mask_absmax + batched GEMM + two reductions.               */
size_t vt_conv1x1_bwd_workspace_bytes(void);
int vt_conv1x1_bwd_masked(const float *dout, const float *y, const float *w, int64_t n, float *g, float *absmax, float *dw, float *db,
                          void *workspace, size_t workspace_bytes, void *stream);
size_t vt_conv3d_wgrad_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout);
int vt_conv3d_wgrad(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                    const float *scale_shift, const float *g, int Cout, void *workspace, size_t workspace_bytes,
                    float *dw, void *stream);
/* vt_conv3d_wgrad on the f16 matrix core with split (hi + lo IEEE-half) operands, f32 accumulation: the same dW to f32     */
/* rounding level (<= 1e-5 relative on the block tests), ~3x faster at 64^3 (MFMA rate 16x the f32 core's, three products).     */
/* `g_absmax`: device scalar max |g| (or NULL) -- g is scaled by the power of two that brings it to ~2^10 before the split        */
/* (output gradients sit far below the half range) and dW scaled back, both exactly.  Sides: D even, H and W multiples of 8        */
/* (workspace_bytes returns 0 otherwise: use vt_conv3d_wgrad).  Chunk-ordered reduction: bit-reproducible.                          */
size_t vt_conv3d_wgrad_f16x3_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout);
int vt_conv3d_wgrad_f16x3(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                          const float *scale_shift, const float *g, int Cout, const float *g_absmax,
                          void *workspace, size_t workspace_bytes, float *dw, void *stream);
/* The same dW for a decoder-entry layer [skip | nearest-upsample(low)] (reference: src/encoder/unet3d.py:283-293 under autograd):     */
/* the skip channels as vt_conv3d_wgrad_f16x3; the upsampled channels per output parity class -- tap t of voxel 2 u + p reads the     */
/* low-resolution voxel u + ((p + t) >> 1), so each class is a 2 x 2 x 2-tap weight gradient over the low-resolution grid (64          */
/* products of N / 8 voxels instead of 27 of N), summed into the 27 taps by the reduction in a fixed order.  Sides in multiples of     */
/* 16 (D: 4), channels of 32 (workspace_bytes returns 0 otherwise: use vt_conv3d_wgrad_f16x3).                                          */
size_t vt_conv3d_wgrad_f16x3_up_workspace_bytes(int B, int D, int H, int W, int C1, int C2, int Cout);
int vt_conv3d_wgrad_f16x3_up(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                             const float *scale_shift, const float *g, int Cout, const float *g_absmax,
                             void *workspace, size_t workspace_bytes, float *dw, void *stream);
/* The same dW for a layer whose input x [B,D,H,W,C] is EXACTLY zero over most of the volume -- the UNet3D's first layer on a scene's */
/* mean grid (reference: src/encoder/pointnet.py:102-114 leaves >= 98.8 % of the grid zero; its gradient, src/conv_onet/training.py   */
/* :757-894).  xn = x * scale + shift inside the volume, 0 outside, so dW = sum_v g[v] (x * scale)[v + tap] + shift * (sum of g over   */
/* the voxels whose tap neighbour is inside): the first sum runs over the 8 x 8 x 2 tiles of the blocks `tile_flags` does not mark     */
/* (vt_voxel_build_clear_flags: bit 0 = no point in the block's 10^3 halo) only, in ascending tile order (bit-reproducible); the       */
/* second is 27 box sums of g per scene times the shift, added by the reduction.  Sides in multiples of 8, channels of 32.            */
size_t vt_conv3d_wgrad_f16x3_sparse_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout);
int vt_conv3d_wgrad_f16x3_sparse(const float *x, int C, int B, int D, int H, int W, const float *scale_shift,
                                 const unsigned char *tile_flags, const float *g, int Cout, const float *g_absmax,
                                 void *workspace, size_t workspace_bytes, float *dw, void *stream);
int vt_gn_bwd(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
              const float *part1, int nblk1, const float *part2, int nblk2,
              const float *dxn, int groups, const float *gamma, double eps,
              float *bpart, int nblkb, float *coef, float *dgb, float *dskip, float *dlow, void *stream);
/* The data-gradient conv of a plain 'gcr' layer (autograd of unet3d.py:20-72: the forward kernels on the weight with channels      */
/* swapped and taps flipped, vt_conv3d_pack_f16x3_t) that also leaves the GroupNorm backward's two sums: out_part                  */
/* [B][vt_conv3d_xstats_blocks][Cout][2] = per workgroup (sum dxn, sum dxn * stat_x) with stat_x [B][D][H][W][Cout] the layer's     */
/* input -- what vt_gn_bwd's statistics pass over dxn and x computes, from the conv's epilogue.  vt_gn_bwd_from_part is            */
/* vt_gn_bwd_masked on such sums (bpart, nblkb = the blocks count) without that pass.  vt_conv3d_xstats_blocks: 0 where the shape    */
/* is not on the specialised-wave kernel (use vt_conv3d_gcr_f16x3_scaled + vt_gn_bwd).                                              */
int vt_conv3d_xstats_blocks(int B, int D, int H, int W, int Cin, int Cout);
int vt_conv3d_gcr_f16x3_xstats(const float *g, int C, int B, int D, int H, int W, const float *packed_w_f16x3, int Cout,
                               const float *in_absmax, const float *stat_x, float *out, float *out_part, void *stream);
int vt_gn_bwd_from_part(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                        const float *part1, int nblk1, const float *part2, int nblk2,
                        const float *dxn, int groups, const float *gamma, double eps,
                        const float *bpart, int nblkb, float *coef, float *dgb, float *dskip, float *dlow,
                        int mask_flags, float *absmax_skip, float *absmax_low, float *dgb_sum, void *stream);
/* vt_gn_bwd that also does the relu_mask pass of the layer(s) in front (autograd of unet3d.py:20-72: ReLU behind the conv whose   */
/* output this GroupNorm reads).  mask_flags bit 0: `skip` is such a ReLU output and dskip is its only gradient -- dskip comes out  */
/* as (skip > 0 ? dskip : 0) with max |dskip| in the device scalar absmax_skip, exactly what vt_relu_mask_absmax(dskip, skip)      */
/* would leave; bit 1: the same for `low` / dlow / absmax_low.  The layer in front then skips its vt_relu_mask_absmax.             */
/* dgb_sum (or NULL; needs dskip or dlow): [2][C] = (dgamma, dbeta) summed over the scenes in scene order (dgb keeps them per scene). */
int vt_gn_bwd_masked(const float *skip, int C1, const float *low, int C2, int B, int D, int H, int W,
                     const float *part1, int nblk1, const float *part2, int nblk2,
                     const float *dxn, int groups, const float *gamma, double eps,
                     float *bpart, int nblkb, float *coef, float *dgb, float *dskip, float *dlow,
                     int mask_flags, float *absmax_skip, float *absmax_low, float *dgb_sum, void *stream);
int vt_maxpool3d_cl_bwd(const float *x, const float *dy, int B, int D, int H, int W, int C, float *dx, void *stream);
/* The gradient of an encoder level's output y (unet3d.py:449-474: it feeds the next level's max-pool AND the decoder's skip) in one  */
/* pass: g = (y > 0 ? dskip + maxpool_backward(dpooled) : 0) -- vt_maxpool3d_cl_bwd, the framework's add of the two gradients and    */
/* the vt_relu_mask_absmax of the layer that produced y -- with max |g| in the device scalar absmax (or NULL).                        */
int vt_maxpool3d_cl_bwd_fork(const float *y, const float *dskip, const float *dpooled, int B, int D, int H, int W, int C, float *g,
                             float *absmax, void *stream);

/* ------------------------------------------------------------------------- */
/* Hand branch (SURVEY.md section 8f "next" row 3).                              */
/* Plane-mode PointNet: replaces normalize_coordinate + coordinate2index('2d')   */
/*   (src/common.py:268-291, 333-345; call sites src/encoder/pointnet.py:141-149) */
/*   and the scatter_mean of generate_plane_features (pointnet.py:85-95).         */
/*   vt_plane_build: plane 0 = 'xz', 1 = 'xy', 2 = 'yz'; idx[b,t] = i(first axis)  */
/*   + R * i(second axis) with the plane constants (divisor 1 + padding + 10e-6,    */
/*   upper clamp 1 - 10e-6); order/seg_lo/seg_hi as vt_voxel_build, so the          */
/*   vt_voxel_pool_max_* kernels serve every plane (pool_local, pointnet.py:116-132, */
/*   sums the per-plane results).  vt_plane_scatter_mean_*: plane [B,C,R,R].          */
/* MANO layer: replaces ManoLayer.forward (src/encoder/manolayer.py:160-364) for the  */
/*   shipped configuration (axis-angle root + joints, use_pca False, hands_mean added, */
/*   model betas, no translation; right hand, or left with vt_mano_pack_side).  vt_mano_pack lays the model out once: */
/*   v_template [778,3], shapedirs [778,3,10] + betas [10] (both may be NULL: betas 0), */
/*   posedirs [778,3,135], j_regressor [16,778] dense, weights [778,16], hands_mean [45] */
/*   -> blob[VT_MANO_BLOB_FLOATS].  vt_mano_fwd: pose [B,48] = root axis-angle + 45 joint */
/*   angles -> verts [B,778,3], joints [B,21,3], both minus joint center_idx (-1: none).   */
/* ------------------------------------------------------------------------- */
#define VT_MANO_BLOB_FLOATS 330240
int vt_plane_build(const float *pts, int B, int T, int R, double padding, int plane,
                   int *idx, int *order, int *seg_lo, int *seg_hi, void *stream);
/* The planes of a scene side by side in ONE launch: `planes` = n_planes ids (0 xz, 1 xy, 2 yz); idx / order / seg_lo / seg_hi are       */
/* [n_planes][B][T], slice k = what vt_plane_build(plane = planes[k]) writes (the hand encoder builds all three per forward).            */
int vt_plane_build_multi(const float *pts, int B, int T, int R, double padding, int n_planes, const int *planes,
                         int *idx, int *order, int *seg_lo, int *seg_hi, void *stream);
/* generate_plane_features (pointnet.py:85-95) for those planes in one launch each way: planes / grad_planes [n_planes][B][C][R*R] (the      */
/* layout of torch.cat over the planes' [B,C,R,R] tensors: what the hand encoder hands its U-Net), index arrays as above; the backward sums */
/* the planes' shares per point in plane order.                                                                                              */
int vt_plane_scatter_mean_multi_fwd(const float *feat, int n_planes, const int *idx, const int *order, const int *seg_lo, const int *seg_hi,
                                    int B, int T, int C, int R, float *planes, void *stream);
int vt_plane_scatter_mean_multi_bwd(const float *grad_planes, int n_planes, const int *idx, const int *seg_lo, const int *seg_hi,
                                    int B, int T, int C, int R, float *grad_feat, void *stream);
int vt_plane_scatter_mean_fwd(const float *feat, const int *idx, const int *order,
                              const int *seg_lo, const int *seg_hi,
                              int B, int T, int C, int R, float *plane, void *stream);
int vt_plane_scatter_mean_bwd(const float *grad_plane, const int *idx, const int *seg_lo, const int *seg_hi,
                              int B, int T, int C, int R, float *grad_feat, void *stream);
int vt_mano_pack(const float *v_template, const float *shapedirs, const float *betas, const float *posedirs,
                 const float *j_regressor, const float *weights, const float *hands_mean, float *blob, void *stream);
/* the same with the hand's side: left != 0 marks a MANO_LEFT model, whose middle-finger tip is vertex 445 instead of 444            */
/* (manolayer.py:327-330); the side travels in the blob, vt_mano_fwd / vt_mano_bwd read it there                                      */
int vt_mano_pack_side(const float *v_template, const float *shapedirs, const float *betas, const float *posedirs,
                      const float *j_regressor, const float *weights, const float *hands_mean, int left, float *blob, void *stream);
int vt_mano_fwd(const float *pose, int B, const float *blob, int center_idx, float *verts, float *joints, void *stream);
/* Backward of vt_mano_fwd (PyTorch autograd through manolayer.py:186-347 under loss_mano / loss_pc, training.py:59-60):   */
/* dpose [B,48] from dverts [B,778,3] and djoints [B,21,3]; one workgroup per hand, the forward's intermediates recomputed,  */
/* every sum in a fixed order (bit-reproducible).                                                                          */
int vt_mano_bwd(const float *pose, int B, const float *blob, int center_idx, const float *dverts, const float *djoints,
                float *dpose, void *stream);

/* ------------------------------------------------------------------------- */
/* The hand encoder's 2-D U-Net over its feature planes.    */
/* Replaces: UNet.forward (src/encoder/unet.py:220-233: DownConv :52-79,         */
/*   UpConv :82-120, conv_final) as LocalPoolPointnet builds and calls it         */
/*   (src/encoder/pointnet.py:49-50, 96-99): UNet(c_dim, in_channels=c_dim,        */
/*   depth, start_filts, merge_mode 'concat', up_mode 'transpose') on the planes   */
/*   [B, c_dim, R, R] of a scene -- here on n_img images at once (the net has no   */
/*   cross-image operation): x [n_img][in_channels][H][W] -> out [n_img][classes]  */
/*   [H][W], both NCHW like the reference's tensors.                               */
/* One launch per layer of ONE kernel template (implicit GEMM on the f32 matrix     */
/*   core: a workgroup per 32 pixels x 32 output channels, K split over its waves); */
/*   bias + ReLU in the epilogue, the 2x2 max-pool and the skip concat in the next  */
/*   layer's loader (no pass of their own).  Weights in nn.Conv2d /                 */
/*   nn.ConvTranspose2d layout; vt_plane_unet_pack lays them out in fragment order */
/*   (blob of vt_plane_unet_blob_bytes; repack after every weight update).         */
/* Covered (vt_plane_unet_supported): depth 2..5; in_channels, start_filts and     */
/*   num_classes multiples of 32; H, W powers of two with at least 4 x 4 pixels at */
/*   the bottom level.  After the call the workspace holds every layer's           */
/*   channels-last activations: vt_plane_unet_bwd reads them (the training forward */
/*   is this same call).                                                           */
/* ------------------------------------------------------------------------- */
#define VT_PLANE_UNET_MAX_DEPTH 5
typedef struct vt_plane_unet_params {
    int32_t depth, in_channels, start_filts, num_classes;
    const float *down_w[VT_PLANE_UNET_MAX_DEPTH][2];   /* down_convs.{l}.conv{1,2}.weight [Cout][Cin][3][3] */
    const float *down_b[VT_PLANE_UNET_MAX_DEPTH][2];
    const float *up_tw[VT_PLANE_UNET_MAX_DEPTH];        /* up_convs.{u}.upconv.weight [Cin][Cout][2][2]      */
    const float *up_tb[VT_PLANE_UNET_MAX_DEPTH];
    const float *up_w[VT_PLANE_UNET_MAX_DEPTH][2];      /* up_convs.{u}.conv{1,2}.weight                     */
    const float *up_b[VT_PLANE_UNET_MAX_DEPTH][2];
    const float *final_w, *final_b;                     /* conv_final [classes][start_filts][1][1]           */
} vt_plane_unet_params;
int vt_plane_unet_supported(int depth, int in_channels, int start_filts, int num_classes, int H, int W);
size_t vt_plane_unet_blob_bytes(int depth, int in_channels, int start_filts, int num_classes);
size_t vt_plane_unet_workspace_bytes(int depth, int in_channels, int start_filts, int num_classes, int n_img, int H, int W);
int vt_plane_unet_pack(const vt_plane_unet_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_plane_unet_fwd(const float *x, int n_img, int H, int W, const vt_plane_unet_params *dims_host, const float *blob,
                      void *workspace, size_t workspace_bytes, float *out, void *stream);
/* Backward of vt_plane_unet_fwd (PyTorch autograd through UNet.forward under the hand encoder's losses, loss_mano / loss_pc,   */
/* src/conv_onet/training.py:59-60, 79-96): from dout [n_img][classes][H][W], the input x, the packed weights and the forward's   */
/* workspace (its activations) -> dx [n_img][in_channels][H][W] and the gradient of every weight and bias in the parameter's own   */
/* layout (vt_plane_unet_grads: the pointers of vt_plane_unet_params, written, not accumulated).  Per layer, in reverse: one       */
/* data-gradient launch of the forward's kernel template (mirrored taps, transposed weights: the second half of the blob) whose     */
/* loader assembles the layer's output gradient from what its consumers left -- the skip concat's and the pooled path's sum, the     */
/* max-pool's routing to the window's first maximum, the ReLU mask -- and one weight-gradient launch (pixels as K, partial sums per   */
/* pixel slice); one finalize launch sums the slices.  Every sum in a fixed order: bit-reproducible.                                   */
typedef struct vt_plane_unet_grads {
    float *down_w[VT_PLANE_UNET_MAX_DEPTH][2], *down_b[VT_PLANE_UNET_MAX_DEPTH][2];
    float *up_tw[VT_PLANE_UNET_MAX_DEPTH], *up_tb[VT_PLANE_UNET_MAX_DEPTH];
    float *up_w[VT_PLANE_UNET_MAX_DEPTH][2], *up_b[VT_PLANE_UNET_MAX_DEPTH][2];
    float *final_w, *final_b;
} vt_plane_unet_grads;
size_t vt_plane_unet_bwd_workspace_bytes(int depth, int in_channels, int start_filts, int num_classes, int n_img, int H, int W);
int vt_plane_unet_bwd(const float *x, int n_img, int H, int W, const vt_plane_unet_params *dims_host, const float *blob,
                      const void *fwd_workspace, const float *dout, void *workspace, size_t workspace_bytes,
                      const vt_plane_unet_grads *grads_host, float *dx, void *stream);

/* ------------------------------------------------------------------------- */
/* Tactile feature encoder, eval mode (resnet2d.hip).  Replaces                  */
/*   ResNet.forward with BasicBlocks (src/layers.py:54-207: conv1 7x7/2, bn1,     */
/*   relu, maxpool 3x3/2, layer1..4, avgpool, flatten, linear, fc :176-190), as   */
/*   ConvolutionalOccupancyNetwork.encode_img_inputs calls it on the five tactile  */
/*   images of a scene (src/conv_onet/models/__init__.py:115-136), with the        */
/*   BatchNorm layers in eval mode (running statistics):                          */
/*   x [n_img][3][H][W] (NCHW) -> out [n_img][num_classes].                        */
/* vt_resnet_pack folds every BatchNorm into the conv before it (f64) and writes   */
/*   the folded weights in fragment order (blob of vt_resnet_blob_bytes; repack    */
/*   after every change of a weight OR a running statistic).  vt_resnet_fwd is     */
/*   2 + 2 * (number of blocks) launches: the stem with the max-pool in its        */
/*   epilogue, one launch per 3x3 conv (bias, residual and ReLU in the epilogue;   */
/*   a stage's 1x1 stride-2 projection rides in its first conv's launch), one      */
/*   tail (average pool, linear, fc).  Exact-f32 matrix core throughout; every     */
/*   sum in a fixed order that does not depend on n_img: bit-reproducible, and an  */
/*   image's features are the same bits in any batch.                             */
/* Covered (vt_resnet_supported): blocks_num entries 1..VT_RESNET_MAX_BLOCKS,      */
/*   num_classes 1..65536, 1 <= n_img <= 1024, 1 <= H, W <= 2048 (any values, odd  */
/*   included), every tensor below 2^31 elements.  Unsupported: the size queries   */
/*   return 0.  Workspace: four buffers of max over the stages s = 0..3 of         */
/*   n_img * Hs * Ws * (64 << s) floats, Hs = ceil(H / 2^(s+2)), Ws alike.         */
/* ------------------------------------------------------------------------- */
#define VT_RESNET_MAX_BLOCKS 36
typedef struct vt_resnet_bn {          /* nn.BatchNorm2d: weight, bias, running_mean, running_var [C]; eps */
    const float *weight, *bias, *running_mean, *running_var;
    double eps;
} vt_resnet_bn;
typedef struct vt_resnet_block {       /* layer{s}.{b}: conv1 [Cout][Cin][3][3], conv2 [Cout][Cout][3][3]     */
    const float *conv1_w;
    vt_resnet_bn bn1;
    const float *conv2_w;
    vt_resnet_bn bn2;
    const float *down_w;               /* downsample.0.weight [Cout][Cin][1][1] (first block of layer2..4), else NULL */
    vt_resnet_bn down_bn;              /* downsample.1 */
} vt_resnet_block;
typedef struct vt_resnet_params {
    int32_t blocks_num[4];
    int32_t num_classes;
    const float *conv1_w;              /* conv1.weight [64][3][7][7] */
    vt_resnet_bn bn1;
    vt_resnet_block block[4][VT_RESNET_MAX_BLOCKS];
    const float *linear_w, *linear_b;  /* linear [100][512], [100] */
    const float *fc_w, *fc_b;          /* fc [num_classes][100], [num_classes] */
} vt_resnet_params;
int vt_resnet_supported(const int32_t *blocks_num, int num_classes, int n_img, int H, int W);
size_t vt_resnet_blob_bytes(const int32_t *blocks_num, int num_classes);
size_t vt_resnet_workspace_bytes(const int32_t *blocks_num, int num_classes, int n_img, int H, int W);
int vt_resnet_pack(const vt_resnet_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_resnet_fwd(const float *x, int n_img, int H, int W, const vt_resnet_params *dims_host, const float *blob,
                  void *workspace, size_t workspace_bytes, float *out, void *stream);

/* ------------------------------------------------------------------------- */
/* Tactile feature encoder with Bottleneck blocks, eval mode                       */
/*   (resnet2d_bneck.hip).  Replaces ResNet.forward with Bottleneck blocks          */
/*   (src/layers.py:86-207: Resnet50 of the encoder registry, Resnet101 / 152):     */
/*   per block conv1 1x1, conv2 3x3 (carries the stride), conv3 1x1 to 4 * width,   */
/*   a 1x1 projection of the block input in the first block of EVERY stage          */
/*   (layer1.0: 64 -> 256 at stride 1), Linear(2048, 100), Linear(100, classes).    */
/*   x [n_img][3][H][W] (NCHW) -> out [n_img][num_classes].                         */
/* vt_resnet_bneck_pack folds every BatchNorm into its conv (f64), fragment order;  */
/*   a projecting block's conv3 and projection share ONE bias, b3 + b_proj summed   */
/*   in f64.  Blob floats: the stem as [64][3][7][8] (kx padded to 8) + 64; per      */
/*   block conv1.weight + width, conv2.weight + width, conv3.weight (+              */
/*   downsample.0.weight) + 4 * width; linear.weight, then linear.bias, fc.weight   */
/*   and fc.bias each padded to a multiple of 4 floats.                             */
/* vt_resnet_bneck_fwd is 2 + 3 * (number of blocks) launches: the stem, conv1 (a   */
/*   GEMM over pixels, bias, ReLU), conv2 (the 3x3 kernel of resnet2d.hip), conv3   */
/*   with its skip (one GEMM over [conv2's output ; block input] in a projecting    */
/*   block, the block input added in the epilogue otherwise), the tail.  Exact-f32  */
/*   matrix core, fixed summation order that does not depend on n_img:              */
/*   bit-reproducible, an image's features are the same bits in any batch.          */
/* stage_out: NULL, or four device pointers (each may be NULL); a set pointer        */
/*   receives the output of layer{s+1}, [n_img][Hs][Ws][4 * (64 << s)] channels-     */
/*   last, by one extra copy launch (for verification).                             */
/* Covered (vt_resnet_bneck_supported): what vt_resnet_supported covers, with the   */
/*   tensors four times as wide: every buffer below 2^31 elements.  Workspace: four */
/*   buffers of max over the stages s = 0..3 of n_img * Hs * Ws * 4 * (64 << s)      */
/*   floats, Hs = ceil(H / 2^(s+2)), Ws alike.                                      */
/* ------------------------------------------------------------------------- */
typedef struct vt_resnet_bneck_block { /* layer{s}.{b}: conv1 [C][Cin][1][1], conv2 [C][C][3][3], conv3 [4C][C][1][1] */
    const float *conv1_w;
    vt_resnet_bn bn1;
    const float *conv2_w;
    vt_resnet_bn bn2;
    const float *conv3_w;
    vt_resnet_bn bn3;
    const float *down_w;               /* downsample.0.weight [4C][Cin][1][1] (first block of layer1..4), else NULL */
    vt_resnet_bn down_bn;              /* downsample.1 */
} vt_resnet_bneck_block;
typedef struct vt_resnet_bneck_params {
    int32_t blocks_num[4];
    int32_t num_classes;
    const float *conv1_w;              /* conv1.weight [64][3][7][7] */
    vt_resnet_bn bn1;
    vt_resnet_bneck_block block[4][VT_RESNET_MAX_BLOCKS];
    const float *linear_w, *linear_b;  /* linear [100][2048], [100] */
    const float *fc_w, *fc_b;          /* fc [num_classes][100], [num_classes] */
} vt_resnet_bneck_params;
int vt_resnet_bneck_supported(const int32_t *blocks_num, int num_classes, int n_img, int H, int W);
size_t vt_resnet_bneck_blob_bytes(const int32_t *blocks_num, int num_classes);
size_t vt_resnet_bneck_workspace_bytes(const int32_t *blocks_num, int num_classes, int n_img, int H, int W);
int vt_resnet_bneck_pack(const vt_resnet_bneck_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_resnet_bneck_fwd(const float *x, int n_img, int H, int W, const vt_resnet_bneck_params *dims_host, const float *blob,
                        void *workspace, size_t workspace_bytes, float *out, float *const *stage_out, void *stream);

/* ------------------------------------------------------------------------- */
/* Tactile feature encoder, train mode: forward with batch statistics and the      */
/*   backward for every parameter (resnet2d_train.hip).  Replaces ResNet.forward   */
/*   with BasicBlocks in train mode under autograd (src/layers.py:54-207) as        */
/*   ConvolutionalOccupancyNetwork.encode_img_inputs calls it once per scene        */
/*   (src/conv_onet/models/__init__.py:115-136).                                    */
/* x [n_img][3][H][W], IMAGE-major: image f of scene b is row f * scenes + b, so    */
/*   the images n with n % scenes == b are one statistics group.  Every conv        */
/*   (no bias) writes its raw output z; per (scene, channel) the mean and biased    */
/*   variance of z; gamma (z - mean) / sqrt(var + eps) + beta fused with the ReLU   */
/*   (and the 3x3/2 max-pool after the stem, the residual after bn2).  The raw      */
/*   weights of params_host are packed at every call; no blob.  momentum >= 0:      */
/*   the running_mean / running_var the params point to are UPDATED in place, per   */
/*   BatchNorm scene after scene: running = (1 - m) running + m batch (unbiased     */
/*   variance); momentum < 0 leaves them alone.  num_batches_tracked (+ scenes per  */
/*   BatchNorm) is the caller's.  out [n_img][num_classes].                         */
/* vt_resnet_bwd: from dout [n_img][num_classes], x and the workspace the forward   */
/*   filled (same shape, same params), the gradient of every parameter              */
/*   (vt_resnet_grads: written, not accumulated).  No gradient for x.               */
/* Exact-f32 matrix core for the convs, their data and weight gradients; the        */
/*   per-channel sums and the weight gradients' partials are combined in f64 in a   */
/*   fixed order that is a function of the layer and of one scene's images alone:   */
/*   no atomics, bit-reproducible, a scene's outputs do not depend on the others.   */
/* Covered (vt_resnet_train_supported): what vt_resnet_supported covers with        */
/*   scenes >= 1 dividing n_img, n_img * ceil(H / 2) * ceil(W / 2) * 64 < 2^31 and   */
/*   at least 2 values per scene and channel at layer4.  Unsupported: the size      */
/*   query returns 0.  The workspace keeps every conv's z and activation, the       */
/*   packed weights, four gradient buffers and the partials (the list:              */
/*   rt_workspace in resnet2d_train.hip, restated in tests/resnet_train_util.py).   */
/* ------------------------------------------------------------------------- */
typedef struct vt_resnet_block_grads {
    float *conv1_w, *bn1_w, *bn1_b, *conv2_w, *bn2_w, *bn2_b;
    float *down_w, *down_bn_w, *down_bn_b;     /* first block of layer2..4, else unused */
} vt_resnet_block_grads;
typedef struct vt_resnet_grads {
    float *conv1_w, *bn1_w, *bn1_b;
    vt_resnet_block_grads block[4][VT_RESNET_MAX_BLOCKS];
    float *linear_w, *linear_b, *fc_w, *fc_b;
} vt_resnet_grads;
int vt_resnet_train_supported(const int32_t *blocks_num, int num_classes, int n_img, int scenes, int H, int W);
size_t vt_resnet_train_workspace_bytes(const int32_t *blocks_num, int num_classes, int n_img, int scenes, int H, int W);
int vt_resnet_train_fwd(const float *x, int n_img, int scenes, int H, int W, const vt_resnet_params *params_host, double momentum,
                        void *workspace, size_t workspace_bytes, float *out, void *stream);
int vt_resnet_bwd(const float *dout, const float *x, int n_img, int scenes, int H, int W, const vt_resnet_params *params_host,
                  void *workspace, size_t workspace_bytes, const vt_resnet_grads *grads_host, void *stream);

/* ------------------------------------------------------------------------- */
/* Tactile depth estimator, eval mode (unet2d.hip).  Replaces UNet.forward        */
/*   (src/layers.py:322-450; up_mode 'transpose', merge_mode 'concat': `depth`     */
/*   DownConvs, depth - 1 UpConvs, conv_final, sigmoid) as                         */
/*   ConvolutionalOccupancyNetwork.encode_img_inputs calls it on the five tactile  */
/*   images of a scene, with the BatchNorm layers in eval mode:                    */
/*   x [n_img][in_channels][H][W] (NCHW) -> out [n_img][num_classes][H][W].        */
/* vt_tactile_unet_pack folds each block's ONE BatchNorm into both of its convs     */
/*   (f64) and writes the folded weights in fragment order (blob of                */
/*   vt_tactile_unet_blob_bytes; repack after every change of a weight OR a         */
/*   running statistic).  vt_tactile_unet_fwd is 2 depth + 3 (depth - 1) launches   */
/*   (12 at depth 3): one per 3x3 conv with bias + ReLU in its epilogue -- a down   */
/*   block's second conv also writes the 2x2 max-pool, an up block's first conv     */
/*   reads the up-conv's result and the skip as two sources (no concat), the last   */
/*   conv ends in conv_final + sigmoid -- and one per transposed conv (its four     */
/*   output parities as four 1x1 GEMMs).  Exact-f32 matrix core, every sum in a     */
/*   fixed order that does not depend on n_img: bit-reproducible, and an image's    */
/*   result is the same bits in any batch.                                          */
/* Covered (vt_tactile_unet_supported): depth 1..5, start_filts 8..64 (multiple of  */
/*   8), in_channels 1..4, num_classes 1..4, 1 <= n_img <= 1024, H and W multiples  */
/*   of 2^(depth-1) up to 2048, n_img * H * W * start_filts < 2^31.  Unsupported:   */
/*   the size queries return 0.                                                     */
/* up_* entries are indexed by the level the block produces: up_*[i] is             */
/*   up_convs[depth - 2 - i] (start_filts << i output channels), i = 0..depth-2.    */
/* ------------------------------------------------------------------------- */
#define VT_TACTILE_UNET_MAX_DEPTH 5
#define VT_TACTILE_UNET_MAX_CLASSES 4
typedef struct vt_tactile_unet_params {
    int32_t depth, start_filts, in_channels, num_classes;
    const float *down_w[VT_TACTILE_UNET_MAX_DEPTH][2], *down_b[VT_TACTILE_UNET_MAX_DEPTH][2];   /* down_convs[i].conv1 / conv2 */
    vt_resnet_bn down_bn[VT_TACTILE_UNET_MAX_DEPTH];                                             /* down_convs[i].bn (behind both convs) */
    const float *up_tw[VT_TACTILE_UNET_MAX_DEPTH], *up_tb[VT_TACTILE_UNET_MAX_DEPTH];           /* upconv.weight [2C][C][2][2], bias [C] */
    const float *up_w[VT_TACTILE_UNET_MAX_DEPTH][2], *up_b[VT_TACTILE_UNET_MAX_DEPTH][2];       /* conv1 [C][2C][3][3], conv2 [C][C][3][3] */
    vt_resnet_bn up_bn[VT_TACTILE_UNET_MAX_DEPTH];
    const float *final_w, *final_b;                                                              /* conv_final [num_classes][start_filts][1][1] */
} vt_tactile_unet_params;
int vt_tactile_unet_supported(int depth, int start_filts, int in_channels, int num_classes, int n_img, int H, int W);
size_t vt_tactile_unet_blob_bytes(int depth, int start_filts, int in_channels, int num_classes);
size_t vt_tactile_unet_workspace_bytes(int depth, int start_filts, int in_channels, int num_classes, int n_img, int H, int W);
int vt_tactile_unet_pack(const vt_tactile_unet_params *params_host, float *blob, size_t blob_bytes, void *stream);
int vt_tactile_unet_fwd(const float *x, int n_img, int H, int W, const vt_tactile_unet_params *dims_host, const float *blob,
                        void *workspace, size_t workspace_bytes, float *out, void *stream);

/* ------------------------------------------------------------------------- */
/* Tactile depth estimator, train mode: forward with batch statistics and the      */
/*   backward for every parameter (unet2d_train.hip).                              */
/* x [n_img][in_channels][H][W], scene-major: images s * group .. s * group +      */
/*   group - 1 are one statistics group (the reference calls the net once per      */
/*   scene on its 5 images).  Every 3x3 conv is z = conv(x) + b, the per-group,    */
/*   per-channel mean and biased variance of z, relu(gamma (z - mean) /            */
/*   sqrt(var + eps) + beta); a block's ONE BatchNorm follows both convs (shared   */
/*   gamma, beta; statistics per use).  The raw weights of params_host are packed  */
/*   at every call; no blob.  momentum >= 0: the running_mean / running_var the    */
/*   params point to are UPDATED in place, per block for each scene in order and   */
/*   per scene conv1's use then conv2's: running = (1 - m) running + m batch       */
/*   (unbiased variance); momentum < 0 leaves them alone.  num_batches_tracked     */
/*   (+ 2 * n_img / group per block) is the caller's.                              */
/* vt_tactile_unet_bwd: from dout [n_img][num_classes][H][W], the forward's out    */
/*   and the workspace the forward filled (same shape, same params), the gradient  */
/*   of every parameter (vt_tactile_unet_grads: written, not accumulated; gamma    */
/*   and beta of a block are the sum over its two uses).  No gradient for x.       */
/* Exact-f32 matrix core for the convs, their data and weight gradients; the       */
/*   per-channel sums and the weight gradients' partials are combined in f64 in a  */
/*   fixed order that depends on neither the number of scenes nor the launch: no   */
/*   atomics, bit-reproducible, a scene's outputs do not depend on the others.     */
/* Covered (vt_tactile_unet_train_supported): what vt_tactile_unet_supported       */
/*   covers with start_filts 8, 16, 32 or 64; group >= 1 dividing n_img; at least  */
/*   2 values per group and channel at the bottom level.  Unsupported: the size    */
/*   query returns 0.  The workspace keeps every conv's z and activation for the   */
/*   backward: about 20 level-0 activations (n_img * H * W * start_filts floats).  */
/* ------------------------------------------------------------------------- */
typedef struct vt_tactile_unet_grads {
    float *down_w[VT_TACTILE_UNET_MAX_DEPTH][2], *down_b[VT_TACTILE_UNET_MAX_DEPTH][2];
    float *down_bn_w[VT_TACTILE_UNET_MAX_DEPTH], *down_bn_b[VT_TACTILE_UNET_MAX_DEPTH];         /* down_convs[i].bn weight (gamma), bias (beta) */
    float *up_tw[VT_TACTILE_UNET_MAX_DEPTH], *up_tb[VT_TACTILE_UNET_MAX_DEPTH];
    float *up_w[VT_TACTILE_UNET_MAX_DEPTH][2], *up_b[VT_TACTILE_UNET_MAX_DEPTH][2];
    float *up_bn_w[VT_TACTILE_UNET_MAX_DEPTH], *up_bn_b[VT_TACTILE_UNET_MAX_DEPTH];
    float *final_w, *final_b;
} vt_tactile_unet_grads;
int vt_tactile_unet_train_supported(int depth, int start_filts, int in_channels, int num_classes, int n_img, int group, int H, int W);
size_t vt_tactile_unet_train_workspace_bytes(int depth, int start_filts, int in_channels, int num_classes, int n_img, int group, int H, int W);
int vt_tactile_unet_train_fwd(const float *x, int n_img, int group, int H, int W, const vt_tactile_unet_params *params_host, double momentum,
                              void *workspace, size_t workspace_bytes, float *out, void *stream);
int vt_tactile_unet_bwd(const float *dout, const float *out, int n_img, int group, int H, int W, const vt_tactile_unet_params *params_host,
                        void *workspace, size_t workspace_bytes, const vt_tactile_unet_grads *grads_host, void *stream);

/* ------------------------------------------------------------------------- */
/* PointNet per-point MLP (inference).  Replaces the nn.Linear / ResnetBlockFC   */
/* calls of LocalPoolPointnet.forward (src/encoder/pointnet.py:154-162;           */
/* src/layers.py:8-50): rows are points, weights in nn.Linear layout [out][in].   */
/*   vt_linear_rows  out[n] = b + W x[n]            (fc_pos, fc_c; b may be NULL)   */
/*   vt_resblock_fc  x = [x1[n] | x2[n]] (x2 may be NULL: no concat);                */
/*                   h = b0 + W0 relu(x); out[n] = b1 + W1 relu(h) + Ws x           */
/*                   (ws NULL: identity shortcut, needs C1 + C2 == O).               */
/* At most 256 hidden / output channels; weights must fit 64 KiB of LDS             */
/* (vt_linear_rows alone: 160 KiB).                                                  */
/* ------------------------------------------------------------------------- */
int vt_linear_rows(const float *x, const float *w, const float *b, int64_t N, int Cin, int Cout, float *out, void *stream);
int vt_resblock_fc(const float *x1, int C1, const float *x2, int C2, int64_t N,
                   const float *w0, const float *b0, const float *w1, const float *b1, const float *ws,
                   int H, int O, float *out, void *stream);
/* The whole per-point MLP of LocalPoolPointnet.forward (pointnet.py:154-162) in one launch for inference with ONE voxel index:     */
/* fc_pos -> block 0 -> 4 x (pool_local, concat, block) -> fc_c.  A workgroup owns every cell whose first sorted point falls into  */
/* its window of 8-16 sorted positions -- complete cells of any size -- so pooling needs no grid-wide step; same arithmetic and        */
/* summation order as vt_linear_rows / vt_resblock_fc / vt_voxel_pool_max_fwd: bit-identical features.  block_w: 25 device pointers, */
/* per block fc_0.weight [32][64], fc_0.bias, fc_1.weight [32][32], fc_1.bias, shortcut.weight [32][64]; hidden must be 32, c_dim     */
/* <= 64 (VT_ERR_UNSUPPORTED otherwise: use the per-layer kernels); scratch [B,T,32] floats; out [B,T,c_dim] by point (or NULL).     */
/* With grid_cl != NULL the kernel is also generate_grid_features (pointnet.py:102-110, scatter_mean): every cell's mean feature,     */
/* summed in ascending point order like vt_voxel_scatter_mean_cl_fwd, goes into the ZERO-FILLED channels-last grid [B,R,R,R,c_dim]   */
/* (idx [B,T] = the points' cell ids) and grid_part [B][vt_pointnet_mlp_stat_blocks(B,T)][c_dim][2] receives the GroupNorm partial    */
/* sums of that grid (the empty voxels contribute nothing): what vt_channel_stats would compute in a pass over the whole grid.        */
int vt_pointnet_mlp_stat_blocks(int B, int T);
int vt_pointnet_mlp_fused(const float *pts, int B, int T, const int *order, const int *seg_lo, const int *seg_hi,
                          const float *pos_w, const float *pos_b, const float *const *block_w, int hidden,
                          const float *c_w, const float *c_b, int c_dim, float *scratch, float *out,
                          const int *idx, int R, float *grid_cl, float *grid_part, void *stream);
/* Backward of the two (training; PyTorch autograd of layers.py:8-50 and of the nn.Linear calls at    */
/* pointnet.py:154-162 under loss.backward(), training.py:79,89,96):                                    */
/*   vt_resblock_fc_bwd  d out [N][O] -> d x1 [N][C1], d x2 [N][C2] (NULL: not wanted), and the two       */
/*                       [N][H] tensors the weight gradients contract over: act = relu(h) (recomputed)   */
/*                       and dh = (W1^T d out) . [h > 0];                                                 */
/*   vt_rows_wgrad       dW [M][K] = sum_n G[n][m] X[n][k], db [M] = sum_n G[n][m] (db may be NULL) with    */
/*                       X = [x1 | x2] (x2 may be NULL), relu'd when relu_x: f32 MFMA outer products over  */
/*                       1024-point chunks, partials summed in chunk order (bit-reproducible).             */
/*                       fc_1: (d out, act); fc_0: (dh, relu [x1|x2]); shortcut: (d out, [x1|x2]);          */
/*                       a plain linear layer: (d out, x).  Its data gradient is vt_linear_rows on W^T.     */
int vt_resblock_fc_bwd(const float *x1, int C1, const float *x2, int C2, int64_t N,
                       const float *w0, const float *b0, const float *w1, const float *ws, int H, int O,
                       const float *dout, float *dx1, float *dx2, float *act, float *dh, void *stream);
size_t vt_rows_wgrad_workspace_bytes(int64_t N, int M, int K);
int vt_rows_wgrad(const float *G, int M, const float *x1, int C1, const float *x2, int C2, int relu_x, int64_t N,
                  void *workspace, size_t workspace_bytes, float *dW, float *db, void *stream);
/* The three weight gradients of a ResnetBlockFC (layers.py:8-50: fc_1 from (dout, relu(h)), fc_0 from (dh, relu(x)), the shortcut  */
/* from (dout, x); x = [x1 | x2]) in one pair of launches instead of three: the same tiles, partial sums and chunk-ordered          */
/* reduction as vt_rows_wgrad (bit for bit).  act / dh: vt_resblock_fc_bwd's outputs; dws NULL without a shortcut layer.           */
size_t vt_resblock_wgrad_workspace_bytes(int64_t N, int C, int H, int O, int has_shortcut);
int vt_resblock_wgrad(const float *x1, int C1, const float *x2, int C2, int64_t N, const float *act, const float *dh, const float *dout,
                      int H, int O, void *workspace, size_t workspace_bytes,
                      float *dw0, float *db0, float *dw1, float *db1, float *dws, void *stream);

/* ------------------------------------------------------------------------- */
/* Generalized winding number of query points against a triangle mesh.          */
/* Stands where the VTacO (t2d) training step calls                              */
/*   igl.fast_winding_number_for_meshes(V, F, Q) (src/conv_onet/training.py:723,  */
/*   862) to label its re-sampled query points.  libigl is an un-vendored,        */
/*   absent dependency and its routine is a hierarchical approximation: this is    */
/*   the exact sum it approximates, w(q) = 1/(4 pi) sum_f Omega_f(q) (float64        */
/*   solid angles): 1 inside a closed outward-oriented mesh, 0 outside.               */
/*   verts [V,3] f32, faces [F,3] i32, pts [N,3] f32 -> out [N] f32.                    */
/* ------------------------------------------------------------------------- */
int vt_winding_number(const float *verts, int V, const int32_t *faces, int F, const float *pts, int64_t N, float *out, void *stream);
/* The same for a batch of scenes in ONE launch (the reference loops over the batch, training.py:723, 862): scenes = device array of  */
/* B records {const float *verts; const int32_t *faces; int32 V; int32 F} (24 bytes each, the meshes anywhere in device memory), */
/* pts [B][N][3], out [B][N].                                                                                                     */
int vt_winding_number_scenes(const void *scenes, int B, const float *pts, int64_t N, float *out, void *stream);

/* Contact clouds of the tactile sensors from their depth images (SURVEY.md section 8f "next" row 2: the training side).          */
/* Replaces: the per-scene, per-sensor numpy passes of src/conv_onet/training.py:817-853 and generation.py:224-244               */
/*   (np.where(abs(depth - depth_origin) > 1e-4), depth_2_camera_pointcloud, np.random.randint, pc_cam_to_world, norm_pc_1).        */
/* vt_contact_scan: depth [n_images][n_pixels] f32, depth_origin [n_pixels] f64 (the sensor's flat reading), touch_success          */
/*   [n_images] u8 or NULL -> index [n_images][n_pixels] i32 (the touched pixels in ascending order = np.where's) and count         */
/*   [n_images]; the comparison in float64 as numpy's.  The host reads the counts, draws np.random.randint(count, size=128) where a  */
/*   count exceeds 128 (the draws stay on the host: a seeded run consumes numpy's generator as the reference does) and inverts the   */
/*   4 x 4 camera poses.                                                                                                             */
/* vt_contact_points: per image kept[i] points (all `count` in order when sel is NULL, else index[sel[i][j]]), pose [n_images][16]  */
/*   f64 = {inverse pose's 3x3 row-major, translation 3, cloud centroid 3, cloud scale 1}: pinhole unprojection (f = height /        */
/*   (2 tan(fov / 2)), principal point at the centre, axes (z, -x, -y)), world = M cam + t, (world - centroid) / scale in float64,    */
/*   written as float32 rows row0[i] .. row0[i] + kept[i] of scene i / 5 in p_sample [B][S][3] (finger [B][S] i64 gets i % 5; may be  */
/*   NULL).  n_images = 5 B.                                                                                                          */
int vt_contact_scan(const float *depth, const double *depth_origin, const unsigned char *touch_success, int n_images, int n_pixels,
                    double threshold, int *index, int *count, void *stream);
int vt_contact_points(const float *depth, const int *index, const int *sel, const int *kept, const int *row0, const double *pose,
                      int n_images, int n_pixels, int width, int height, double fov_deg, int max_points, int S,
                      float *p_sample, long long *finger, void *stream);

/* vt_depth_cloud: EVERY pixel of the predicted depth images as a world-space point (Generator3D.generate_tactile_pc,             */
/*   src/conv_onet/generation.py:286-333): pred [n_images][n_pixels] f32 (the depth estimator's sigmoid output); depth = pred *      */
/*   0.005f + 0.019f in float32 (numpy on a float32 array), then vt_contact_points' unprojection, pose and normalisation in float64   */
/*   with the same pose records [n_images][16] -> out [n_images][n_pixels][3], float64 (what the reference returns) or, with          */
/*   out_f32 != 0, float32.                                                                                                           */
int vt_depth_cloud(const float *pred, const double *pose, int n_images, int n_pixels, int width, int height, double fov_deg,
                   void *out, int out_f32, void *stream);

/* Evaluation metrics of the visualise block: the reference's generate_obj_mesh_wnf ends with                                   */
/*   cd = chamfer_distance(points_obj, vertices[:2048], use_kdtree=False); emd = EarthMoverDistance(points_obj[0], vertices)     */
/* (src/conv_onet/generation.py:274-284; src/common.py:45-51 cdist + scipy linear_sum_assignment, :69-91 the naive Chamfer).      */
/* vt_chamfer_nn: a [B][N][3], b [B][M][3] f32 -> for every point of a the squared distance to its nearest point of b and that  */
/*   point's index (d_ab, i_ab [B][N]), and the same from b to a (d_ba, i_ba [B][M]), one launch.  d = (dx*dx + dy*dy) + dz*dz  */
/*   in f32, unfused (the minima are numpy's f32 restatement bit for bit); equal minima give the smallest index.                 */
int vt_chamfer_nn(const float *a, const float *b, int B, int N, int M, float *d_ab, int *i_ab, float *d_ba, int *i_ba, void *stream);
/* vt_emd_auction: the minimum-cost assignment between a [B][N][3] and b [B][M][3] under Euclidean cost (what cdist +          */
/*   linear_sum_assignment computes), by an epsilon-scaling auction, one workgroup per problem with its state in LDS.  The       */
/*   smaller side is padded with dummy points of cost 0 to everything, to n = max(N, M) <= VT_EMD_MAX_POINTS (VT_ERR_UNSUPPORTED  */
/*   beyond).  Outputs per problem: assign [B][n] i32 (person -> object of the padded problem: rows of a, then dummies),        */
/*   prices [B][n] f32 (the dual prices of the objects), cost_f64 [B] = sum |a_i - b_assign[i]| over the real pairs in float64    */
/*   (cdist's arithmetic) / N (len(d)), status [B] i32 (0 = converged, 1 = max_rounds Jacobi rounds spent before the last phase  */
/*   ended: the outputs are not an assignment; 2 = a NaN or infinite coordinate, or a cost range beyond f32, found before the    */
/*   first round: assign is -1, prices 0 and cost_f64 NaN for that problem, the others of the batch are unaffected; the host     */
/*   raises for both).  Epsilon starts at the cost range / 5 (the cost range is the f32 diagonal of the two clouds' common       */
/*   bounding box) and is divided by 5 per phase down to eps = eps_final * 2^floor(log2(cost range)) (eps_final itself for a     */
/*   cost range of 0): relative to the cost range's binade, so clouds scaled by a power of two give the same assignment and      */
/*   rounds and prices scaled alike.  The result satisfies eps-complementary slackness, so cost <= optimum + n eps / N.          */
/*   ws: NULL or B * vt_emd_workspace_bytes(N, M) bytes that receive per-problem counters {i64 rounds, i64 bids, i32 phases,   */
/*   f32 last eps (in input units), i64 0}.  vt_emd_workspace_bytes returns 0 for sizes the kernel does not cover.               */
#define VT_EMD_MAX_POINTS 4096
#define VT_EMD_WORKSPACE_PER_PROBLEM 32
size_t vt_emd_workspace_bytes(int n, int m);
int vt_emd_auction(const float *a, int N, const float *b, int M, int B, float eps_final, int max_rounds,
                   int *assign, float *prices, double *cost_f64, int *status, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* Voxel-input encoder front end (voxel_encoder.hip).                                                                            */
/* Replaces: conv_in (Conv3d 1 -> C, kernel 3 with zero padding 1, or kernel 1), ReLU and the scatter_mean of the voxel features  */
/* onto the grid or the planes in LocalVoxelEncoder.forward (src/encoder/voxels.py:56-119).  Exact f32.                           */
/*   x [B,D1,D2,D3] f32 (every dimension >= 2, need not be equal); weight [C,1,k,k,k], bias [C], k = ksize in {1, 3};             */
/*   f[b,c,v] = max(0, bias[c] + sum W x), one fused multiply-add per tap in (t1,t2,t3) order.                                    */
/* A voxel's cell depends on the volume's shape alone, per axis and monotonically, so the caller supplies per-axis tables         */
/* (vtaco_amd/ops/voxel_encoder.py builds them with the reference's f32 expressions):                                              */
/*   index  int32 [D1 + D2 + D3]: a1[i1] | a2[i2] | a3[i3], each in [0, R);                                                        */
/*   ranges int32 [3][R][2]: per axis and output index r the voxel indices [lo, hi) with a[i] == r (lo == hi: none).               */
/* vt_voxel_encode_grid: grid_cl [B,R,R,R,C] channels-last, cell (z,y,x) = (a3,a2,a1), flat a1 + R (a2 + R a3); the value is the   */
/*   sum of f over the cell's box in (i1,i2,i3) order divided by the voxel count, cells without a voxel exactly 0.0f.  Every cell  */
/*   is written by the one launch (no clear pass).                                                                                */
/* vt_voxel_encode_planes: plane_mask = xz (1) | xy (2) | yz (4), at least one; planes [P B,C,R,R], the present planes in that     */
/*   order one after the other.  xz projects (p0,p2), xy (p0,p1), yz (p1,p2) (p_k along x's dimension k + 1); pixel [v][u] with u */
/*   the first projected axis.  A cell is the mean over its two ranges times the whole dropped axis.  One launch for all planes.   */
/* vt_voxel_encode_bwd: grad_weight [C,1,k,k,k] and grad_bias [C] from x, the weights and the upstream gradient of the grid        */
/*   (grad_grid_cl, with grid_index / grid_ranges / Rg) and / or of the stacked planes (grad_planes, plane_index / plane_ranges /  */
/*   Rp / plane_mask); NULL = that output had no gradient.  The pre-activation is recomputed (the forward saves nothing), masked   */
/*   pre > 0; a voxel takes g[cell] / n from every output it fed.  Two deterministic stages through `workspace`                    */
/*   (vt_voxel_encode_bwd_workspace_bytes bytes), no float atomics; both outputs are written, not accumulated into.  x gets no     */
/*   gradient.                                                                                                                      */
/* All three are bit-identical from run to run, and a scene's forward result does not depend on B.  C % 32 == 0, C <= 128, D <=    */
/* 4096, R <= 1024 (VT_ERR_UNSUPPORTED otherwise, before any launch).                                                              */
int vt_voxel_encode_grid(const float *x, int B, int D1, int D2, int D3, const float *weight, const float *bias, int C, int ksize,
                         const int *ranges, int R, float *grid_cl, void *stream);
int vt_voxel_encode_planes(const float *x, int B, int D1, int D2, int D3, const float *weight, const float *bias, int C, int ksize,
                           const int *ranges, int R, int plane_mask, float *planes, void *stream);
size_t vt_voxel_encode_bwd_workspace_bytes(int B, int D1, int D2, int D3, int C);
int vt_voxel_encode_bwd(const float *x, int B, int D1, int D2, int D3, const float *weight, const float *bias, int C, int ksize,
                        const float *grad_grid_cl, const int *grid_index, const int *grid_ranges, int Rg,
                        const float *grad_planes, const int *plane_index, const int *plane_ranges, int Rp, int plane_mask,
                        float *grad_weight, float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the PointConv baseline: point-feature sampler (point_sample.hip) and PointNet++ geometry (pointnetpp.hip) ------------------ */
/* The sampler: out [B,M,C], c_m = sum_n w[m,n] fea_n / sum_n w[m,n] over the cloud [B,N,3] with features fea [B,N,C]              */
/*   (reference decoder.py:468-485).  gaussian != 0: w = exp(-(|p_n - q_m| + 10e-6)^2 / gaussian_val^2), evaluated with the query's  */
/*   largest exponent subtracted (shift): equal to the reference wherever its own sum does not underflow, finite where it returns  */
/*   NaN.  gaussian == 0: w = 1 / (|p_n - q_m| + 10e-6), shift = 0.  Queries: q [B,M,3], or NULL with the lattice (lattice_nx,       */
/*   lattice_box, lattice_first, M) in vt_sample_grid's arithmetic -- bit for bit the point form on those points.  shift, sum [B,M]: */
/*   what the backward rebuilds the normalised weights from.  Exact-f32 matrix products.  C % 32 == 0, C <= 256, N >= 1.           */
/* The backward: grad_fea [B,N,C] = sum_m (w[m,n] / sum_m) grad_c [b,m,:]; ordered sums, no float atomics, every element written.   */
/*   Neither q nor the cloud gets a gradient.  workspace: vt_point_sample_bwd_workspace_bytes(B, M, N, C) bytes (0 for M <= 512).   */
int vt_point_sample_fwd(const float *q, int64_t M, int lattice_nx, float lattice_box, int64_t lattice_first,
                        const float *cloud, const float *fea, int B, int64_t N, int C, int gaussian, double gaussian_val,
                        float *out, float *shift, float *sum, void *stream);
size_t vt_point_sample_bwd_workspace_bytes(int B, int64_t M, int64_t N, int C);
int vt_point_sample_bwd(const float *q, int64_t M, const float *cloud, int B, int64_t N, int C, int gaussian, double gaussian_val,
                        const float *shift, const float *sum, const float *grad_c, float *grad_fea,
                        void *workspace, size_t workspace_bytes, void *stream);
/* Farthest-point sampling (pointnetpp.py:188-209): out [B,npoint] i64, out[b,0] = start[b] (i64, clamped into the cloud), then    */
/*   the arg-max of the running minimum of ((dx dx + dy dy) + dz dz), the lowest index among equal maxima.  dist_ws: [B,N] floats    */
/*   of scratch.  N < npoint is VT_ERR_INVALID.                                                                                    */
int vt_fps(const float *xyz, int B, int N, int npoint, const int64_t *start, float *dist_ws, int64_t *out, void *stream);
/* Ball query (pointnetpp.py:212-232): out [B,S,nsample] i64, per centre the lowest nsample indices n with                         */
/*   |xyz_n - centre|^2 <= (float)(radius^2) in ascending order, a short row padded with its first entry (an empty one with 0).    */
int vt_ball_query(const float *xyz, int B, int N, const float *centres, int S, double radius, int nsample, int64_t *out, void *stream);
/* The k = min(3, S) nearest sources src [B,S,3] of every target tgt [B,N,3] (pointnetpp.py:84-90): idx [B,N,k] i64 in ascending     */
/*   distance (the lowest index among equals), weight [B,N,k] = (1 / (d^2 + 1e-8)) / their sum.                                    */
int vt_three_nn(const float *tgt, int B, int N, const float *src, int S, int64_t *idx, float *weight, void *stream);

/* ---- mesh -> occupancy volume (voxelize.hip) ------------------------------------------------------------------------------------ */
/* Stands where VoxelGrid.from_mesh (src/utils/voxels.py:16-42) calls voxelize_ray / voxelize_fill (:201-216), whose voxelize_surface  */
/*   and voxelize_interior the reference never defines (upstream: Cython extensions), and scipy's binary_fill_holes (:215).          */
/* verts [V,3] f32, faces [F,3] i32, loc_host [3] f64 on the HOST, scale > 0.  Grid units: g = ((v - loc) / scale + 0.5) * res per    */
/*   component in that order, float64; voxel (i,j,k) is the closed box [i,i+1] x [j,j+1] x [k,k+1], centre (i+.5, j+.5, k+.5).        */
/* vt_voxelize_surface: occ u8 [res][res][res] ([x][y][z]), cleared by the caller; a voxel is set to 1 when its box overlaps a       */
/*   triangle by the 13-axis separating-axis test (3 box axes, the normal, 9 edge x box-axis products; equality = overlap), over     */
/*   the triangle's bounding box clipped to the grid.  One wave per triangle; plain byte stores of 1.                                */
/* vt_voxelize_interior: bits u32 [res][res][ceil(res / 32)] (bit k % 32 of word k / 32), cleared by the caller; parity of the       */
/*   crossings of the +z ray from every voxel centre, per triangle: every column centre of the projected bounding box is tested      */
/*   against the three edge functions -- each evaluated on the edge's canonical direction (lower vertex index first), negated when   */
/*   the triangle walks it the other way, an exact 0 decided as if the centre sat at (+eps, +eps^2) -- and an inside column flips    */
/*   the voxels k < clamp(ceil(z - .5), 0, res), z = (e0 z0 + e1 z1 + e2 z2) / A, with integer XOR atomics (bit-reproducible).        */
/*   Triangles of projected area A == 0 are skipped.                                                                                  */
/* vt_voxel_fill: ONE round of binary_fill_holes with 6-connectivity: six launches (three axes, forward and backward), one thread    */
/*   per grid line; outside u8 [res]^3 (cleared by the caller before the first round) gains every unoccupied voxel that an outside   */
/*   voxel, or the grid's boundary, reaches along a line; *changed (i32, cleared by the caller) becomes 1 when a voxel was gained.   */
/*   The host repeats the round until changed stays 0; the filled volume is outside == 0.                                            */
/* 1 <= res <= VT_VOXELIZE_MAX_RES (VT_ERR_INVALID otherwise, before any launch); V == 0 or F == 0 launches nothing.  Triangles with */
/*   a vertex index outside [0, V) are skipped (the host refuses such meshes).                                                       */
#define VT_VOXELIZE_MAX_RES 512
int vt_voxelize_surface(const float *verts, int V, const int32_t *faces, int F, const double *loc_host, double scale, int res,
                        uint8_t *occ, void *stream);
int vt_voxelize_interior(const float *verts, int V, const int32_t *faces, int F, const double *loc_host, double scale, int res,
                         uint32_t *bits, void *stream);
int vt_voxel_fill(const uint8_t *occ, int res, uint8_t *outside, int32_t *changed, void *stream);

/* ---- closest point on a triangle mesh (closest_point.hip) ------------------------------------------------------------------------- */
/* Replaces: trimesh.proximity.closest_point(mesh, points) of the reference's eval_step (src/conv_onet/training.py:413-416: the          */
/*   penetration depth of the predicted hand into the object mesh).                                                                    */
/* verts [V,3] f32, faces [F,3] i32, pts [N,3] f32 -> d2 [N] f64: the minimum over the faces of the squared Euclidean distance to the   */
/*   closed triangle, face [N] i32: the face that attains it (the lowest index among equal minima), closest [N,3] f64 (or NULL): the    */
/*   point on it.  All arithmetic is float64 on the exactly converted inputs, unfused, in the order DESIGN.md's section                 */
/*   "closest_point.hip" lists (tests/closest_point_ref.py, by_regions, restates it in numpy: the outputs are equal bit for bit).       */
/*   A face whose normal (b - a) x (c - a) is exactly zero in float64 (a repeated index, collinear corners) is the union of its three   */
/*   edges; no face produces NaN.  Queries and faces are both tiled; per-(query, face slab) partial minima are combined in ascending    */
/*   slab order by a finish pass: no atomics on a result, run-to-run equal bits.                                                        */
/* Errors: V <= 0 or F <= 0 (a mesh without faces has no closest point) or a NULL array is VT_ERR_INVALID and a short workspace          */
/*   VT_ERR_WORKSPACE, before any launch; N == 0 launches nothing.  Face indices are checked on the device by the prepare pass: a face  */
/*   with an index outside [0, V) is never dereferenced and takes no part, and sets bit 0 of the status word -- the int32 at the start  */
/*   of `workspace` -- which the caller reads after the call (ops.metrics raises); bit 1: a scene record with V <= 0, F <= 0 or         */
/*   F > max_F (that scene's outputs are d2 = +inf, face = -1).                                                                         */
/* workspace: vt_closest_point_mesh_workspace_bytes(F, N) bytes (0 for F <= 0): the status word, the face records (112 bytes each) and  */
/*   the partial minima.  vt_closest_point_mesh_slab_faces: the faces per slab the launch of B scenes uses (a multiple of 256).          */
/* _scenes: B meshes of different sizes in one launch sequence: scenes = device array of B records {const float *verts; const int32_t   */
/*   *faces; int32 V; int32 F} (vt_winding_number_scenes' 24-byte records), max_F >= every F, pts [B][N][3], d2 / face [B][N], closest   */
/*   [B][N][3]; workspace: B * vt_closest_point_mesh_workspace_bytes(max_F, N) bytes.  Each scene equals its single call bit for bit.   */
size_t vt_closest_point_mesh_workspace_bytes(int F, int64_t N);
int vt_closest_point_mesh_slab_faces(int F, int64_t N, int B);
int vt_closest_point_mesh(const float *verts, int V, const int32_t *faces, int F, const float *pts, int64_t N, double *d2, int32_t *face,
                          double *closest, void *workspace, size_t workspace_bytes, void *stream);
int vt_closest_point_mesh_scenes(const void *scenes, int B, int max_F, const float *pts, int64_t N, double *d2, int32_t *face, double *closest,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* ---- rigid registration of point sets (icp.hip) ----------------------------------------------------------------------------------- */
/* Replaces: src/utils/icp.py of the reference for 3-D points, B problems per call.  Everything is float64; every product, sum,         */
/*   division and square root is a separate IEEE rounding in the fixed order DESIGN.md's section "icp.hip" lists (tests/icp_ref.py,    */
/*   kernel_order, restates it in numpy: the outputs are equal bit for bit).  No atomics; run-to-run equal bits.  A 4x4 transform is    */
/*   row-major; T p = ((T00 x + T01 y) + T02 z) + T03 per row.  1 <= N, M; 1 <= B <= 65535 (VT_ERR_INVALID otherwise, before any launch); */
/*   a short workspace is VT_ERR_WORKSPACE.                                                                                            */
/* vt_nn_points -- nearest_neighbor (icp.py:50-66; sklearn's kd-tree there): src [B][N][3], dst [B][M][3], T [B][4][4] or NULL (applied  */
/*   to src first) -> d2 [B][N]: the squared distance (dx dx + dy dy) + dz dz to the nearest dst point, idx [B][N] i32: its index, the  */
/*   lowest among equal minima.  Queries and targets are both tiled (256 queries per workgroup, targets staged through LDS in chunks of */
/*   256 and read by broadcast); per-(query, slab) partial minima, then a finish pass in ascending slab order.  workspace:              */
/*   vt_nn_points_workspace_bytes(N, M, B); vt_nn_points_slab_points: the targets per slab that launch uses (a multiple of 256).        */
/* vt_icp_fit -- best_fit_transform (icp.py:5-47): a [B][N][3], b [B][M][3], idx [B][N] i32 or NULL: a_i corresponds to b[idx[i]] (an   */
/*   index outside [0, M) is clamped into it), or to b_i (then M == N) -> T [B][4][4], the least-squares rigid map of a onto b.         */
/*   Centroids and H = sum (a_i - abar)(b_i - bbar)^T by a two-stage reduction (chunks of 256 points summed by a fixed tree, the chunk  */
/*   sums added in chunk order); the SVD of H by one-sided Jacobi rotations with a fixed sweep count, singular values descending;       */
/*   R = V U^T, with V's last column negated when det R < 0 (icp.py:35-37); t = bbar - R abar.  H == 0 gives R = I.                     */
/*   workspace: vt_icp_fit_workspace_bytes(N, B).                                                                                      */
/* vt_icp -- icp (icp.py:69-121), the loop of :102-121 enqueued in full, no host synchronisation: A [B][N][3], Bp [B][M][3], init_pose    */
/*   [B][4][4] or NULL (applied to the working copy of A first, :97-98).  Per iteration: neighbours of the working copy, the fit onto   */
/*   them, working copy <- T working copy, then |prev_error - mean distance| < tolerance ends the problem (:113-116).  Every kernel of a */
/*   later iteration returns at once for an ended problem: its working copy, distances, idx and counter stay while its batch mates go    */
/*   on.  -> T [B][4][4] = vt_icp_fit(A, working copy) (:119), distances [B][N] (Euclidean) and idx [B][N] of the last executed         */
/*   iteration, iterations [B] i32: its 0-based index (the reference's i; max_iterations - 1 when the cap is reached).                  */
/*   max_iterations >= 1, tolerance >= 0.  workspace: vt_icp_workspace_bytes(N, M, B).                                                 */
size_t vt_nn_points_workspace_bytes(int64_t N, int64_t M, int B);
int vt_nn_points_slab_points(int64_t N, int64_t M, int B);
int vt_nn_points(const double *src, int64_t N, const double *dst, int64_t M, int B, const double *T, double *d2, int32_t *idx, void *workspace,
                 size_t workspace_bytes, void *stream);
size_t vt_icp_fit_workspace_bytes(int64_t N, int B);
int vt_icp_fit(const double *a, const double *b, int64_t N, int64_t M, const int32_t *idx, int B, double *T, void *workspace, size_t workspace_bytes,
               void *stream);
size_t vt_icp_workspace_bytes(int64_t N, int64_t M, int B);
int vt_icp(const double *A, int64_t N, const double *Bp, int64_t M, int B, const double *init_pose, int max_iterations, double tolerance, double *T,
           double *distances, int32_t *idx, int32_t *iterations, void *workspace, size_t workspace_bytes, void *stream);

/* ---- mesh topology (mesh_topo.hip) ------------------------------------------------------------------------------------------------ */
/* Replaces: what the reference gets from wrapping its meshes in trimesh.Trimesh -- split, area, volume, is_watertight, euler_number.   */
/* faces [F,3] i32, vertices [V,3] f32 (verts_f64 = 0) or f64 (1) as vt_mc_emit leaves them.  1 <= V, F (VT_ERR_INVALID otherwise,     */
/*   before any launch); a short workspace is VT_ERR_WORKSPACE.  A face with an index outside [0, V) is never dereferenced: the calls   */
/*   that read a count back return VT_ERR_INVALID for such a mesh, the two asynchronous ones leave the face out.                      */
/* vt_mesh_components: labels [V] i32, the smallest vertex index of the vertex's connected component (vertices joined by a face edge;  */
/*   an unreferenced vertex keeps its own index).  Hooking by integer atomicMin on roots and pointer jumping, one launch per round,   */
/*   repeated until a hooking round changed nothing (the flags are read in batches; there is no cap); *rounds: the rounds run.        */
/*   Waits for the stream.                                                                                                            */
/* vt_mesh_component_table: *n_components = the roots that own a face; comp_of_vertex [V]: the rank of the vertex's root among them,   */
/*   ascending by root index (-1: unreferenced); comp_of_face [F].  Waits for the stream (one read: the count and the status).        */
/* vt_mesh_component_stats (asynchronous): per component n_faces, n_vertices [C] i32; bbox [C][2][3] (min, max) in the vertices' type;  */
/*   area [C] f64 = sum 0.5 |(v1-v0) x (v2-v0)|; volume [C] f64 = sum v0.(v1 x v2) / 6.  Each face term is float64 on the exactly      */
/*   widened coordinates, one rounding per operation; the sums are exact fixed-point accumulations by integer atomics (DESIGN.md,     */
/*   "mesh_topo.hip"), rounded once at the end: equal bits from run to run.                                                           */
/* vt_mesh_edge_stats (asynchronous): per component, over the undirected edges {a,b}, a != b: n_edges (distinct), n_boundary (one     */
/*   incident face), n_nonmanifold (three or more), n_misoriented (two faces that run along it in one direction), each [C] i32, by a  */
/*   hash table of vt_mesh_edge_stats_workspace_bytes(F) bytes, sized from F: it cannot fill.                                         */
/* vt_mesh_filter: keep [C] u8 -> out_verts (capacity V), out_faces (capacity F): the kept components' vertices and re-indexed faces   */
/*   in their original order; vertex_map [V] i32 (new index or -1); the two counts.  Waits for the stream (one read).                  */
size_t vt_mesh_components_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_components(const int32_t *faces, int64_t F, int64_t V, int32_t *labels, int *rounds, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_mesh_component_table_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_component_table(const int32_t *faces, int64_t F, int64_t V, const int32_t *labels, int32_t *comp_of_vertex, int32_t *comp_of_face,
                            int *n_components, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_mesh_component_stats_workspace_bytes(int64_t C);
int vt_mesh_component_stats(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, const int32_t *comp_of_vertex,
                            const int32_t *comp_of_face, int64_t C, int32_t *n_faces, int32_t *n_vertices, void *bbox, double *area, double *volume,
                            void *workspace, size_t workspace_bytes, void *stream);
size_t vt_mesh_edge_stats_workspace_bytes(int64_t F);
int vt_mesh_edge_stats(const int32_t *faces, int64_t F, int64_t V, const int32_t *comp_of_vertex, int64_t C, int32_t *n_edges, int32_t *n_boundary,
                       int32_t *n_nonmanifold, int32_t *n_misoriented, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_mesh_filter_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_filter(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, const int32_t *comp_of_vertex,
                   const int32_t *comp_of_face, const uint8_t *keep, int64_t C, void *out_verts, int32_t *out_faces, int32_t *vertex_map,
                   int *n_out_verts, int *n_out_faces, void *workspace, size_t workspace_bytes, void *stream);

/* ---- mesh simplification and welding (mesh_simplify.hip) --------------------------------------------------------------------------- */
/* Replaces: the reference's generation.simplify_nfaces (simplify_mesh of its ConvONet tool chain) and trimesh's merge_vertices         */
/*   (process=True).  Vertex clustering on a grid of `resolution` cells along the box's longest side, one vertex per occupied cell      */
/*   placed by the summed quadric of the faces that touch it (Lindstrom 2000); tests/mesh_simplify_ref.py is the definition and the     */
/*   kernels equal it bit for bit.  Topology is not preserved.  Meshes and size rules as in the block above.                            */
/* state [32] i32, 8-byte aligned, owned by the caller and shared by the calls of one simplification: words 0..11 the bounding box of   */
/*   the referenced vertices (six u64 images of doubles; it never leaves the device), 16 the status bits (1 a face index outside        */
/*   [0, V), 2 a non-finite referenced coordinate, 4 K >= 2^21, 8 a weld key beyond int64, 16 a map that is not of these faces),        */
/*   17 K, 18 the face count, 19 the placement's fallbacks.  vt_mesh_cluster / vt_mesh_weld initialise it.                              */
/* vt_mesh_cluster (asynchronous): cluster_of_vertex [V] i32, the cluster of every referenced vertex (-1: unreferenced); clusters are   */
/*   the occupied cells, numbered by ascending representative = the cell's lowest vertex index; cluster_rep (capacity V): the           */
/*   representatives; K into state.  1 <= resolution <= 2^20.                                                                           */
/* vt_mesh_weld (asynchronous): the same two maps with the key of merge_vertices: tol = 0 equal coordinates (-0.0 = +0.0, a vertex with */
/*   a NaN merges with nothing), tol > 0 equal rint(x / tol) per axis.                                                                  */
/* vt_mesh_cluster_faces: the faces on cluster ids, those with two equal ids dropped and, with `unique`, of the faces with one          */
/*   unordered triple the lowest kept, in the original order, into out_faces (capacity F); out_faces = NULL counts only.  Waits for     */
/*   the stream (one read of state: *n_clusters, *n_out_faces and the status bits, which make it VT_ERR_INVALID).                       */
/* vt_mesh_cluster_place (asynchronous): out_verts [K][3] in the vertices' type: placement 0 the quadric minimiser about the cluster's  */
/*   mean (eigenvalues <= 1e-3 of the largest dropped; outside the cell: the mean, counted in state word 19), 1 the mean, 2 the         */
/*   representative's own coordinates (welding).  The sums are exact fixed-point accumulations by integer atomics.                     */
size_t vt_mesh_cluster_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_cluster(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int resolution, int32_t *cluster_of_vertex,
                    int32_t *cluster_rep, int32_t *state, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_mesh_weld_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_weld(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, double tol, int32_t *cluster_of_vertex, int32_t *cluster_rep,
                 int32_t *state, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_mesh_cluster_faces_workspace_bytes(int64_t F);
int vt_mesh_cluster_faces(const int32_t *faces, int64_t F, int64_t V, const int32_t *cluster_of_vertex, int unique, int32_t *out_faces, int32_t *state,
                          int *n_clusters, int *n_out_faces, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_mesh_cluster_place_workspace_bytes(int64_t K);
int vt_mesh_cluster_place(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int resolution, const int32_t *cluster_of_vertex,
                          const int32_t *cluster_rep, int64_t K, int placement, void *out_verts, int32_t *state, void *workspace, size_t workspace_bytes,
                          void *stream);

/* ---- mesh decimation by edge collapse (mesh_collapse.hip) --------------------------------------------------------------------------- */
/* Replaces: the reference's generation.simplify_nfaces as its tool chain means it (simplify_mesh: quadric edge-collapse decimation).    */
/*   Rounds of independent collapses: an edge {u, v}, u < v, is a candidate when neither end touches an edge that is not used once in     */
/*   each direction, the ends share exactly two neighbours, the link is no tetrahedron, the position and cost are finite and no face     */
/*   around it flips; of the candidates an independent set is taken by a key (12 bits of the float32 cost, 20 hash bits, the edge's       */
/*   lowest half-edge) that has to be the smallest within both ends' closed one-rings; of those the first ceil((F - target) / 2) by       */
/*   lowest half-edge are applied, each removing two faces.  A closed manifold stays one and lands on the largest even count <=           */
/*   target_faces; boundary and non-manifold edges never move.  tests/mesh_collapse_ref.py is the definition and the kernels equal it     */
/*   bit for bit ("mesh_collapse.hip").  Meshes and size rules as in the topology block; F <= (2^31 - 1) / 6.                  */
/* vt_mesh_collapse: placement 0 ('optimal': the minimiser of the summed quadrics about the midpoint, the midpoint where that is not      */
/*   finite or not better) or 1 ('midpoint'); max_rounds >= 1 bounds the rounds that collapse something.  out_verts (capacity V, the      */
/*   vertices' type), out_faces (capacity F), vertex_map [V] (the output vertex every input vertex went into; -1: unreferenced);          */
/*   *rounds counts the rounds that collapsed something, *stalled is 1 when a round found no candidate above the target.  Waits for       */
/*   the stream: one read after the prologue (a face index outside [0, V) or a non-finite referenced coordinate: VT_ERR_INVALID, before   */
/*   any such index is dereferenced), one per batch of 4 rounds, one at the end.                                                          */
size_t vt_mesh_collapse_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_collapse(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int64_t target_faces, int placement, int max_rounds,
                     void *out_verts, int32_t *out_faces, int32_t *vertex_map, int *n_out_verts, int *n_out_faces, int *rounds, int *stalled,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- mesh normals (mesh_normals.hip) ----------------------------------------------------------------------------------------------- */
/* Replaces: trimesh.Trimesh.face_normals / .vertex_normals of the meshes the reference builds (src/conv_onet/generation.py:273-284;     */
/*   Generator3D's with_normals, generation.py:34,46).  tests/mesh_normals_ref.py restates the rule in numpy float64.                    */
/* vt_mesh_normals: face_normals [F][3] and vertex_normals [V][3] in the vertices' type; either may be NULL, not both.  A face is        */
/*   degenerate unless the squared length of (v1 - v0) x (v2 - v0), in float64, is positive and finite: its normal is (0,0,0) and it     */
/*   adds nothing to a vertex.  weight 0 ('area'): a vertex sums the raw cross products of its faces; 1 ('angle'): their unit normals    */
/*   times the interior angle at the vertex.  The sums are exact fixed-point accumulations by integer atomics (no float atomic), so      */
/*   the result has equal bits from run to run and under any order of the faces; a vertex without a live face, or whose terms cancel     */
/*   exactly, gets (0,0,0).  Sizes as in the topology block.  A face index outside [0, V) is never dereferenced and makes the call       */
/*   VT_ERR_INVALID.  Waits for the stream (one read of the status word).                                                                */
size_t vt_mesh_normals_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_normals(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int weight, void *face_normals,
                    void *vertex_normals, void *workspace, size_t workspace_bytes, void *stream);

/* ---- mesh hole filling (mesh_fill.hip) --------------------------------------------------------------------------------------------- */
/* Replaces: trimesh.repair.fill_holes on the meshes the reference wraps in trimesh.Trimesh -- without its limit to 3- and 4-edge       */
/*   holes.  tests/mesh_fill_ref.py is the definition and the kernels equal it bit for bit ("mesh_fill.hip").  Meshes and    */
/*   size rules as in the topology block.  Half-edge h = 3 f + k runs from faces[f][k] to faces[f][(k+1)%3]; it is a boundary half-edge */
/*   when its undirected edge is used by no other half-edge.  succ(h): the boundary half-edge that leaves head(h) when exactly one      */
/*   leaves and one enters that vertex; a loop is a cycle of succ; the boundary half-edges on no cycle are `irregular`.  Loops are      */
/*   numbered by their smallest half-edge, and start there.                                                                              */
/* vt_mesh_boundary: the edge table, the boundary half-edges compacted in half-edge order and succ over them, left in the workspace     */
/*   (vt_mesh_boundary_workspace_bytes(V, F) bytes) for vt_mesh_boundary_loops; *n_boundary = NB.  Waits for the stream (one read; a    */
/*   face index outside [0, V) makes it VT_ERR_INVALID; NB = 0 launches nothing further).                                               */
/* vt_mesh_boundary_loops: on the workspace vt_mesh_boundary left for the same faces, NB >= 1 its count.  Pointer doubling (ceil(log2   */
/*   NB) rounds for the loop's smallest element, as many for the position; enqueued at once), then loop_offsets [L+1] (capacity NB+1),  */
/*   loop_vertices and loop_half_edges [NB - n_irregular] (capacity NB): loop l owns [loop_offsets[l], loop_offsets[l+1]), element p    */
/*   the p-th half-edge after the loop's smallest and its tail vertex.  Waits for the stream (one read: *n_loops, *n_irregular).        */
/* vt_mesh_fill_count: per loop of n edges, filled when 3 <= n <= max_edges (max_edges 0: no limit): method 0 ('fan') n - 2 faces       */
/*   (v_0, v_{i+1}, v_i), i = 1 .. n-2; method 1 ('centroid') for n >= 4 one new vertex c and n faces (c, v_{i+1}, v_i), i = 0 .. n-1,  */
/*   for n = 3 the one face (v_0, v_2, v_1).  Leaves the loops' face and vertex offsets in the workspace                                 */
/*   (vt_mesh_fill_workspace_bytes(L) bytes).  Waits for the stream (one read: the three totals).                                       */
/* vt_mesh_fill_emit (asynchronous): on the workspace vt_mesh_fill_count left for the same loops and method.  out_verts [V +            */
/*   n_new_verts][3] in the vertices' type and out_faces [F + n_new_faces][3]: the originals copied, then the new faces by (loop, i)    */
/*   and the new vertices by loop.  c = (the exact fixed-point sum of the loop's coordinates, as vt_mesh_component_stats sums) / n in   */
/*   float64, rounded to the vertices' type: the bits depend on no order.  F = 0 is allowed here (nothing is copied).                   */
size_t vt_mesh_boundary_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_boundary(const int32_t *faces, int64_t F, int64_t V, int *n_boundary, void *workspace, size_t workspace_bytes, void *stream);
int vt_mesh_boundary_loops(const int32_t *faces, int64_t F, int64_t V, int64_t NB, int32_t *loop_offsets, int32_t *loop_vertices,
                           int32_t *loop_half_edges, int *n_loops, int *n_irregular, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_mesh_fill_workspace_bytes(int64_t L);
int vt_mesh_fill_count(const int32_t *loop_offsets, int64_t L, int method, int64_t max_edges, int *n_filled, int *n_new_faces, int *n_new_verts,
                       void *workspace, size_t workspace_bytes, void *stream);
int vt_mesh_fill_emit(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, const int32_t *loop_offsets,
                      const int32_t *loop_vertices, int64_t L, int method, int64_t n_new_faces, int64_t n_new_verts, void *out_verts,
                      int32_t *out_faces, void *workspace, size_t workspace_bytes, void *stream);

/* ---- vertex adjacency and mesh smoothing (mesh_smooth.hip) ------------------------------------------------------------------------ */
/* Replaces: trimesh.Trimesh.vertex_neighbors and trimesh.smoothing.filter_laplacian / filter_taubin / filter_humphrey.                 */
/*   tests/mesh_smooth_ref.py is the definition and the kernels equal it bit for bit ("mesh_smooth.hip").  Meshes as in the  */
/*   topology block; F <= (2^31 - 1) / 6 = 357913941, because nnz <= 6 F has to fit the int32 offsets (a larger F is VT_ERR_INVALID).   */
/* vt_mesh_adjacency_count: the undirected edges {a, b}, a != b, each once however many faces share it, counted per vertex and scanned: */
/*   offsets [V+1], *nnz = offsets[V] = twice the number of edges.  Leaves the edge table in the workspace                               */
/*   (vt_mesh_adjacency_workspace_bytes(V, F) bytes).  Waits for the stream (one read; a face index outside [0, V) is VT_ERR_INVALID).  */
/* vt_mesh_adjacency_fill (asynchronous): on the workspace vt_mesh_adjacency_count left for the same faces, nnz >= 1 its count:         */
/*   neighbors [nnz], every row ascending; boundary_edge [nnz], 1 where the edge has exactly one face; boundary_vertex [V], 1 where a   */
/*   boundary edge ends at the vertex.  An unreferenced vertex has an empty row.                                                         */
/* vt_mesh_smooth_weights (asynchronous): w [nnz] f64.  scheme 0 ('uniform') 1.0; scheme 1 ('inverse_distance')                          */
/*   1 / sqrt((dx*dx + dy*dy) + dz*dz) of the given positions in float64, 0 for a coincident neighbour.                                 */
/* vt_mesh_smooth (asynchronous; every pass is enqueued, nothing is read back): positions are carried in float64 (three buffers,         */
/*   vt_mesh_smooth_workspace_bytes(V) bytes) and rounded once into out_verts [V][3] of the vertices' type.  The row mean m_i = (sum_j   */
/*   w_ij x_j) / (sum_j w_ij), both sums over j in ascending neighbour order, per coordinate, in double, without FMA; w NULL: every     */
/*   weight 1; a weight 0 is left out of both sums.  A vertex with an empty row, a zero weight sum or a pinned flag keeps its bits.     */
/*   method 0 ('laplacian'): x <- x + lam (m - x), `iterations` passes.  method 1 ('taubin'): `iterations` pairs of passes, lam then mu. */
/*   method 2 ('humphrey'): per iteration q <- x; x <- m(q); b <- x - (alpha o + (1 - alpha) q), o the input; x <- x - (beta b +        */
/*   (1 - beta) m(b)).  boundary 0 ('pin'): vertices with boundary_vertex set never move; 1 ('free'): no special case; 2 ('loop'): a    */
/*   boundary vertex averages only the neighbours across boundary edges.  iterations 0, or nnz 0, copies the input's bits.              */
/*   form 1: one launch per pass, positions in the workspace; form 2: every pass in one launch of one workgroup, positions in LDS       */
/*   (V <= 2048, no workspace); form 0: form 2 where it fits, form 1 elsewhere.  The two forms return equal bits.                        */
size_t vt_mesh_adjacency_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_adjacency_count(const int32_t *faces, int64_t F, int64_t V, int32_t *offsets, int *nnz, void *workspace, size_t workspace_bytes,
                            void *stream);
int vt_mesh_adjacency_fill(int64_t F, int64_t V, int64_t nnz, int32_t *neighbors, uint8_t *boundary_edge, uint8_t *boundary_vertex, void *workspace,
                           size_t workspace_bytes, void *stream);
int vt_mesh_smooth_weights(const void *verts, int verts_f64, int64_t V, const int32_t *offsets, const int32_t *neighbors, int64_t nnz, int scheme,
                           double *w, void *stream);
size_t vt_mesh_smooth_workspace_bytes(int64_t V);
int vt_mesh_smooth(const void *verts, int verts_f64, int64_t V, const int32_t *offsets, const int32_t *neighbors, const uint8_t *boundary_edge,
                   const uint8_t *boundary_vertex, int64_t nnz, const double *w, int method, int iterations, double lam, double mu, double alpha,
                   double beta, int boundary, int form, void *out_verts, void *workspace, size_t workspace_bytes, void *stream);

/* ---- mesh subdivision (mesh_subdivide.hip) ----------------------------------------------------------------------------------------- */
/* Replaces: UpSampleLayer of the reference (src/encoder/manopth/upsample_layer.py: a dict of edges filled face by face on the host)     */
/*   and trimesh.remesh.subdivide / subdivide_to_size / subdivide_loop.  tests/mesh_subdivide_ref.py is the definition and the kernels   */
/*   equal it bit for bit ("mesh_subdivide.hip").  Meshes as in the topology block; F = 0 is allowed.  One pipeline: mark a   */
/*   set of edges, give each marked edge one new vertex V + e, split each face by how many of its edges are marked.                      */
/* vt_mesh_subdivide_count: mark 0 every edge; mark 1 the edges with (dx*dx + dy*dy) + dz*dz > max_edge^2 in double, d from the lower    */
/*   index to the higher; mark 2 the edges of the faces with face_mask [F] != 0.  Marked edges are numbered in the order in which a      */
/*   walk over the half-edges 3 f + k first meets them.  *n_marked; *n_out_faces = sum of 1 + marks(f); *n_irregular = the marked edges  */
/*   whose direction counts are neither (1, 1) nor (1, 0) / (0, 1).  Leaves table, numbering and face offsets in the workspace           */
/*   (vt_mesh_subdivide_workspace_bytes(V, F) bytes).  Waits for the stream (one read).  A face with an index outside [0, V) or with a  */
/*   repeated index makes it VT_ERR_INVALID, and so does V + n_marked >= 2^31; such an index is never dereferenced.                      */
/* vt_mesh_subdivide_emit (asynchronous): on the workspace vt_mesh_subdivide_count left for the same faces.  out_verts [V + n_marked]    */
/*   [3] in the vertices' type, out_faces [n_out_faces][3], edge_verts [n_marked][2] = (lo, hi), face_parent [n_out_faces] = the face    */
/*   every child came from; a face's children are contiguous, faces in their order.  Face (a, b, c) with x on ab, y on bc, z on ca:      */
/*   3 marks (x,y,z) (a,x,z) (b,y,x) (c,z,y); 0 marks (a,b,c); 1 mark, rotated to the marked edge (p, q), r opposite, m its vertex:      */
/*   (p,m,r) (m,q,r); 2 marks, rotated to the unmarked edge (p, q), s on qr, t on rp: (r,t,s) and the quad p q s t cut along the         */
/*   shorter of p-s and q-t (squared lengths in double, s and t the double midpoints of the input positions; a tie: the diagonal at the  */
/*   lower of the indices p and q): (p,q,s) (p,s,t) or (p,q,t) (q,s,t).  scheme 0 ('midpoint'): originals copied bit for bit, a new      */
/*   vertex (x_lo + x_hi) * 0.5 in the vertices' type.  scheme 1 ('loop', with mark 0 only; offsets [V+1], neighbors, boundary_edge      */
/*   [nnz], boundary_vertex [V] from vt_mesh_adjacency_count / _fill), in double, rounded once: a new vertex on a (1, 1) edge            */
/*   0.375 (x_lo + x_hi) + 0.125 (x_c + x_d), c and d opposite in the lo -> hi and the hi -> lo face, on any other edge the midpoint;   */
/*   an interior vertex of degree n (1 - n b) x + b sum_j x_j over its row in ascending order, b = 3/16 for n = 3 and 3 / (8 n)          */
/*   otherwise; a boundary vertex with exactly two boundary neighbours 0.75 x + 0.125 (x_j + x_k); a vertex at an irregular edge, with   */
/*   another boundary count or with an empty row keeps its bits.                                                                         */
/* vt_mesh_subdivide_midpoints (asynchronous): the midpoint scheme's vertices for a batch that shares edge_verts [E][2]: out_verts       */
/*   [B][V + E][3] from verts [B][V][3].  A pair outside [0, V) is not dereferenced; its vertex is NaN.                                  */
/* vt_mesh_subdivide_bwd (asynchronous): the midpoint scheme's gradient, grad_verts [V][3] from grad_out [V + E][3] of one type:         */
/*   g_v[i] = g[i] + 0.5 sum of g[V + e] over the edges e at i, every sum exact in two fixed-point limbs against its largest term and    */
/*   rounded once (vt_mesh_subdivide_bwd_workspace_bytes(V) bytes): equal bits from run to run.  A sum with a term that is not finite    */
/*   is NaN; a pair outside [0, V) takes no part and sets bit 0 of the workspace's first word.                                           */
size_t vt_mesh_subdivide_workspace_bytes(int64_t V, int64_t F);
int vt_mesh_subdivide_count(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int mark, double max_edge,
                            const uint8_t *face_mask, int *n_marked, int *n_out_faces, int *n_irregular, void *workspace, size_t workspace_bytes,
                            void *stream);
int vt_mesh_subdivide_emit(const void *verts, int verts_f64, int64_t V, const int32_t *faces, int64_t F, int64_t n_marked, int64_t n_out_faces,
                           int scheme, const int32_t *offsets, const int32_t *neighbors, const uint8_t *boundary_edge, const uint8_t *boundary_vertex,
                           int64_t nnz, void *out_verts, int32_t *out_faces, int32_t *edge_verts, int32_t *face_parent, void *workspace,
                           size_t workspace_bytes, void *stream);
int vt_mesh_subdivide_midpoints(const void *verts, int verts_f64, int64_t B, int64_t V, const int32_t *edge_verts, int64_t E, void *out_verts,
                                void *stream);
size_t vt_mesh_subdivide_bwd_workspace_bytes(int64_t V);
int vt_mesh_subdivide_bwd(const int32_t *edge_verts, int64_t V, int64_t E, const void *grad_out, int grad_f64, void *grad_verts, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------------------------ */
/* Fast winding number (csrc/winding_fast.hip; DESIGN.md section "winding_fast.hip"; tests/winding_fast_ref.py restates it in numpy):     */
/* an octree over the faces' centroids, `depth` levels below the root (1 .. VT_WN_MAX_DEPTH), whose occupied cells carry the dipole       */
/* expansion of their faces to order 2 (Barill et al. 2018).  Replaces: igl.fast_winding_number_for_meshes(V, F, Q) of the reference     */
/* (src/conv_onet/training.py:307, 359, 723, 862), which vt_winding_number evaluates exactly.                                            */
/* verts [V,3] f32, faces [F,3] i32 (indices clamped to [0, V) as vt_winding_number clamps them), pts [N,3] f32.                          */
/* A tree is built by two asynchronous calls with one host read between them:                                                            */
/*   vt_winding_tree_count  frame, leaf codes, the index pyramids and the list offsets, into the workspace                                 */
/*                          (vt_winding_tree_workspace_bytes(V, F, depth) bytes, 0 for sizes outside the limits).  Its first 16 int32      */
/*                          are the state the caller reads back: word 0 the status (bit 0: a vertex coordinate that is not finite),        */
/*                          words 1 .. 8 the occupied cells of level 0 .. 7.                                                              */
/*   vt_winding_tree_layout host only: from those 16 words, offsets[0..4] = the byte offsets in the tree of the pyramids (int32, level l   */
/*                          at word (8^l - 1) / 7), the records (36 doubles per occupied cell, level by level: p[3], r, N0[3], M1[3][3],  */
/*                          M2[6][3], area, faces), the list offsets (leaves + 1 int32), the lists (F int32, ascending inside a leaf)     */
/*                          and the faces' corners in list order (F x 9 f32); offsets[5] = the tree's bytes.                              */
/*   vt_winding_tree_build  the lists and every record, into `tree`; the same workspace, untouched since the count.  state_host[0] != 0   */
/*                          (a bounding box that is not finite) is VT_ERR_INVALID.  The workspace is free afterwards.                      */
/* vt_winding_tree_query (asynchronous, reads nothing back, safe to capture): out [N] f32, or f64 with out_f64; stats NULL or [N][2]     */
/*   int32 (cells accepted, faces summed exactly).  A cell is accepted when |q - p|^2 > accuracy^2 r^2; order 0, 1 or 2.                  */
/* Errors, all before any launch: a NULL array or a negative size is VT_ERR_INVALID; depth outside [1, VT_WN_MAX_DEPTH], F or V beyond    */
/*   the mesh kernels' limits VT_ERR_UNSUPPORTED; a short workspace or tree VT_ERR_WORKSPACE.  F == 0 gives zeros, N == 0 launches        */
/*   nothing.  Trees and results are bit-reproducible: no float atomic, one summation order.                                              */
#define VT_WN_MAX_DEPTH 7
int vt_winding_tree_default_depth(int64_t F);
size_t vt_winding_tree_workspace_bytes(int64_t V, int64_t F, int depth);
int vt_winding_tree_count(const float *verts, int64_t V, const int32_t *faces, int64_t F, int depth, void *workspace, size_t workspace_bytes,
                          void *stream);
int vt_winding_tree_layout(int64_t F, int depth, const int32_t *state_host, size_t *offsets);
int vt_winding_tree_build(const float *verts, int64_t V, const int32_t *faces, int64_t F, int depth, const int32_t *state_host, void *workspace,
                          size_t workspace_bytes, void *tree, size_t tree_bytes, void *stream);
int vt_winding_tree_query(const void *tree, size_t tree_bytes, int64_t F, int depth, const int32_t *state_host, const float *pts, int64_t N,
                          double accuracy, int order, void *out, int out_f64, int32_t *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------------------------------ */
/* Closest point on a mesh through that octree (csrc/closest_point_tree.hip; DESIGN.md section "closest_point_tree.hip";                  */
/* tests/closest_point_tree_ref.py restates it in numpy): the d2, face and closest of vt_closest_point_mesh, bit for bit -- both call     */
/* one cp_face (csrc/closest_point_face.h) -- from a walk that skips every cell whose bounding box is farther than the best face so far.  */
/* `tree`, `depth` and `state_host` are a built winding tree's (vt_winding_tree_build) and the 16 words its caller read back.             */
/*   vt_closest_tree_layout host only: offsets[0..1] = the byte offsets in the side buffer of the boxes (6 doubles lo[3], hi[3] per       */
/*                          occupied cell, level by level as the tree's records) and of the face records (14 doubles per face, in list    */
/*                          order: slot t is face lists[t]); offsets[2] = the side buffer's bytes.  Its first int32 is the status word    */
/*                          (bit 0: a face index outside [0, V); that face is in no box and is never read).                              */
/*   vt_closest_tree_build  the boxes and the records, into `side`, from the tree and the mesh it was built on.                           */
/*   vt_closest_tree_query  d2 [N] f64, face [N] i32, closest NULL or [N][3] f64, stats NULL or [N][2] int32 (boxes tested, faces        */
/*                          tested).  A cell is skipped when lb - delta > best, delta = 2^-40 S^2 (S from the frame and the query).       */
/*                          VTACO_CLOSEST_TREE_WALK = plain | seed | order | seed+order (the default) picks the walk: equal results.      */
/* Both launch functions are asynchronous, read nothing back and allocate nothing.  Errors, all before any launch: a NULL array, F <= 0   */
/*   or V <= 0 is VT_ERR_INVALID (a mesh needs vertices and faces, as for vt_closest_point_mesh); depth outside [1, VT_WN_MAX_DEPTH]      */
/*   VT_ERR_UNSUPPORTED; a short tree or side buffer VT_ERR_WORKSPACE.  N == 0 launches nothing.                                          */
int vt_closest_tree_layout(int64_t F, int depth, const int32_t *state_host, size_t *offsets);
int vt_closest_tree_build(const float *verts, int64_t V, const int32_t *faces, int64_t F, int depth, const int32_t *state_host, const void *tree,
                          size_t tree_bytes, void *side, size_t side_bytes, void *stream);
int vt_closest_tree_query(const void *tree, size_t tree_bytes, const void *side, size_t side_bytes, int64_t F, int depth, const int32_t *state_host,
                          const float *pts, int64_t N, double *d2, int32_t *face, double *closest, int32_t *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------------------------------ */
/* Nearest point of a point set through an octree over the points (csrc/point_tree.hip; DESIGN.md section "point_tree.hip";               */
/* tests/point_tree_ref.py restates it in numpy): vt_nn_points' d2 and idx, bit for bit, without testing every target.  Stands where the   */
/* reference searches a kd-tree (src/utils/icp.py:50-66, src/common.py:94-175).  B problems per call, dst [B][M][3] f64 with one M and    */
/* one depth; every kernel covers the batch in one launch.  Frame, cells, Morton numbering, pyramids and lists are the winding tree's      */
/* with points for centroids; each occupied cell carries the tight box lo[3], hi[3] of its points; the points are copied in list order.    */
/*   vt_point_tree_default_depth  the smallest L in 1 .. VT_WN_MAX_DEPTH with 8^L * 8 >= M                                                 */
/*   vt_point_tree_count    frames, leaf codes, the pyramids and the list offsets of all B problems, into the workspace                    */
/*                          (vt_point_tree_workspace_bytes(M, B, depth) bytes, 0 for sizes outside the limits).  Its first 16 B int32      */
/*                          are the state words the caller reads back, once per batch: per problem word 0 the status (bit 0: a target      */
/*                          coordinate is not finite), words 1 .. 1 + depth the occupied cells of level 0 .. depth.                        */
/*   vt_point_tree_layout   host only: from those words, offsets[0..4] = the byte offsets inside one problem's tree of the pyramids        */
/*                          (int32, level l at word (8^l - 1) / 7), the boxes (6 f64 per cell), the list offsets (int32, leaves + 1), the  */
/*                          lists (int32 [M]) and the points in list order (f64 [M][3]); offsets[5] = the bytes from one problem's tree     */
/*                          to the next, offsets[6] = the bytes of all B.  The per-problem descriptors: every problem's tree has the same  */
/*                          offsets, a level's boxes having room for that level's largest count over the batch (level l starts at box      */
/*                          sum of those maxima over the levels above); the launch functions recompute this from state_host and pass it     */
/*                          to the kernels by value, which find their problem at blockIdx.y * offsets[5].  Bytes past a problem's own      */
/*                          counts are not written.                                                                                        */
/*   vt_point_tree_build    lists, points, boxes and headers into `tree`; the same workspace, untouched since the count.  A status word     */
/*                          != 0 is VT_ERR_INVALID ("a target coordinate is not finite").                                                  */
/*   vt_point_tree_query    (asynchronous, allocates nothing, reads nothing back, safe to capture) src [B][N][3] f64, T [B][4][4] or NULL   */
/*                          (applied to src first, vt_nn_points' arithmetic) -> d2 [B][N] f64, idx [B][N] i32; stats NULL or [B][N][2]     */
/*                          int32: boxes tested, points tested.  One lane per query, a walk without a stack that skips a cell exactly      */
/*                          when its box's lower bound exceeds the best d2 so far.  VTACO_POINT_TREE_WALK = plain | seed | order |         */
/*                          seed+order (the default) picks the walk; all give equal results.                                               */
/*                          perm NULL or [B][N] i32, a permutation of 0 .. N-1 per problem: lane i answers query perm[i].  Outputs stay    */
/*                          in query order; no result depends on it.                                                                      */
/*   vt_point_tree_lanes    perm for vt_point_tree_query: the queries (moved by T when given) in Morton order of the tree's leaves, by      */
/*                          count / scan / fill through an integer cursor; the order inside a leaf is whatever the cursor hands out.       */
/*                          workspace: vt_point_tree_lanes_workspace_bytes(N, B, depth).  Asynchronous, reads nothing back.                */
/* Errors, all before any launch: a NULL array, M < 1, N < 1 or B outside [1, 65535] is VT_ERR_INVALID, as are counts no tree of this size  */
/* has; depth outside [1, VT_WN_MAX_DEPTH] is VT_ERR_UNSUPPORTED; a short workspace or tree VT_ERR_WORKSPACE.                              */
/* vt_icp_tree -- vt_icp with the neighbour search of every iteration done by vt_point_tree_query on the built trees of Bp (tree, depth,    */
/*   state_host as above); the partners are still read from Bp through idx.  Fit, move, state and the gate of finished problems are        */
/*   vt_icp's: equal bits in every output.  Enqueued in full, no host read.  morton_lanes != 0: the queries are handed to lanes in the    */
/*   order vt_point_tree_lanes gives for the working copy the loop starts with, built once.  workspace:                                  */
/*   vt_icp_tree_workspace_bytes(N, B, depth).                                                                                           */
int vt_point_tree_default_depth(int64_t M);
size_t vt_point_tree_workspace_bytes(int64_t M, int B, int depth);
int vt_point_tree_count(const double *dst, int64_t M, int B, int depth, void *workspace, size_t workspace_bytes, void *stream);
int vt_point_tree_layout(int64_t M, int depth, int B, const int32_t *state_host, size_t *offsets);
int vt_point_tree_build(const double *dst, int64_t M, int B, int depth, const int32_t *state_host, void *workspace, size_t workspace_bytes, void *tree,
                        size_t tree_bytes, void *stream);
int vt_point_tree_query(const void *tree, size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, const double *src, int64_t N,
                        const double *T, double *d2, int32_t *idx, int32_t *stats, const int32_t *perm, void *stream);
size_t vt_point_tree_lanes_workspace_bytes(int64_t N, int B, int depth);
int vt_point_tree_lanes(const void *tree, size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, const double *src, int64_t N,
                        const double *T, int32_t *perm, void *workspace, size_t workspace_bytes, void *stream);
size_t vt_icp_tree_workspace_bytes(int64_t N, int B, int depth);
int vt_icp_tree(const double *A, int64_t N, const double *Bp, int64_t M, int B, const void *tree, size_t tree_bytes, int depth,
                const int32_t *state_host, int morton_lanes, const double *init_pose, int max_iterations, double tolerance, double *T,
                double *distances, int32_t *idx, int32_t *iterations, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------------------------ */
/* What a ray hits first on a mesh, and the sensor camera on it (csrc/ray_mesh.hip; DESIGN.md section "ray_mesh.hip";                     */
/* tests/ray_mesh_ref.py restates it in numpy).  Stands where a trimesh.Trimesh offers mesh.ray.intersects_first /                        */
/* intersects_location; the reference takes its tactile depth images from a simulator outside its tree.                                  */
/* Rays are o + s d in float64, d NOT normalised, s in units of d: origins [N / rays_per_origin][3] (ray n starts at origin               */
/* n / rays_per_origin: 1 for one origin per ray, N for one origin, H * W for camera images), dirs [N][3].  The rule is the watertight   */
/* test of Woop, Benthin and Wald (2013), two-sided, in float64 (csrc/ray_face.h): zeros are accepted on both sides of an edge and the   */
/* two faces of an edge compute exact negatives there, so no ray passes between them.  Per ray: s [N] f64 the smallest hit parameter in  */
/* [t_min, t_max], face [N] i32 its face (the lowest index among equal s), bary NULL or [N][3] f64 the weights of the face's three        */
/* corners.  A miss is +inf, -1, NaN weights.  A ray with a zero direction, or an origin or direction that is not finite, misses.         */
/*   vt_ray_mesh         every face per ray: the definition.  workspace: vt_ray_mesh_workspace_bytes(F, N) bytes (0 for F <= 0); its     */
/*                       first int32 is the status word (bit 0: a face index outside [0, V); that face is never read).                  */
/*   vt_ray_tree_query   the same s, face and weights, bit for bit, from a walk of a built winding tree and its closest-point side       */
/*                       buffer (vt_winding_tree_build, vt_closest_tree_build: nothing more is built per mesh; the side buffer's status   */
/*                       word reports a bad index).  A cell is skipped when the segment [t_min, min(t_max, best)] misses its box grown    */
/*                       by 2^-40 S (S from the frame and the origin).  stats NULL or [N][2] int32 (boxes tested, faces tested).          */
/*                       VTACO_RAY_TREE_WALK = plain | order (the default) picks the walk: equal results.                                 */
/*   vt_camera_rays      the inverse of vt_contact_points' unprojection, from the same pose records [n_images][16] f64: origins           */
/*                       [n_images][3] = (t - centroid) / scale, dirs [n_images][height * width][3] = M (1, -(u - W/2) / f,               */
/*                       -(v - H/2) / f) / scale, f = height / (2 tan(fov / 2)).  The camera-axis component is 1, so the s of a hit is    */
/*                       the planar depth vt_contact_points and vt_depth_cloud unproject.                                                 */
/*   vt_depth_from_hits  depth [N] f32 = min(s, depth_origin[n % n_pixels]) clamped below at `near`; depth_origin NULL: no minimum (a     */
/*                       miss stays +inf).                                                                                                */
/* All four are asynchronous, read nothing back and allocate nothing.  Errors, all before any launch: a NULL array, a negative size, a   */
/*   mesh without vertices or faces, or rays_per_origin < 1 is VT_ERR_INVALID; depth outside [1, VT_WN_MAX_DEPTH] VT_ERR_UNSUPPORTED;    */
/*   a short workspace, tree or side buffer VT_ERR_WORKSPACE.  N == 0 launches nothing.                                                  */
size_t vt_ray_mesh_workspace_bytes(int F, int64_t N);
int vt_ray_mesh(const float *verts, int V, const int32_t *faces, int F, const double *origins, int64_t rays_per_origin, const double *dirs, int64_t N,
                double t_min, double t_max, double *s, int32_t *face, double *bary, void *workspace, size_t workspace_bytes, void *stream);
int vt_ray_tree_query(const void *tree, size_t tree_bytes, const void *side, size_t side_bytes, int64_t F, int depth, const int32_t *state_host,
                      const double *origins, int64_t rays_per_origin, const double *dirs, int64_t N, double t_min, double t_max, double *s,
                      int32_t *face, double *bary, int32_t *stats, void *stream);
int vt_camera_rays(const double *pose, int n_images, int width, int height, double fov_deg, double *origins, double *dirs, void *stream);
int vt_depth_from_hits(const double *s, const double *depth_origin, int64_t n_pixels, int64_t N, double near, float *depth, void *stream);

/* ------------------------------------------------------------------------------------------------------------------------------------ */
/* The field's second-order jet and mesh refinement on it (csrc/field_jet.hip, csrc/refine.hip; DESIGN.md section "field_jet / refine";  */
/* tests/refine_ref.py states both in float64 autograd).  Stands where the Convolutional Occupancy Networks generator's refine_mesh     */
/* differentiates the decoder twice (generation.refinement_step).  The 32 / 32 / 5 plain decoder only: C != 32 is VT_ERR_UNSUPPORTED.   */
/*   vt_decode_jet           jet [B*N][8] f32 = (f, f_x, f_y, f_z, f_xy, f_xz, f_yz, 0) at pts [B][N][3]: the logit, its gradient with      */
/*                           respect to the point and the three mixed second derivatives (the pure ones are zero: the field is           */
/*                           multilinear inside a cell between ReLU kinks).  An axis whose coordinate the normalisation clamps has zero  */
/*                           derivatives.  blob / blob_t: vt_decoder_pack / vt_decoder_pack_t of the plain decoder.  One kernel, exact-   */
/*                           f32 matrix core; f is vt_decode_fwd's logit bit for bit.                                                     */
/*   vt_decode_jet_composed  the same numbers, bit for bit, from vt_decode_fwd (save) + vt_decode_bwd_dc (grad_out = 1) + one gather     */
/*                           kernel.  workspace: vt_decode_jet_composed_workspace_bytes(B, N) (B = 1 runs in passes of 2^17 points).      */
/*   vt_refine_sample        pts [F][3] = (eps_0 v_0 + eps_1 v_1) + eps_2 v_2 per face; eps_in [F][3] given, or NULL: eps [F][3] is drawn   */
/*                           as Dirichlet(1/2,1/2,1/2) from a counter hash of (seed, step, face).  eps may be eps_in.                     */
/*   vt_refine_face_grad     the vertex gradient of L = mean (sigmoid(f) - threshold)^2 + normal_weight mean |n_face - n_target|^2,       */
/*                           n_target = -g / (|g| + 1e-10), g = grad sigmoid(f), differentiated through g: added into accum as exact      */
/*                           fixed-point sums (vt_refine_accum_bytes(V) bytes, zero before the first call; equal bits under any face      */
/*                           order).  terms NULL or [F][2] f32: (sigmoid(f) - threshold)^2 and |n_face - n_target|^2 per face.            */
/*   vt_refine_step          grad (NULL or [V][3] f32) = the sums, which it zeroes; sq = alpha sq + (1 - alpha) grad^2;                    */
/*                           verts -= lr grad / (sqrt(sq) + eps): torch.optim.RMSprop.                                                     */
/*   vt_refine               `steps` iterations of sample -> jet -> face_grad -> step (RMSprop alpha 0.99, eps 1e-8) on one stream, no    */
/*                           host read.  Iteration i draws with step = first_step + i; eps_given (steps <= 1) replaces the draw.  sq      */
/*                           [V][3] is the caller's (zeros at the start).  composed_jet != 0 takes vt_decode_jet_composed.  terms NULL or  */
/*                           [steps][F][2].  workspace: vt_refine_workspace_bytes(V, F, composed_jet).                                     */
/* A face with an index outside [0, V) is never dereferenced and contributes nothing.  All are asynchronous and read nothing back.       */
int vt_decode_jet(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N, const float *blob, const float *blob_t,
                  double padding, float *jet, void *stream);
size_t vt_decode_jet_composed_workspace_bytes(int B, int64_t N);
int vt_decode_jet_composed(const float *grid_cl, int B, int R, int C, const float *pts, int64_t N, const float *blob, const float *blob_t,
                           double padding, float *jet, void *workspace, size_t workspace_bytes, void *stream);
int vt_refine_sample(const float *verts, int64_t V, const int32_t *faces, int64_t F, const float *eps_in, uint64_t seed, uint64_t step,
                     float *eps, float *pts, void *stream);
size_t vt_refine_accum_bytes(int64_t V);
int vt_refine_face_grad(const float *verts, int64_t V, const int32_t *faces, int64_t F, const float *eps, const float *jet,
                        double threshold, double normal_weight, float *terms, void *accum, size_t accum_bytes, void *stream);
int vt_refine_step(float *verts, int64_t V, void *accum, size_t accum_bytes, float *sq, double lr, double alpha, double eps, float *grad,
                   void *stream);
size_t vt_refine_workspace_bytes(int64_t V, int64_t F, int composed_jet);
int vt_refine(const float *grid_cl, int R, int C, float *verts, int64_t V, const int32_t *faces, int64_t F, const float *blob,
              const float *blob_t, double padding, double threshold, double normal_weight, double lr, int steps, uint64_t seed,
              uint64_t first_step, const float *eps_given, float *sq, int composed_jet, float *terms, void *workspace, size_t workspace_bytes,
              void *stream);

/* ------------------------------------------------------------------------------------------------------------------------------------ */
/* k nearest points of a point set, and normals from them (csrc/knn.hip; DESIGN.md section "knn.hip"; tests/knn_ref.py restates it in     */
/* numpy).  Stands where the reference asks pykdtree for k neighbours (get_nearest_neighbors_indices_batch, src/common.py:158-175) and     */
/* where its visualize_pointcloud is handed normals (src/utils/visualize.py:51).  Everything is float64 in a fixed order; no atomics;      */
/* run-to-run equal bits.  src [B][N][3], dst [B][M][3], T [B][4][4] or NULL (applied to src first, vt_nn_points' arithmetic).            */
/* The result, for both searches: per query the k targets smallest in the order (d2, index), d2 = (dx dx + dy dy) + dz dz, written         */
/*   ascending to d2 [B][N][k] f64 and idx [B][N][k] i32.  The list starts as k entries (+inf, -1); a target is taken when                 */
/*   d < worst || (d == worst && m < worst_m), worst the list's last entry.  With M < k the tail stays (+inf, -1); a query with a NaN or   */
/*   an infinite coordinate returns all (+inf, -1).  1 <= k <= VT_KNN_MAX_K.  k = 1 is vt_nn_points bit for bit.                            */
/*   vt_knn_points       every target per query: 256 queries per workgroup and one slab of targets, one partial list per (query, slab)     */
/*                       in the workspace, a finish pass that merges them in ascending slab order.  slab_points: 0 for                    */
/*                       vt_knn_points_slab_points(N, M, B), else a multiple of 256; no result depends on it.  workspace:                  */
/*                       vt_knn_points_workspace_bytes(N, M, B, k, slab_points) (0 for arguments outside the limits).                      */
/*   vt_point_tree_knn   the same lists, bit for bit, from vt_point_tree_query's walk of a built point tree (tree, depth, state_host as    */
/*                       there): a cell is skipped exactly when its box's lower bound exceeds worst, which is +inf until the list holds    */
/*                       k targets.  stats, perm and VTACO_POINT_TREE_WALK as for vt_point_tree_query.                                     */
/*   vt_knn_normals      pts [B][M][3], idx [B][N][k] (entries outside [0, M) are left out) -> normal [B][N][3]: the unit eigenvector of    */
/*                       the smallest eigenvalue of the neighbours' covariance (centroid and covariance in ascending slot order, by        */
/*                       differences from the first valid neighbour; divided by the count; cyclic Jacobi with a fixed sweep count), eig    */
/*                       [B][N][3]: the eigenvalues ascending.  view NULL: the normal's component of largest magnitude is positive (the    */
/*                       lowest axis among equals); view [B][3] (view_per_point == 0) or [B][N][3]: negated when                          */
/*                       n . (view - pts[idx[..][0]]) < 0.  Fewer than 3 valid neighbours or an exactly zero covariance: zeros.            */
/* All are asynchronous, allocate nothing and read nothing back.  Errors, all before any launch: a NULL array, N or M < 1, B outside       */
/*   [1, 65535] or a slab_points that is no multiple of 256 is VT_ERR_INVALID; k outside [1, VT_KNN_MAX_K] VT_ERR_UNSUPPORTED; a short      */
/*   workspace VT_ERR_WORKSPACE.                                                                                                          */
#define VT_KNN_MAX_K 32
size_t vt_knn_points_workspace_bytes(int64_t N, int64_t M, int B, int k, int slab_points);
int vt_knn_points_slab_points(int64_t N, int64_t M, int B);
int vt_knn_points(const double *src, int64_t N, const double *dst, int64_t M, int B, const double *T, int k, int slab_points, double *d2, int32_t *idx,
                  void *workspace, size_t workspace_bytes, void *stream);
int vt_point_tree_knn(const void *tree, size_t tree_bytes, int64_t M, int depth, int B, const int32_t *state_host, const double *src, int64_t N,
                      const double *T, int k, double *d2, int32_t *idx, int32_t *stats, const int32_t *perm, void *stream);
int vt_knn_normals(const double *pts, int64_t M, const int32_t *idx, int64_t N, int k, int B, const double *view, int view_per_point, double *normal,
                   double *eig, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VTACO_HIP_H */
