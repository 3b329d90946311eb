/* vitpe.h -- C ABI of libvitpe.so: the MI355X (gfx950) kernels behind the ViT
 * attention-with-positional-encoding hot path of zhengyk19/vit-rpe-rope.
 *
 * The reference is pure Python on ATen ops and has no FFI of its own; the boundary it
 * exposes is the Python API models.vit.VisionTransformer(...) + --pos_encoding (reference
 * models/vit.py:148-151, train.py:33-34).  Each entry point below replaces the ATen op
 * sequence of the cited reference lines; the Python host (vit-rpe-rope_amd/vitpe) binds
 * them with ctypes and registers them as torch.library custom ops.
 *
 * Conventions
 *  - every function returns a hipError_t as int (0 = success); nothing throws, nothing
 *    synchronises, nothing allocates: the caller owns every buffer (device pointers);
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*); re-entrant, no global
 *    state, capturable into a hipGraph;
 *  - `dtype` selects the arithmetic/storage type T of activations and GEMM weights:
 *    VITPE_F32 (exact fp32 MFMA, the 1e-4 parity mode) or VITPE_BF16 (bf16 MFMA, fp32
 *    accumulate).  LayerNorm/bias/positional parameters, statistics, logits, gradients of
 *    parameters and optimizer state are always fp32;
 *  - matrices are dense row-major.
 */
#ifndef VITPE_H
#define VITPE_H

#ifdef __cplusplus
extern "C" {
#endif

#define VITPE_F32 0
#define VITPE_BF16 1

/* --pos_encoding switch, reference train.py:33-34 / models/vit.py:170-196 */
#define VITPE_PE_NONE 0
#define VITPE_PE_ABSOLUTE 1
#define VITPE_PE_RELATIVE 2
#define VITPE_PE_POLYNOMIAL 3
#define VITPE_PE_ROPE_AXIAL 4
#define VITPE_PE_ROPE_MIXED 5

/* gemm_nt epilogues */
#define VITPE_EPI_BIAS 0      /* C = A W^T + bias                       (attn.qkv / any Linear)        */
#define VITPE_EPI_BIAS_GELU 1 /* U = A W^T + bias ; C = gelu_erf(U)     (timm Mlp fc1+act, vit.py:118) */
#define VITPE_EPI_BIAS_RESID 2/* C = A W^T + bias + R                   (attn.proj / fc2 + residual, vit.py:91,122,124) */
#define VITPE_EPI_PATCH 3     /* patch-embed: row remap + cls row + APE (vit.py:248-258)               */
#define VITPE_EPI_GELU_BWD 4  /* C = (A W^T) * gelu'(U)                 (autograd of fc1's GELU)       */

typedef void* vitpe_stream_t; /* hipStream_t */

int vitpe_abi_version(void);

/* ---- fused attention (the north-star op) --------------------------------------------------
 * Replaces reference models/vit.py:47-88 (qkv Linear, head split, RoPE rotate-half on patch
 * tokens via rope_utils.py:18-37, QK^T*hd^-0.5, + RelativePositionalEncoding /
 * PolynomialRPE bias (positional_encoding.py:82-95,127-171), softmax, @V, head merge).
 *   xn    [B,N,D] T   layer-normed tokens (N = patches+1, class token first)
 *   wqkv  [3D,D]  T   attn.qkv.weight (no bias: Block passes qkv_bias=False, vit.py:110,200),
 *                     PACKED fragment-major by vitpe_pack_qkv_weights (same element count)
 *   out   [B,N,D] T   merged heads, input of attn.proj
 *   cos/sin: rope-axial [P,HD/2], rope-mixed [H,P,HD/2] contiguous fp32 (else NULL)
 *   table : relative [H,2N-1] fp32 ; coeff: polynomial [deg+1] or [H,deg+1] fp32 (else NULL)
 *   grid  : patches per side (sqrt(P)); degree <= 7.
 * Supported shapes: vitpe_fused_attention_supported() (HD=32, 65<=N<=80, D in {96,192});
 * anything else returns hipErrorNotSupported.                                              */
int vitpe_fused_attention_supported(int dtype, int N, int D, int HD);
/* fp32 master [3D,D] -> T, re-ordered so that each MFMA weight fragment of a wave is one contiguous
 * 1 KB read: block (head, {q,k,v}, 16-row tile, 32-deep K chunk) x 64 lanes x 8 elements          */
int vitpe_pack_qkv_weights(int dtype, const float* wqkv, void* packed, int D, int HD, vitpe_stream_t stream);
int vitpe_fused_attention_fwd(int dtype, const void* xn, const void* wqkv, void* out, int B, int N,
                              int D, int HD, int mode, const float* cos, const float* sin,
                              const float* table, const float* coeff, int grid, int degree,
                              int coeff_per_head, vitpe_stream_t stream);
/* Same with the preceding LayerNorm fused into the token staging: x = RAW tokens, mean/rstd their
 * row statistics, xn_out (nullable) receives LayerNorm(x) (needed by the backward pass).          */
int vitpe_fused_attention_fwd_ln(int dtype, const void* x, const float* gamma, const float* beta,
                                 const float* mean, const float* rstd, void* xn_out, const void* wqkv,
                                 void* out, int B, int N, int D, int HD, int mode, const float* cos,
                                 const float* sin, const float* table, const float* coeff, int grid,
                                 int degree, int coeff_per_head, vitpe_stream_t stream);
/* ---- the "wide" forward: 32x32x16 matrix-core tiles for the benchmark geometry (bf16, N = 65, D = 192, HD = 32) ------
 * Same operation as vitpe_fused_attention_fwd(_ln) (reference models/vit.py:47-88, LayerNorm vit.py:113,122 optional),
 * on weights packed by vitpe_pack_qkv_weights_wide: vitpe_qkv_wide_pack_elems(D) = 3 D D elements of T, the
 * 32x32x16 operand fragments (block (head, {q,k,v}, 16-deep k step) x 64 lanes x 8 = 1 KB, what one LDS-DMA
 * instruction moves); the q rows are pre-multiplied by HD^-0.5 * log2(e).
 * gamma == NULL: x is already layer-normed (beta / mean / rstd / xn_out ignored).  Other shapes: hipErrorNotSupported. */
int vitpe_fused_attention_wide_supported(int dtype, int N, int D, int HD);
int vitpe_qkv_wide_pack_elems(int D);
int vitpe_pack_qkv_weights_wide(int dtype, const float* wqkv, void* packed, int D, int HD, vitpe_stream_t stream);
int vitpe_fused_attention_fwd_wide(int dtype, const void* x, const float* gamma, const float* beta,
                                   const float* mean, const float* rstd, void* xn_out, const void* wqkv_wide,
                                   void* out, int B, int N, int D, int HD, int mode, const float* cos,
                                   const float* sin, const float* table, const float* coeff, int grid, int degree,
                                   int coeff_per_head, vitpe_stream_t stream);
/* Backward of the above (the reference relies on autograd).  dqkv [B,N,3D] T is the gradient of
 * the qkv Linear's output (columns [q|k|v] x heads, like the forward's qkv buffer); the caller
 * finishes with dxn = dqkv Wqkv (vitpe_gemm_nt on the transposed shadow) and dWqkv = dqkv^T xn
 * (vitpe_gemm_tn).  dtable / dcoeff / dfreqs are ACCUMULATED into (fp32 atomics).           */
int vitpe_fused_attention_bwd(int dtype, const void* xn, const void* wqkv, const void* dout,
                              void* dqkv, int B, int N, int D, int HD, int mode, const float* cos,
                              const float* sin, const float* table, const float* coeff, int grid,
                              int degree, int coeff_per_head, float* dtable, float* dcoeff,
                              float* dfreqs, vitpe_stream_t stream);
/* The same with the LayerNorm recomputed while staging: x = RAW tokens, mean / rstd their row statistics (as
 * vitpe_fused_attention_fwd_ln) -- the forward then need not store LayerNorm(x) at all.                       */
int vitpe_fused_attention_bwd_ln(int dtype, const void* x, const float* gamma, const float* beta,
                                 const float* mean, const float* rstd, const void* wqkv, const void* dout,
                                 void* dqkv, int B, int N, int D, int HD, int mode, const float* cos,
                                 const float* sin, const float* table, const float* coeff, int grid,
                                 int degree, int coeff_per_head, float* dtable, float* dcoeff,
                                 float* dfreqs, vitpe_stream_t stream);

/* ---- attention core on a qkv buffer (geometries the fused kernels do not cover) -----------
 * Replaces models/vit.py:49-92 between `qkv = self.qkv(x)` and `self.proj`: head split, RoPE on
 * q,k (rope_utils.py:85-101; class token not rotated), QK^T*hd^-0.5 + relative / polynomial bias
 * (positional_encoding.py:82-95,127-171), softmax, @V, head merge.  One workgroup per (image, head).
 *   qkv  [B,N,3*H*HD] T  output of the qkv Linear (vitpe_linear), columns [q|k|v] x heads x HD
 *   out  [B,N,H*HD]   T  merged heads ; dqkv same layout as qkv
 * PE operands and gradient accumulation as for vitpe_fused_attention_*.  Supported:
 * vitpe_attention_core_supported() -- HD in {24, 32, 48, 64, 96, 128} (24 / 48 on 32- / 64-wide padded tiles) and
 * ceil(N/16) in {2, 4, 5, 10, 13, 17} (N = 17, 50, 65, 145..160, 197, 257..272), except where the backward's two LDS tiles
 * exceed 160 KB: bf16 HD=128 at 17 tiles, fp32 HD=96 at >= 13 tiles, fp32 HD=128 at >= 10 tiles;
 * rope-mixed needs H <= 16.  Anything else returns hipErrorNotSupported.                         */
int vitpe_attention_core_supported(int dtype, int N, int HD);
int vitpe_attention_core_fwd(int dtype, const void* qkv, void* out, int B, int N, int H, int HD, int mode,
                             const float* cos, const float* sin, const float* table, const float* coeff,
                             int grid, int degree, int coeff_per_head, vitpe_stream_t stream);
int vitpe_attention_core_bwd(int dtype, const void* qkv, const void* dout, void* dqkv, int B, int N, int H,
                             int HD, int mode, const float* cos, const float* sin, const float* table,
                             const float* coeff, int grid, int degree, int coeff_per_head, float* dtable,
                             float* dcoeff, float* dfreqs, vitpe_stream_t stream);
/* vitpe_attention_core_probs: the attention probabilities themselves -- models/vit.py:71-84, the tensor `attn` after
 * `.softmax(dim=-1)` and before `self.attn_drop` (what a forward hook on softmax sees; never dropped out), computed from the
 * same qkv buffer and PE operands as vitpe_attention_core_fwd, for attention maps, class-token saliency and attention
 * distance.  No gradient.
 *   probs  fp32 [B,H,N,N], element ((b H + h) N + i) N + j = probability of key j for query i   (cls_only == 0)
 *          fp32 [B,H,N]  : row i = 0 only, the class token's attention over all tokens, bitwise row 0 of the above
 *                          (cls_only != 0: one query-tile job per (image, head))
 * 4 B H N^2 bytes (52 MB at B 512 / H 6 / N 65).  Rows are written with 16-byte stores where N % 4 == 0 and probs is
 * 16-byte aligned, with 4-byte stores otherwise; nothing is written past query or key N - 1.  Arguments are checked and
 * refused exactly as by vitpe_attention_core_fwd (same supported shapes, B == 0 is a no-op); no sync, no allocation.   */
int vitpe_attention_core_probs(int dtype, const void* qkv, float* probs, int cls_only, int B, int N, int H, int HD,
                               int mode, const float* cos, const float* sin, const float* table, const float* coeff,
                               int grid, int degree, int coeff_per_head, vitpe_stream_t stream);
/* vitpe_attention_core_stats: statistics of those probabilities -- models/vit.py:71-84, the tensor `attn` after
 * `.softmax(dim=-1)` and before `self.attn_drop` -- reduced on the chip, the [N,N] maps never stored: 4 (4 + N) bytes per
 * (image, head) instead of 4 N^2.  With p the softmax of image b, head h, P = N - 1 and token t >= 1 at the raster position
 * (y, x) = ((t - 1) / grid, (t - 1) % grid) (any admitted N: the raster may be ragged; grid >= 1 in EVERY mode):
 *   stats fp32 [B,H,4]
 *     [VITPE_STAT_DISTANCE]     unit / P . sum_{i>=1} sum_{j>=1} p_ij sqrt((y_i - y_j)^2 + (x_i - x_j)^2)
 *                               (patch queries and patch keys only, not renormalised: the ViT paper's mean attention
 *                               distance; unit = patch size gives pixels)
 *     [VITPE_STAT_ENTROPY]      1 / N . sum_i (- sum_j p_ij ln p_ij)   (nats, 0 ln 0 = 0)
 *     [VITPE_STAT_CLS_MASS]     1 / P . sum_{i>=1} p_i0
 *     [VITPE_STAT_CLS_ENTROPY]  - sum_j p_0j ln p_0j
 *   weights fp32 [B,N], colsum fp32 [B,H,N]: both NULL, or both set: colsum[b,h,j] = sum_i weights[b,i] p_ij, the
 *     vector-times-map product of attention rollout.  The stats are bitwise the same either way.
 * Every sum runs in a fixed order without atomics: two calls on the same inputs give the same bits.  Nothing is read at
 * token rows >= N of qkv or weights, nothing is written outside stats and colsum.  No gradient.  Arguments are checked and
 * refused exactly as by vitpe_attention_core_fwd (same supported shapes, B == 0 is a no-op); no sync, no allocation.   */
#define VITPE_STAT_DISTANCE 0
#define VITPE_STAT_ENTROPY 1
#define VITPE_STAT_CLS_MASS 2
#define VITPE_STAT_CLS_ENTROPY 3
int vitpe_attention_core_stats(int dtype, const void* qkv, float* stats, const float* weights, float* colsum, float unit,
                               int B, int N, int H, int HD, int mode, const float* cos, const float* sin,
                               const float* table, const float* coeff, int grid, int degree, int coeff_per_head,
                               vitpe_stream_t stream);
/* vitpe_attention_core_relevance: one propagation step of the gradient-weighted attention relevance of Chefer, Gur & Wolf
 * ("Generic Attention-model Explainability", ICCV 2021), reduced on the chip.  With, for image b and head h,
 *   A  = models/vit.py:71-84, the tensor `attn` after `.softmax(dim=-1)` and before `self.attn_drop`,
 *   V  = the head's value rows of qkv (unrotated), dO = the head's columns of dout [B,N,H HD], the gradient of a scalar
 *        w.r.t. the merged-head output of the core (the tensor in front of proj),
 *   G  = dO V^T [N,N] = the gradient w.r.t. A with V held fixed (what a backward hook on `attn` sees; NOT the gradient
 *        w.r.t. the logits),
 *   colsum fp32 [B,H,N]:  colsum[b,h,j] = sum_i weights[b,i] f(G_ij A_ij),   f = max(0, .) if clamp != 0, else f(x) = x.
 * weights fp32 [B,N] is required.  Neither A nor G is stored.  qkv and dout have the compute type (fp32 accumulation of
 * G on the matrix core).  Every sum runs in a fixed order without atomics: two calls on the same inputs give the same
 * bits.  Nothing is read at token rows >= N, a padding query or key contributes exactly 0, nothing is written outside
 * colsum.  No gradient.  Arguments are checked as by vitpe_attention_core_fwd (B == 0 is a no-op).  Supported shapes:
 * those of vitpe_attention_core_fwd whose K~ and V tiles and reduction slabs fit the 160 KB LDS together (DESIGN.md,
 * "Attention relevance", lists the refused ones); hipErrorNotSupported otherwise, the outputs untouched.  No sync, no
 * allocation.   */
int vitpe_attention_core_relevance(int dtype, const void* qkv, const void* dout, const float* weights, float* colsum,
                                   int clamp, int B, int N, int H, int HD, int mode, const float* cos, const float* sin,
                                   const float* table, const float* coeff, int grid, int degree, int coeff_per_head,
                                   vitpe_stream_t stream);
/* vitpe_attention_core_bwd_tables: vitpe_attention_core_bwd under RoPE with the CALLER's tables (mode rope-axial: cos / sin
 * [P,HD/2]; rope-mixed: [H,P,HD/2]), which also returns their gradients -- the autograd of the reference's rotation
 * w.r.t. cos and sin as independent inputs (models/rope_utils.py:3-37, models/vit.py:51-68): per rotate-half pair
 * (x1, x2) of q and of k with upstream gradient (g1, g2) w.r.t. the rotated pair,
 *   dcos[.., p, j] += g1 x1 + g2 x2 ,  dsin[.., p, j] += g2 x1 - g1 x2 ,
 * summed over the batch, q and k (and the heads for a 2-D table) in a fixed order: bit-reproducible, no float atomics.
 * dcos / dsin (shape of cos / sin) are ACCUMULATED.  dqkv is bitwise what vitpe_attention_core_bwd writes; dfreqs and the
 * other PE-gradient arguments are ignored.  workspace: 4*B*H*(N-1)*(HD/2) floats (the per-(q/k, image, head) partial
 * slabs), clobbered.  Same supported shapes as vitpe_attention_core_bwd.                                                */
int vitpe_attention_core_bwd_tables(int dtype, const void* qkv, const void* dout, void* dqkv, int B, int N, int H,
                                    int HD, int mode, const float* cos, const float* sin, const float* table,
                                    const float* coeff, int grid, int degree, int coeff_per_head, float* dtable,
                                    float* dcoeff, float* dfreqs, float* dcos, float* dsin, float* workspace,
                                    vitpe_stream_t stream);
/* vitpe_attention_fused64_fwd: the reference's Attention.forward before self.proj (models/vit.py:47-88) at the ViT-B/16
 * geometry (BASELINE config 5: hd = 64, N = 197) as ONE kernel -- the head's slice of the qkv projection, the rotation /
 * bias, QK^T, softmax and .V per (image, head); q and k never leave the chip.  xn [B,N,D] T = LayerNorm1's output
 * (D = 64 H); wqkv_packed = vitpe_pack_weight_frags(attn.qkv.weight [3D,D], kchunk 64, phi 0); qkv_out (nullable)
 * [B,N,3D] T receives the raw projection, which is what vitpe_attention_core_bwd reads in training; out [B,N,D] T merged
 * heads.  bf16, hd = 64, 193 <= N <= 208, H <= 16 (vitpe_attention_fused64_supported); else hipErrorNotSupported: run
 * vitpe_linear + vitpe_attention_core_fwd.  PE arguments as vitpe_attention_core_fwd.                                   */
int vitpe_attention_fused64_supported(int dtype, int N, int H, int HD);
int vitpe_attention_fused64_fwd(int dtype, const void* xn, const void* wqkv_packed, void* qkv_out, void* out, int B,
                                int N, int H, int HD, int mode, const float* cos, const float* sin,
                                const float* table, const float* coeff, int grid, int degree, int coeff_per_head,
                                vitpe_stream_t stream);

/* ---- dropout ------------------------------------------------------------------------------
 * The reference's nn.Dropout sites (models/vit.py:36,38 attn_drop / proj_drop, applied at vit.py:85,92; timm Mlp's drop1 /
 * drop2 behind vit.py:118) and timm's DropPath (vit.py:115, used at vit.py:122,124).  torch draws those masks from its own
 * generator; here every keep decision is a pure function of (seed, offset, logical element e, p) on Philox4x32-10:
 *   key = (lo32 seed, hi32 seed) ; counter = (lo32(e >> 2), hi32(e >> 2), lo32 offset, hi32 offset) ; word = e & 3
 *   keep(e) = word >= floor(p * 2^32) ; kept values are multiplied by 1 / (1 - p)
 * so a backward regenerates the forward's mask and no mask is ever stored.  `rng` is a DEVICE pointer to the two 64-bit
 * words (seed, offset), read by the kernels when they run: a captured graph replays with the pair's current contents.
 * 0 <= p < 1 and rng != NULL, else hipErrorInvalidValue (nothing is launched).
 *
 * vitpe_philox4x32_10: host-only, the generator itself (key2[2], ctr4[4] -> out4[4]); same source as the device code.
 * vitpe_dropout_mask : uint8 keep mask of a site, for tests (the product path never materialises a mask).
 *   site 0 (elementwise) and 1 (per sample): e = index, mask [n];   site 2 (attention probabilities): mask [B,H,N,N],
 *   e = ((b H + h) N + i) NP + j with NP = N rounded up to a multiple of 4 (n ignored).
 * vitpe_dropout_fwd  : y = [resid +] x . m / (1-p), n elements of T, e = element index (resid nullable).
 * vitpe_dropout_bwd  : dx = dy . m / (1-p) with the same pair.
 * vitpe_drop_path_fwd: y = [resid +] x * m_b / (1-p), one decision per sample b < B (e = b) of `per` elements each: timm
 *   DropPath with scale_by_keep=True (third-party code, parity unpinned).  vitpe_drop_path_bwd: dx = dy * m_b / (1-p).  B <= 2^24
 *   (64 workgroups per sample in one grid dimension), else hipErrorInvalidValue.   */
int vitpe_philox4x32_10(const unsigned int* key2, const unsigned int* ctr4, unsigned int* out4);
int vitpe_dropout_mask(int site, const unsigned long long* rng, unsigned char* mask, long long n, int B, int H, int N,
                       float p, vitpe_stream_t stream);
int vitpe_dropout_fwd(int dtype, const void* x, const void* resid, void* y, long long n, const unsigned long long* rng,
                      float p, vitpe_stream_t stream);
int vitpe_dropout_bwd(int dtype, const void* dy, void* dx, long long n, const unsigned long long* rng, float p,
                      vitpe_stream_t stream);
int vitpe_drop_path_fwd(int dtype, const void* x, const void* resid, void* y, int B, long long per,
                        const unsigned long long* rng, float p, vitpe_stream_t stream);
int vitpe_drop_path_bwd(int dtype, const void* dy, void* dx, int B, long long per, const unsigned long long* rng, float p,
                        vitpe_stream_t stream);
/* vitpe_branch_drop_fwd: one residual branch's elementwise dropout, per-sample drop-path and residual add in one pass over
 *   [B, per]: y = [resid +] f_b * round_T(x . m_e / (1 - p_elem)), f_b = m_b / (1 - p_path); m_e on the flat element index
 *   (as vitpe_dropout_fwd), m_b on e = b (as vitpe_drop_path_fwd).  Bit for bit vitpe_dropout_fwd followed by
 *   vitpe_drop_path_fwd on the same pairs.  A NULL rng_elem / rng_path leaves that site out (its p is then ignored) and the
 *   result is that of the single remaining kernel; both NULL, per % 4 != 0 or B > 2^24: hipErrorInvalidValue, nothing is
 *   launched.  vitpe_branch_drop_bwd: dx = the same factors on dy (the forward without a residual).
 * vitpe_rng_advance: offset += inc (mod 2^64) in each of the n_sites (seed, offset) pairs of `table`; seeds untouched.  The
 *   launch that moves a captured step's masks on between replays.                                                       */
int vitpe_branch_drop_fwd(int dtype, const void* x, const void* resid, void* y, int B, long long per,
                          const unsigned long long* rng_elem, float p_elem, const unsigned long long* rng_path,
                          float p_path, vitpe_stream_t stream);
int vitpe_branch_drop_bwd(int dtype, const void* dy, void* dx, int B, long long per, const unsigned long long* rng_elem,
                          float p_elem, const unsigned long long* rng_path, float p_path, vitpe_stream_t stream);
int vitpe_rng_advance(unsigned long long* table, int n_sites, unsigned long long inc, vitpe_stream_t stream);
/* vitpe_attention_core_fwd_drop / _bwd_drop: vitpe_attention_core_fwd / _bwd with the reference's attention-probability
 * dropout (models/vit.py:84-88: softmax -> attn_drop -> @ v) applied to P in registers, site 2 above.  The backward
 * regenerates the mask in both of its passes: dV from P . m / (1-p), dP = (dO V^T) . m / (1-p).  p == 0 launches exactly
 * the kernels of vitpe_attention_core_fwd / _bwd (bitwise the same result).  Same supported shapes and PE modes; there is
 * no dropout variant of vitpe_attention_core_bwd_tables.                                                                */
int vitpe_attention_core_fwd_drop(int dtype, const void* qkv, void* out, int B, int N, int H, int HD, int mode,
                                  const float* cos, const float* sin, const float* table, const float* coeff,
                                  int grid, int degree, int coeff_per_head, const unsigned long long* rng, float p,
                                  vitpe_stream_t stream);
int vitpe_attention_core_bwd_drop(int dtype, const void* qkv, const void* dout, void* dqkv, int B, int N, int H,
                                  int HD, int mode, const float* cos, const float* sin, const float* table,
                                  const float* coeff, int grid, int degree, int coeff_per_head, float* dtable,
                                  float* dcoeff, float* dfreqs, const unsigned long long* rng, float p,
                                  vitpe_stream_t stream);

/* ---- GEMMs ------------------------------------------------------------------------------
 * vitpe_gemm_nt: C[M,N] = epi(A[M,K] W[N,K]^T).  nn.Linear forward (vit.py:35,37; timm Mlp
 * fc1/fc2), nn.Conv2d-as-GEMM patch embed (vit.py:164,248), and -- on a transposed weight
 * shadow -- the data gradients.  N % 8 == 0; K % 8 == 0 (bf16) / K % 4 == 0 (fp32).
 *   bias [N] fp32 or NULL; R residual [M,N] T (EPI_BIAS_RESID); U [M,N] T pre-activation
 *   (written by EPI_BIAS_GELU, read by EPI_GELU_BWD); EPI_PATCH: A = unfolded patches
 *   [B*P,K], C = tokens [B*(P+1),N], ape [P,N] fp32 or NULL, cls [N] fp32.                 */
int vitpe_gemm_nt(int dtype, int epi, const void* A, const void* W, void* C, const float* bias,
                  const void* R, void* U, const float* ape, const float* cls, int M, int N, int K,
                  int P, int Ntok, vitpe_stream_t stream);
/* vitpe_linear: same contract as vitpe_gemm_nt (minus EPI_PATCH) on the second-generation panel
 * kernel (144x192 tiles = full output rows for N = 192; used whenever N % 192 == 0, otherwise it
 * forwards to vitpe_gemm_nt).  mean_out/rstd_out (both or neither; N == 192 only) receive the
 * LayerNorm statistics of the OUTPUT rows (eps as in nn.LayerNorm), so the following LayerNorm
 * (vit.py:113,116) needs no pass of its own.                                                 */
int vitpe_linear(int dtype, int epi, const void* A, const void* W, void* C, const float* bias,
                 const void* R, void* U, float* mean_out, float* rstd_out, float eps, int M, int N,
                 int K, vitpe_stream_t stream);
/* LayerNorm fused into its neighbours (removes the stand-alone LayerNorm passes of vit.py:113,116):
 *  vitpe_linear_ln    : C = epi(LN(X) W^T), X raw [M,K] with row statistics mean/rstd (e.g. the stats
 *                       output of vitpe_linear); xn_out (nullable) receives LN(X) for the backward pass;
 *                       epi in {BIAS, BIAS_GELU}, N % 192 == 0.
 *  vitpe_linear_lnbwd : dx = dres + LN'(dY Wt^T) for the LayerNorm with input rows x [M,192]; dgamma/dbeta
 *                       accumulated.  (data gradient of qkv / fc1 + LayerNorm backward + residual add)      */
int vitpe_linear_ln(int dtype, int epi, const void* X, const float* gamma, const float* beta,
                    const float* mean, const float* rstd, void* xn_out, const void* W, void* C,
                    const float* bias, void* U, int M, int N, int K, vitpe_stream_t stream);
int vitpe_linear_lnbwd(int dtype, const void* dY, const void* Wt, void* dx, const void* x, const float* mean,
                       const float* rstd, const float* gamma, const void* dres, float* dgamma, float* dbeta,
                       int M, int K, vitpe_stream_t stream);
/* vitpe_linear_lnbwd2: the same function on the wave-per-tile mapping of vitpe_block_tail2_*, with the weight given as
 * Wt_packed = vitpe_pack_weight_frags(W^T [192,K], kchunk 64, phi 0), W = the Linear's weight [K,192] (attn.qkv.weight:
 * K = 576).  bf16, K % 192 == 0; otherwise hipErrorNotSupported.                                                        */
int vitpe_linear_lnbwd2(int dtype, const void* dY, const void* Wt_packed, void* dx, const void* x, const float* mean,
                        const float* rstd, const float* gamma, const void* dres, float* dgamma, float* dbeta, int M,
                        int K, vitpe_stream_t stream);
/* vitpe_block_tail2_fwd: the attention branch's tail and the MLP branch of a block in one kernel (vit.py:91,116-118,
 * 122-124 with timm Mlp):
 *   x_mid = x_in + attn_out Wp^T + bp ;  xn = LayerNorm2(x_mid) ;  u = xn W1^T + b1 ;  h = gelu(u) ;  out = x_mid + h W2^T + b2
 * x_mid [M,192] and its LayerNorm statistics mean2 / rstd2 [M] are outputs (backward needs them); xn_out (nullable) is kept
 * for fc1's weight gradient; mean_out / rstd_out (both or neither) receive the statistics of the OUTPUT rows (the next
 * block's LayerNorm1; eps2: norm2, eps_next: those).  Each wave carries one 16-token tile through the whole chain (hidden
 * activation in registers between fc1 and fc2) and reads the weights as MFMA fragments from fragment-major packed copies
 * made by vitpe_pack_weight_frags:
 *   Wp_packed = pack(attn.proj.weight [192,192], kchunk 192, phi 0)
 *   W1_packed = pack(mlp.fc1.weight  [HID,192], kchunk 192, phi 1)
 *   W2_packed = pack(mlp.fc2.weight  [192,HID], kchunk  32, phi 1)
 * What it keeps of the hidden layer for backward is h_out = gelu(u) (bf16) and gp_out = gelu'(u) [M,HID] as IEEE HALF
 * (2 bytes like bf16, 11 significant bits: vitpe_block_tail2_bwd multiplies every du element by it) -- NOT u: the
 * backward multiplies by the stored derivative; pass both or, for inference, neither.  bf16, D = 192, HID % 64 == 0, 128 <= HID <= 1536 (vitpe_block_tail2_supported); otherwise
 * hipErrorNotSupported -- run vitpe_linear / vitpe_linear_ln instead.
 * vitpe_pack_weight_frags: W fp32 [R,C] (R % 16 == 0, kchunk % 32 == 0, C % kchunk == 0) -> 1-KB fragments
 * (64 lanes x 8 elements) at fragment index ((kc * R/16 + nt) * kchunk/32 + ks); lane 16g + cc, element e holds
 * W[16nt + cc][kchunk*kc + 32ks + k], k = 8g + e (phi 0) or (e < 4 ? 4g + e : 16 + 4g + e - 4) (phi 1).          */
int vitpe_pack_weight_frags(int dtype, const float* W, void* packed, int R, int C, int kchunk, int phi,
                            vitpe_stream_t stream);
int vitpe_block_tail2_supported(int dtype, int D, int HID);
int vitpe_block_tail2_fwd(int dtype, const void* attn_out, const void* x_in, const void* Wp_packed, const float* bp,
                          const float* gamma, const float* beta, void* x_mid, float* mean2, float* rstd2,
                          void* xn_out, const void* W1_packed, const float* b1, const void* W2_packed,
                          const float* b2, void* gp_out, void* h_out, void* out, float* mean_out, float* rstd_out,
                          float eps2, float eps_next, int M, int D, int HID, vitpe_stream_t stream);
/* vitpe_block_tail2_bwd: backward of vitpe_block_tail2_fwd w.r.t. its inputs, the same pipeline on the transposes:
 *   du = (dy fc2.weight) * gp  [M,HID] (stored: fc1's weight gradient reads it),  dx_mid = dy + LayerNorm2'(du fc1.weight)
 *   da = dx_mid attn.proj.weight  [M,192] (input of the attention backward);  dgamma / dbeta of norm2 accumulated (fp32
 *   atomics, one per column and workgroup).  gp = gelu'(u) as saved by vitpe_block_tail2_fwd (IEEE half); x_mid / mean2 / rstd2 its
 *   LayerNorm2 input rows and statistics.  Weights as vitpe_pack_weight_frags copies of the TRANSPOSES:
 *   W2t_packed = pack(fc2.weight^T [HID,192], kchunk 192, phi 1), W1t_packed = pack(fc1.weight^T [192,HID], kchunk 32, phi 1),
 *   WpT_packed = pack(attn.proj.weight^T [192,192], kchunk 192, phi 1).  Support as vitpe_block_tail2_fwd.                 */
int vitpe_block_tail2_bwd(int dtype, const void* dy, const void* gp, const void* W2t_packed, const void* W1t_packed,
                          const void* x_mid, const float* mean2, const float* rstd2, const float* gamma, void* du,
                          void* dx_mid, float* dgamma, float* dbeta, const void* WpT_packed, void* da, int M, int D,
                          int HID, vitpe_stream_t stream);
/* vitpe_block_tail2_bwd_pre: the same preceded, in the same kernel, by the qkv data gradient + LayerNorm1 backward + residual
 * of the block ABOVE (vitpe_linear_lnbwd2's function):  dy_out = dres1 + LayerNorm1'(d_qkv Wqkv)  is written (the weight
 * gradients read it) and feeds the MLP backward from registers -- one launch, one HBM round trip of dy and one kernel
 * prologue less per layer.  WqT_packed = pack(attn.qkv.weight^T [192,K1], kchunk 64, phi 0) of the upper block; x1 / mean1 /
 * rstd1 / gamma1: its LayerNorm1 input rows, statistics and weight; dgamma1 / dbeta1 accumulated.  K1 % 64 == 0, K1 <= 640. */
int vitpe_block_tail2_bwd_pre(int dtype, const void* d_qkv, const void* WqT_packed, const void* x1, const float* mean1,
                              const float* rstd1, const float* gamma1, const void* dres1, float* dgamma1, float* dbeta1,
                              int K1, void* dy_out, const void* gp, const void* W2t_packed, const void* W1t_packed,
                              const void* x_mid, const float* mean2, const float* rstd2, const float* gamma, void* du,
                              void* dx_mid, float* dgamma, float* dbeta, const void* WpT_packed, void* da, int M, int D,
                              int HID, vitpe_stream_t stream);
/* vitpe_tail_cls_fwd / vitpe_tail_cls_bwd: vitpe_block_tail2_fwd (training form: x_mid, LayerNorm2 statistics, xn_out, gp_out,
 * h_out and out written) and vitpe_block_tail2_bwd on B rows that lie `row_step` rows apart in every [*, .] operand and
 * statistic: logical row r = row r * row_step of the buffers; no other row is read or written.  The model pools the class
 * token (vit.py:285: the head reads x[:, 0] alone), so the TOP block's tail (vit.py:116-118,122-124) and its backward
 * are needed on one row per image: row_step = tokens per image on the [batch x tokens, .] buffers.  Same packed weights,
 * arithmetic and rounding points as the full-row kernels; a 12-wave workgroup per 16-row tile, columns split over the
 * waves.  xn_out nullable; gp_out / h_out: both or neither (neither: evaluation).  Any B >= 0.                          */
int vitpe_tail_cls_fwd(int dtype, const void* attn_out, const void* x_in, const void* Wp_packed, const float* bp,
                       const float* gamma, const float* beta, void* x_mid, float* mean2, float* rstd2, void* xn_out,
                       const void* W1_packed, const float* b1, const void* W2_packed, const float* b2, void* gp_out,
                       void* h_out, void* out, float eps2, int B, int row_step, int D, int HID, vitpe_stream_t stream);
int vitpe_tail_cls_bwd(int dtype, const void* dy, const void* gp, const void* W2t_packed, const void* W1t_packed,
                       const void* x_mid, const float* mean2, const float* rstd2, const float* gamma, void* du,
                       void* dx_mid, float* dgamma, float* dbeta, const void* WpT_packed, void* da, int B, int row_step,
                       int D, int HID, vitpe_stream_t stream);
/* vitpe_gemm_tn: dW[N,K] += dY[M,N]^T X[M,K] ; dbias[N] += colsum(dY) (NULL to skip).  fp32
 * outputs, accumulated with atomics over `splits` token slices.                             */
int vitpe_gemm_tn(int dtype, const void* dY, const void* X, float* dW, float* dbias, int M, int N,
                  int K, int splits, vitpe_stream_t stream);

/* vitpe_wgrad_group: the same product for a LIST of independent problems (<= 28) in one launch --
 * e.g. every nn.Linear weight/bias gradient of the model (autograd's addmm backward in the
 * reference: vit.py:35,37 and timm Mlp fc1/fc2, once per block).  `problems` is a HOST array; the
 * descriptors travel as kernel arguments (no device table, graph-capture safe).  Work is cut into
 * (192x192 output block, 64-token stage) units spread evenly over the CUs, so each output block is
 * accumulated (fp32 atomics) by only a handful of workgroups.  N, K multiples of 8 (bf16) / 4 (fp32).  Lists whose every
 * problem has N % 192 == 0 and K % 384 == 0 (bf16, x_op 0: the ViT-B/16 shapes) run on 192 x 384 blocks instead.
 * In ANY list, problems with an eighth of the longest problem's stages or fewer are kept out of the placement of the blocks
 * over the chip (they would cap every other block's row ranges) and run as extra slots of two stages each behind it;
 * both figures are reasoned, not tuned (csrc/wgrad.hip).                                                              */
typedef struct {
  const void* dY; /* [M,N] T */
  const void* X;  /* [M,K] T */
  float* dW;      /* [N,K] fp32, accumulated into */
  float* dbias;   /* [N] fp32 or NULL, accumulated into */
  int M, N, K;
  int x_op;       /* VITPE_XOP_NONE, or VITPE_XOP_LAYERNORM: the operand is LayerNorm(X) with the row statistics and
                   * affine parameters below, recomputed while staging (the normalised tensor is never stored: it is
                   * a pure function of X, which the forward keeps anyway, vit.py:122,124) */
  const float* x_mean;  /* [M] */
  const float* x_rstd;  /* [M] */
  const float* x_gamma; /* [K] */
  const float* x_beta;  /* [K] */
} vitpe_wgrad_problem;
#define VITPE_XOP_NONE 0
#define VITPE_XOP_LAYERNORM 1
int vitpe_wgrad_group(int dtype, const vitpe_wgrad_problem* problems, int nprob, vitpe_stream_t stream);
/* ... with a row step per problem (`row_step` HOST array of nprob entries >= 1, or NULL = all 1): logical row m of problem
 * i's dY, X, x_mean and x_rstd is row m * row_step[i] of the buffers, M counts logical rows.  The top block's fc2 / fc1 /
 * proj weight gradients contract over the class-token rows only (every other row of their dY is zero: vit.py:285).
 * Problems much shorter than the longest of the list are kept out of its placement and run as short extra slots.      */
int vitpe_wgrad_group_rows(int dtype, const vitpe_wgrad_problem* problems, const int* row_step, int nprob,
                           vitpe_stream_t stream);

/* ---- LayerNorm (nn.LayerNorm(d), eps 1e-5: vit.py:113,116,210) ------------------------------ */
/* y == NULL: row statistics only (mean and rstd required) */
int vitpe_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y,
                        float* mean, float* rstd, int M, int D, float eps, vitpe_stream_t stream);
int vitpe_layernorm_bwd_blocks(int M); /* workspace = blocks * 2 * D floats */
/* dx = (dres ? dres : 0) + LN'(dy): also folds the residual-branch gradient of vit.py:122,124 */
int vitpe_layernorm_bwd(int dtype, const void* dy, const void* x, const float* mean,
                        const float* rstd, const float* gamma, const void* dres, void* dx,
                        float* dgamma, float* dbeta, float* workspace, int M, int D,
                        vitpe_stream_t stream);

/* ---- transforms.Resize (train.py:69-70,78-79) -------------------------------------------------
 * Resize(S) on the square uint8 images of datasets.MNIST (mode L) / datasets.CIFAR10 (mode RGB) is PIL's
 * img.resize((S, S), Image.BILINEAR): per channel plane a horizontal pass to a uint8 intermediate [S0][S], then a
 * vertical pass, each integer arithmetic on fixed-point coefficients -- reproduced bit for bit.
 * vitpe_resize_coeffs: PURE HOST.  One pass from length `in` to length `out`: bounds [out][2] = (first source index,
 * tap count), kk [out][ksize] = round(weight * 2^22) (zero past the tap count); returns ksize = 2 ceil(max(in/out, 1))
 * + 1, or a negative value (and writes nothing) when ksize_cap < ksize or an argument is invalid.                    */
int vitpe_resize_coeffs(int in, int out, int* bounds, int* kk, int ksize_cap);
/* src [planes][S0][S0] -> dst [planes][S][S] uint8, planes = images x channels; the tables are DEVICE copies of
 * vitpe_resize_coeffs(S0, S) for the horizontal (_h) and vertical (_v) pass, ksize its return value.  S == S0 is a
 * copy (tables may be NULL).  Supported: S0 in 8..64, S in 4..512; anything else is hipErrorNotSupported.          */
int vitpe_resize_u8_supported(int S0, int S);
int vitpe_resize_u8(const unsigned char* src, unsigned char* dst, long long planes, int S0, int S,
                    const int* bounds_h, const int* kk_h, const int* bounds_v, const int* kk_v, int ksize,
                    vitpe_stream_t stream);

/* ---- patch embed (vit.py:164,245-258) ------------------------------------------------------- */
/* img [B,C,S,S] fp32 -> patches [B*P, C*p*p] T, column = c*p*p + ky*p + kx                    */
int vitpe_unfold(int dtype, const float* img, void* patches, int B, int C, int S, int p,
                 vitpe_stream_t stream);
/* The same from a uint8 dataset resident in HBM -- replaces the DataLoader gather + ToTensor + Normalize
 * of train.py:69-92 in front of the patch embed: record index[b] (NULL: record b) of data [Ndata,C,S,S]
 * uint8 is turned into ((x/255) - mean[c]) / std[c] (fp32, the reference's operation order) and written as
 * the patch matrix; img_out (nullable) receives the normalised fp32 image [B,C,S,S].                   */
int vitpe_unfold_u8(int dtype, const unsigned char* data, const long long* index, const float* mean,
                    const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                    vitpe_stream_t stream);
/* Fused patch embedding for the small-K geometries (K = C p^2 <= 64, (S/p)^2 <= 64 patches, D <= 256, D % 16 == 0:
 * vitpe_patch_embed_supported): unfold (from fp32 images `img`, XOR from the resident uint8 dataset `data` + `index` with
 * ToTensor + Normalize as vitpe_unfold_u8) + Conv2d-as-GEMM + bias + absolute PE rows `ape` [P,D] (nullable) + class
 * token in row 0 -> tokens [B,P+1,D]; `patches` [B*P,K] (nullable) receives the patch matrix for the weight gradient;
 * mean / rstd (both or neither) the LayerNorm statistics of every token row (vit.py:113).  One launch instead of
 * vitpe_unfold + vitpe_gemm_nt(EPI_PATCH) + vitpe_layernorm_fwd.                                                   */
int vitpe_patch_embed_supported(int dtype, int C, int S, int p, int D);
int vitpe_patch_embed(int dtype, const float* img, const unsigned char* data, const long long* index,
                      const float* nmean, const float* nstd, const void* W, const float* bias, const float* cls,
                      const float* ape, void* tokens, void* patches, float* mean, float* rstd, int B, int C, int S,
                      int p, int D, float eps, vitpe_stream_t stream);
/* Augmentation stream: transforms.RandomCrop(S, padding=pad) + transforms.RandomHorizontalFlip() between the Resize and the
 * ToTensor of the reference's input pipeline (train.py:69-92, which has neither), applied inside the two gather kernels
 * above.  `rng` is a DEVICE pointer to the site's two 64-bit words (seed, offset), as for a dropout site.  Batch slot b (the
 * position in the batch, not the record) makes ONE Philox4x32-10 call,
 *   key = (lo32 seed, hi32 seed) ; counter = (lo32 b, hi32 b, lo32 offset, hi32 offset) -> words w0..w3
 *   oy = mulhi32(w0, 2 pad + 1) ; ox = mulhi32(w1, 2 pad + 1) ; flip = hflip && (w2 >> 31)
 * and its output pixel (c, y, x) is the source byte u = data[index[b], c, y + oy - pad, (flip ? S-1-x : x) + ox - pad], or
 * u = 0 outside the image (zero padding of the uint8 image), then ((float)u / 255 - mean[c]) / std[c] as above.
 * 0 <= pad <= S, else hipErrorInvalidValue.  rng == NULL, or pad == 0 with hflip == 0: the unaugmented result, bit for bit.
 * vitpe_unfold_u8_aug  : vitpe_unfold_u8 + (rng, pad, hflip); img_out receives the augmented image.
 * vitpe_patch_embed_aug: vitpe_patch_embed + (rng, pad, hflip), on the `data` path only: img != NULL with rng != NULL is
 *   hipErrorInvalidValue; at p == 4 with rng != NULL `data` must be 4-byte aligned (the rows are read as aligned dwords).
 * vitpe_augment_params : the draws themselves, out [B,3] int = (oy, ox, flip) of slots 0..B-1, for tests.
 * vitpe_rng_advance moves the pair on between steps.                                                                  */
int vitpe_unfold_u8_aug(int dtype, const unsigned char* data, const long long* index, const float* mean,
                        const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                        const unsigned long long* rng, int pad, int hflip, vitpe_stream_t stream);
int vitpe_patch_embed_aug(int dtype, const float* img, const unsigned char* data, const long long* index,
                          const float* nmean, const float* nstd, const void* W, const float* bias, const float* cls,
                          const float* ape, void* tokens, void* patches, float* mean, float* rstd, int B, int C, int S,
                          int p, int D, float eps, const unsigned long long* rng, int pad, int hflip,
                          vitpe_stream_t stream);
int vitpe_augment_params(const unsigned long long* rng, int* out, int B, int pad, int hflip, vitpe_stream_t stream);
/* Erasing stream: torchvision.transforms.RandomErasing(p, scale, ratio, value) after Normalize, on the OUTPUT pixel
 * coordinates (after crop and flip), with timm's three fill modes, on the same pair.  Every draw is a Philox4x32-10 call with
 * key = (lo32 seed, hi32 seed) and counter = (c0, c1, lo32 offset, hi32 offset); (c0, c1) = (b, 0) is the crop/flip call.
 *   u(w)   = ((w >> 9) + 0.5f) 2^-23                        (exact in fp32, strictly inside (0, 1))
 *   switch : slot b is erased iff (uint64)w3 < erase_thr, w3 the fourth word of the call (b, 0);
 *            erase_thr = floor((double)(float)prob 2^32) computed by the caller: 0 off, 2^32 always
 *   rectangle: up to 10 attempts a = 0..9, call (b, a + 1), fp32 without fused multiply-add:
 *            area = (float)(S S) (smin + u(w0) (smax - smin)) ; r = expf(lmin + u(w1) (lmax - lmin))
 *            h = (int)rintf(sqrtf(area r)) ; w = (int)rintf(sqrtf(area / r)) ; accepted iff h < S && w < S, then
 *            i = mulhi32(w2, S - h + 1) ; j = mulhi32(w3, S - w + 1).  No accepted attempt: nothing is erased.
 *            lmin = (float)log(rmin), lmax = (float)log(rmax), computed by the caller.
 *   fill of output pixel (c, y, x), i <= y < i + h, j <= x < j + w (every other pixel is the crop/flip result, bit for bit):
 *            erase_mode 0 const: 0.0f ;  1 rand: one normal per channel for the rectangle, call (b, 11) ;
 *            2 pixel: one normal per pixel and channel, call (lo32 e, 0x80000000 | hi32 e), e = (b S + y) S + x ;
 *            normal of channel c, k = c >> 1:  sqrtf(-2 logf(u(w[2k]))) * ((c & 1) ? sinf : cosf)(6.2831853f u(w[2k+1]))
 * erase_thr <= 2^32, erase_mode 0..2 (1 and 2: C <= 4), 0 < smin <= smax <= 1, finite lmin <= lmax, else hipErrorInvalidValue
 * (nothing is launched).  The erased value goes to `patches` and img_out alike.
 * vitpe_unfold_u8_erase: vitpe_unfold_u8_aug + the erasing arguments.  erase_thr == 0: the _aug entry, bit for bit;
 *   rng == NULL: the plain entry (the erasing arguments are then not looked at).  pad == 0 with hflip == 0 erases the
 *   uncropped image.  The fused vitpe_patch_embed has no erasing entry: feed it the img_out of this one.
 * vitpe_erase_params     : the draws themselves, out [B,5] int = (on, i, j, h, w) of slots 0..B-1 (DEVICE pointers), for tests.
 * vitpe_erase_params_host: host only, the same function compiled for the CPU; rng and out are HOST pointers.            */
int vitpe_unfold_u8_erase(int dtype, const unsigned char* data, const long long* index, const float* mean,
                          const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                          const unsigned long long* rng, int pad, int hflip, unsigned long long erase_thr, int erase_mode,
                          float smin, float smax, float lmin, float lmax, vitpe_stream_t stream);
int vitpe_erase_params(const unsigned long long* rng, int* out, int B, int S, unsigned long long thr, float smin, float smax,
                       float lmin, float lmax, vitpe_stream_t stream);
int vitpe_erase_params_host(const unsigned long long* rng, int* out, int B, int S, unsigned long long thr, float smin,
                            float smax, float lmin, float lmax);
/* dcls[d] += sum_b dtok[b,0,d]; dape[p,d] += sum_b dtok[b,1+p,d] (NULL to skip);
 * dpatch [B*P,D] T = patch rows of dtok (input of the patch-embed weight gradient)            */
int vitpe_embed_bwd(int dtype, const void* dtok, float* dcls, float* dape, void* dpatch, int B,
                    int Ntok, int D, vitpe_stream_t stream);
/* Patch-embed data gradient: the Conv2d of vit.py:164, 248-250 differentiated with respect to the images,
 *   dimg[b, c, gy p + ky, gx p + kx] = sum_d dtok[b, 1 + gy G + gx, d] W[d, c p^2 + ky p + kx],   G = S / p.
 * dtok [B, P+1, D] T is the token gradient itself (the class row is skipped, vitpe_embed_bwd's dpatch is not needed), W the
 * flattened Conv2d weight [D, C p p] T, dimg [B,C,S,S] fp32: fully overwritten, never accumulated into, no zero-init
 * needed.  fp32 accumulation in both types; no atomics, the summation order is fixed.  dtok 16-byte aligned.
 * vitpe_patch_embed_dgrad_supported: 0 refused (S % p != 0, D % 8 != 0, D < 8, bad dtype / C / p: hipErrorNotSupported,
 * nothing is written), 1 the MFMA branch (S / p <= 64 and p <= 64), 2 the plain-FMA branch.  The admitted set holds every
 * geometry vitpe_unfold + vitpe_gemm_nt(EPI_PATCH) admit and, beyond them, every K = C p p (49, 12 in bf16, ...).
 * B == 0 returns 0.                                                                                                  */
int vitpe_patch_embed_dgrad_supported(int dtype, int C, int S, int p, int D);
int vitpe_patch_embed_dgrad(int dtype, const void* dtok, const void* W, float* dimg, int B, int C, int S, int p, int D,
                            vitpe_stream_t stream);

/* ---- positional-encoding tables (models/positional_encoding.py) --------------------------- */
int vitpe_relative_position_index(long long* out, int L, vitpe_stream_t stream);   /* :67-75, int64 [L,L], bit-exact */
int vitpe_l1_distance_matrix(long long* out, int G, vitpe_stream_t stream);        /* :136-142, int64 [G*G,G*G], bit-exact */
int vitpe_rope_axial_tables(const float* inv_freq, float* cosv, float* sinv, int G, int half,
                            vitpe_stream_t stream);                                /* :228-245 */
int vitpe_rope_mixed_tables(const float* freqs, float* cosv, float* sinv, int H, int G, int half,
                            vitpe_stream_t stream);                                /* :325-351 incl. the view-scramble */
int vitpe_relative_bias(const float* table, float* out, int H, int L, vitpe_stream_t stream); /* :82-95 */
int vitpe_polynomial_bias(const float* coeff, float* out, int H, int G, int degree, int per_head,
                          vitpe_stream_t stream);                                  /* :127-171 */
/* transposes of the three builders above (autograd of the stand-alone modules' get_bias() / get_freqs_cis(), which
 * the reference returns as differentiable tensors): dtable [H,2L-1], dcoeff [deg+1] or [H,deg+1], dfreqs [2,H,half]
 * are OVERWRITTEN with the gradient w.r.t. the parameter given d bias [H,L,L] resp. d cos / d sin [H,P,half].       */
int vitpe_relative_bias_bwd(const float* dbias, float* dtable, int H, int L, vitpe_stream_t stream);
int vitpe_polynomial_bias_bwd(const float* dbias, float* dcoeff, int H, int G, int degree, int per_head,
                              vitpe_stream_t stream);
int vitpe_rope_mixed_tables_bwd(const float* freqs, const float* dcos, const float* dsin, float* dfreqs, int H,
                                int G, int half, vitpe_stream_t stream);
/* models/rope_utils.py:3-37 on x [B,H,P,HD] fp32 (called once for q, once for k)              */
int vitpe_apply_rotary(const float* x, float* y, const float* cosv, const float* sinv, int B, int H,
                       int P, int HD, int per_head, vitpe_stream_t stream);
/* backward of vitpe_apply_rotary (autograd of models/rope_utils.py:3-37, cos and sin independent inputs): dy, x, dx
 * [B,H,P,HD] fp32, dx = the transposed rotation of dy (dx1 = g1 c + g2 s, dx2 = g2 c - g1 s; NULL to skip);
 * dcos / dsin [P,HD/2] or [H,P,HD/2] (per_head) ACCUMULATE g1 x1 + g2 x2 / g2 x1 - g1 x2 summed over B (and H for a
 * shared table) in a fixed order (NULL to skip; q and k can share one output).  workspace (needed with dcos / dsin):
 * 2*S*T floats, T = (per_head ? H : 1)*P*(HD/2), S = min(R, 64), R = per_head ? B : B*H.                              */
int vitpe_apply_rotary_bwd(const float* dy, const float* x, const float* cosv, const float* sinv, float* dx,
                           float* dcos, float* dsin, float* workspace, int B, int H, int P, int HD, int per_head,
                           vitpe_stream_t stream);

/* ---- classifier head + loss (vit.py:284-285, train.py:113,119-121,194) -------------------- */
int vitpe_head_fwd(int dtype, const void* x, const float* gamma, const float* beta, const float* Wh,
                   const float* bh, float* logits, float* ws_xhat, float* ws_yn, float* ws_rstd,
                   int B, int Ntok, int D, int Cn, float eps, vitpe_stream_t stream);
/* out2[0] = mean CE, out2[1] = #correct; dlogits (NULL to skip) = (softmax-onehot)*grad_scale */
int vitpe_cross_entropy(const float* logits, const long long* labels, float* dlogits, float* out2,
                        int B, int Cn, float grad_scale, vitpe_stream_t stream);
/* The same with its scalars read ON THE DEVICE (a captured step follows a ragged last batch; reference train.py:89-90
 * has no drop_last): ctl = {grad_scale, loss_scale, n_valid}.  Rows b >= n_valid are padding: dlogits = 0 (so every
 * gradient downstream is untouched by them), left out of loss and accuracy.  out2[0] = loss_scale * sum of the valid
 * rows' losses, out2[1] = #correct; metric_acc (nullable) += out2.                                                  */
int vitpe_cross_entropy_ctl(const float* logits, const long long* labels, float* dlogits, float* out2,
                            float* metric_acc, const float* ctl, int B, int Cn, vitpe_stream_t stream);
int vitpe_head_bwd(int dtype, const float* dlogits, const float* Wh, const float* gamma,
                   const float* ws_xhat, const float* ws_yn, const float* ws_rstd, float* ws_dyn,
                   void* dx, float* dWh, float* dbh, float* dgamma, float* dbeta, int B, int Ntok,
                   int D, int Cn, vitpe_stream_t stream);
/* The train step's head: vitpe_head_fwd + vitpe_cross_entropy_ctl + vitpe_head_bwd in one launch pair (classes <= 64,
 * D <= 768, else hipErrorNotSupported).  ctl as vitpe_cross_entropy_ctl.  dx: ONLY the class rows are written -- the
 * caller keeps rows 1.. of every image zero (they never change).  per_image: [B,2] work buffer ((loss, correct) per
 * image, summed in fixed order: no atomics on the totals).  Parameter gradients are accumulated.  hp_tick (nullable): the
 * optimizer's hp block -- the launch also advances hp[STEP], hp[BC1] and hp[BC2], which lets the following
 * vitpe_adamw_step skip its own one-thread launch (zero_grad bit 1).                                              */
int vitpe_head_step(int dtype, const void* x, const float* gamma, const float* beta, const float* Wh,
                    const float* bh, const long long* labels, float* logits, float* dlogits, float* ws_xhat,
                    float* ws_yn, float* ws_dyn, void* dx, float* out2, float* metric_acc, float* per_image,
                    const float* ctl, float* dWh, float* dbh, float* dgamma, float* dbeta, int B, int Ntok,
                    int D, int Cn, float eps, float* hp_tick, vitpe_stream_t stream);

/* ---- optimizer + weight shadows (train.py:116,195) ------------------------------------------
 * hp (device, VITPE_HP_COUNT floats) and sched (device, VITPE_SCHED_COUNT floats) are the two blocks the calls below share;
 * both live on the device so that the calls can be replayed from a hipGraph.  In the comments below hp[X] is short for
 * hp[VITPE_HP_X] and sched[X] for sched[VITPE_SCHED_X].                                                              */
enum vitpe_hp_slot {
  VITPE_HP_LR = 0,            /* learning rate (host; vitpe_lr_schedule while a schedule is on) */
  VITPE_HP_BETA1 = 1,         /* host */
  VITPE_HP_BETA2 = 2,         /* host */
  VITPE_HP_EPS = 3,           /* host */
  VITPE_HP_WEIGHT_DECAY = 4,  /* host */
  VITPE_HP_STEP = 5,          /* step counter (the tick: vitpe_adamw_step*, or vitpe_head_step's hp_tick) */
  VITPE_HP_BC1 = 6,           /* bias correction 1 - beta1^step (the tick) */
  VITPE_HP_BC2 = 7,           /* bias correction 1 - beta2^step (the tick) */
  VITPE_HP_GRAD_SCALE = 8,    /* host: 1 / world */
  VITPE_HP_CLIP_SCALE = 9,    /* effective gradient scale, GRAD_SCALE * CLIP_COEF (vitpe_grad_clip) */
  VITPE_HP_TOTAL_NORM = 10,   /* vitpe_grad_clip */
  VITPE_HP_CLIP_COEF = 11,    /* vitpe_grad_clip */
  VITPE_HP_MAX_NORM = 12,     /* host */
  VITPE_HP_EMA_DECAY = 13,    /* host */
  VITPE_HP_EMA_ORIGIN = 14,   /* host side: STEP when the EMA was switched on */
  VITPE_HP_EMA_DT = 15,       /* the decay d_t vitpe_ema_update used last */
  VITPE_HP_COUNT = 16
};
enum vitpe_sched_slot {
  VITPE_SCHED_BASE_LR = 0,
  VITPE_SCHED_MIN_LR = 1,
  VITPE_SCHED_WARMUP = 2,        /* W warm-up steps */
  VITPE_SCHED_TOTAL = 3,         /* T total steps */
  VITPE_SCHED_START_FACTOR = 4,  /* s0 */
  VITPE_SCHED_ORIGIN = 5,        /* hp[STEP] when the schedule was switched on, less the steps already done */
  VITPE_SCHED_LAST_LR = 6,       /* the last lr written (vitpe_lr_schedule); everything else is the host's */
  VITPE_SCHED_SPARE = 7,
  VITPE_SCHED_COUNT = 8
};
/* Fused AdamW on the flat buffers.  zero_grad: bit 0 = clear g after the update, bit 1 = the step counter / bias
 * corrections were already advanced (vitpe_head_step hp_tick), bit 2 = the gradient is scaled by hp[CLIP_SCALE]
 * instead of hp[GRAD_SCALE] (after vitpe_grad_clip).  Values 0..3 never read hp[CLIP_SCALE].                            */
int vitpe_adamw_step(float* p, float* g, float* m, float* v, void* shadow_bf16, float* hp,
                     long long n, int zero_grad, vitpe_stream_t stream);
/* AdamW with parameter groups (replaces the one group of train.py:195-196): vitpe_adamw_step's arithmetic, hp slots and
 * zero_grad bits, with a (learning-rate, weight-decay) SCALE pair per group.  The 8-element granule i / 8 of the flat
 * buffers belongs to group k = gid[i / 8] (one byte per granule; n_gid >= ceil(n / 8) bytes; ids >= n_groups are read as
 * n_groups - 1), and group k uses lr_k = hp[LR] * gtab[2k], wd_k = hp[WEIGHT_DECAY] * gtab[2k+1] (gtab: n_groups fp32 pairs): decay
 * factor 1 - lr_k * wd_k, step size lr_k / bc1.  With every scale 1.0 the result is vitpe_adamw_step's bit for bit (p, m,
 * v, g, shadow).  One lane per granule (16-byte loads and stores, 8-byte shadow stores), the n % 8 last elements one lane
 * each; grid-stride over vitpe_adamw_groups_blocks(n) workgroups of 256: the grid depends on n alone.  n == 0 launches only
 * the tick (unless bit 1 is set).  hipErrorInvalidValue, and nothing launched, for NULL hp; NULL p / g / m / v / gid / gtab
 * with n > 0; n < 0; n_groups outside 1..256; n_gid < ceil(n / 8); p, g, m or v not 16-byte aligned; a shadow not 8-byte
 * aligned.                                                                                                           */
int vitpe_adamw_step_groups(float* p, float* g, float* m, float* v, void* shadow_bf16, float* hp, long long n,
                            int zero_grad, const unsigned char* gid, long long n_gid, const float* gtab, int n_groups,
                            vitpe_stream_t stream);
/* workgroups vitpe_adamw_step_groups launches for n elements: min(2048, max(1, ceil(ceil(n / 8) / 256))); 0 for n <= 0 */
int vitpe_adamw_groups_blocks(long long n);
/* Linear warm-up + cosine learning rate, stepped once per iteration on the device (replaces the per-epoch
 * CosineAnnealingLR of train.py:205; equals SequentialLR(LinearLR(start_factor=s0, total_iters=W),
 * CosineAnnealingLR(T_max=T-W, eta_min=min_lr), milestones=[W]) for k <= T).  sched: enum vitpe_sched_slot (base, min_lr, W,
 * T, s0 below).  One lane, fp64:
 *   k = max(0, hp[STEP] - sched[ORIGIN] - (ticked ? 1 : 0))   (ticked: vitpe_head_step already advanced the counter)
 *   k < W : lr = base * (s0 + (1 - s0) * k / W)
 *   k >= T: lr = min_lr
 *   else  : c = cos(pi / 2 * (k - W) / (T - W)),  lr = min_lr + (base - min_lr) * c * c
 * hp[LR] = sched[LAST_LR] = (float)lr; nothing else is written.  Call it before vitpe_grad_clip / the AdamW call of the step.
 * T > W >= 0, 0 < s0 <= 1, 0 <= min_lr <= base are the writer's duty.  hipErrorInvalidValue for NULL pointers.       */
int vitpe_lr_schedule(float* hp, const float* sched, int ticked, vitpe_stream_t stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0, error_if_nonfinite=False) on the flat gradient g [n]
 * (4-byte aligned; any offset inside a 16-byte line), as two launches without atomics and without a host read:
 *   hp[TOTAL_NORM] = hp[GRAD_SCALE] * sqrt(sum g[i]^2)      (the norm of the gradient AdamW uses, g * grad_scale)
 *   hp[CLIP_COEF]  = min(1, hp[MAX_NORM] / (total_norm + 1e-6))
 *   hp[CLIP_SCALE] = hp[GRAD_SCALE] * clip_coef      (fp32 product: clip_coef == 1 gives GRAD_SCALE's bits)
 * g itself is not changed: vitpe_adamw_step with zero_grad bit 2 scales by hp[CLIP_SCALE].  Non-finite values follow the formula
 * (a NaN norm gives a NaN coefficient, as torch's clamp does).  partial: work buffer of n_partial >=
 * vitpe_grad_clip_blocks(n) floats, one per workgroup of the first launch, summed in fp64 in a fixed order by the
 * second.  The grid depends on n alone, so the result is the same bit for bit from run to run and from device to device.
 * n == 0 (g and partial may be NULL): norm 0, coef 1.  hipErrorInvalidValue for NULL hp, NULL g / partial with n > 0,
 * n < 0, a g that is not 4-byte aligned, or n_partial too small; nothing is launched then.                          */
int vitpe_grad_clip(const float* g, long long n, float* hp, float* partial, int n_partial, vitpe_stream_t stream);
/* workgroups (= floats of `partial`) vitpe_grad_clip uses for n elements: min(1024, ceil(n / 4096)); 0 for n <= 0 */
int vitpe_grad_clip_blocks(long long n);
/* Exponential moving average of the flat fp32 parameters p [n] into e [n], one launch, elementwise:
 *   e[i] = fmaf(w, p[i] - e[i], e[i]),  w = 1.0f - d_t                         (all fp32; p is only read)
 *   d_t  = hp[EMA_DECAY]                                                       (warmup == 0)
 *   d_t  = fminf(hp[EMA_DECAY], (1.0f + t) / (10.0f + t)),  t = hp[STEP] - hp[EMA_ORIGIN]   (warmup != 0: TF's num_updates rule)
 * hp[STEP] is AdamW's step counter, already advanced for this step (call it after vitpe_adamw_step); hp[EMA_ORIGIN] its value
 * when the average was switched on.  Those three are only read; one lane stores d_t to hp[EMA_DT].  The division is
 * correctly rounded.  p[i] == e[i] leaves e[i]'s bits (fmaf(w, 0, e) == e): a converged average is a fixed point.
 * p and e 16-byte aligned (16-byte loads and stores per lane, the n % 4 last elements one lane each; the grid is
 * vitpe_ema_blocks(n) workgroups of 256, grid-stride).  n == 0 launches nothing (hp[EMA_DT] keeps its value).
 * hipErrorInvalidValue for NULL hp, NULL p / e with n > 0, n < 0, or a p / e that is not 16-byte aligned; nothing is
 * launched then.                                                                                                     */
int vitpe_ema_update(const float* p, float* e, float* hp, long long n, int warmup, vitpe_stream_t stream);
/* p[i] <-> e[i] in place; shadow_bf16 (nullable) [i] = bf16 of the NEW p[i], the rounding of vitpe_cast bit for bit.  Two
 * calls restore every bit.  Alignment, n == 0 and refusals as vitpe_ema_update (shadow_bf16 16-byte aligned too).     */
int vitpe_ema_swap(float* p, float* e, void* shadow_bf16, long long n, vitpe_stream_t stream);
/* workgroups the two calls above launch for n elements: min(2048, max(1, ceil((n / 4) / 256))); 0 for n <= 0 */
int vitpe_ema_blocks(long long n);
int vitpe_cast(int dtype, const float* src, void* dst, long long n, vitpe_stream_t stream);
int vitpe_transpose_cast(int dtype, const float* src, void* dst, int R, int C, vitpe_stream_t stream);
/* every weight shadow of the model in one launch.  desc: device array of ndesc records
 * {int64 src_off (elements into flat), int64 dst_off, int64 dst_off2 (elements into dst_base), int32 R, C, tile0,
 *  kind, HD, kind2, HD2, pad}: the fp32 matrix [R,C] at src_off is written as shadow `kind` at dst_off and, when
 *  kind2 >= 0, as shadow `kind2` at dst_off2 (one load of the source tile for both).  kind: 0 = transpose,
 *  1 = vitpe_pack_qkv_weights layout (HD = head dim), 2 / 3 = vitpe_pack_weight_frags of the matrix (natural / phi k
 *  order, HD = k chunk), 4 / 5 = vitpe_pack_weight_frags of its TRANSPOSE, 6 = vitpe_pack_qkv_weights_wide (HD = 32).  tile0 = running sum of
 *  ceil(R/32)*ceil(C/32); total_tiles = that sum over all records; tile_map (nullable): uint16[total_tiles], the record
 *  index of every 32x32 tile (without it each workgroup scans the records).                                        */
int vitpe_refresh_shadows(int dtype, const float* flat, void* dst_base, const void* desc, int ndesc,
                          int total_tiles, const unsigned short* tile_map, vitpe_stream_t stream);

/* Self-tests and residency / phase-census instrumentation are NOT part of this boundary: include/vitpe_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* VITPE_H */
