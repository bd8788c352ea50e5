/*
 * basd_hip.h -- C-ABI of the MI355X (gfx950) BASD loss-path kernels.
 *
 * Every entry takes raw DEVICE pointers, explicit shapes and a hipStream_t
 * (passed as void*), never allocates / frees / synchronises the device, and
 * returns an int status (0 = ok).  basd_last_error() returns a thread-local
 * message for the last non-zero status.  No C++ exception crosses this
 * boundary, no torch type appears in any signature.  The library reads no
 * environment variables: which kernel runs depends on the arguments alone.
 *
 * The reference project is pure Python and has no FFI layer; the entries
 * below replace the library calls its loss path makes (citations are
 * file:line in the reference repository):
 *
 *   basd_token_gram        src/losses/layer_selector.py:72,135 (projection GEMM)
 *                          + :13 (X^T X) + :35 (column mean)
 *   basd_pchol_f64 +
 *   basd_jacobi_svd        torch.linalg.eigvalsh  layer_selector.py:16
 *                          torch.linalg.svd       layer_selector.py:36,92
 *                          torch.linalg.svdvals   layer_selector.py:99
 *                          matrix_norm(ord="nuc") src/losses/relational.py:48
 *   basd_mp_rank           layer_selector.py:17-20 (.median/.sum, on device, no .item())
 *   basd_sym_tridiag_f64, basd_sym_tridiag_f64_workspace_bytes, basd_tridiag_mp_rank
 *                          layer_selector.py:8-20 for 1024 < min(M, D) <= 2048 (ViT-H .. 2048-channel teachers at
 *                          start-up): torch.linalg.eigvalsh + .median / .sum replaced by eigenvalue COUNTS of the
 *                          fp64 Gram (Householder tridiagonal form + Sturm bisection), no spectrum, no fp32
 *   basd_angle_weights     layer_selector.py:100-108 (acos / spectral weighting / softmax over teacher layers)
 *   basd_angle_weights_bwd autograd of layer_selector.py:86-108 (student frame, angles, softmax, temperatures)
 *   basd_selector_frames   layer_selector.py:69-74, 133-138 (teacher: MP rank, PCA frame cut at the rank) and
 *                          :84-92 (student PCA frame), from the Gram statistics of basd_token_gram
 *   basd_selector_weights  layer_selector.py:93-108 (principal angles between the frames -> mixing weights), plus
 *                          the seeds basd_angle_weights_bwd takes
 *   basd_mix_tokens        layer_selector.py:110-112 (+ torch.stack :128-129 eliminated)
 *   basd_procrustes_prep   src/losses/relational.py:29-46, src/losses/combined.py:9-14
 *   basd_mix_grad_dots     autograd of layer_selector.py:111-112 w.r.t. the mixing weights
 *   basd_gemm_bf16         timm nn.Linear (+ nn.GELU) forward of the ViT blocks, teacher.py:212 / trainer.py:33
 *   basd_gemm_bf16_act     the same with the MLP activation of a timm CLIP / SigLIP teacher (QuickGELU, tanh-GELU)
 *   basd_vit_embed_bf16    timm VisionTransformer._pos_embed + norm_pre of a frozen teacher (teacher.py:113-148 loads any)
 *   basd_gemm_bf16_swiglu  w12 + SiLU gate of DINOv2's SwiGLU MLP (dinov2_vitg14: teacher.py:114-116 loads every dinov2_* name)
 *   basd_vit_embed_reg_bf16  the DINOv2 forward's token assembly with register tokens (the dinov2_*_reg models, same lines)
 *   basd_gemm_bf16_gelu_fwd, basd_gemm_bf16_gelu_bwd
 *                          timm Mlp (fc1 -> nn.GELU -> fc2) of the TRAINED student: forward and autograd (trainer.py:33,157)
 *   basd_gemm_bf16x3_f32   the teacher-token projection tokens.reshape(-1, D_t) @ proj_t.T (layer_selector.py:72 / :135)
 *                          at student widths > 256
 *   basd_transpose_bf16_table
 *                          the W^T operands autograd's nn.Linear backward forms per call (trainer.py:157)
 *   basd_procrustes_fwd    src/losses/relational.py:47-48 (cross-covariance, nuclear norm, U V^T) as one call
 *   basd_procrustes_bwd    autograd of relational.py:29-48 (svd_backward of the nuclear norm + centring / weighting)
 *   basd_ce_uwso           nn.CrossEntropyLoss(label_smoothing) (trainer.py:47) + UW-SO (src/losses/combined.py:57,78-85)
 *   basd_wgrad_bf16        autograd of the student's timm nn.Linear layers (trainer.py:157)
 *   basd_sf_adamw_step     schedulefree.AdamWScheduleFree.step  src/training/trainer.py:54-58,158
 *   basd_bgemm_f64, basd_trinv_f64
 *                          the products / triangular solves around the SVD of relational.py:47-48 and its backward
 *                          (torch.linalg.svd backward -> U V^T), formed in fp64
 *   basd_procrustes_bwd_rows
 *                          autograd of relational.py:29-46 (centring, sqrt-weights, traces)
 *   basd_attention_bwd_bf16
 *                          autograd through timm Attention.forward of the student (trainer.py:157)
 *   basd_attention_fwd_bf16, basd_attention_fwd_qmean_bf16, basd_cls_importance_bf16
 *                          timm Attention.forward of the frozen teacher (teacher.py:118 creates it) and the
 *                          attention capture hook src/models/teacher.py:27-39 + relational.py:22-27
 *   basd_attention_fwd_long_bf16, basd_attention_bwd_long_bf16
 *                          the same forward (with both taps) and backward for 1 <= T <= 1024 tokens (hd 64 | 80):
 *                          /14 grids, 384 px inputs and hd-80 students, where the kernels above refuse the shape
 *   basd_attention_fwd_relbias_bf16
 *                          timm Beit Attention.forward of a frozen BEiT / BEiT-v2 teacher (learned relative-position
 *                          bias on the logits, teacher.py:118 creates it) with the CLS-row tap
 *   basd_attention_fwd_rope_bf16
 *                          timm Eva EvaAttention.forward of a frozen EVA-02 teacher (rotary position embedding on q and
 *                          k, teacher.py:118 creates it) with the CLS-row tap
 *   basd_attention_fwd_long_rope_bf16
 *                          the same rotary forward for 273 .. 1024 tokens (DINOv3 and EVA-02 teachers at 384 px) on
 *                          the tiled kernels; DINOv3's half-split pairs are interleaved in the weights at load time
 *   basd_attention_fwd_long_relbias_bf16
 *                          the same biased forward for 273 .. 1024 tokens (BEiT teachers at 384 px) on the tiled kernels
 *   basd_layernorm_fwd_bf16 / _bwd_bf16, basd_add_layernorm_fwd_bf16
 *                          timm nn.LayerNorm of the ViT blocks (student: with backward; frozen teacher: fused with
 *                          the residual add in front of it)
 *   basd_split_bf16x2_table, basd_split_patches_bf16x2, basd_gemm_f32x3, basd_attention_fwd_f32x3,
 *   basd_add_layernorm_fwd_f32
 *                          the fp32 evaluation forward of a ViT under torch.set_float32_matmul_precision("high")
 *                          (src/training/trainer.py:183-188, src/train.py:153-160, src/eval.py:16): nn.Linear,
 *                          Attention, nn.LayerNorm and the patch-embedding convolution on split-bf16 (bf16x3) MFMA
 *                          products, fp32 everywhere else
 *   basd_attention_fwd_f32x3_long
 *                          the Attention of that forward for 1 <= T <= 1024 tokens (384 px inputs, /14 grids), where
 *                          basd_attention_fwd_f32x3 refuses the shape
 *   basd_dwconv7_ln_bf16, basd_grn_bf16, basd_patchify_bf16
 *                          the frozen ConvNeXt-V2 teacher trunk (src/models/teacher.py through timm)
 *   basd_conv3x3_bf16, basd_conv7x7s2_relu_bf16, basd_maxpool3x3s2_bf16, basd_add_relu_bf16
 *                          the frozen ResNet teacher trunk (src/models/teacher.py through timm)
 *   basd_window_attention_fwd_bf16, basd_patch_merge_ln_bf16
 *                          the frozen Swin teacher trunk (src/models/teacher.py through timm: the `layers` container and
 *                          the nhwc feature map its probe understands)
 *   basd_window_attention_fwd_wide_bf16
 *                          the window attention of that trunk for windows 9 .. 16 (the window-12 checkpoints at 384 px)
 *   basd_resample_u8, basd_ta_normalize_u8
 *                          the torchvision v2 transforms of both training views (src/data/datasets.py:80-94 clean /
 *                          evaluation view, :137-149 augmented view), which the reference runs in its loader workers
 *   basd_resample_u8_packed
 *                          the resize / crop / flip of those views for images of different sizes (directory splits),
 *                          packed into one byte buffer
 *   basd_cls_tally         src/evaluation/metrics.py:19-55: outputs[:, valid_indices], MulticlassAccuracy(top_k = 1 | 5)
 *                          and criterion(outputs, labels) of one evaluation batch, accumulated on the device
 *   basd_mixup_cutmix      src/training/trainer.py:89-92,138: RandomChoice([MixUp, CutMix]) of one batch and its soft
 *                          targets, written into the captured step's input buffers in one launch
 *   basd_resample_tokens, basd_resample_tokens_adjoint
 *                          src/losses/combined.py:9-14 (_align_token_count) and its autograd
 *   basd_procrustes_importance_bwd
 *                          autograd of relational.py:29-33 w.r.t. the importance, back through the token resample
 *
 * 81 entries in all (basd_version and basd_last_error included).
 */
#ifndef BASD_HIP_H
#define BASD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BASD_OK 0
#define BASD_ERR_SHAPE 1        /* bad / unsupported shape                       */
#define BASD_ERR_LAUNCH 2       /* HIP launch error                              */
#define BASD_ERR_WORKSPACE 3    /* workspace too small                           */
#define BASD_ERR_DTYPE 4        /* unsupported dtype code                        */

/* Device-side health flags: kernels whose failure is data dependent OR them (atomically) into an optional
 * caller-owned int32 word instead of returning them -- no entry ever synchronises with the device.  The host
 * side reads the word when it chooses to (the Python binding: once per step, one step late, and raises a
 * torch.linalg.LinAlgError, which is what the reference's torch.linalg calls raise on such input). */
#define BASD_STATUS_NONCONVERGED 1   /* a Jacobi solve used all max_sweeps sweeps and was still rotating      */
#define BASD_STATUS_NONFINITE 2      /* NaN / Inf among the singular values (non-finite input)               */
#define BASD_STATUS_RANK0 4          /* Marchenko-Pastur rank 0: the reference divides by sum(sw) = 0 here   */
/* bits 8 .. 27: diagnostics OR-ed in with BASD_STATUS_NONCONVERGED (informational): bits 8-11 the Jacobi kernel variant
 * (2 / 3 odd-even with a double / single mailbox, 6 quad-block, 7 hex-block; 1, 4, 5: kernels that no longer exist),
 * bits 12-27 the index of the matrix in its launch (saturating at 65535) */

#define BASD_DTYPE_F32 0
#define BASD_DTYPE_BF16 1
#define BASD_DTYPE_F64 2

/* widest Jacobi input, and the LDS a Jacobi workgroup may use (the mailboxes of the register-resident kernels) */
#define BASD_JACOBI_MAX_COLS 256
#define BASD_JACOBI_LDS_BYTES 163840

int basd_version(void);
const char* basd_last_error(void);

/* z = X P^T (fp32 MFMA), gram = z^T z and colsum = 1^T z accumulated in fp64.
 * x: [rows, d_in] row-major (dtype code), proj: [d_out, d_in] fp32 row-major,
 * gram: [d_out, d_out] fp64 (MUST be zeroed by the caller), colsum: [d_out] fp64 (zeroed).
 * Only the LOWER 16x16 tiles of gram are accumulated (fp64 atomics are the kernel's HBM write
 * traffic: 41 MB per call at d_out = 192); the caller mirrors them.
 * d_out <= 256 and d_out % 16 == 0; d_in % 32 == 0.
 * Strided token views: logical row r is token r % rows_per_batch of batch r / rows_per_batch and
 * lives at x + (r / rows_per_batch) * batch_stride + (r % rows_per_batch) * d_in (elements); a
 * contiguous matrix is rows_per_batch = rows, batch_stride = 0.  This is how the CLS-stripped view
 * out[:, 1:, :] of a block output is consumed without a copy. */
int basd_token_gram(const void* x, int x_dtype, int64_t rows, int d_in,
                    int rows_per_batch, int64_t batch_stride,
                    const float* proj, int d_out,
                    double* gram, double* colsum, void* stream);

/* bf16-input fast path of basd_token_gram: x [rows, d_in] bf16, proj_split [3, d_out, d_in] bf16 =
 * the three-term bf16 split of the fp32 projection (P = Ph + Pm + Pl, each term the bf16
 * rounding of the remainder).  Same outputs / zeroing contract.  d_out in {32, 64, 128, 192},
 * d_in % 32 == 0.  x is read in 16-byte fragments: x must be 16-byte aligned and batch_stride a multiple of 8
 * elements (BASD_ERR_SHAPE otherwise). */
int basd_token_gram_bf16x3(const void* x, int64_t rows, int d_in, int rows_per_batch, int64_t batch_stride,
                           const void* proj_split, int d_out, double* gram, double* colsum, void* stream);

/* Gram of a tall fp32 matrix z [rows, d] (row-major, 16-byte aligned, d % 16 == 0): gram [d, d] fp64 += z^T z (lower
 * 16 x 16 tiles only), colsum [d] fp64 += column sums; both MUST be zeroed by the caller (atomics).  Tile-centred: per
 * 64 rows the column means are subtracted, the centred tile runs on the fp32 matrix cores and the exact uncentred
 * statistics are restored with fp64 rank-1 terms (the arithmetic of the fused kernel's Gram phase).  The statistics of
 * src/losses/layer_selector.py:13,35 at student widths beyond 256 (BASELINE c4 / c5), after basd_gemm_bf16x3_f32. */
int basd_gram_f32_centred(const float* z, int64_t rows, int d, double* gram, double* colsum, void* stream);

/* Pivoted (diagonal pivoting) Cholesky of `batch` symmetric PSD fp64 matrices
 * a[b] (n x n).  Writes
 *   w0   [batch, n, ld] fp32: column k (contiguous, ld floats) = k-th Cholesky column,
 *        rows in ORIGINAL order (a[b] = W0 W0^T), columns >= rank zeroed;
 *   lwork[batch, n, n] fp64: the same columns in fp64 (column-major by step);
 *   piv  [batch, n] int32: pivot row chosen at step k (a permutation of 0..n-1);
 *   rank [batch] int32: number of pivots > tol * dmax, dmax = the largest diagonal entry of a[b], or
 *        dmax_ref[b] when dmax_ref (device fp64 [batch], nullable) is given: the panels of a BLOCKED
 *        factorisation of a wider matrix stop relative to the diagonal of the whole matrix, not of their
 *        own Schur complement.
 * Only the LOWER triangle of a[b] (row >= column) is read.  n <= 256. */
int basd_pchol_f64(const double* a, int batch, int n, double tol, const double* dmax_ref,
                   float* w0, int ld, double* lwork, int32_t* piv, int32_t* rank,
                   void* stream);
/* The same with a problem mask: skip (device int32 [batch], nullable): skip[b] != 0 leaves every output of matrix b
 * untouched (its workgroup returns at once).  For batched pipelines whose set of live problems is known on the DEVICE
 * only -- the block pairs of the wide students' eigensolver that contain an all-zero block (rank-masked
 * principal-angle problems, src/losses/layer_selector.py:84-92): no host sync, no re-packing of the batch. */
int basd_pchol_f64_masked(const double* a, int batch, int n, double tol, const double* dmax_ref,
                          float* w0, int ld, double* lwork, int32_t* piv, int32_t* rank,
                          const int32_t* skip, void* stream);

/* Inverse of the pivoted Cholesky factor left by basd_pchol_f64, fp64, block triangle in LDS:
 * out[b] = L_p^-1 P  ([n, n] row-major; P = pivot permutation, L_p = P L lower triangular), so
 * out @ M == L_p^-1 (P M) for M with rows in ORIGINAL order.  Rows >= rank[b] are zero.  n <= 208 (blocked on the fp64
 * matrix cores up to 192; 193 .. 208: blocked leading 192 rows + border rows). */
int basd_trinv_f64(const double* lwork, const int32_t* piv, const int32_t* rank, int batch, int n,
                   double* out, void* stream);
/* skip[b] != 0: out[b] untouched (see basd_pchol_f64_masked) */
int basd_trinv_f64_masked(const double* lwork, const int32_t* piv, const int32_t* rank, int batch, int n,
                          double* out, const int32_t* skip, void* stream);

/* One-sided (Hestenes) Jacobi in LDS on `batch` column-major matrices
 * w[b]: n_cols columns of `ld` floats, first m_rows rows significant
 * (rows m_rows..ld-1 must be zero).  Columns are orthogonalised in place;
 * on return column c holds sigma_c * u_c.  If sort != 0 columns are permuted
 * so that norms descend.  sigma [batch, n_cols] receives the column norms of
 * the first `norm_rows` rows (norm_rows = m_rows normally; for a stacked
 * [A; I] input pass the row count of A so that the bottom block -- the
 * accumulated right singular vectors -- is excluded from the norm).
 * sweeps [batch] (optional, may be NULL) receives the sweeps used, NEGATED if the matrix was still rotating when
 * max_sweeps was reached (with max_sweeps = 1: "this visit still made a large rotation").
 * active (optional, device int32 [batch], may be NULL): matrix b has non-zero entries only in its
 * leading active[b] columns (and rows, if active_rows != 0); the sweeps then run over that
 * block only (rank-masked principal-angle problems, no host sync on the ranks).  active[b] < 0 skips matrix b
 * altogether (w, sigma untouched, sweeps[b] = 0): converged matrices of a block tournament cost a 5 us launch instead
 * of a sweep.
 * active_rows == 2 declares `active` a pure MASK -- every entry is either < 0 (skip) or n_cols (solve completely).
 * status (optional, device int32 word, may be NULL): BASD_STATUS_NONCONVERGED / BASD_STATUS_NONFINITE are OR-ed in.
 * Requires n_cols <= 256, ld % 4 == 0, m_rows <= ld and one of: m_rows <= 224; m_rows <= 256 with n_cols <= 196;
 * m_rows <= 384 with n_cols <= 192 (tall block pairs; with max_sweeps = 1 and sort = 0 this is one visit of a
 * block-Jacobi tournament over wider matrices).  Anything else is BASD_ERR_SHAPE, at every batch size.  The kernel is
 * chosen from (m_rows, n_cols) alone (the hex-block kernel also looks at batch > 256 for its occupancy). */
int basd_jacobi_svd(float* w, int batch, int m_rows, int n_cols, int ld, int norm_rows,
                    float tol, int max_sweeps, int sort,
                    float* sigma, int32_t* sweeps, const int32_t* active, int active_rows,
                    int32_t* status, void* stream);

/* Marchenko-Pastur rank on device (no host sync).  evals [batch, n] (any order),
 * rows = M of the [M, D] token matrix, d = D; uses the min(M, D) largest eigenvalues,
 * LOWER median, lambda_+ = med * (1 + sqrt(D/M))^2, count > lambda_+, clamp to cap.  n <= 1024.
 * status (optional device int32 word): BASD_STATUS_RANK0 when a count is 0, BASD_STATUS_NONFINITE for a NaN spectrum. */
int basd_mp_rank(const float* evals, int batch, int n, int64_t rows, int d, int cap,
                 int32_t* ranks, int32_t* status, void* stream);

/* Householder reduction of a symmetric fp64 matrix to tridiagonal form with the same eigenvalues (unblocked, one
 * reflector per column: LAPACK dsytd2 without the reflectors kept).  a [n, n] row-major, BOTH triangles valid; it is
 * scratch and is overwritten.  diag [n], off [n - 1] receive the tridiagonal matrix.  work: at least
 * basd_sym_tridiag_f64_workspace_bytes(n) bytes of device memory.  2 <= n <= 2048, anything else is BASD_ERR_SHAPE and
 * no pointer is touched.  2 (n - 2) + 1 launches on `stream` (two per column, one for the last 2 x 2 block), no host
 * sync, no grid-wide wait, no floating-point atomics: every reduction has a fixed order, so two runs on the same input
 * agree bit for bit.  A column that is already zero below the sub-diagonal takes tau = 0 (no update); NaN / Inf in `a`
 * propagate into diag / off. */
int64_t basd_sym_tridiag_f64_workspace_bytes(int n);
int basd_sym_tridiag_f64(double* a, int n, double* diag, double* off, void* work, void* stream);

/* Marchenko-Pastur rank (reference layer_selector.py:8-20) from the tridiagonal form of the smaller-side Gram
 * (X^T X or X X^T, NOT divided by rows) of an [rows, d] matrix, by Sturm counts: the lower median eigenvalue
 * (ascending index (n - 1) / 2, what torch.median returns) by 256-section inside the Gershgorin bracket down to
 * 2^-48 of its width, lambda_+ = med / rows * (1 + sqrt(d / rows))^2, rank[0] = min(cap, #eigenvalues of Gram / rows
 * at or above lambda_+).  One workgroup, fp64 throughout.  2 <= n <= 2048 and n <= min(rows, d), else BASD_ERR_SHAPE.
 * status (optional device int32 word): BASD_STATUS_RANK0 when the count is 0 on a finite spectrum; any NaN / Inf in
 * diag / off gives rank 0 and BASD_STATUS_NONFINITE. */
int basd_tridiag_mp_rank(const double* diag, const double* off, int n, int64_t rows, int d, int cap,
                         int32_t* rank, int32_t* status, void* stream);

/* Data-dependent failure raised from host-orchestrated checks (the blocked eigensolver's orthogonality test): ORs
 * `bit` (a BASD_STATUS_* value) into the device health word if any of the n fp64 values is NOT <= tol -- a NaN raises it
 * too -- with an atomic OR (the word is shared with kernels of other streams).  Counterpart of the
 * torch._C._LinAlgError the reference's torch.linalg calls raise (layer_selector.py:16,36,92,99). */
int basd_flag_if_exceeds_f64(const double* values, int64_t n, double tol, int bit, int32_t* status, void* stream);

/* Principal-angle distances -> mixing weights of the Grassmannian selector, fused (reference
 * src/losses/layer_selector.py:100-108).  sigma [E, L, D] fp32: cosines of the principal angles between student
 * extraction point i and teacher layer j (descending; zero beyond the layer's rank), sw [L, D] fp32: the teacher's
 * singular values masked at the MP rank, log_temp [E].  Outputs (fp32): d2 [E, L] = sum_m sw theta^2 / sum_m sw with
 * theta = acos(min(sigma, 1 - eps)); pre [E, L] = -d2 / softplus(log_temp); weights [E, L] = softmax_j(pre);
 * coef [E, L, D] = (d d2 / d sigma) / sigma (divided by sigma^2 once more when unnormalised != 0: the caller's
 * singular vectors are then the Jacobi's sigma_m u_m columns) -- the diagonal of the backward seed Phi.  L <= 64. */
int basd_angle_weights(const float* sigma, const float* sw, const float* log_temp, int E, int L, int D,
                       int unnormalised, float* d2, float* pre, float* weights, float* coef, void* stream);

/* Backward of the selector weights (autograd of src/losses/layer_selector.py:86-108 w.r.t. the student tokens and the
 * temperatures).  g_w [E, L]: gradient w.r.t. the mixing weights; g_pre_out [E, L] (nullable): gradient w.r.t. the
 * pre-softmax values; weights, d2 [E, L], log_temp [E]: forward values; t_seed [E, L, D, D] fp32: the forward's seeds
 * A_full A_bar^T Phi (rows b >= k_j only); v_s [E, D, D] fp32 (rows = eigenvectors of the student's centred Gram),
 * lam_s [E, D] fp64 (its eigenvalues); proj_s [D, D_s] fp32.  Outputs: g_log_temp [E] fp32, w_tok [E, D_s, D_s] fp32 with
 * d loss / d s_i = (s_i - column mean) w_tok[i].  One reduction launch, four basd_bgemm_f64 products, one store, on a
 * workspace of basd_angle_weights_bwd_workspace_bytes(E, D, D_s) bytes.  L <= 64. */
int64_t basd_angle_weights_bwd_workspace_bytes(int E, int D, int D_s);
int basd_angle_weights_bwd(const float* g_w, const float* g_pre_out, const float* weights, const float* d2,
                           const float* log_temp, const float* t_seed, const float* v_s, const double* lam_s,
                           const float* proj_s, int E, int L, int D, int D_s, float* g_log_temp, float* w_tok,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* Selector frames of one side from its Gram statistics (reference src/losses/layer_selector.py:69-74, 133-138 for the
 * teacher, :84-92 for the student).  unc [n, D, D] fp64: uncentred Grams (lower triangles, as
 * basd_token_gram(..., mirror = False) writes them), csum [n, D] fp64: their column sums, m_rows: tokens per layer.
 * Centred Gram unc - csum csum^T / m_rows -> eigen-decomposition (basd_pchol_f64 + basd_jacobi_svd) ->
 *   sigma [n, D] fp32 descending (square roots of the eigenvalues), lam [n, D] fp64 = sigma^2 (nullable),
 *   v [n, D, D] fp32: row m = unit eigenvector m (zero rows beyond the numerical rank).
 * with_ranks != 0 (the teacher half): the uncentred Grams are decomposed in the same launches and give
 *   ranks [n] int32 (basd_mp_rank, capped at D - 1); v rows and sigma entries m >= ranks[b] are then zeroed (the
 *   reference's frame cut at the rank and the spectral weights sw); lam stays unmasked.
 * status (nullable device word): BASD_STATUS_* OR-ed in by the Jacobi and the rank count.  D <= 192 (BASD_ERR_SHAPE
 * otherwise).  workspace: >= basd_selector_frames_workspace_bytes(n, D) bytes of scratch (BASD_ERR_WORKSPACE).  The
 * shapes and the workspace are checked before anything is enqueued. */
int64_t basd_selector_frames_workspace_bytes(int n, int D);
int basd_selector_frames(const double* unc, const double* csum, int n, int64_t m_rows, int D, int with_ranks,
                         int32_t* ranks, float* sigma, double* lam, float* v, int32_t* status, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* Selector mixing weights from the two frames (reference src/losses/layer_selector.py:93-108): v_s [E, D, D] fp32
 * (student frames, basd_selector_frames with_ranks = 0), ranks [L] int32, vm_t [L, D, D] fp32, sw [L, D] fp32 (teacher
 * frames, with_ranks != 0), log_temp [E] fp32 ->
 *   weights, pre, d2 [E, L] fp32 as basd_angle_weights, and t_seed [E, L, D, D] fp32: the backward seeds
 *   A_full A_bar^T Phi (rows b >= k_j only) with A_full = V_s V_t^T, A_bar its rows b < k_j and Phi the coefficient
 *   form of basd_angle_weights -- exactly the inputs of basd_angle_weights_bwd.
 * The four products run on the fp32-input matrix cores, one launch each over the E L pairs; the principal angles come
 * from the rank-masked basd_jacobi_svd.  status as above.  L <= 64, D <= 192 (BASD_ERR_SHAPE otherwise).
 * workspace: >= basd_selector_weights_workspace_bytes(E, L, D) bytes (BASD_ERR_WORKSPACE). */
int64_t basd_selector_weights_workspace_bytes(int E, int L, int D);
int basd_selector_weights(const float* v_s, const int32_t* ranks, const float* vm_t, const float* sw,
                          const float* log_temp, int E, int L, int D, float* weights, float* pre, float* d2,
                          float* t_seed, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* mixed[i] = sum_j w[i, j] * x_j   (all E mixes from ONE pass over the teacher layers)
 * x_layers: HOST array of L device pointers to [elems] tensors (dtype code; the pointers are
 * passed to the kernel by value, no device-side table), w: [E, L] fp32,
 * out: [E, elems] fp32 (contiguous).  Each source layer is a batch-strided view: logical element e
 * is at layer + (e / per_batch) * batch_stride + e % per_batch (contiguous: per_batch = elems). */
int basd_mix_tokens(const void* const* x_layers, int x_dtype, int L, int E,
                    const float* w, int64_t elems, int64_t per_batch, int64_t batch_stride,
                    float* out, void* stream);

/* Procrustes prep for `batch` = B samples of one extraction point:
 * s [B, N_s, D_s] (dtype; sample b at s + b * s_batch_stride), t [B, N_t, D_t] fp32 (mixed teacher),
 * imp [B, N_t] fp32.
 * Resamples t and imp to N_s (2-tap linear, align_corners=False), normalises imp,
 * weighted-centres and sqrt-weights:
 *   s_w [B, N_s, D_s], t_w [B, N_s, D_t] fp32, a [B, N_s], tr [B, 2] = (tr_s, tr_t). */
int basd_procrustes_prep(const void* s, int s_dtype, int64_t s_batch_stride, const float* t, const float* imp,
                         int B, int N_s, int N_t, int D_s, int D_t,
                         float* s_w, float* t_w, float* a, float* tr, void* stream);

/* dots[i, j] = sum_e g[i, e] * x_j[e]  for all (i, j) from ONE pass over the teacher layers.
 * g: [E, elems] fp32, dots: [E, L] fp64 (MUST be zeroed by the caller; fp64 atomics keep the
 * result independent of the arrival order to ~1e-16). */
int basd_mix_grad_dots(const void* const* x_layers, int x_dtype, int L, int E,
                       const float* g, int64_t elems, int64_t per_batch, int64_t batch_stride,
                       double* dots, void* stream);

/* Batched GEMM with fp64 accumulation on the fp64 matrix cores: C[b] = op(A[b]) op(B[b]).
 * Row-major, explicit leading dimensions and batch strides (in elements); A/B dtype F32 or F64,
 * C dtype F32 or F64; trans_x != 0 means the stored matrix is the transpose of op(X).
 * symmetric != 0 (M == N, result known symmetric, e.g. X X^T): only the lower triangle is the product; the upper one is
 * a copy of it.  Tiles of 64x64 above the diagonal are not computed but mirrored from their transposes on store; the
 * pipelined kernel (aligned shapes) also mirrors the 16x16 sub-tiles above the diagonal inside a diagonal tile, and every
 * kernel computes the sub-tiles (or tiles) ON the diagonal in full, both triangles.  So c == c^T bit for bit holds for
 * true X X^T operands only (the same numbers on both sides: (i, j) and (j, i) are then the same sum in the same order);
 * for a product that is symmetric only in exact arithmetic (X^T (G X)) the elements above the diagonal inside a diagonal
 * sub-tile are the rounded (i, j) sums, the others copies of (j, i).  Callers of that form read the lower triangle only
 * (basd_pchol_f64 does).
 * Replaces the torch.bmm / matmul calls of the Procrustes core that must not round to fp32
 * (reference src/losses/relational.py:47 forms the cross-covariance in fp32). */
int basd_bgemm_f64(const void* a, int a_dtype, int64_t a_stride, int lda, int trans_a,
                   const void* b, int b_dtype, int64_t b_stride, int ldb, int trans_b,
                   void* c, int c_dtype, int64_t c_stride, int ldc,
                   int batch, int M, int N, int K, int symmetric, void* stream);
/* skip[b] != 0: c[b] untouched (see basd_pchol_f64_masked) */
int basd_bgemm_f64_masked(const void* a, int a_dtype, int64_t a_stride, int lda, int trans_a,
                          const void* b, int b_dtype, int64_t b_stride, int ldb, int trans_b,
                          void* c, int c_dtype, int64_t c_stride, int ldc,
                          int batch, int M, int N, int K, int symmetric, const int32_t* skip, void* stream);

/* ViT linear layer on the bf16 matrix cores with a fused epilogue (timm nn.Linear + nn.GELU of the blocks; reference
 * call sites src/models/teacher.py:212 and src/training/trainer.py:33; with w := W^T also the input gradient
 * dX = dY W of trainer.py:157):   y[m][n] = epi(sum_k x[m][k] w[n][k] + bias[n]),
 * x [M, K], w [N, K], y [M, N], bias [N] (nullable) all bf16 row-major, fp32 accumulation.
 * epilogue: 0 = none, 1 = + bias, 2 = exact-erf GELU(+ bias).  K % 64 == 0, N a multiple of 256, 192 or 128.
 * tile_run: how many output tiles a workgroup of the persistent kernel (large M, N % 256 == 0, K >= 192) multiplies
 * before it retires: 0 = its whole share (one workgroup per CU for the whole launch: fastest when the GEMM has the GPU
 * to itself), k >= 1 = at most k (the CUs come free every k tiles: for launches that share the GPU with another
 * stream; the pipelined BASD step uses 1 for the frozen teacher's launches and 0 for the student's own), k < 0 = fully
 * persistent on -k (8 .. 32) workgroups per XCD, i.e. the launch leaves the other CUs to another stream for its whole
 * duration (measured at -16 .. -28: equal to 1 within the noise; -12: the teacher branch becomes the critical path);
 * a negative value outside that range is clamped to it (-1 .. -7 run 8 workgroups per XCD, below -32 run 32).  The
 * results do not depend on it: every tile_run gives bitwise the same output. */
int basd_gemm_bf16(const void* x, const void* w, const void* bias, void* y, int64_t M, int N, int K,
                   int epilogue, int tile_run, void* stream);

/* The same GEMM with the activation of a frozen teacher's MLP named explicitly (timm Mlp.act of the CLIP / SigLIP ViTs):
 *   y[m][n] = bf16(act(sum_k x[m][k] w[n][k] + bias[n])),   bias nullable,
 * act: 0 = none, 1 = exact-erf GELU (bitwise basd_gemm_bf16 with epilogue 2), 2 = QuickGELU x sigmoid(1.702 x)
 * (OpenAI-weight CLIP), 3 = tanh-GELU 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) (SigLIP).  The activation is
 * taken in fp32 on the fp32 sum before the single rounding to bf16; 2 and 3 are evaluated as x / (1 + 2^(-s log2 e))
 * with the hardware's 1-ulp exp2 and reciprocal: absolute error <= 8 * 2^-24 * max(1, |x|) before the rounding, no
 * overflow for any finite x (a saturated exponential gives 0 or x).  Shapes, tile_run, kernels and schedule as
 * basd_gemm_bf16.  Any other act is BASD_ERR_SHAPE before anything is enqueued. */
int basd_gemm_bf16_act(const void* x, const void* w, const void* bias, void* y, int64_t M, int N, int K,
                       int act, int tile_run, void* stream);

/* The first half of a SwiGLU MLP (DINOv2 ViT-g/14: w3(silu(x1) * x2) with x1, x2 = w12(x).chunk(2, -1)) as ONE GEMM
 * with the gate in its epilogue:
 *   y[m][h] = bf16(silu(a1) * a2),   a1 = sum_k x[m][k] w1[h][k] + b1[h],   a2 = sum_k x[m][k] w2[h][k] + b2[h],
 * both sums, the sigmoid and the two products in fp32, one rounding to bf16.  x [M, K] bf16, y [M, H] bf16 with row
 * pitch H.  The sigmoid is 1 / (1 + 2^(-a1 log2 e)) on the hardware's exp2 and reciprocal, as in basd_gemm_bf16_act:
 * no overflow for any finite input (a saturated exponential gives -0 or a1 * a2).
 * w12p [2 H, K] / bias12p [2 H] (nullable) are the PACKED forms of the hub's w12.weight / w12.bias, whose rows
 * 0 .. H - 1 are w1 (the x1 half) and H .. 2 H - 1 are w2.  Row map, with p the packed row:
 *   p = 64 * (h / 32) + 32 * s + h % 32   <->   source row s * H + h      (s = 0: w1 / x1, s = 1: w2 / x2, 0 <= h < H)
 * i.e. blocks of 32 w1 rows alternate with the 32 w2 rows of the same h: a wave of the 256-column tile owns 64 packed
 * columns = both pre-activations of 32 outputs, in matching registers.  Build it once per frozen layer
 * (_native.swiglu_pack).  H % 128 == 0 and K % 64 == 0, else BASD_ERR_SHAPE before anything is enqueued (the caller
 * runs the unfused composition).  Kernels: only the 256-column ring kernels carry this epilogue -- the persistent ring
 * where basd_gemm_bf16 would choose it for N = 2 H (large M, K >= 192), the ring kernel for every other shape; the
 * 192- and 128-column tiles are never chosen.  tile_run as basd_gemm_bf16; the output does not depend on it. */
int basd_gemm_bf16_swiglu(const void* x, const void* w12p, const void* bias12p, void* y, int64_t M, int H, int K,
                          int tile_run, void* stream);

/* Teacher-statistics projection z = X P^T at student widths > 256 (src/losses/layer_selector.py:72 / :135: the fixed fp32 projection of
 * the teacher tokens in front of the subspace SVD): x [M, K] bf16 row-major, w3 [ceil(N / 256) * 256, 3 K] bf16 = the
 * (hi | mid | lo) bf16 splits of P's rows side by side (zero rows behind N), y [M, N] fp32.  One persistent bf16-MFMA
 * GEMM of depth 3 K, fp32 accumulation over all three splits.  K % 64 == 0, K >= 128, N % 8 == 0, M > 1792. */
int basd_gemm_bf16x3_f32(const void* x, const void* w3, float* y, int64_t M, int N, int K, void* stream);

/* The trained student's MLP (timm Mlp: fc1 -> nn.GELU -> fc2, trainer.py:33 / :157) without a separate GELU pass:
 *   fwd:  pre[m][n] = bf16(sum_k x[m][k] w[n][k] + bias[n])   (saved for backward),   y = bf16(gelu(pre))
 *   bwd:  dpre[m][n] = bf16((sum_k dy[m][k] wt[n][k]) * gelu'(pre[m][n]))   with wt = fc2.weight^T  [N = hidden, K = out]
 * exact-erf GELU and its derivative Phi(x) + x phi(x), evaluated in fp32 on the bf16-rounded pre-activation (what
 * nn.GELU and its autograd see behind a bf16 nn.Linear).  Shapes and tile_run as basd_gemm_bf16. */
int basd_gemm_bf16_gelu_fwd(const void* x, const void* w, const void* bias, void* pre, void* y, int64_t M, int N,
                            int K, int tile_run, void* stream);
int basd_gemm_bf16_gelu_bwd(const void* dy, const void* wt, const void* pre, void* dpre, int64_t M, int N, int K,
                            int tile_run, void* stream);

/* ViT weight-gradient GEMM (backward of nn.Linear): dw[n][k] += sum_m dy[m][n] x[m][k],
 * db[n] += sum_m dy[m][n] (db may be NULL).  dy [M, N], x [M, K] bf16 row-major, dw [N, K] /
 * db [N] fp32, ACCUMULATED with atomics (caller zero-initialises or accumulates on purpose).
 * N % 64 == 0, K % 64 == 0. */
int basd_wgrad_bf16(const void* dy, const void* x, int64_t M, int N, int K, float* dw, float* db,
                    void* stream);

/* The same with a caller-provided workspace: shapes with N % 192 == 0, K % 192 == 0, M >= 4096 (every ViT student
 * width) run as 192 x 192 tiles whose per-slab partial sums go through the workspace and a reduction launch instead of
 * 256-way fp32 atomics (which execute at the memory side: 31 - 48 us per launch).  basd_wgrad_workspace_bytes returns
 * the bytes this shape needs (0: no workspace used; <= 37.75 MB); the workspace is scratch, 16-byte aligned, and may
 * be shared by all launches of a stream. */
int64_t basd_wgrad_workspace_bytes(int64_t M, int N, int K);
int basd_wgrad_bf16_ws(const void* dy, const void* x, int64_t M, int N, int K, float* dw, float* db,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* LayerNorm of the ViT blocks (timm nn.LayerNorm, eps 1e-6): bf16 activations in/out, fp32 gamma/beta,
 * fp32 statistics.  fwd saves mean / rstd [rows]; bwd writes dx and ACCUMULATES dgamma / dbeta
 * (fp32 atomics; pass NULL for a frozen layer).  D % 8 == 0, D <= 2048. */
int basd_layernorm_fwd_bf16(const void* x, const float* gamma, const float* beta, int64_t rows, int D,
                            float eps, void* y, float* mean, float* rstd, void* stream);
/* Pre-norm residual step of a block: sum_out = bf16(residual + scale * x), y = LayerNorm(sum_out).
 * row_scale (nullable, fp32 [rows / rows_per_scale]): per-SAMPLE scale of the branch x = the stochastic-depth keep
 * mask divided by the keep probability (timm DropPath); NULL = 1.  mean / rstd may be NULL (frozen block). */
int basd_add_layernorm_fwd_bf16(const void* x, const void* residual, const float* gamma, const float* beta,
                                int64_t rows, int D, float eps, void* sum_out, void* y, float* mean,
                                float* rstd, const float* row_scale, int rows_per_scale, void* stream);
/* Token assembly in front of block 0 of a ViT (timm _pos_embed + CLIP's norm_pre) in one launch:
 *   out[b, t, :] = LN(bf16(src(b, t) + pos[t, :])),   src = cls for t = 0 when cls != NULL, else the patch row.
 * patches [B, N, D] bf16 (the patch-embedding GEMM's output), cls [D] bf16 or NULL, pos [T, D] bf16 with
 * T = N + (cls != NULL), out [B, T, D] bf16, must not overlap patches.  gamma / beta fp32 [D], both or neither: NULL =
 * the plain assembly, bitwise torch's cat + add on bf16; otherwise the rounded sum is layer-normalised with the
 * arithmetic of basd_layernorm_fwd_bf16 (fp32 two-pass statistics, one rounding) and only the normalised row is written.
 * 16-byte accesses when all four pointers are 16-byte aligned, element accesses otherwise.  No workspace, no
 * allocation, no synchronisation.  D % 8 == 0, 8 <= D <= 2048, B >= 0, N >= 0, T >= 1, else BASD_ERR_SHAPE before
 * anything is enqueued. */
int basd_vit_embed_bf16(const void* patches, const void* cls, const void* pos, const float* gamma, const float* beta,
                        float eps, int B, int N, int D, void* out, void* stream);
/* The same assembly for a model with R register tokens (the DINOv2 "_reg" models): R learned rows behind the CLS row,
 * which take no position embedding:
 *   out[b, 0] = cls + pos[0],   out[b, 1 + r] = reg[r] (r < R),   out[b, 1 + R + n] = patches[b, n] + pos[1 + n],
 * reg [R, D] bf16, pos [1 + N, D], out [B, 1 + R + N, D]; every row then goes through LN when gamma / beta are given
 * (register rows included), exactly as above.  R > 0 needs cls and reg (BASD_ERR_SHAPE otherwise: no model of the
 * family lacks a CLS token).  R = 0: reg is ignored and the output is bitwise basd_vit_embed_bf16's -- one kernel
 * serves both entries.  Limits, alignment rule (reg counts among the pointers when R > 0) and errors as above. */
int basd_vit_embed_reg_bf16(const void* patches, const void* cls, const void* reg, int R, const void* pos,
                            const float* gamma, const float* beta, float eps, int B, int N, int D, void* out,
                            void* stream);
/* dx = LayerNorm backward (+ dres when given: the gradient that arrives through the residual connection of a pre-norm
 * block, so dx is the whole gradient of the block's residual stream); dbranch (nullable) = row_scale * dx, the
 * gradient of the branch input of basd_add_layernorm_fwd_bf16.  dgamma / dbeta are accumulated (nullable). */
int basd_layernorm_bwd_bf16(const void* dy, const void* x, const float* gamma, const float* mean,
                            const float* rstd, int64_t rows, int D, void* dx, float* dgamma, float* dbeta,
                            const void* dres, void* dbranch, const float* row_scale, int rows_per_scale,
                            void* stream);

/* Row epilogue of the Procrustes backward (reference src/losses/relational.py:22-45 differentiated):
 * p [rows, D] = (other side) G^T from the GEMM, w [rows, D] the weighted centred tokens, R = w - p,
 * a [rows] the normalised importance, gl [rows / rows_per_batch] the incoming gradient per sample ->
 *   out[row, :] = 2 gl sqrt(a[row]) R[row, :]   (fp32, may alias p, or bf16)
 *   rowdot[row] = 2 gl sum_d R[row, d] w[row, d].          D % 4 == 0. */
int basd_procrustes_bwd_rows(const float* p, const float* w, const float* a, const float* gl, int64_t rows,
                             int rows_per_batch, int D, void* out, int out_dtype, float* rowdot, void* stream);

/* Teacher attention tap (reference src/models/teacher.py:33-37 hook + src/losses/relational.py:22-27):
 * qkv [B, T, 3, H, hd] bf16 (the packed output of a block's qkv projection, CLS token first) ->
 * out[b, t-1] = mean_h softmax_t(bf16(q_cls . k_t) * scale), t = 1..T-1, fp32.  T <= 256, hd in {32, 64}. */
int basd_cls_importance_bf16(const void* qkv, int B, int T, int H, int hd, float scale, float* out,
                             void* stream);

/* Fused attention forward of a frozen block (inference): qkv [B, T, 3, H, hd] bf16 (packed projection) ->
 * out [B, T, H * hd] bf16 = softmax(Q K^T * scale) V per head (fp32 logits / probabilities, P rounded to bf16
 * for the second product, like the library flash kernel it replaces on the teacher: torch SDPA called at
 * timm Attention.forward).  importance (nullable): [B, H, T-1] fp32; receives per head the CLS-row softmax of
 * basd_cls_importance_bf16 divided by H (the tap is the sum over the H axis).  lse (nullable): [B, H, T] fp32,
 * log-sum-exp of the scaled logits per query (input of basd_attention_bwd_bf16).  hd == 64, T <= 272. */
int basd_attention_fwd_bf16(const void* qkv, int B, int T, int H, int hd, float scale, void* out,
                            float* importance, float* lse, void* stream);

/* The same forward for a teacher WITHOUT a CLS token (reference src/losses/relational.py:25-27: the tap is the
 * attention map averaged over heads and QUERIES): importance [B, H, T] fp32 receives per head
 * sum_q softmax(q . k * scale)[q][key] / (H T) -- the tap is the sum over the H axis.  Same shapes as above. */
int basd_attention_fwd_qmean_bf16(const void* qkv, int B, int T, int H, int hd, float scale, void* out,
                                  float* importance, void* stream);

/* The same forward for a frozen block whose attention carries BEiT's learned relative-position bias (timm Beit /
 * BEiT-v2 Attention.forward): qkv [B, T, 3, H, hd] bf16 with the CLS token first, T = gh * gw + 1 -> out [B, T, H * hd]
 * bf16 = softmax(Q K^T * scale + bias) V per head.  table: fp32 [R, H], R = (2 gh - 1)(2 gw - 1) + 3 -- timm's
 * relative_position_bias_table, heads on the fast axis.  Logit of query i and key j:
 *   fp32(q_i . k_j) * scale + table[idx(i, j)][h],
 *   idx = (y_i - y_j + gh - 1)(2 gw - 1) + (x_i - x_j + gw - 1)   both patches, patch p at (y, x) = ((p - 1) / gw, (p - 1) % gw)
 *   idx = R - 3 (i == 0, j >= 1),  R - 2 (i >= 1, j == 0),  R - 1 (i == j == 0).
 * The bias is gathered in the kernel from the head's column of the table (staged in LDS): no [T, T] or [H, T, T] array
 * is read or written.  importance (nullable): [B, H, T-1] fp32; receives per head the CLS row of that biased softmax
 * (fp32 logits) without the CLS column, divided by H (the tap is the sum over the H axis).  Arithmetic otherwise as
 * basd_attention_fwd_bf16: bf16 products with fp32 accumulation, fp32 logits and softmax (maximum subtracted), P rounded
 * to bf16 for the second product, one rounding at the store.  hd == 64, gh, gw >= 1, 2 <= T <= 272; anything else is
 * BASD_ERR_SHAPE without a launch.  No allocation, no synchronisation. */
int basd_attention_fwd_relbias_bf16(const void* qkv, const float* table, int B, int gh, int gw, int H, int hd,
                                    float scale, void* out, float* importance, void* stream);

/* The same forward for a frozen block whose attention rotates q and k with a rotary position embedding (timm Eva
 * EvaAttention.forward with RotaryEmbeddingCat: EVA-02): qkv [B, T, 3, H, hd] bf16 -> out [B, T, H * hd] bf16 =
 * softmax(Q' K'^T * scale) V per head, where for every head, token t and channel pair i
 *   x'[2i]     = x[2i] c - x[2i + 1] s
 *   x'[2i + 1] = x[2i + 1] c + x[2i] s,      (c, s) = rope[t][i],      x = q and x = k;  v is untouched.
 * rope: fp32 [T, hd / 2, 2], 16-byte aligned -- (cos, sin) of pair i of token t.  Row t applies to token t whatever it
 * is: the kernel knows no grid, frequency bands or prefix tokens, and a token that is not rotated (the CLS token) has
 * the row (1, 0).  The rotation happens in registers, between the global loads of the K chunks / Q fragments and their
 * use: fp32 arithmetic on the bf16 inputs, ONE rounding back to bf16, so the matrix cores see bf16 operands as in
 * basd_attention_fwd_bf16; no rotated copy of q or k and nothing [T, T] is read or written.  importance (nullable):
 * [B, H, T-1] fp32; receives per head the CLS row of that softmax (fp32 logits) without the CLS column, divided by H
 * (the tap is the sum over the H axis) -- layout and meaning of basd_attention_fwd_relbias_bf16's.  Arithmetic otherwise
 * as basd_attention_fwd_bf16.  hd == 64, 2 <= T <= 272, B >= 1, H >= 1, rope != NULL; anything else is BASD_ERR_SHAPE
 * without a launch.  No allocation, no synchronisation. */
int basd_attention_fwd_rope_bf16(const void* qkv, const float* rope, int B, int T, int H, int hd, float scale, void* out,
                                 float* importance, void* stream);

/* The rotary forward on the tiled kernels of basd_attention_fwd_long_bf16, for the token counts the entry above refuses
 * (a rotary teacher at 384 px: DINOv3 /16 has 581 tokens, EVA-02 /14 has 730): same qkv, rope, rotation rule (fp32
 * arithmetic, ONE rounding to bf16, before the logits; v untouched) and out.  cls_importance (nullable): [B, H, T-1]
 * fp32, the CLS tap of basd_attention_fwd_long_bf16 computed on the rotated operands: q_0 and every k row are rotated
 * and rounded to bf16, then fp32 dot, logit rounded to bf16, scale, expf, softmax without the CLS column, divided by H.
 * (The short entry taps its main softmax with fp32 logits instead; both are within bf16 rounding of the exact row.)
 * No LSE and no query-mean output: only frozen teachers with a CLS token use this entry.  hd == 64, 2 <= T <= 1024,
 * B >= 1, H >= 1, rope != NULL; anything else is BASD_ERR_SHAPE without a launch.  No allocation, no
 * synchronisation. */
int basd_attention_fwd_long_rope_bf16(const void* qkv, const float* rope, int B, int T, int H, int hd, float scale,
                                      void* out, float* cls_importance, void* stream);

/* BEiT's relative-position bias on the tiled kernels of basd_attention_fwd_long_bf16, for the token counts
 * basd_attention_fwd_relbias_bf16 refuses (BEiT at 384 px: 577 tokens): same qkv ([B, T, 3, H, hd] bf16, CLS token
 * first, T = gh * gw + 1), table (fp32 [R, H], R = (2 gh - 1)(2 gw - 1) + 3), index rule and out ([B, T, H * hd] bf16).
 * Logit of query i and key j: fp32(q_i . k_j) * scale + table[idx(i, j)][h]; the kernel stages the head's column
 * divided by scale in LDS and adds it to the raw fp32 dot in front of the online softmax's running maximum, so with an
 * all-zero table out and cls_importance are basd_attention_fwd_long_bf16's bit for bit.  No [T, T] or [H, T, T] array is
 * read or written.  cls_importance (nullable): [B, H, T-1] fp32, the CLS tap of basd_attention_fwd_long_bf16 plus the
 * bias: fp32 dot in d order, rounded to bf16, times scale, + table[R - 1][h] for key 0 and table[R - 3][h] for every
 * patch key, expf, softmax without the CLS column, divided by H.  (The short entry taps its main softmax with fp32
 * logits instead; both are within bf16 rounding of the exact row.)  No LSE and no query-mean output: BEiT always has a
 * CLS token.  hd == 64, gh, gw >= 1, 2 <= T <= 1024 (the short entry's range included), B, H >= 1, qkv, table and out
 * != NULL, scale finite and > 0; anything else is BASD_ERR_SHAPE without a launch and nothing is written.  No
 * allocation, no synchronisation. */
int basd_attention_fwd_long_relbias_bf16(const void* qkv, const float* table, int B, int gh, int gw, int H, int hd,
                                         float scale, void* out, float* cls_importance, void* stream);

/* Fused attention backward of a trained block (the student; reference src/training/trainer.py:157 through timm
 * Attention.forward): qkv [B, T, 3, H, hd] bf16, out / dout [B, T, H * hd] bf16 (forward output and its gradient),
 * lse [B, H, T] fp32 from basd_attention_fwd_bf16 -> dqkv [B, T, 3, H, hd] bf16, the gradient of the packed
 * projection.  P is recomputed (nothing T x T is stored); fp32 accumulation, P and dS rounded to bf16 for the second
 * products like a flash kernel.  hd == 64, T <= 224. */
int basd_attention_bwd_bf16(const void* qkv, const void* out, const void* dout, const float* lse, int B, int T, int H,
                            int hd, float scale, void* dqkv, void* stream);

/* Tiled (flash) attention forward for 1 <= T <= 1024, hd 64 | 80: the contract of basd_attention_fwd_bf16 /
 * basd_attention_fwd_qmean_bf16 at token counts they refuse.  qkv [B, T, 3, H, hd] bf16 ->
 *   out [B, T, H * hd] bf16 (nullable: then only the CLS tap is computed), lse [B, H, T] fp32 (nullable unless the
 *   query-mean tap is asked for: it reads the LSE back), cls_importance [B, H, T-1] fp32 (nullable, T >= 2: per head
 *   the CLS-row softmax of basd_cls_importance_bf16 divided by H), qmean_importance [B, H, T] fp32 (nullable, needs out
 *   and lse: per head sum_q softmax(q . k * scale)[q][key] / (H T), summed in a fixed order).
 * The taps are summed over the H axis by the caller.  BASD_ERR_SHAPE outside the range. */
int basd_attention_fwd_long_bf16(const void* qkv, int B, int T, int H, int hd, float scale, void* out,
                                 float* cls_importance, float* qmean_importance, float* lse, void* stream);

/* Tiled (FA2) attention backward for 1 <= T <= 1024, hd 64 | 80: the contract of basd_attention_bwd_bf16 (lse from
 * basd_attention_fwd_bf16 or basd_attention_fwd_long_bf16).  The workspace (workspace_bytes >=
 * basd_attention_bwd_long_workspace_bytes(B, T, H, hd), else BASD_ERR_WORKSPACE) holds delta = rowsum(dO * O) and one
 * fp32 dQ partial per 128-key block, added in key-block order: the result is bitwise reproducible.  No allocation, no
 * synchronisation. */
int64_t basd_attention_bwd_long_workspace_bytes(int B, int T, int H, int hd);
int basd_attention_bwd_long_bf16(const void* qkv, const void* out, const void* dout, const float* lse, int B, int T,
                                 int H, int hd, float scale, void* dqkv, void* workspace, int64_t workspace_bytes,
                                 void* stream);

/* Forward of the attention-weighted Procrustes term between basd_procrustes_prep and the loss value, as one chain of
 * launches on a caller-provided workspace (src/losses/relational.py:47-48: cross = s_w^T t_w, its nuclear norm, and
 * U V^T for the backward; cross is never formed).  s_w [batch, n, d_s], t_w [batch, n, d_t] fp32 (prep outputs);
 * tol: relative stop of the pivoted Cholesky factorisations (1e-13).  Outputs (fp32):
 *   nuc [batch]: nuclear norm of cross;   a_t [batch, n, n]:  s_w (U V^T) = a_t t_w;
 *   fac_s: n > d_s  ("feature side"): [batch, n, d_s] = t_w (U V^T)^T;
 *          n <= d_s ("token side"):   [batch, n, n]   = a_s with t_w (U V^T)^T = a_s s_w.
 * status: device health word (BASD_STATUS_* OR-ed in by the Jacobi solve; nullable).  min(n, d_s) <= 256.
 * basd_procrustes_workspace_bytes gives the workspace size (256-byte aligned scratch; 5 or 10 fp64 [batch, n, n]
 * matrices plus the fp32 Jacobi image). */
int64_t basd_procrustes_workspace_bytes(int batch, int n, int d_s, int d_t);
int basd_procrustes_fwd(const float* s_w, const float* t_w, int batch, int n, int d_s, int d_t, double tol,
                        float* nuc, float* fac_s, float* a_t, int32_t* status, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* Backward of the same term (autograd of src/losses/relational.py:29-48: svd_backward of the nuclear norm = the polar
 * factor, then the centring / weighting), from the factors basd_procrustes_fwd saved.  Per side, with W the weighted
 * tokens [batch, n, d] and fac [batch, n, n] (a_t for the teacher side, a_s for the student side of the token-side form):
 *     out[b, i, :]  = 2 gl[b] sqrt(a[b, i]) (W - fac W)[b, i, :]        (fp32 or bf16)
 *     rowdot[b, i]  = 2 gl[b] <(W - fac W)[b, i, :], W[b, i, :]>
 * in one launch: the product runs on the bf16 matrix cores as a three-product split of both fp32 operands (relative
 * error 2^-16), residual / scaling / row dots in its epilogue.  4 <= n <= 1024, d % 16 == 0, d >= 16; w and out 16-byte
 * aligned.  n <= 256 with n % 4 == 0 (fac 16-byte aligned): one workgroup per matrix; every other n: row tiles of 128
 * rows, one workgroup each (fac 4-byte aligned; 4-byte factor loads when n % 4 != 0 or fac is not 16-byte aligned).  The
 * row dots are summed in a fixed order, without atomics: the results are bitwise reproducible.  BASD_ERR_SHAPE outside
 * the range. */
int basd_procrustes_bwd_side(const float* fac, const float* w, const float* a, const float* gl, int batch, int n, int d,
                             void* out, int out_dtype, float* rowdot, void* stream);

/* The whole backward: s_w [batch, n, d_s], t_w [batch, n, d_t], a [batch, n] (basd_procrustes_prep outputs), gl [batch]
 * (d loss / d value), fac_s / a_t (basd_procrustes_fwd outputs; fac_s is [batch, n, n] when n <= d_s, else
 * [batch, n, d_s]) -> g_s [batch, n, d_s] (g_s_dtype: BASD_DTYPE_F32 | BASD_DTYPE_BF16), g_t [batch, n, d_t] fp32
 * (gradients w.r.t. the RAW student tokens and the resampled teacher tokens), g_a [batch, n] (w.r.t. the normalised
 * importance).  workspace: >= basd_procrustes_bwd_workspace_bytes(batch, n) bytes (the two row-dot vectors).
 * 4 <= n <= 1024 and d_t % 16 == 0; token side (n <= d_s): d_s % 16 == 0, both sides through basd_procrustes_bwd_side;
 * feature side (n > d_s, the only one basd_procrustes_fwd reaches past 256 tokens): d_s % 4 == 0, the student side
 * through basd_procrustes_bwd_rows. */
int64_t basd_procrustes_bwd_workspace_bytes(int batch, int n);
int basd_procrustes_bwd(const float* s_w, const float* t_w, const float* a, const float* gl, const float* fac_s,
                        const float* a_t, int batch, int n, int d_s, int d_t, void* g_s, int g_s_dtype, float* g_t,
                        float* g_a, void* workspace, int64_t workspace_bytes, void* stream);

/* 1-D linear resampling along the token axis, the rule of F.interpolate(mode="linear", align_corners=False) that
 * basd_procrustes_prep applies to the teacher tokens and the importance (reference src/losses/combined.py:9-14).  Output
 * index i of an n_in -> n_out resample has the taps, in fp32 with every operation rounded on its own (no FMA):
 *     pos = max(0, (i + 0.5) * (n_in / n_out) - 0.5),  lo = min((int)pos, n_in - 1),  hi = min(lo + 1, n_in - 1),
 *     fr = pos - lo;    lo = hi = i, fr = 0 when n_in == n_out.
 * x [batch, n_in, d] -> out [batch, n_out, d]:  out[b, i, :] = (1 - fr_i) x[b, lo_i, :] + fr_i x[b, hi_i, :].
 * dtype: BASD_DTYPE_F32 | BASD_DTYPE_BF16, of x and out alike; fp32 arithmetic.  1 <= n_in, n_out <= 1024, d >= 4,
 * d % 4 == 0, batch >= 1; BASD_ERR_SHAPE (nothing launched) outside the range or for a NULL pointer.  16-byte accesses
 * when x and out are 16-byte aligned (bf16: and d % 8 == 0), narrower ones down to one element otherwise.  One launch,
 * no workspace, no host synchronisation. */
int basd_resample_tokens(const void* x, int dtype, int batch, int n_in, int n_out, int d, void* out, void* stream);

/* The adjoint (transpose) of basd_resample_tokens with the same taps: the gradient of an n_in -> n_out resample.
 * g [batch, n_out, d] -> out [batch, n_in, d]:
 *     out[b, j, :] = sum_{i: lo_i = j} (1 - fr_i) g[b, i, :] + sum_{i: hi_i = j, fr_i != 0} fr_i g[b, i, :].
 * Gather form: every output row is summed by one thread per vector in ascending i, without atomics, so the result is
 * bitwise reproducible; a row that no i reaches is written as zeros.  Ranges, dtypes, alignment and errors as above. */
int basd_resample_tokens_adjoint(const void* g, int dtype, int batch, int n_in, int n_out, int d, void* out,
                                 void* stream);

/* The way from basd_procrustes_bwd's g_a back to the importance the caller gave basd_procrustes_prep
 * (src/losses/relational.py:29-33: a = v / sum(v), v = R imp with R the n_t -> n_s resample above, the identity when
 * n_t == n_s).  g_a, a [batch, n_s] (a: the prep output), imp [batch, n_t] -> g_imp [batch, n_t], all fp32:
 *     g_v[i] = (g_a[i] - sum_k a[k] g_a[k]) / sum(R imp),    g_imp = R^T g_v,
 * per sample in fp64 from the fp32 inputs and taps, sums in a fixed order, one rounding at the store.
 * 1 <= n_s, n_t <= 1024, batch >= 1; BASD_ERR_SHAPE (nothing launched) outside the range or for a NULL pointer.
 * A C-only caller finishes the Procrustes backward for any token counts with
 * basd_resample_tokens_adjoint(g_t, BASD_DTYPE_F32, batch, n_t, n_s, d_t, ...) (not needed when n_t == n_s) and this. */
int basd_procrustes_importance_bwd(const float* g_a, const float* a, const float* imp, int batch, int n_s, int n_t,
                                   float* g_imp, void* stream);

/* Cross-entropy with label smoothing on soft targets [B, C] (MixUp / CutMix) or class indices [B] (exactly one of the
 * two non-NULL), its gradient, and the UW-SO combination with the Procrustes term (src/losses/combined.py:57,78-85;
 * nn.CrossEntropyLoss(label_smoothing) of trainer.py:47):  ce = mean_b -sum_c t'_bc log_softmax(z_b)_c,
 * w_ce = (1/ce) / (1/ce + 1/geo), w_geo = 1 - w_ce (detached, clamped at eps), total = w_ce ce + w_geo geo.
 * geo: DEVICE scalar (NULL: plain CE, w_ce = 1).  Outputs: dlogits [B, C] = d total / d logits, out4 = {total, ce,
 * w_ce, w_geo} (device; d total / d geo = w_geo); row_loss [B] is scratch.  All fp32. */
int basd_ce_uwso(const float* logits, const float* soft_targets, const int64_t* labels, int B, int C,
                 float smoothing, const float* geo, float* row_loss, float* dlogits, float* out4, void* stream);

/* Fused Schedule-Free AdamW step (schedulefree 1.4.1 AdamWScheduleFree, train mode;
 * reference src/training/trainer.py:54-58,158-159) over one flat fp32 buffer of n params:
 *   v = b2 v + (1-b2) g^2 ; gn = g / (sqrt(v / bias_correction2) + eps) + wd * y
 *   y = lerp(y, z, ckp1) + lr (b1 (1 - ckp1) - 1) gn ; z = z - lr gn
 * ckp1 / bias_correction2 / lr are the per-step scalars computed on the host. */
int basd_sf_adamw_step(float* y, const float* g, float* z, float* v, int64_t n, double lr,
                       double beta1, double beta2, double eps, double weight_decay, double ckp1,
                       double bias_correction2, void* stream);

/* y <- y + w (z - y): optimizer.train() / optimizer.eval() switch (trainer.py:180,184). */
int basd_lerp(float* y, const float* z, int64_t n, float w, void* stream);

/* Transposed bf16 images of n_entries weight matrices of the flat fp32 master buffer in one launch (the operands of
 * the input-gradient GEMMs dX = dY W of trainer.py:157; refreshed once per step after the optimizer update).
 * table: HOST array of n_entries x {src offset, dst offset, rows, cols} (int64, offsets in elements):
 * out[dst + c * rows + r] = bf16(master[src + r * cols + c]). */
int basd_transpose_bf16_table(const float* master, void* out, const int64_t* table, int n_entries, void* stream);

/* ---- fp32 evaluation forward on split-bf16 products (torch.set_float32_matmul_precision("high"); reference
 * src/training/trainer.py:183-188, src/train.py:153-160, src/eval.py:16).  A SPLIT IMAGE of fp32 values v [rows, k] is
 * a bf16 [rows, 2 k_pad] array: columns [0, k) hold hi = bf16_rne(v), columns [k_pad, k_pad + k) hold
 * lo = bf16_rne(v - hi), the columns up to k_pad of either half are zero.  A product of two images is
 * x_hi w_hi + x_hi w_lo + x_lo w_hi with fp32 accumulation (~16 significand bits). */

/* Images of n_entries fp32 weight matrices in one launch (the nn.Linear / patch-embedding weights of the model, rebuilt
 * every forward).  table: HOST array of n_entries x {src address, dst address, rows, k, k_pad} (int64; addresses of
 * DEVICE memory): dst [rows, 2 k_pad] bf16 = image of src [rows, k] fp32. */
int basd_split_bf16x2_table(const int64_t* table, int n_entries, void* stream);

/* Image of the unfolded patches of x [B, C, H, W] fp32 (non-overlapping p x p; the stride-p Conv2d of the patch
 * embedding as a GEMM): out [B (H/p) (W/p), 2 k_pad] with k = c p p + i p + j, k_pad >= C p p, k_pad % 32 == 0. */
int basd_split_patches_bf16x2(const float* x, int B, int C, int H, int W, int p, int k_pad, void* out, void* stream);

/* nn.Linear in fp32 "high": y = epi(x w^T + bias) from the images x [M, 2 k_pad] and w [N, 2 k_pad] (bf16), bias fp32
 * [N] or NULL.  epilogue 0: y fp32 [M, N]; 1: y = GELU (exact erf) fp32; 2 / 3: the same written as the image
 * y [M, 2 N] bf16 (the next GEMM's input, k_pad = N).  Any M >= 1; N % 16 == 0, k_pad % 32 == 0; 16-byte aligned. */
int basd_gemm_f32x3(const void* x_img, const void* w_img, const float* bias, void* y, int64_t M, int N, int k_pad,
                    int epilogue, void* stream);

/* timm Attention.forward in fp32 "high": softmax(q k^T scale) v from the packed projection qkv [B, T, 3, H, hd] fp32,
 * logits and softmax in fp32, both products on images; out = the image [B T, 2 H hd] of the [B, T, H hd] output (the
 * proj GEMM's input).  hd in {64, 80}, 1 <= T <= 272. */
int basd_attention_fwd_f32x3(const float* qkv, int B, int T, int H, int hd, float scale, void* out_img, void* stream);

/* The same contract (inputs, arithmetic, output image) for 1 <= T <= 1024, hd in {64, 80}, without the T x T state:
 * keys are walked in blocks of 128 with an online softmax (running maximum and sum, rescaled fp32 accumulators), P is
 * split relative to the running maximum and 1 / sum is applied once to the fp32 output.  The blocks are summed in key
 * order: the result is bitwise reproducible.  The whole range is accepted (also T <= 272, where callers normally use
 * the entry above).  No workspace.  BASD_ERR_SHAPE outside the range, checked before anything is enqueued. */
int basd_attention_fwd_f32x3_long(const float* qkv, int B, int T, int H, int hd, float scale, void* out_img,
                                  void* stream);

/* nn.LayerNorm in fp32 with the residual step in front of it: s = residual + xscale * x (residual / xscale NULL: no
 * add / no LayerScale gamma [D]), y = LayerNorm(s) with fp32 statistics.  Outputs (NULL: not written): s_out fp32
 * [rows, D] (may alias residual), y fp32 [rows, D], y_img [rows, 2 D] bf16.  D % 4 == 0, D <= 2048. */
int basd_add_layernorm_fwd_f32(const float* x, const float* residual, const float* xscale, const float* gamma,
                               const float* beta, int64_t rows, int D, float eps, float* s_out, float* y, void* y_img,
                               void* stream);

/* ---- frozen ConvNeXt-V2 teacher trunk (models/convnext.py).  A feature map [B, H, W, C] is a channels-last matrix of
 * B H W bf16 rows with row stride ld >= C (elements); the columns C .. ld are zero (padded layout of the widths the GEMM
 * does not tile: 96 channels in rows of 128).  The pointwise layers are basd_gemm_bf16 on these rows. */

/* Depthwise 7 x 7 convolution (zero padding 3, bias) followed by LayerNorm over the C channels of every output pixel,
 * one launch; the convolution output is never stored.  x [B, H, W, ld_in] bf16, w49 [49, C] bf16 tap-major
 * (w49[(dy * 7 + dx) * C + c] = conv weight[c, 0, dy, dx]), bias / gamma / beta fp32 [C]; fp32 accumulation and two-pass
 * fp32 statistics -> y [B, H, W, ld_out] bf16, columns C .. ld_out written as zero.  Any H, W >= 1; C % 8 == 0,
 * 8 <= C <= 2048; ld % 8 == 0, C <= ld_in, C <= ld_out <= 2 C; 16-byte aligned buffers; y must not alias x.
 * With H = W = 1 and the one-hot centre tap it is LayerNorm over the first C columns of rows of stride ld. */
int basd_dwconv7_ln_bf16(const void* x, const void* w49, const float* bias, const float* gamma, const float* beta,
                         int B, int H, int W, int C, int ld_in, int ld_out, float eps, void* y, void* stream);

/* Global response normalisation of ConvNeXt-V2, in place on x [B, HW, C] bf16 (contiguous; fc1's output):
 *   g[b, c] = ||x[b, :, c]||_2,  n = g / (mean_c g + eps),  x <- bf16(x + bias + weight x n),  weight / bias fp32 [C].
 * Two launches: sums of squares in fp32 into the workspace (>= basd_grn_workspace_bytes(B, HW, C) bytes, else
 * BASD_ERR_WORKSPACE; fixed summation order, no atomics), then the apply pass.  C % 8 == 0, 8 <= C <= 4096. */
int64_t basd_grn_workspace_bytes(int B, int HW, int C);
int basd_grn_bf16(void* x, const float* weight, const float* bias, int B, int HW, int C, float eps, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* Non-overlapping p x p patches of a bf16 image / feature map as GEMM rows (a stride-p, kernel-p convolution is the
 * GEMM of these rows with the re-laid weight).  x is addressed through ELEMENT strides (sb, sc, sh, sw) of its
 * [B, C, H, W] index, so NCHW and channels-last sources (and padded rows: C = ld) are the same call:
 *   out[(b (H/p) + oh) (W/p) + ow, (i p + j) C + c] = x[b, c, oh p + i, ow p + j],  columns C p p .. K_pad zero.
 * H % p == 0, W % p == 0, K_pad % 8 == 0, K_pad >= C p p; out 16-byte aligned.  Exact (a copy). */
int basd_patchify_bf16(const void* x, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                       int p, int K_pad, void* out, void* stream);

/* ---- frozen ResNet teacher trunk (models/cnn.py, ResNet-v1.5 bottlenecks with BatchNorm folded into weight and bias).
 * Activations use the channels-last rows of the ConvNeXt section above: [B, H, W, ld] bf16, columns C .. ld zero on
 * output and never read on input (a 64-channel map lives in rows of 128, the narrowest N of basd_gemm_bf16); 16-byte
 * aligned buffers.  The 1 x 1 convolutions are basd_gemm_bf16 on these rows, the strided one behind
 * basd_patchify_bf16 at p = 1 on the [:, :, ::2, ::2] view. */

/* 3 x 3 convolution, zero padding 1, stride 1 or 2, C -> C channels, as an implicit GEMM on the bf16 matrix cores
 * (fp32 accumulation, one rounding at the store; the im2col matrix is never stored):
 *   y[b, oh, ow, n] = epi(sum_{dy, dx, c} in(x[b, oh s + dy - 1, ow s + dx - 1, c]) w9[n][(dy 3 + dx) C + c] + bias[n])
 * x [B, H, W, ld_in], w9 [C, 9 C] bf16 tap-major, bias [C] bf16, y [B, Ho, Wo, ld_out] with Ho = (H - 1) / s + 1.
 * relu_in != 0: in = max(0, .) on every input element as it is staged (the 1 x 1 convolution in front stays a plain
 * GEMM + bias); relu_out != 0: epi = max(0, .) before the bf16 rounding.  C % 64 == 0, 64 <= C <= 512; any H, W >= 1;
 * ld % 8 == 0, C <= ld_in, C <= ld_out <= 2 C; B Ho Wo <= 0x7fffff00 output pixels (the kernel decodes pixel indices
 * in int); y must not alias x. */
int basd_conv3x3_bf16(const void* x, const void* w9, const void* bias, int B, int H, int W, int C, int stride,
                      int ld_in, int ld_out, int relu_in, int relu_out, void* y, void* stream);

/* The stem: 7 x 7 convolution, padding 3, stride 2, 3 -> 64 channels, + bias, ReLU.  x [B, 3, H, W] bf16 addressed
 * through ELEMENT strides (sb, sc, sh, sw) as in basd_patchify_bf16 (NCHW and channels-last are the same call),
 * w [64, K_pad] bf16 with column (dy 7 + dx) 3 + c and zero columns behind 147 (K_pad % 8 == 0, K_pad >= 160),
 * bias [64] bf16 -> y [B, H1, W1, ld_out], H1 = (H - 1) / 2 + 1, 64 <= ld_out <= 128, ld_out % 8 == 0. */
int basd_conv7x7s2_relu_bf16(const void* x, const void* w, const void* bias, int B, int H, int W, int64_t sb,
                             int64_t sc, int64_t sh, int64_t sw, int K_pad, int ld_out, void* y, void* stream);

/* 3 x 3 max pool, stride 2, padding 1 (the padding never wins): x [B, H, W, ld_in] -> y [B, Ho, Wo, ld_out],
 * Ho = (H - 1) / 2 + 1.  Exact.  C % 8 == 0, ld % 8 == 0, C <= ld; y must not alias x. */
int basd_maxpool3x3s2_bf16(const void* x, int B, int H, int W, int C, int ld_in, int ld_out, void* y, void* stream);

/* The end of a bottleneck block, in place:  y <- bf16(max(0, float(y) + float(r)))  on rows x C with row strides
 * ld_y, ld_r (elements; the columns behind C are not touched).  C % 8 == 0, ld % 8 == 0, C <= ld. */
int basd_add_relu_bf16(void* y, const void* r, int64_t rows, int C, int ld_y, int ld_r, void* stream);

/* ---- frozen Swin teacher trunk (models/swin.py).  Token grids use the channels-last rows of the ConvNeXt section above:
 * [B, H, W, ld] bf16, columns C .. ld zero on output and never read on input; 16-byte aligned buffers.  The linear layers
 * are basd_gemm_bf16 on these rows, the LayerNorms basd_layernorm_fwd_bf16 / basd_add_layernorm_fwd_bf16 (ld == C) or
 * basd_dwconv7_ln_bf16 at H = W = 1 (ld > C). */

/* (Shifted-)window attention of one Swin block, from the packed qkv rows into the rows the output projection reads:
 *   out[token] = softmax_keys(scale q . k + bias[head][slot_q][slot_k] + mask) v   per window and head, head dim 32.
 * qkv [B, H, W, ld_qkv] bf16 with q | k | v in the first 3 C columns, each laid out [heads, 32] (the columns behind 3 C
 * are never read); out [B, H, W, ld_out] bf16, head h in columns 32 h .. 32 h + 31, columns C .. ld_out written as zero.
 * The cyclic roll by -shift, the partition into ws x ws windows and their inverses are index arithmetic: slot
 * iy ws + ix of window (wy, wx) is token ((wy ws + iy + shift) mod H, (wx ws + ix + shift) mod W), on the loads and on the
 * store; no rolled or partitioned copy exists.  mask (shift > 0 only): every slot carries the label 3 ly + lx of its
 * ROLLED coordinate (wy ws + iy, wx ws + ix), with l = 0 on [0, n - ws), 1 on [n - ws, n - shift), 2 on [n - shift, n)
 * per axis of length n; a pair of slots with different labels gets -100.0 added (not -inf).
 * bias: the IMAGE fp32 [heads, 64, 64], entry [h][i][j] = relative-position bias of query slot i and key slot j for
 * i, j < ws^2 (table[index[i][j]][h]); the rest of a 64 x 64 plane must be allocated and is ignored.
 * Arithmetic: bf16 products with fp32 accumulation, fp32 logits and softmax (maximum subtracted), probabilities rounded
 * to bf16 for the second product, fp32 accumulation, one rounding at the store.  Slots behind ws^2 of the 64-slot tile
 * enter no softmax and are not stored.
 * 1 <= ws <= 8, 0 <= shift < ws, H % ws == 0, W % ws == 0, C == 32 heads, ld % 8 == 0, 3 C <= ld_qkv, C <= ld_out; out
 * must not alias qkv.  Anything else is BASD_ERR_SHAPE without a launch. */
int basd_window_attention_fwd_bf16(const void* qkv, const float* bias, int B, int H, int W, int heads, int C, int ws,
                                   int shift, int ld_qkv, int ld_out, float scale, void* out, void* stream);

/* The same attention for windows of 9 x 9 to 16 x 16 slots (window 12 of the 384 px Swin checkpoints), which the entry
 * above refuses: rows, roll / partition index arithmetic, label mask (-100.0 in fp32), rounding points (fp32 logits
 * fmaf(q . k, scale, bias) + mask, fp32 softmax over the whole row, probabilities rounded to bf16, one rounding at the
 * store) and the zero pad columns of out are exactly those of basd_window_attention_fwd_bf16.
 * table: timm's relative_position_bias_table itself, fp32 [(2 ws - 1)^2, heads] (NOT an expanded image); the logit of
 * query slot (iy_q, ix_q) and key slot (iy_k, ix_k) reads row (iy_q - iy_k + ws - 1)(2 ws - 1) + (ix_q - ix_k + ws - 1).
 * One workgroup of four waves per (window, head); no atomics: the same input gives the same bits.
 * 9 <= ws <= 16, 0 <= shift < ws, H % ws == 0, W % ws == 0, C == 32 heads, ld % 8 == 0, 3 C <= ld_qkv, C <= ld_out,
 * 16-byte aligned buffers, B (H / ws)(W / ws) heads < 2^31; out must not alias qkv.  Anything else is BASD_ERR_SHAPE
 * without a launch. */
int basd_window_attention_fwd_wide_bf16(const void* qkv, const float* table, int B, int H, int W, int heads, int C,
                                        int ws, int shift, int ld_qkv, int ld_out, float scale, void* out, void* stream);

/* Patch merging + LayerNorm: x [B, H, W, ld_in] bf16 with C channels -> y [B, H/2, W/2, 4 C] bf16 (contiguous),
 *   y[b, r, c, :] = LayerNorm_{4 C}(concat(x[b, 2r, 2c], x[b, 2r+1, 2c], x[b, 2r, 2c+1], x[b, 2r+1, 2c+1])),
 * gamma / beta fp32 [4 C], two-pass fp32 statistics in a fixed summation order (the same input gives the same bits).
 * C % 8 == 0, 8 <= 4 C <= 4096, H and W even, ld_in % 8 == 0, C <= ld_in; y must not alias x. */
int basd_patch_merge_ln_bf16(const void* x, const float* gamma, const float* beta, int B, int H, int W, int C, int ld_in,
                             float eps, void* y, void* stream);

/* ---- both training views from one uint8 batch (data/device_views.py).  The CPU functions of data/transforms.py are the
 * definition, stage by stage. */

/* Window -> antialiased bilinear resize -> offset crop -> horizontal flip, uint8 in and out.  src [B, 3, H, W] uint8
 * (contiguous); rec [B, 9] int32 on the device, per sample
 *   {top, left, h, w}   the source window inside the H x W canvas (the sample's own size for the clean view),
 *   {nh, nw}            the size the window is resized to (virtual: only the S x S part below is computed),
 *   {off_y, off_x}      the output's offset inside that resized image,
 *   flip                non-zero: the S x S output is mirrored horizontally;
 * out [B, 3, S, S] uint8, 4-byte aligned, written as packed 32-bit words.  The arithmetic is that of
 * F.interpolate(mode="bilinear", antialias=True, align_corners=False) on the fp32 window (separable triangle filter,
 * scale = n_in / n_out, support = max(scale, 1), weights normalised per output index, the horizontal pass first with an
 * fp32 value between the passes), then round-half-even and a clamp to 0 .. 255: against the CPU at most one level off at
 * fp32 near-ties, and exact where a window has the output's size.  Clean view: window = the image, (nh, nw) =
 * Resize(int)'s size, offset = CenterCrop's; augmented view: window = the RandomResizedCrop, (nh, nw) = (S, S), offset 0.
 * Every index is clamped into the canvas and the resized image: a bad record cannot read out of bounds.
 * 3 <= S <= 1024, 1 <= H, W <= 16384. */
int basd_resample_u8(const void* src, const int* rec, int B, int H, int W, int S, void* out, void* stream);

/* basd_resample_u8 for samples of different sizes.  pixels: one flat uint8 device buffer of pixels_bytes bytes; sample b
 * is a planar [3, h_b, w_b] image that starts at byte geom[b][0].  geom [B, 3] int64 on the device: {offset, h, w}.
 * rec [B, 9] int32 as above, its canvas being the sample's own h_b x w_b.  out [B, 3, S, S] uint8, 4-byte aligned (odd S
 * leaves a sample's first byte unaligned: byte head and tail, 32-bit words between).  Per output byte the arithmetic is
 * that of basd_resample_u8 with (H, W) = (h_b, w_b): bit-equal to that entry run on the sample alone.
 * One workgroup per (sample, band of 16 output rows), all three channels: the taps of the S columns and of the band's
 * rows (window start, count, weight sum, the first 8 normalised weights) are built once per workgroup in LDS,
 * 44 (S + 16) bytes; wider filters recompute the weights past the eighth.
 * A sample is read only if offset >= 0, 1 <= h, w <= 16384 and offset + 3 h w <= pixels_bytes (64-bit arithmetic);
 * otherwise nothing of it is read and its output is all zeros.  Record fields are clamped as in basd_resample_u8.
 * Allocates nothing and does not synchronise.  3 <= S <= 1024; B < 0, a null pointer or a negative pixels_bytes is
 * BASD_ERR_SHAPE. */
int basd_resample_u8_packed(const void* pixels, int64_t pixels_bytes, const int64_t* geom, const int* rec, int B, int S,
                            void* out, void* stream);

/* One TrivialAugmentWide operation per image, then ToDtype(float32, scale=True) and Normalize: img [B, 3, S, S] uint8,
 * ops [B] int32 (index into TA_WIDE_OPS: Identity, ShearX, ShearY, TranslateX, TranslateY, Rotate, Brightness, Color,
 * Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize; anything else is Identity) and mags [B] fp64 (the
 * signed magnitude apply_ta_op is called with), both on the device; ops NULL: Identity for every image (the clean
 * view; mags is then not read).  out [B, 3, S, S] fp32, 16-byte aligned, = ((op(img) / 255) - mean_c) / std_c.
 * One workgroup per image: the reductions its operation needs in LDS (fp32 gray mean for Contrast, per-channel min / max
 * for AutoContrast, per-channel 256-bin histogram and integer LUT for Equalize), then 16-byte stores with a scalar head
 * and tail.  The affine coordinates and the blends keep the CPU's fp32 operation order (no contraction).
 * 3 <= S <= 1024. */
int basd_ta_normalize_u8(const void* img, const int* ops, const double* mags, int B, int S, float mean0, float mean1,
                         float mean2, float std0, float std1, float std2, float* out, void* stream);

/* Evaluation tally of one batch (reference src/evaluation/metrics.py:19-55): logits [B, C] fp32 (logits_bf16 == 0) or
 * bf16 (!= 0), rows row_stride >= C ELEMENTS apart; keep: K distinct column indices in [0, C), any order (the class
 * subset outputs[:, valid_indices]), or NULL with K == C for the identity; labels [B] index the SUBSET, so the target
 * column is keep[labels[b]].  Per row, with z_j = logits[b, keep[j]], y = labels[b] and s = smoothing (taken as the
 * float it is passed as), all in fp64 on the values as stored:
 *   rank = #{j : z_j > z_y} + #{j < y : z_j == z_y}   -- a tie goes to the lowest subset position (argmax's rule); NaN
 *                                                        orders above every number and equal to NaN (topk's rule);
 *   loss = lse(z) - (1 - s) z_y - (s / K) sum_j z_j   -- nn.CrossEntropyLoss(label_smoothing = s, reduction = "none");
 *                                                        the last term only when s != 0, so a -inf logit away from
 *                                                        the target is legal at s = 0 and adds 0 to lse;
 *   lse(z) = m + log(sum_j exp(z_j - m)), m = the largest non-NaN z_j, or 0 where that is infinite.
 * A label outside [0, K) reads nothing and gives rank = K (a miss at every k) and loss = NaN; a keep entry outside
 * [0, C) reads nothing and counts as a NaN logit.
 * Outputs: row_rank [B] int32 and row_loss [B] fp64 (both required: they are the staging area), and tally [4] fp64,
 * ADDED TO in place: {#(rank == 0), #(rank < top_k), sum_b loss, B}.  1 <= top_k <= K.  Two launches: one workgroup per
 * row, then one workgroup that sums the rows in a fixed order; no floating-point atomics, so the tally is bitwise
 * reproducible.  B == 0 is BASD_OK with nothing enqueued and tally untouched.  BASD_ERR_SHAPE (nothing enqueued): top_k
 * outside 1 .. K, keep NULL with K != C, row_stride < C, a non-positive C or K, a missing pointer.  No allocation: legal
 * inside a stream capture. */
int basd_cls_tally(const void* logits, int logits_bf16, int64_t row_stride, const int64_t* labels,
                   const int64_t* keep, int B, int C, int K, int top_k, float smoothing, int* row_rank,
                   double* row_loss, double* tally, void* stream);

/* MixUp or CutMix of one batch with its soft targets (reference src/training/trainer.py:89-92,138, torchvision v2's
 * RandomChoice([MixUp, CutMix])): images [B, C_img, H, W] contiguous, fp32 (img_bf16 == 0) or bf16 (!= 0); labels [B]
 * int64 on the device; out_images like images, out_targets [B, num_classes] fp32.  The random draws (mode, lam, box) are
 * the caller's, on the host.  The partner of sample i is sample (i - 1) mod B; the rolled batch is never materialised.
 *   mode 0, MixUp:   out_images[i] = lerp(x[i-1], x[i], lam) with torch's formula in fp32, a + w (b - a) for |w| < 0.5,
 *                    b - (b - a) (1 - w) otherwise; bf16 images are blended in fp32 and rounded once, to nearest even.
 *                    lam = 0 / 1 returns x[i-1] / x[i] exactly.
 *   mode 1, CutMix:  out_images[i] = x[i-1] on rows y0 .. y1 - 1, columns x0 .. x1 - 1 of every channel and x[i]
 *                    elsewhere: bit copies, every pixel written exactly once.  The box is half-open and already clipped,
 *                    0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W; an empty box copies the images through (lam is then 1).
 *                    lam is the weight of the TARGETS only, 1 - box area / (H W).  The box is ignored in mode 0.
 *   targets:         out_targets[i, c] = lerp(onehot(y[i-1])[c], onehot(y[i])[c], lam), same formula: every element of
 *                    the B x num_classes buffer is written, zeros included; y[i] == y[i-1] gives exactly 1.  A label
 *                    outside [0, num_classes) matches no column and writes nothing out of bounds.
 * One launch: up to 2048 workgroups walk the flat image array in 16-byte vectors (one-element vectors when images /
 * out_images are not 16-byte aligned; element loads of the partner when C_img H W is no multiple of the vector; the
 * elements behind the last whole vector one by one), a CutMix vector reading only the source(s) its pixels come from;
 * min(B, 256) workgroups behind them write the target rows.  No workspace, no allocation, no synchronisation: legal
 * inside a stream capture.  BASD_ERR_SHAPE, checked on the host before anything is enqueued: B < 1, num_classes < 1, an
 * empty image, C_img H W >= 2^31, mode outside {0, 1}, a box outside [0, H] x [0, W] (mode 1), a null pointer, a pointer
 * not aligned to its element, or out_images overlapping images (the partner row would be read after it was written). */
int basd_mixup_cutmix(const void* images, int img_bf16, int B, int C_img, int H, int W, const int64_t* labels,
                      int num_classes, int mode, float lam, int y0, int y1, int x0, int x1, void* out_images,
                      float* out_targets, void* stream);

/* Gradient of the selector term with respect to the E tapped student token tensors (the loop at the end of
 * _SelectorWeightsFn.backward: sf = s.float(); row = -(sf.mean(0) @ W); addmm(row, sf, W).to(bf16)), all taps in one
 * call:   out_e[b, n, :] = bf16((s_e[b, n, :] - mean_e) W_e),   mean_e = the column mean of s_e over all B N rows.
 * tokens: HOST array of E device pointers to bf16 [B, N, D_s] views (sample b at + b * batch_stride elements, rows
 * dense; the CLS-stripped block outputs are consumed in place), w [E, D_s, D_s] fp32, out: HOST array of E device
 * pointers to contiguous bf16 [B, N, D_s] tensors.  Column sums in fp64; the centring is applied after the product
 * (s W - mean W); the product runs on the bf16 matrix cores over a three-way bf16 split of W with fp32 accumulation
 * (s is exact in bf16).  Two launches on `stream`, no allocation, no synchronisation, legal inside a stream capture.
 * D_s in {192, 384, 768}, 1 <= E <= 8, batch_stride % 8 == 0, B * batch_stride < 2^31, every pointer 16-byte aligned
 * (BASD_ERR_SHAPE);
 * workspace >= basd_selector_token_grad_workspace_bytes(E, D_s) bytes, 16-byte aligned (BASD_ERR_WORKSPACE). */
int64_t basd_selector_token_grad_workspace_bytes(int E, int D_s);
int basd_selector_token_grad(const void* const* tokens, int E, int B, int N, int D_s, int64_t batch_stride,
                             const float* w, void* const* out, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* Backward of a token tap out[:, offset:, :] of a block output [B, T, D_s] (offset 1 strips the CLS token, 0 = none),
 * everything autograd did around it in one pass:   out = g_out (+) pad(g_a (+) g_b),   all bf16.
 * g_out [B, T, D_s] (gradient of the block output; NULL = zero), g_a, g_b [B, T - offset, D_s] contiguous (gradients
 * of the token view; either may be NULL), out [B, T, D_s].  Rounding as autograd's chain of bf16 adds:
 * r = bf16(float(g_a) + float(g_b)), out = bf16(float(g_out) + float(r)) on rows offset .. T - 1; rows below offset
 * are copies of g_out; an absent operand is skipped, not added as zero.  One launch of 16-byte accesses on `stream`.
 * D_s % 64 == 0, 0 <= offset < T, pointers 16-byte aligned (BASD_ERR_SHAPE). */
int basd_tap_grad_scatter(const void* g_out, const void* g_a, const void* g_b, int B, int T, int D_s, int offset,
                          void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BASD_HIP_H */
