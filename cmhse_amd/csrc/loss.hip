// loss.hip — the training losses, forward and backward: every entry point between the
// encoder outputs and their gradients.
//
//   cmhse_contrastive_fwd / _bwd          loss.ContrastiveLoss (/root/reference/loss.py:86-117) from the
//                                         stored score matrix; _blocks_: several losses in one launch set
//   cmhse_groupwise_fwd / _bwd            loss.GroupWiseContrastiveLoss (loss.py:26-41)
//   cmhse_step_losses_fwd / _bwd          F.normalize + the step's contrastive terms + their weighted total
//   cmhse_euclid_fwd / _bwd               decoder.loss.EuclideanLoss
//   cmhse_l2norm_rows_bwd                 F.normalize backward (the forward is gru.hip's cmhse_l2norm_rows)
//
// The scores come from sim.hip's stored-score GEMM (sim_store.hpp), d im = G . s and d s = G^T . im
// from the TN product of tn_core.hpp; the kernels of this file are in loss_kernels.hpp, its workspace
// layouts in loss_layout.hpp.  Determinism: every reduction runs in a fixed order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "gru_ws.hpp"
#include "nt_core.hpp"
#include "tn_core.hpp"
#include "norm_rows.hpp"
#include "sim_store.hpp"
#include "loss_layout.hpp"

#include "loss_kernels.hpp"

namespace cmhse {

// contrastive_partial_kernel + contrastive_final_kernel over n_blocks stored score matrices of up to
// n rows (blk_off == nullptr: the single n x n matrix)
static int launch_contrastive_reduce(const float* scores, int n, const LossFwdLayout& L, void* workspace,
                                     float margin, int max_violation, int norm, float* loss,
                                     const int32_t* blk_off, int n_blocks, int64_t blk_stride,
                                     hipStream_t stream) {
  LossParams lp;
  lp.scores = scores;
  lp.n = n;
  lp.nrb = L.nrb;
  lp.margin = margin;
  lp.max_violation = max_violation;
  lp.norm = norm;
  lp.partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + L.partial);
  lp.loss = loss;
  lp.blk_off = blk_off;
  lp.blk_stride = blk_stride;
  hipLaunchKernelGGL(contrastive_partial_kernel, dim3(2 * lp.nrb, n_blocks), dim3(kThreads), 0, stream, lp);
  hipLaunchKernelGGL(contrastive_final_kernel, dim3(1, n_blocks), dim3(64), 0, stream, lp);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

// loss_bwd_stats_kernel + loss_bwd_build_kernel into the gradient block L at ws: G = d loss / d scores
// and G^T of n_blocks losses of up to n rows (blk_off == nullptr: the single loss).  Block b's stored
// scores start b * score_stride floats into `scores`, its upstream gradient is gout[b].
static LossBwdParams launch_loss_grad(const LossGradLayout& L, char* ws, const float* scores,
                                      const float* gout, int n, float margin, int max_violation,
                                      int norm, const int32_t* blk_off, int n_blocks,
                                      int64_t score_stride, hipStream_t st) {
  LossBwdParams q;
  q.scores = scores; q.gout = gout; q.n = n; q.max_violation = max_violation; q.norm = norm;
  q.margin = margin;
  q.G = reinterpret_cast<float*>(ws + L.G);
  q.GT = reinterpret_cast<float*>(ws + L.GT);
  q.row_arg = reinterpret_cast<int32_t*>(ws + L.row_arg);
  q.col_arg = reinterpret_cast<int32_t*>(ws + L.col_arg);
  q.row_cnt = reinterpret_cast<float*>(ws + L.row_cnt);
  q.col_cnt = reinterpret_cast<float*>(ws + L.col_cnt);
  q.blk_off = blk_off;
  q.blk_stride = L.blk_stride;
  q.score_stride = score_stride;
  q.vec_stride = L.vec_stride;
  hipLaunchKernelGGL(loss_bwd_stats_kernel, dim3((2 * n + 3) / 4, n_blocks), dim3(kThreads), 0, st, q);
  const int64_t elems = static_cast<int64_t>(n) * n;
  hipLaunchKernelGGL(loss_bwd_build_kernel,
                     dim3(static_cast<unsigned>((elems + kThreads - 1) / kThreads), n_blocks),
                     dim3(kThreads), 0, st, q);
  return q;
}

}  // namespace cmhse

using namespace cmhse;

extern "C" int cmhse_l2norm_rows_bwd(const float* x, const float* g, float* dx, int32_t rows,
                                     int32_t cols, void* stream_) {
  if (!x || !g || !dx || rows < 0 || cols <= 0) return CMHSE_ERR_ARG;
  if (rows == 0) return CMHSE_OK;
  hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(rows), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream_), x, g, dx, cols);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

// ContrastiveLoss over n_blocks row blocks of up to n rows (blk_off == nullptr: the single n x n loss,
// whose scores may go to scores_out): the stored scores, then their reduction
static int contrastive_fwd(const float* im, const float* s, const int32_t* blk_off, int n_blocks, int n, int D,
                           float margin, int max_violation, int norm, float* loss, float* scores_out,
                           void* workspace, size_t workspace_bytes, void* stream_) {
  const LossFwdLayout L = contrastive_fwd_layout(n_blocks, n);
  if (!ws_ok(workspace, workspace_bytes, L.bytes)) return CMHSE_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  // the stored scores the backward reads: block b at scores + b * n * n, leading dimension = its own size
  float* scores = scores_out ? scores_out : reinterpret_cast<float*>(static_cast<char*>(workspace) + L.scores);
  const int64_t blk_stride = static_cast<int64_t>(n) * n;
  const int rc = launch_sim_store(im, s, n, n, D, scores, stream, blk_off, n_blocks, blk_stride);
  if (rc != CMHSE_OK) return rc;
  return launch_contrastive_reduce(scores, n, L, workspace, margin, max_violation, norm, loss, blk_off, n_blocks,
                                   blk_stride, stream);
}

// ... and its backward from those stored scores: G and G^T, then d im = G . s and d s = G^T . im
static int contrastive_bwd(const float* im, const float* s, const float* scores, const int32_t* blk_off,
                           int n_blocks, int n, int D, float margin, int max_violation, int norm,
                           const float* grad_out, float* d_im, float* d_s, void* workspace,
                           size_t workspace_bytes, void* stream_) {
  const LossGradLayout L = loss_grad_layout(n_blocks, n);
  if (!ws_ok(workspace, workspace_bytes, L.bytes)) return CMHSE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const LossBwdParams q = launch_loss_grad(L, static_cast<char*>(workspace), scores, grad_out, n, margin,
                                           max_violation, norm, blk_off, n_blocks, static_cast<int64_t>(n) * n, st);
  // (blocks of different sizes: always the scalar-load form)
  const bool vec = blk_off == nullptr && (n % 4 == 0) && (D % 4 == 0);
  // d im[i][d] = sum_j G[i][j] s[j][d]  = TN(A = G^T, B = s);  d s[j][d] = sum_i G[i][j] im[i][d]
  launch_tn(q.GT, n, s, D, nullptr, d_im, D, n, D, n, nullptr, vec, st, blk_off, n_blocks, q.blk_stride);
  launch_tn(q.G, n, im, D, nullptr, d_s, D, n, D, n, nullptr, vec, st, blk_off, n_blocks, q.blk_stride);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" size_t cmhse_contrastive_workspace(int32_t n) {
  return n <= 0 ? 0 : contrastive_fwd_layout(1, n).bytes;
}

extern "C" int cmhse_contrastive_fwd(const float* im, const float* s, int32_t n, int32_t D,
                                     float margin, int32_t max_violation, int32_t norm,
                                     float* loss, float* scores_out, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
  if (!im || !s || !loss || !workspace || n <= 0 || D <= 0) return CMHSE_ERR_ARG;
  return contrastive_fwd(im, s, nullptr, 1, n, D, margin, max_violation, norm, loss, scores_out, workspace,
                         workspace_bytes, stream_);
}

extern "C" size_t cmhse_contrastive_bwd_workspace(int32_t n) {
  return n <= 0 ? 0 : loss_grad_layout(1, n).bytes;
}

extern "C" int cmhse_contrastive_bwd(const float* im, const float* s, const float* scores,
                                     int32_t n, int32_t D, float margin, int32_t max_violation,
                                     int32_t norm, const float* grad_out, float* d_im, float* d_s,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
  if (!im || !s || !scores || !grad_out || !d_im || !d_s || !workspace || n <= 0 || D <= 0)
    return CMHSE_ERR_ARG;
  return contrastive_bwd(im, s, scores, nullptr, 1, n, D, margin, max_violation, norm, grad_out, d_im, d_s,
                         workspace, workspace_bytes, stream_);
}

extern "C" size_t cmhse_contrastive_blocks_workspace(int32_t n_blocks, int32_t max_n) {
  return (n_blocks <= 0 || max_n <= 0) ? 0 : contrastive_fwd_layout(n_blocks, max_n).bytes;
}

extern "C" int cmhse_contrastive_blocks_fwd(const float* im, const float* s,
                                            const int32_t* blk_off, int32_t n_blocks,
                                            int32_t max_n, int32_t D, float margin,
                                            int32_t max_violation, int32_t norm, float* losses,
                                            void* workspace, size_t workspace_bytes,
                                            void* stream_) {
  if (!im || !s || !blk_off || !losses || !workspace || n_blocks <= 0 || max_n <= 0 || D <= 0)
    return CMHSE_ERR_ARG;
  if (n_blocks > 65535) return CMHSE_ERR_UNSUPPORTED;
  return contrastive_fwd(im, s, blk_off, n_blocks, max_n, D, margin, max_violation, norm, losses, nullptr,
                         workspace, workspace_bytes, stream_);
}

extern "C" size_t cmhse_contrastive_blocks_bwd_workspace(int32_t n_blocks, int32_t max_n) {
  return (n_blocks <= 0 || max_n <= 0) ? 0 : loss_grad_layout(n_blocks, max_n).bytes;
}

extern "C" int cmhse_contrastive_blocks_bwd(const float* im, const float* s, const float* scores,
                                            const int32_t* blk_off, int32_t n_blocks, int32_t max_n,
                                            int32_t D, float margin, int32_t max_violation,
                                            int32_t norm, const float* grad_out, float* d_im,
                                            float* d_s, void* workspace, size_t workspace_bytes,
                                            void* stream_) {
  if (!im || !s || !scores || !blk_off || !grad_out || !d_im || !d_s || !workspace || n_blocks <= 0 ||
      max_n <= 0 || D <= 0)
    return CMHSE_ERR_ARG;
  if (n_blocks > 65535) return CMHSE_ERR_UNSUPPORTED;
  return contrastive_bwd(im, s, scores, blk_off, n_blocks, max_n, D, margin, max_violation, norm, grad_out,
                         d_im, d_s, workspace, workspace_bytes, stream_);
}

extern "C" size_t cmhse_step_losses_workspace(const cmhse_step_losses* d) {
  StepLossLayout L;
  return step_loss_layout(d, &L) ? L.bytes : 0;
}

extern "C" int cmhse_step_losses_fwd(const cmhse_step_losses* d, float* values, float* total,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
  StepLossLayout L;
  if (!values || !total || !workspace || !step_loss_layout(d, &L)) return CMHSE_ERR_ARG;
  for (int e = 0; e < d->n_emb; ++e)
    if (!d->x[e]) return CMHSE_ERR_ARG;
  if (!ws_ok(workspace, workspace_bytes, L.bytes)) return CMHSE_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  StepNormParams p = {};
  for (int k = 0; k < d->n_terms; ++k) {
    p.src[0][k] = d->x[d->term_a[k]];
    p.src[1][k] = d->x[d->term_b[k]];
    p.n[k] = d->rows[d->term_a[k]];
    p.weight[k] = d->weight[k];
  }
  p.n_terms = d->n_terms;
  p.D = d->D;
  p.R = L.R;
  p.y[0] = reinterpret_cast<float*>(ws + L.y_im);
  p.y[1] = reinterpret_cast<float*>(ws + L.y_s);
  p.blk_off = reinterpret_cast<int32_t*>(ws + L.blk_off);
  hipLaunchKernelGGL(step_norm_kernel, dim3(2u * L.R), dim3(kThreads), 0, stream, p);
  const int rc = cmhse_contrastive_blocks_fwd(
      p.y[0], p.y[1], p.blk_off, d->n_terms, L.max_n, d->D, d->margin, d->max_violation, d->norm,
      values, ws + L.fwd_ws, cmhse_contrastive_blocks_workspace(d->n_terms, L.max_n), stream_);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(step_total_kernel, dim3(1), dim3(64), 0, stream, p, values, total);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" int cmhse_step_losses_bwd(const cmhse_step_losses* d, const float* grad_total,
                                     float* const* dx, void* workspace, size_t workspace_bytes,
                                     void* stream_) {
  StepLossLayout L;
  if (!grad_total || !dx || !workspace || !step_loss_layout(d, &L)) return CMHSE_ERR_ARG;
  if (!ws_ok(workspace, workspace_bytes, L.bytes)) return CMHSE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  StepNormBwdParams p = {};
  int64_t total_rows = 0;
  for (int e = 0; e < d->n_emb; ++e) {
    if (!d->x[e] || !dx[e]) return CMHSE_ERR_ARG;
    p.x[e] = d->x[e];
    p.dx[e] = dx[e];
    p.rows[e] = d->rows[e];
    total_rows += d->rows[e];
  }
  if (total_rows > 0x7fffffffLL) return CMHSE_ERR_UNSUPPORTED;
  int32_t off = 0;
  for (int k = 0; k < d->n_terms; ++k) {
    p.term_a[k] = d->term_a[k];
    p.term_b[k] = d->term_b[k];
    p.term_off[k] = off;
    p.weight[k] = d->weight[k];
    off += d->rows[d->term_a[k]];
  }
  p.n_emb = d->n_emb;
  p.n_terms = d->n_terms;
  p.D = d->D;
  float* d_im = reinterpret_cast<float*>(ws + L.d_im);
  float* d_s = reinterpret_cast<float*>(ws + L.d_s);
  p.d_im = d_im;
  p.d_s = d_s;
  float* gout = reinterpret_cast<float*>(ws + L.gout);
  hipLaunchKernelGGL(step_gout_kernel, dim3(1), dim3(64), 0, st, p, grad_total, gout);
  const int rc = cmhse_contrastive_blocks_bwd(
      reinterpret_cast<const float*>(ws + L.y_im), reinterpret_cast<const float*>(ws + L.y_s),
      reinterpret_cast<const float*>(ws + L.fwd_ws), reinterpret_cast<const int32_t*>(ws + L.blk_off),
      d->n_terms, L.max_n, d->D, d->margin, d->max_violation, d->norm, gout, d_im, d_s,
      ws + L.bwd_ws, cmhse_contrastive_blocks_bwd_workspace(d->n_terms, L.max_n), stream_);
  if (rc != CMHSE_OK) return rc;
  hipLaunchKernelGGL(step_norm_bwd_kernel, dim3(static_cast<unsigned>(total_rows)), dim3(kThreads), 0,
                     st, p);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" size_t cmhse_groupwise_workspace(int32_t n, int32_t B) {
  return (n <= 0 || B <= 0) ? 0 : groupwise_fwd_layout(n, B).bytes;
}

extern "C" int cmhse_groupwise_fwd(const float* im, const float* s, int32_t n, int32_t D,
                                   const int32_t* row_off, const int32_t* col_off, int32_t B,
                                   float margin, int32_t max_violation, int32_t norm, float* loss,
                                   float* reduced, int32_t* arg, float* scores_out,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
  if (!im || !s || !row_off || !col_off || !loss || !reduced || !arg || !workspace || n <= 0 ||
      D <= 0 || B <= 0 || B > 65535)
    return CMHSE_ERR_ARG;
  const LossFwdLayout L = groupwise_fwd_layout(n, B);
  if (!ws_ok(workspace, workspace_bytes, L.bytes)) return CMHSE_ERR_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  float* scores = scores_out ? scores_out : reinterpret_cast<float*>(static_cast<char*>(workspace) + L.scores);
  const int rc = launch_sim_store(im, s, n, n, D, scores, stream);
  if (rc != CMHSE_OK) return rc;
  BlockReduceParams bp;
  bp.scores = scores; bp.row_off = row_off; bp.col_off = col_off; bp.reduced = reduced;
  bp.arg = arg; bp.n = n; bp.B = B; bp.use_max = max_violation;
  hipLaunchKernelGGL(block_reduce_kernel, dim3(B, B), dim3(kThreads), 0, stream, bp);
  return launch_contrastive_reduce(reduced, B, L, workspace, margin, max_violation, norm, loss, nullptr, 1, 0,
                                   stream);
}

extern "C" size_t cmhse_groupwise_bwd_workspace(int32_t n, int32_t B) {
  return (n <= 0 || B <= 0) ? 0 : groupwise_bwd_layout(n, B).bytes;
}

extern "C" int cmhse_groupwise_bwd(const float* im, const float* s, int32_t n, int32_t D,
                                   const int32_t* row_off, const int32_t* col_off, int32_t B,
                                   float margin, int32_t max_violation, int32_t norm,
                                   const float* reduced, const int32_t* arg, const float* grad_out,
                                   float* d_im, float* d_s, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
  if (!im || !s || !row_off || !col_off || !reduced || !arg || !grad_out || !d_im || !d_s ||
      !workspace || n <= 0 || D <= 0 || B <= 0 || B > 65535)
    return CMHSE_ERR_ARG;
  const GroupwiseBwdLayout L = groupwise_bwd_layout(n, B);
  if (!ws_ok(workspace, workspace_bytes, L.bytes)) return CMHSE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  float* dS = reinterpret_cast<float*>(ws + L.dS);
  float* dST = reinterpret_cast<float*>(ws + L.dST);
  const LossBwdParams q = launch_loss_grad(loss_grad_layout(1, B), ws + L.grad, reduced, grad_out, B, margin,
                                           max_violation, norm, nullptr, 1, 0, st);
  ExpandParams ep;
  ep.g_red = q.G; ep.arg = arg; ep.row_off = row_off; ep.col_off = col_off; ep.dS = dS;
  ep.dST = dST; ep.n = n; ep.B = B; ep.use_max = max_violation;
  hipLaunchKernelGGL(groupwise_expand_kernel, dim3(B, B), dim3(kThreads), 0, st, ep);
  const bool vec = (n % 4 == 0) && (D % 4 == 0);
  launch_tn(dST, n, s, D, nullptr, d_im, D, n, D, n, nullptr, vec, st);
  launch_tn(dS, n, im, D, nullptr, d_s, D, n, D, n, nullptr, vec, st);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" int cmhse_euclid_fwd(const float* a, const float* b, const uint64_t* b_rows, int32_t rows,
                                int32_t cols, int32_t norm, float* loss, float* row_dist,
                                void* stream_) {
  if (!a || (!b && !b_rows) || !loss || !row_dist || rows <= 0 || cols <= 0) return CMHSE_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream_);
  EuclidParams q;
  q.a = a; q.b = b; q.b_rows = b_rows; q.dist = row_dist; q.d_a = nullptr; q.gout = nullptr;
  q.loss = loss; q.rows = rows; q.cols = cols; q.norm = norm;
  hipLaunchKernelGGL(euclid_rows_kernel, dim3(rows), dim3(kThreads), 0, st, q, 0);
  hipLaunchKernelGGL(euclid_final_kernel, dim3(1), dim3(kThreads), 0, st, q);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}

extern "C" int cmhse_euclid_bwd(const float* a, const float* b, const uint64_t* b_rows, int32_t rows,
                                int32_t cols, int32_t norm, const float* grad_out, float* d_a,
                                void* stream_) {
  if (!a || (!b && !b_rows) || !grad_out || !d_a || rows <= 0 || cols <= 0) return CMHSE_ERR_ARG;
  EuclidParams q;
  q.a = a; q.b = b; q.b_rows = b_rows; q.dist = nullptr; q.d_a = d_a; q.gout = grad_out;
  q.loss = nullptr; q.rows = rows; q.cols = cols; q.norm = norm;
  hipLaunchKernelGGL(euclid_rows_kernel, dim3(rows), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream_), q, 1);
  return (hipGetLastError() == hipSuccess) ? CMHSE_OK : CMHSE_ERR_LAUNCH;
}
