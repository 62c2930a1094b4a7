// loss_layout.hpp — the workspace layout of every training-loss entry point of loss.hip, one struct
// each.  A cmhse_*_workspace() query returns its layout's `bytes`, and the entry point carves its
// pointers from the same layout, so no size is stated twice.  The offsets are ABI: Python keeps a
// forward workspace as the stored scores of the backward (block b at scores + b * max_n * max_n,
// unaligned between blocks), and the step's two host calls share ONE caller-provided workspace.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cmhse_hip.h"
#include "gru_ws.hpp"

namespace cmhse {

// what every workspace-taking entry point asks of its workspace before the first HIP call
static inline bool ws_ok(const void* workspace, size_t workspace_bytes, size_t need) {
  return (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0 && workspace_bytes >= need;
}

// Forward: the stored scores, then the fp64 partial sums of contrastive_partial_kernel (2 * nrb per
// loss: nrb workgroups of 64 rows, nrb of 64 columns).
struct LossFwdLayout {
  int32_t nrb;
  size_t scores;    // float [score_floats]
  size_t partial;   // double [n_losses, 2 * nrb]
  size_t bytes;
};

static inline LossFwdLayout loss_fwd_layout(size_t score_floats, int32_t n_losses, int32_t nrb) {
  LossFwdLayout L;
  L.nrb = nrb;
  L.scores = 0;
  L.partial = ws_align(score_floats * sizeof(float));
  L.bytes = L.partial + ws_align(static_cast<size_t>(n_losses) * 2 * nrb * sizeof(double));
  return L;
}

// ContrastiveLoss over n_blocks score matrices of up to max_n rows (the single loss: n_blocks = 1)
static inline LossFwdLayout contrastive_fwd_layout(int32_t n_blocks, int32_t max_n) {
  return loss_fwd_layout(static_cast<size_t>(n_blocks) * max_n * max_n, n_blocks, (max_n + 63) / 64);
}

// GroupWiseContrastiveLoss: the n x n clip x caption scores; the loss runs on the [B, B] block reduction
static inline LossFwdLayout groupwise_fwd_layout(int32_t n, int32_t B) {
  return loss_fwd_layout(static_cast<size_t>(n) * n, 1, (B + 63) / 64);
}

// The loss-gradient block of n_blocks losses of up to n rows (LossBwdParams): every region holds
// n_blocks slots, `blk_stride` / `vec_stride` floats apart.
struct LossGradLayout {
  size_t G, GT;               // float [n_blocks][n, n]
  size_t row_arg, col_arg;    // int32 [n_blocks][n]
  size_t row_cnt, col_cnt;    // float [n_blocks][n]
  int64_t blk_stride;
  int32_t vec_stride;
  size_t bytes;
};

static inline LossGradLayout loss_grad_layout(int32_t n_blocks, int32_t n) {
  const size_t mat = ws_align(static_cast<size_t>(n) * n * sizeof(float));
  const size_t vec = ws_align(static_cast<size_t>(n) * sizeof(float));
  LossGradLayout L;
  size_t off = 0;
  L.G = off;        off += n_blocks * mat;
  L.GT = off;       off += n_blocks * mat;
  L.row_arg = off;  off += n_blocks * vec;
  L.col_arg = off;  off += n_blocks * vec;
  L.row_cnt = off;  off += n_blocks * vec;
  L.col_cnt = off;  off += n_blocks * vec;
  L.blk_stride = static_cast<int64_t>(mat / sizeof(float));
  L.vec_stride = static_cast<int32_t>(vec / sizeof(float));
  L.bytes = off;
  return L;
}

// GroupWiseContrastiveLoss backward: d scores and its transpose, then the gradient block of the [B, B] loss
struct GroupwiseBwdLayout {
  size_t dS, dST;    // float [n, n]
  size_t grad;       // loss_grad_layout(1, B)
  size_t bytes;
};

static inline GroupwiseBwdLayout groupwise_bwd_layout(int32_t n, int32_t B) {
  const size_t big = ws_align(static_cast<size_t>(n) * n * sizeof(float));
  GroupwiseBwdLayout L;
  L.dS = 0;
  L.dST = big;
  L.grad = 2 * big;
  L.bytes = L.grad + loss_grad_layout(1, B).bytes;
  return L;
}

// cmhse_step_losses_fwd / _bwd: everything a training step's contrastive terms need between
// F.normalize of the encoder outputs and the gradients wrt those outputs lives in ONE workspace, so
// the step runs the whole block in two host calls and ten launches (model.py:333-343 and its share
// of loss.backward(), model.py:367).
struct StepLossLayout {
  int32_t R;        // rows of the row-blocked operands: sum over terms of the term's size
  int32_t max_n;    // largest term
  size_t blk_off;   // int32 [n_terms + 1]
  size_t gout;      // float [n_terms]: weight_k * upstream gradient
  size_t y_im, y_s; // float [R, D]: normalised rows, term by term (left / right operand)
  size_t fwd_ws;    // cmhse_contrastive_blocks_fwd's workspace (stored scores first)
  size_t bwd_ws;    // cmhse_contrastive_blocks_bwd's workspace
  size_t d_im, d_s; // float [R, D]
  size_t bytes;
};

// false: the descriptor is not a valid set of terms
static inline bool step_loss_layout(const cmhse_step_losses* d, StepLossLayout* L) {
  if (!d || d->n_emb <= 0 || d->n_emb > CMHSE_STEP_LOSS_MAX || d->n_terms <= 0 ||
      d->n_terms > CMHSE_STEP_LOSS_MAX || d->D <= 0)
    return false;
  int64_t R = 0;
  int32_t mx = 0;
  for (int e = 0; e < d->n_emb; ++e)
    if (d->rows[e] <= 0) return false;
  for (int k = 0; k < d->n_terms; ++k) {
    const int a = d->term_a[k], b = d->term_b[k];
    if (a < 0 || a >= d->n_emb || b < 0 || b >= d->n_emb || d->rows[a] != d->rows[b]) return false;
    R += d->rows[a];
    mx = d->rows[a] > mx ? d->rows[a] : mx;
  }
  if (R > 0x7fffffffLL / d->D) return false;
  L->R = static_cast<int32_t>(R);
  L->max_n = mx;
  const size_t mat = ws_align(static_cast<size_t>(R) * d->D * sizeof(float));
  size_t off = 0;
  L->blk_off = off; off += 256;
  L->gout = off;    off += 256;
  L->y_im = off;    off += mat;
  L->y_s = off;     off += mat;
  L->fwd_ws = off;  off += contrastive_fwd_layout(d->n_terms, mx).bytes;
  L->bwd_ws = off;  off += loss_grad_layout(d->n_terms, mx).bytes;
  L->d_im = off;    off += mat;
  L->d_s = off;     off += mat;
  L->bytes = off;
  return true;
}

}  // namespace cmhse
