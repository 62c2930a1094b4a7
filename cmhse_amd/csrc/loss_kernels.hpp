// loss_kernels.hpp
//
// The kernels of the training losses, forward and backward: ContrastiveLoss and its batched form (reduction
// of the stored scores; G = d loss / d scores), GroupWiseContrastiveLoss's block reduction and expansion,
// F.normalize's backward, decoder.loss.EuclideanLoss, the step's fused terms.  Included by loss.hip only.
#pragma once

namespace cmhse {

// ---------------------------------------------------------------------------------------------
// Contrastive loss reduction over a stored n x n score matrix (loss.py:89-117).
// Workgroup b < nrb reduces rows [64b, 64b+64) (cost_s); workgroup nrb + c reduces columns
// [64c, 64c+64) (cost_im).  fp64 partial sums, fixed order -> bitwise reproducible.
// ---------------------------------------------------------------------------------------------
struct LossParams {
  const float* scores;  // [n, n]
  int32_t n, nrb;
  float margin;
  int32_t max_violation, norm;
  double* partial;  // [2 * nrb]
  float* loss;
  const int32_t* blk_off;  // batched blocks (blockIdx.y): see SimParams
  int64_t blk_stride;
};

__device__ __forceinline__ LossParams loss_block(const LossParams& q) {
  LossParams p = q;
  if (p.blk_off != nullptr) {
    p.n = p.blk_off[blockIdx.y + 1] - p.blk_off[blockIdx.y];
    p.scores += static_cast<int64_t>(blockIdx.y) * p.blk_stride;
    p.partial += static_cast<int64_t>(blockIdx.y) * 2 * p.nrb;
    p.loss += blockIdx.y;
  }
  return p;
}

__global__ __launch_bounds__(kThreads) void contrastive_partial_kernel(const LossParams p_) {
  const LossParams p = loss_block(p_);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = p.n;
  const float* S = p.scores;
  __shared__ double s_part[kThreads];
  double total = 0.0;
  if (static_cast<int>(blockIdx.x) < p.nrb) {
    // rows: one wave per row, lanes stride the columns
    const int r0 = blockIdx.x * 64;
    for (int i = r0 + wave; i < r0 + 64 && i < n; i += kThreads / 64) {
      const float dii = S[static_cast<int64_t>(i) * n + i];
      double sum = 0.0;
      float mx = 0.f;
      for (int j = lane; j < n; j += 64) {
        float c = fmaxf(p.margin + S[static_cast<int64_t>(i) * n + j] - dii, 0.f);
        if (j == i) c = 0.f;
        sum += c;
        mx = fmaxf(mx, c);
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        mx = fmaxf(mx, __shfl_xor(mx, d, 64));
      }
      total += p.max_violation ? static_cast<double>(mx) : sum;
    }
    s_part[tid] = (lane == 0) ? total : 0.0;
  } else {
    // columns: thread c < 64 owns column j (coalesced across the wave), 4 waves split the rows
    const int j = (blockIdx.x - p.nrb) * 64 + lane;
    double sum = 0.0;
    float mx = 0.f;
    if (j < n) {
      const float djj = S[static_cast<int64_t>(j) * n + j];
      for (int i = wave; i < n; i += kThreads / 64) {
        float c = fmaxf(p.margin + S[static_cast<int64_t>(i) * n + j] - djj, 0.f);
        if (i == j) c = 0.f;
        sum += c;
        mx = fmaxf(mx, c);
      }
    }
    // combine the 4 waves' shares of each column, then the 64 columns
    __shared__ double c_sum[kThreads];
    __shared__ float c_max[kThreads];
    c_sum[tid] = sum;
    c_max[tid] = mx;
    __syncthreads();
    double v = 0.0;
    if (wave == 0) {
      const double cs = c_sum[lane] + c_sum[64 + lane] + c_sum[128 + lane] + c_sum[192 + lane];
      const float cm = fmaxf(fmaxf(c_max[lane], c_max[64 + lane]),
                             fmaxf(c_max[128 + lane], c_max[192 + lane]));
      v = p.max_violation ? static_cast<double>(cm) : cs;
    }
    s_part[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < kThreads; ++i) t += s_part[i];
    p.partial[blockIdx.x] = t;
  }
}

__global__ void contrastive_final_kernel(const LossParams p_) {
  const LossParams p = loss_block(p_);
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double cs = 0.0, ci = 0.0;
    for (int b = 0; b < p.nrb; ++b) cs += p.partial[b];
    for (int b = 0; b < p.nrb; ++b) ci += p.partial[p.nrb + b];
    // loss.py:113-117: cost_s.sum() + cost_im.sum(), each an fp32 tensor sum
    float loss = static_cast<float>(cs) + static_cast<float>(ci);
    if (p.norm) loss = loss / static_cast<float>(static_cast<int64_t>(p.n) * p.n);
    *p.loss = loss;
  }
}

// ---------------------------------------------------------------------------------------------
// ContrastiveLoss backward: G = d loss / d scores (loss.py:94-117 differentiated), then
// d im = G . s and d s = G^T . im as TN GEMMs on G^T and G.
// ---------------------------------------------------------------------------------------------
struct LossBwdParams {
  const float* scores;  // [n, n]
  const float* gout;    // device scalar: upstream gradient
  int32_t n, max_violation, norm;
  float margin;
  int32_t* row_arg;  // [n] max_violation: argmax_j cost_s(i,j) (or -1 when the max is 0)
  int32_t* col_arg;  // [n] max_violation: argmax_i cost_im(i,j)
  float* row_cnt;    // [n] sum_j g_s(i,j)
  float* col_cnt;    // [n] sum_i g_im(i,j)
  float* G;          // [n, n]
  float* GT;         // [n, n]
  // several independent losses in one launch set (cmhse_contrastive_blocks_bwd): block
  // b = blockIdx.y has n = blk_off[b+1] - blk_off[b]; its scores / G / GT start b * blk_stride
  // floats into their buffers (leading dimension = its own n), its vectors b * vec_stride, its
  // upstream gradient is gout[b]
  const int32_t* blk_off;
  int64_t blk_stride;     // floats between the blocks of G / GT
  int64_t score_stride;   // floats between the blocks of the stored scores (the forward's layout)
  int32_t vec_stride;
};

// the parameters of block blockIdx.y (or the struct itself for a single loss)
__device__ __forceinline__ LossBwdParams loss_bwd_block(const LossBwdParams& q_) {
  LossBwdParams q = q_;
  if (q.blk_off != nullptr) {
    const int b = blockIdx.y;
    q.n = q.blk_off[b + 1] - q.blk_off[b];
    q.scores += b * q.score_stride;
    q.G += b * q.blk_stride;
    q.GT += b * q.blk_stride;
    q.row_arg += b * q.vec_stride;
    q.col_arg += b * q.vec_stride;
    q.row_cnt += b * q.vec_stride;
    q.col_cnt += b * q.vec_stride;
    q.gout += b;
  }
  return q;
}

// one wave per row (rows pass) or per column (columns pass): counts / argmax of violating entries
__global__ __launch_bounds__(kThreads) void loss_bwd_stats_kernel(const LossBwdParams q_) {
  const LossBwdParams q = loss_bwd_block(q_);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = q.n;
  const int idx = blockIdx.x * 4 + wave;  // [0, 2n): rows then columns
  if (idx >= 2 * n) return;
  const bool is_row = idx < n;
  const int i = is_row ? idx : idx - n;
  const float dii = q.scores[static_cast<int64_t>(i) * n + i];
  float cnt = 0.f, best = 0.f;
  int arg = 0x7fffffff;
  for (int j = lane; j < n; j += 64) {
    if (j == i) continue;
    const float sv = is_row ? q.scores[static_cast<int64_t>(i) * n + j]
                            : q.scores[static_cast<int64_t>(j) * n + i];
    const float c = fmaxf(q.margin + sv - dii, 0.f);
    cnt += (c > 0.f) ? 1.f : 0.f;
    if (c > best) {  // first maximum along the reduced index
      best = c;
      arg = j;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    const float ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (ob > best || (ob == best && oa < arg)) {
      best = ob;
      arg = oa;
    }
  }
  if (lane == 0) {
    const int a = (best > 0.f) ? arg : -1;
    const float c = q.max_violation ? ((best > 0.f) ? 1.f : 0.f) : cnt;
    if (is_row) {
      q.row_arg[i] = a;
      q.row_cnt[i] = c;
    } else {
      q.col_arg[i] = a;
      q.col_cnt[i] = c;
    }
  }
}

__global__ __launch_bounds__(kThreads) void loss_bwd_build_kernel(const LossBwdParams q_) {
  const LossBwdParams q = loss_bwd_block(q_);
  const int n = q.n;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= static_cast<int64_t>(n) * n) return;
  const int i = static_cast<int>(e / n), j = static_cast<int>(e % n);
  float scale = *q.gout;
  if (q.norm) scale /= static_cast<float>(static_cast<int64_t>(n) * n);
  float g;
  if (i == j) {
    g = -(q.row_cnt[i] + q.col_cnt[i]);
  } else if (q.max_violation) {
    g = ((q.row_arg[i] == j) ? 1.f : 0.f) + ((q.col_arg[j] == i) ? 1.f : 0.f);
  } else {
    const float sv = q.scores[e];
    const float cs = q.margin + sv - q.scores[static_cast<int64_t>(i) * n + i];
    const float ci = q.margin + sv - q.scores[static_cast<int64_t>(j) * n + j];
    g = ((cs > 0.f) ? 1.f : 0.f) + ((ci > 0.f) ? 1.f : 0.f);
  }
  g *= scale;
  q.G[e] = g;
  q.GT[static_cast<int64_t>(j) * n + i] = g;
}

// GroupWiseContrastiveLoss backward: spread G_red[i][j] over block (i, j) of d scores (uniformly
// for the block mean, onto the arg-max for the block max); writes dS and dS^T.
struct ExpandParams {
  const float* g_red;  // [B, B]
  const int32_t* arg;  // [B, B]
  const int32_t* row_off;
  const int32_t* col_off;
  float* dS;
  float* dST;
  int32_t n, B, use_max;
};

__global__ __launch_bounds__(kThreads) void groupwise_expand_kernel(const ExpandParams q) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  const int r0 = q.row_off[bi], r1 = q.row_off[bi + 1], c0 = q.col_off[bj], c1 = q.col_off[bj + 1];
  const int w = c1 - c0, cnt = (r1 - r0) * w;
  const float g = q.g_red[bi * q.B + bj];
  const int a = q.arg[bi * q.B + bj];
  for (int e = threadIdx.x; e < cnt; e += kThreads) {
    const int r = r0 + e / w, c = c0 + e % w;
    const float v = q.use_max ? ((r * q.n + c == a) ? g : 0.f) : g / static_cast<float>(cnt);
    q.dS[static_cast<int64_t>(r) * q.n + c] = v;
    q.dST[static_cast<int64_t>(c) * q.n + r] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// F.normalize backward: dx = (g - y (y.g)) / max(||x||, eps), y = x / max(||x||, eps)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void l2norm_bwd_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ g,
                                                              float* __restrict__ dx, int cols) {
  const int64_t row = blockIdx.x;
  const float* xr = x + row * cols;
  const float* gr = g + row * cols;
  l2norm_bwd_row(xr, dx + row * cols, cols, [&](int c) { return gr[c]; });   // norm_rows.hpp
}

// ---------------------------------------------------------------------------------------------
// EuclideanLoss (decoder/loss.py:17-26): per-row distances, fixed-order fp64 total
// ---------------------------------------------------------------------------------------------
struct EuclidParams {
  const float* a;
  const float* b;
  const uint64_t* b_rows;
  float* dist;  // [rows]
  float* d_a;   // backward
  const float* gout;
  float* loss;
  int32_t rows, cols, norm;
};

__global__ __launch_bounds__(kThreads) void euclid_rows_kernel(const EuclidParams q, int backward) {
  const int64_t r = blockIdx.x;
  const float* ar = q.a + r * q.cols;
  const float* br = q.b_rows ? reinterpret_cast<const float*>(q.b_rows[r]) : q.b + r * q.cols;
  float ss = 0.f;
  for (int c = threadIdx.x; c < q.cols; c += kThreads) {
    const float d = ar[c] - br[c];
    ss += d * d;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
  __shared__ float part[4];
  __shared__ float s_d;
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) s_d = sqrtf(part[0] + part[1] + part[2] + part[3]);
  __syncthreads();
  const float dist = s_d;
  if (!backward) {
    if (threadIdx.x == 0) q.dist[r] = dist;
    return;
  }
  // d sqrt(ss) / d a = (a - b) / dist: no epsilon, like autograd through torch.sqrt upstream
  // (decoder/loss.py:21) — an exactly reconstructed row (dist == 0) gives NaN there and here
  float sc = *q.gout / dist;
  if (q.norm) sc /= static_cast<float>(q.rows);
  for (int c = threadIdx.x; c < q.cols; c += kThreads) q.d_a[r * q.cols + c] = (ar[c] - br[c]) * sc;
}

// Sum of the row distances in a FIXED order (bitwise reproducible): thread i adds rows i, i + 256,
// ... in double, then a pairwise LDS tree.  (--lowest_reconstruct_loss sums one row per frame /
// word of the batch, 1e4 and more: a single-thread dependent load chain took milliseconds.)
__global__ __launch_bounds__(kThreads) void euclid_final_kernel(const EuclidParams q) {
  __shared__ double part[kThreads];
  double t = 0.0;
  for (int r = threadIdx.x; r < q.rows; r += kThreads) t += q.dist[r];
  part[threadIdx.x] = t;
  __syncthreads();
  for (int w = kThreads / 2; w >= 1; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double total = part[0];
    if (q.norm) total /= q.rows;
    *q.loss = static_cast<float>(total);
  }
}

}  // namespace cmhse

// The kernels below keep the names they have always had, in the global namespace: profiles and traces
// key on kernel names.
using namespace cmhse;

// GroupWiseContrastiveLoss (loss.py:26-38): block (video i's clips x video j's captions) max or
// mean of the clip x caption score matrix.  One workgroup per block; the arg-max (row-major first
// maximum) is kept for the backward pass.
struct BlockReduceParams {
  const float* scores;  // [n, n]
  const int32_t* row_off;
  const int32_t* col_off;
  float* reduced;   // [B, B]
  int32_t* arg;     // [B, B] flat index r*n + c of the block maximum
  int32_t n, B, use_max;
};

__global__ __launch_bounds__(kThreads) void block_reduce_kernel(const BlockReduceParams q) {
  const int bi = blockIdx.y, bj = blockIdx.x, tid = threadIdx.x;
  const int r0 = q.row_off[bi], r1 = q.row_off[bi + 1], c0 = q.col_off[bj], c1 = q.col_off[bj + 1];
  const int w = c1 - c0, cnt = (r1 - r0) * w;
  double sum = 0.0;
  float best = -INFINITY;
  int arg = 0x7fffffff;
  for (int e = tid; e < cnt; e += kThreads) {
    const int r = r0 + e / w, c = c0 + e % w;
    const float v = q.scores[static_cast<int64_t>(r) * q.n + c];
    sum += v;
    const int flat = r * q.n + c;
    if (v > best || (v == best && flat < arg)) {
      best = v;
      arg = flat;
    }
  }
  __shared__ double s_sum[kThreads];
  __shared__ float s_best[kThreads];
  __shared__ int s_arg[kThreads];
  s_sum[tid] = sum;
  s_best[tid] = best;
  s_arg[tid] = arg;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    float b = -INFINITY;
    int a = 0x7fffffff;
    for (int i = 0; i < kThreads; ++i) {
      t += s_sum[i];
      if (s_best[i] > b || (s_best[i] == b && s_arg[i] < a)) {
        b = s_best[i];
        a = s_arg[i];
      }
    }
    q.reduced[bi * q.B + bj] = q.use_max ? b : static_cast<float>(t / cnt);
    q.arg[bi * q.B + bj] = a;
  }
}

// ---------------------------------------------------------------------------------------------
// cmhse_step_losses_fwd: F.normalize of the step's encoder outputs written straight into the
// row-blocked operands of the batched ContrastiveLoss, the losses, and their weighted total.
// ---------------------------------------------------------------------------------------------
struct StepNormParams {
  const float* src[2][CMHSE_STEP_LOSS_MAX];  // [side][term]: the embedding that is the term's a / b
  int32_t n[CMHSE_STEP_LOSS_MAX];            // term sizes
  float weight[CMHSE_STEP_LOSS_MAX];
  int32_t n_terms, D, R;
  float* y[2];        // [R, D] each
  int32_t* blk_off;   // [n_terms + 1]
};

// one workgroup per operand row (2R of them); l2norm_rows_kernel's row function
__global__ __launch_bounds__(kThreads) void step_norm_kernel(const StepNormParams p) {
  const int side = (static_cast<int>(blockIdx.x) >= p.R) ? 1 : 0;
  const int r = static_cast<int>(blockIdx.x) - side * p.R;
  const float* xr = nullptr;
  int off = 0;
#pragma unroll
  for (int k = 0; k < CMHSE_STEP_LOSS_MAX; ++k) {
    if (k < p.n_terms) {
      if (r >= off && r < off + p.n[k])
        xr = (side ? p.src[1][k] : p.src[0][k]) + static_cast<int64_t>(r - off) * p.D;
      off += p.n[k];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int o = 0;
    p.blk_off[0] = 0;
#pragma unroll
    for (int k = 0; k < CMHSE_STEP_LOSS_MAX; ++k)
      if (k < p.n_terms) {
        o += p.n[k];
        p.blk_off[k + 1] = o;
      }
  }
  float* yr = p.y[side] + static_cast<int64_t>(r) * p.D;
  l2norm_row(xr, yr, p.D);
}

__global__ void step_total_kernel(const StepNormParams p, const float* values, float* total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < CMHSE_STEP_LOSS_MAX; ++k)
      if (k < p.n_terms) t += p.weight[k] * values[k];
    *total = t;
  }
}

// ---------------------------------------------------------------------------------------------
// cmhse_step_losses_bwd: per-term upstream gradients, the batched ContrastiveLoss backward, then
// F.normalize's backward over the sum of every use of each encoder output.
// ---------------------------------------------------------------------------------------------
struct StepNormBwdParams {
  const float* x[CMHSE_STEP_LOSS_MAX];
  float* dx[CMHSE_STEP_LOSS_MAX];
  int32_t rows[CMHSE_STEP_LOSS_MAX];
  int32_t term_a[CMHSE_STEP_LOSS_MAX], term_b[CMHSE_STEP_LOSS_MAX], term_off[CMHSE_STEP_LOSS_MAX];
  float weight[CMHSE_STEP_LOSS_MAX];
  int32_t n_emb, n_terms, D;
  const float* d_im;  // [R, D]
  const float* d_s;   // [R, D]
};

__global__ void step_gout_kernel(const StepNormBwdParams p, const float* grad_total, float* gout) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float g = *grad_total;
#pragma unroll
    for (int k = 0; k < CMHSE_STEP_LOSS_MAX; ++k)
      if (k < p.n_terms) gout[k] = p.weight[k] * g;
  }
}

// one workgroup per encoder-output row: g = sum over the terms that use the row (term order, left
// operand before right), then l2norm_bwd_kernel's row function
__global__ __launch_bounds__(kThreads) void step_norm_bwd_kernel(const StepNormBwdParams p) {
  int e = -1, i = 0, off = 0;
  const float* xr = nullptr;
  float* dxr = nullptr;
#pragma unroll
  for (int k = 0; k < CMHSE_STEP_LOSS_MAX; ++k) {
    if (k < p.n_emb) {
      const int r = static_cast<int>(blockIdx.x) - off;
      if (r >= 0 && r < p.rows[k]) {
        e = k;
        i = r;
        xr = p.x[k] + static_cast<int64_t>(r) * p.D;
        dxr = p.dx[k] + static_cast<int64_t>(r) * p.D;
      }
      off += p.rows[k];
    }
  }
  if (e < 0) return;
  const float* use[2 * CMHSE_STEP_LOSS_MAX];
#pragma unroll
  for (int k = 0; k < CMHSE_STEP_LOSS_MAX; ++k) {
    const bool live = k < p.n_terms;
    const int64_t row = static_cast<int64_t>(p.term_off[k] + i) * p.D;
    use[2 * k] = (live && p.term_a[k] == e) ? p.d_im + row : nullptr;
    use[2 * k + 1] = (live && p.term_b[k] == e) ? p.d_s + row : nullptr;
  }
  auto grad = [&](int c) {
    float g = 0.f;
#pragma unroll
    for (int u = 0; u < 2 * CMHSE_STEP_LOSS_MAX; ++u)
      if (use[u] != nullptr) g += use[u][c];
    return g;
  };
  l2norm_bwd_row(xr, dxr, p.D, grad);
}
