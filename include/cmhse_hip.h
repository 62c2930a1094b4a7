/* cmhse_hip.h — C ABI of libcmhse_hip.so, the MI355X (gfx950) hot-path library.
 *
 * The reference (zbwglory/CMHSE) has no FFI layer: its hot path calls third-party PyTorch / NumPy
 * operators from Python.  Each entry point below replaces one of those call sites; the citation
 * (file:line into the reference tree) says which.  A maintainer of the reference binds these with
 * `ctypes`; cmhse_amd/_lib.py is that binding.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in signatures (`stream` is a hipStream_t
 *     passed as void*; NULL = the null stream);
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - all float data is IEEE fp32, row-major, 16-byte aligned rows are the fast path (feature
 *     width and hidden size multiples of 4); indices are int32 unless stated (token ids: int64,
 *     as torch.LongTensor);
 *   - calls are asynchronous on `stream` and re-entrant; they allocate NO device memory: scratch
 *     is an explicit caller-owned workspace whose size the matching `*_workspace` function
 *     returns.  Host-side objects a call may take and give back before it returns: HIP events for
 *     stream fork / join (`tail_stream`, `stream`, `side_stream` of the job structs) and the event
 *     pairs owned by a cmhse_timer handle when the caller passes one (measurement only);
 *   - workspaces and outputs may hold anything on entry and no result depends on what they held
 *     (an arena reused across calls of other shapes is fine), except the three accumulation targets
 *     whose comment says "zero it first": cmhse_rows_differ's flag, d_emb_table and the dx row of a
 *     time-constant input (tests/test_gpu_dirty_workspace.py);
 *   - process-wide state, all of it host-side and mutex- or atomic-guarded: (o) 64 bytes of pinned
 *     host memory per device for cmhse_async_status, allocated at the first resident launch;
 *     (i) per-device free
 *     lists of those HIP events (creating an event while the GPU is busy can stall the host for
 *     tens of milliseconds, so events are recycled; an event returns to the list of the device
 *     that is current in the calling thread — use one device per thread across a call); (ii) the
 *     DEFAULT kernel-shape crossovers of cmhse_tune() below (a caller that must not share them
 *     enters a tuning context, cmhse_ctx_*: its own copy, current per thread).  Nothing else: no
 *     cached device memory, no cached streams, no environment variables;
 *   - return value: 0 = success, negative = error code (cmhse_strerror); no exceptions or aborts
 *     cross the ABI.
 */
#ifndef CMHSE_HIP_H_
#define CMHSE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  CMHSE_OK = 0,
  CMHSE_ERR_ARG = -1,        /* invalid argument (null pointer, non-positive size, bad mode) */
  CMHSE_ERR_WORKSPACE = -2,  /* workspace too small or misaligned */
  CMHSE_ERR_LAUNCH = -3,     /* HIP launch / runtime error (hipGetLastError text via strerror) */
  CMHSE_ERR_UNSUPPORTED = -4, /* shape outside what the kernels support */
  CMHSE_ERR_TIMEOUT = -5      /* an earlier resident-kernel launch on this device gave up at a grid
                                 barrier (see cmhse_async_status) */
};

/* pooling applied on top of the GRU hidden states (reference: model.py:27-34 `rnn_type`) */
enum {
  CMHSE_POOL_LAST = 0, /* layers.Seq2Seq.forward   layers.py:47-66   h at t = len-1            */
  CMHSE_POOL_ATTN = 1, /* layers.Attention.forward layers.py:93-119  masked exp-softmax pooling */
  CMHSE_POOL_MAX = 2,  /* layers.Maxout.forward    layers.py:185-204 max over valid steps       */
  CMHSE_POOL_ALL = 3,  /* decoder Seq2Seq_Decode + DecoderSequence.forward (decoder/layers.py:34-52,
                          decoder/model.py:36-45): every hidden state, sequence after sequence:
                          out[out_row[s] + t, :] = h_{s,t} */
  /* OR-ed into pool_mode for training: the forward also keeps gate activations (and the arg-max
   * step / tanh(lin(h))) in its workspace, which cmhse_gru_pool_bwd consumes. */
  CMHSE_SAVE_FOR_BACKWARD = 0x100,
  /* OR-ed into pool_mode: run the large GEMMs of the call on the bf16 matrix pipe with a 3-term
   * hi/lo split (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulate): ~2^-17 relative error per
   * product, ~1e-6 on the embeddings (parity bar 1e-4); 2.7x less matrix time per product than exact
   * fp32 on the v_mfma_f32_32x32x8_bf16_1k pairs this library restricts itself to, 1.8x per validation
   * pass.  Inference calls only (ignored with CMHSE_SAVE_FOR_BACKWARD); applies to the steps with more
   * than `tiny_max_seqs` active sequences and to the attention projection of their rows; those
   * kernels stage pre-split operands by LDS-DMA and use 60 KB (steps) / 72 KB (projection) of LDS per
   * workgroup.  Outside the bit-identical-ranks contract.  Default (flag clear) is exact fp32. */
  CMHSE_MATH_BF16X3 = 0x200,
  /* OR-ed into the pool_mode of a cmhse_gru_job / cmhse_gru_bwd_job that has its own `stream`: the
   * call does NOT order its own stream argument behind that stream when it returns.  The job's
   * results are then ready on the job's stream only; a later job on the same stream may consume
   * them at once (level 2 of a tower right behind its level 1, without waiting for the other
   * tower), anything else must be ordered by the caller — a later call on the same job stream
   * without this flag does that for everything queued before it.  Buffers the job uses must stay
   * allocated until then. */
  CMHSE_NO_JOIN = 0x400
};

/* Weights of one encoder layer, laid out exactly as the reference's state-dict tensors
 * (layers.py:70-91; checkpoint keys rnn.rnn.weight_ih_l0 ...). */
typedef struct cmhse_gru_weights {
  const float* w_ih;  /* [3H, I]  rnn.rnn.weight_ih_l0, gate row order r,z,n (torch.nn.GRU) */
  const float* w_hh;  /* [3H, H]  rnn.rnn.weight_hh_l0 */
  const float* b_ih;  /* [3H]     rnn.rnn.bias_ih_l0 */
  const float* b_hh;  /* [3H]     rnn.rnn.bias_hh_l0 */
  const float* w_lin; /* [H, H]   rnn.lin.weight   (CMHSE_POOL_ATTN only, else NULL) */
  const float* b_lin; /* [H]      rnn.lin.bias */
  const float* w_att; /* [H]      rnn.att_w.weight ([1,H]) */
} cmhse_gru_weights;

/* A ragged batch of S sequences, already ordered by length, longest first — the order
 * torch.nn.utils.rnn.pack_padded_sequence imposes (layers.py:94-97).  The caller (host logic in
 * cmhse_amd/layers.py) sorts and fills these small arrays; the feature / token storage itself is
 * never copied or re-laid-out: each sequence is addressed through its own base pointer, so padded
 * [S,T,I] batches, several loader batches at once, and the consecutive-row inputs of
 * VSE.structure_emb (model.py:238-255) are all consumed in place. */
typedef struct cmhse_seq_batch {
  int32_t S;    /* sequences */
  int32_t Tmax; /* longest length (= lens[0]) */
  int32_t I;    /* input width: img_dim, word_dim or first-level size */
  int32_t H;    /* hidden size (embed_size) */
  const uint64_t* x_rows;   /* [S] address of step 0 of sequence s: fp32 rows, stride I floats;
                               NULL when tok_rows is used */
  int32_t x_step_floats;    /* floats between consecutive steps of a sequence in x_rows storage: I for
                               ordinary [T, I] rows, 0 for a time-constant input (the repeated
                               embedding a decoder is fed, model.py:261-265) */
  const uint64_t* tok_rows; /* [S] address of token 0 of sequence s (int64 ids, contiguous);
                               the embedding lookup of model.EncoderText.forward (model.py:94) is
                               fused into the operand load.  NULL when x_rows is used */
  const float* emb_table;   /* [vocab, I] embed.weight (tok_rows only) */
  int32_t vocab;
  const uint64_t* h0_rows;  /* [S] address of the initial hidden row of sequence s (H floats), or
                               NULL for h0 = 0 (layers.py:98-102 `hidden`) */
  const int32_t* lens;      /* [S] lengths, non-increasing, all >= 1 */
  const int32_t* out_row;   /* [S] row of `out` that receives sequence s (undoes the sort,
                               layers.py:116-117) */
  const int32_t* step_off;  /* [Tmax+1] step_off[t] = sum_{t'<t} #{s : lens[s] > t'}: row offset
                               of step t in the time-major packed hidden-state buffer */
  const int32_t* step_count_host; /* HOST [Tmax] #{s : lens[s] > t} (sizes the per-step grids) */
  void* step_timer;         /* optional cmhse_timer (or NULL): brackets the per-step GRU kernels of
                               this call on `stream` — measurement only, no effect on results */
  const void* const* step_events_host; /* optional HOST [Tmax] of hipEvent_t (NULL entries allowed), or
                               NULL: before step t's kernel is launched, its stream waits on entry t.
                               Lets the caller feed x rows chunk by chunk (cmhse_pull_steps on a copy
                               stream) while earlier steps compute */
  const int32_t* step_plan_host; /* optional HOST [Tmax], or NULL: #{s : lens[s] > t} over the WHOLE set of
                               sequences this batch is a share of (one rank's part of a validation
                               split, one super-batch of several: >= step_count_host[t], non-increasing).
                               Which kernel serves step t — the LDS-tiled one (one k-ordered sum over
                               [x_t | h_{t-1}]) or the small-batch one (hoisted input projection + K in
                               8 slices) — is then chosen from THIS count instead of the batch's own, so
                               a sequence is encoded bit for bit the same whatever share of the split
                               it is encoded with (parallel_eval: integer ranks identical for any
                               number of ranks).  NULL = the batch's own counts */
  /* Prefix aliases (0 / NULL = none): extra OUTPUT rows pooled from the first steps of sequences of this
   * batch.  When sequence a is a prefix of sequence b (same input rows, both from h0 = 0: a video's first
   * caption and its paragraph, activity_net/data.py:78), the hidden states and attention energies of a
   * ARE those of b's first len_a steps, so a is left out of the batch and alias i stands in for it:
   *   out[alias_out_row[i], :] = attention pooling of steps 0 .. alias_len[i]-1 of sequence alias_src[i]
   * (alias_src: SORTED index, the index of lens / out_row), evaluated exactly as for a real sequence of
   * that length: the same bits.  CMHSE_POOL_ATTN inference requests only (CMHSE_ERR_ARG with another
   * pooling or CMHSE_SAVE_FOR_BACKWARD), every alias_src in [0, S) and 1 <= alias_len <= lens[alias_src]
   * (CMHSE_ERR_ARG otherwise).  The *_host copies are what the call validates (it never reads device
   * memory on the host); the kernels read the device copies, which must hold the same values (a device
   * length beyond its source is clamped to it).  `out` then has more rows than S: out_row and
   * alias_out_row together name each of them once.  The caller keeps the step plan of the ORIGINAL
   * sequences in step_plan_host, so that every remaining step is served by the kernel it had with them. */
  int32_t n_alias;
  const int32_t* alias_src;     /* [n_alias] device */
  const int32_t* alias_len;     /* [n_alias] device */
  const int32_t* alias_out_row; /* [n_alias] device */
  const int32_t* alias_src_host; /* HOST [n_alias] */
  const int32_t* alias_len_host; /* HOST [n_alias] */
} cmhse_seq_batch;

/* Bytes of workspace cmhse_gru_pool_fwd needs for this batch: the time-major packed hidden states
 * hs[sumT, H] (kept for the attention pooling and for a later backward pass) plus the attention
 * energy partials. */
size_t cmhse_gru_pool_workspace(int32_t S, int32_t Tmax, int64_t sum_T, int32_t I, int32_t H,
                                int32_t pool_mode);
/* The same for a token-fed batch (tok_rows, emb_table of `vocab` rows): adds the token projection
 * table G[vocab, 3H] f32 (vocab * 3H * 4 bytes: 160 MB at vocab 13 058, H 1024) when the request
 * qualifies — inference, exact math (no CMHSE_SAVE_FOR_BACKWARD, no CMHSE_MATH_BF16X3), I and H
 * multiples of 4, sum_T >= 4 * vocab, tunable "tok_table" on.  The call then computes G = emb W_ih^T
 * once and its steps read their input projection from G[token] instead of multiplying
 * x_t = emb[token] by W_ih themselves (bit-identical).  A token-fed request whose workspace was
 * sized by cmhse_gru_pool_workspace (no room for G) runs without the table.  vocab <= 0: equal to
 * cmhse_gru_pool_workspace. */
size_t cmhse_gru_pool_workspace_tok(int32_t S, int32_t Tmax, int64_t sum_T, int32_t I, int32_t H,
                                    int32_t pool_mode, int32_t vocab);

/* Where a named region of that workspace lives (tests and tools that inspect what a training
 * forward kept: the gate activations, the arg-max step of the max pooling ...).  name: "hs"
 * [sum_T, H] f32 | "gates" [sum_T, 4H] f32 (r, z, n, W_hn h + b_hn) | "argmax" [S, H] int32, rows in
 * SORTED sequence order (CMHSE_POOL_MAX with CMHSE_SAVE_FOR_BACKWARD) | "v" [sum_T, H] f32
 * (CMHSE_POOL_ATTN with CMHSE_SAVE_FOR_BACKWARD) | with CMHSE_MATH_BF16X3 the pre-split rows, dwords
 * of bf16 pairs, rows of K rounded up to whole 16-k chunks (per chunk 8 dwords of hi pairs, then 8 of
 * lo pairs): "xs" [sum_T, ..] the inputs, "hs_s" [sum_T, ..] the hidden states (only the rows of the
 * bf16x3 steps are written), "h0_s" [S, ..] the initial states.  *bytes = 0 when the mode does not
 * keep the region.  Unknown name: CMHSE_ERR_ARG.  No effect on any computation. */
int cmhse_gru_pool_ws_region(int32_t S, int32_t Tmax, int64_t sum_T, int32_t I, int32_t H,
                             int32_t pool_mode, const char* name, size_t* offset, size_t* bytes);

/* Replaces the body of layers.{Seq2Seq,Attention,Maxout}.forward (layers.py:47-66, 93-119,
 * 185-204): 1-layer unidirectional GRU over the packed batch (nn.GRU, layers.py:31-34) followed
 * by the pooling `pool_mode`.  out[out_row[s], :] (row stride H) receives the un-normalised
 * embedding of sequence s.  The first sum_T*H floats of `workspace` hold, on return, the hidden
 * states in pack_padded_sequence's time-major packed order. */
int cmhse_gru_pool_fwd(const cmhse_seq_batch* seqs, const cmhse_gru_weights* w, int32_t pool_mode,
                       float* out, void* workspace, size_t workspace_bytes, void* stream);

#define CMHSE_MAX_JOBS 4
/* Several INDEPENDENT cmhse_gru_pool_fwd requests in one call (at most CMHSE_MAX_JOBS).  Results are bit-identical
 * to the separate calls; step t of every request shares one launch, so two encoders that do not
 * depend on each other — the clip and sentence encoders of VSE.forward_emb (model.py:222-236), the
 * video and paragraph encoders of structure_emb (model.py:238-255) — pay one launch latency and one
 * partially filled last wave of workgroups per time step instead of two — and, for inference calls,
 * the LDS-tiled steps of all requests that run them together are ONE launch altogether (the step
 * chain, "chain_min_steps" below: per-row-tile dependencies instead of a launch per time step).
 * The first request's step_timer (if set) brackets the step launches of the whole group. */
typedef struct cmhse_gru_job {
  const cmhse_seq_batch* seqs;
  const cmhse_gru_weights* weights;
  int32_t pool_mode;
  float* out;
  void* workspace;
  size_t workspace_bytes;
  void* tail_stream;   /* optional second hipStream_t (or NULL), ideally of higher priority.  When
                          this request's last time step is launched while other requests of the
                          call still have steps to go (a short chain beside a long one), the
                          REMAINING step launches of the call continue on tail_stream (ordered by
                          an event) and this request's attention projection + pooling start at
                          once on `stream`, beside that few-sequence, latency-bound tail.  The
                          call rejoins `stream` (event wait) before its last launches, so the
                          caller needs no extra ordering.  The same side stream also takes a
                          request whose chain has dropped to small-batch steps while another
                          request still launches LDS-tiled steps that do not fill the chip, so
                          that its short launches run beside those instead of between them. */
  void* stream;        /* optional hipStream_t of this request's OWN launches (or NULL = the call's
                          stream).  The towers of a training step are independent latency chains of
                          short dependent launches: given a stream each, they advance side by side
                          from their first step — the host queues step t of every request before
                          step t + 1 of any, so no chain waits for another chain's launches to be
                          queued.  The call forks the stream from, and joins it back into, the
                          call's stream.  Results do not depend on it. */
  void* side_stream;   /* optional hipStream_t (or NULL) for throughput work beside a chain that is
                          small-batch from its first step (a training batch): the hoisted input
                          projection x W_ih^T is then cut into chunks of time steps — only the first
                          stands in front of the chain, the others run on side_stream beside it, step
                          t waiting (event) for the chunk that holds its rows.  Results do not
                          depend on it. */
  void* out_ready_event; /* optional hipEvent_t (or NULL), recorded by the call where this request's
                          `out` becomes final: right behind its pooling pass when that is launched
                          early (tail_stream: its chain ended while other requests still step), else
                          at the end of the call: on `stream`, or on this request's own `stream`
                          when CMHSE_NO_JOIN leaves that un-joined (its output completes there).
                          A consumer on another stream — the device-to-host hand-over of
                          evaluation.encode_data (evaluation.py:120-125) — waits on it instead of on
                          the whole call, and so runs beside the other requests' remaining steps. */
} cmhse_gru_job;
int cmhse_gru_pool_fwd_multi(const cmhse_gru_job* jobs, int32_t n_jobs, void* stream);

/* Host -> HBM hand-over of the loader's feature tensors (the `.cuda()` of model.py:225-227,
 * evaluation.py:97-104), in the unit the step pipeline consumes: time steps [t0, t1) of the first
 * n_active sequences of a length-sorted batch.  src_rows_pinned[s] is the HOST address of step 0 of
 * sequence s inside page-locked memory (the DataLoader's pin_memory=True tensors,
 * activity_net/data.py:157-162; it must be device-readable, as hipHostMalloc / torch pinned memory
 * is), dst_rows[s] its device address; rows are row_floats floats apart in both.  Only valid steps
 * (t < lens[s]) are moved: zero padding never crosses PCIe.  Runs as a kernel on `stream` (give it a
 * stream of its own, record an event, hand it to the consumer via step_events_host). */
int cmhse_pull_steps(const uint64_t* src_rows_pinned, const uint64_t* dst_rows, const int32_t* lens,
                     int32_t n_active, int32_t row_floats, int32_t t0, int32_t t1, void* stream);

/* HBM -> host hand-over of finished embedding rows: what evaluation.encode_data does with
 * `.data.cpu()` + list.extend per batch (evaluation.py:120-125, 139-144).  `bytes` bytes from `src`
 * (device) to `dst_pinned` (page-locked host memory that is device-writable, as hipHostMalloc /
 * torch pinned memory is; both 16-byte aligned), as a kernel of `workgroups` workgroups (0 = 8) of
 * `waves` wavefronts (1..4, 0 = 1) on `stream`: small enough to run beside the level-2 encoders
 * and the ranking without taking their CUs, which the runtime's chip-wide blit copy does.
 * Asynchronous; record an event on `stream` (or synchronise it) before the host reads. */
int cmhse_push_rows(const void* src, void* dst_pinned, size_t bytes, int32_t workgroups, int32_t waves,
                    void* stream);

/* Do `bytes` bytes at `a` and at `b` differ?  `a`: device memory or page-locked host memory that the
 * device can read (read in place, over PCIe); `b`: device memory; both 16-byte aligned.  ORs 1 into
 * the device word *flag (zeroed by the caller) when they do.  evaluation.i2t / t2i (evaluation.py:
 * 160-213) use it to make sure the NumPy arrays they are handed still hold what encode_data wrote
 * before they report the ranking encode_data already queued on the device copies.  Asynchronous. */
int cmhse_rows_differ(const void* a, const void* b, size_t bytes, int32_t* flag, void* stream);

/* Is token sequence a a prefix of token sequence b?  For each of n pairs: flags[i] = 1 iff
 * b_len[i] >= a_len[i] and the first a_len[i] int64 ids at a_rows[i] and at b_rows[i] (device addresses,
 * as cmhse_seq_batch.tok_rows) are equal, else 0.  Raw ids are compared (the encoders clamp both sides
 * to [0, vocab) alike).  The precondition of the prefix aliases above, checked on the data of every
 * call: one wave per pair, all arrays on the device, flags int32 [n].  Asynchronous. */
int cmhse_tok_prefix_check(int32_t n, const uint64_t* a_rows, const uint64_t* b_rows, const int32_t* a_len,
                           const int32_t* b_len, int32_t* flags, void* stream);

/* The padding half of the loader's collate_fn (activity_net/data.py:114-150, didemo_dev/data.py:
 * 133-165) as an index kernel: S ragged sequences stored back to back, row r of sequence s at
 * src + (first_row[s] + r) * row_bytes (frame features: row_bytes = 4 * img_dim; token ids: 8), are
 * written into the zero-padded block dst[S, Tmax, row_bytes].  The encoders do not need it (they
 * address ragged storage through cmhse_seq_batch.x_rows / tok_rows directly, so a packed batch is
 * uploaded without its padding and never padded); it exists for callers that want the reference's
 * padded tensors on the device.  row_bytes must be a multiple of 4. */
int cmhse_pad_rows(const void* src, const int64_t* first_row, const int32_t* lens, int32_t S,
                   int32_t Tmax, int32_t row_bytes, void* dst, void* stream);

/* torch.nn.functional.normalize(x) (p=2, dim=1, eps=1e-12) — call sites model.py:333-343,
 * evaluation.py:111-116.  y may alias x.  Rows have stride `ld` floats. */
int cmhse_l2norm_rows(const float* x, float* y, int32_t rows, int32_t cols, int64_t ld,
                      void* stream);

/* nn.Embedding lookup (model.EncoderText.forward, model.py:94): out[r,:] = table[ids[r],:] for
 * n ids (int64).  Only needed when the caller wants the word tensor itself (`return_word`,
 * model.py:233); the encoders fuse the lookup into cmhse_gru_pool_fwd. */
int cmhse_gather_rows(const float* table, const int64_t* ids, int64_t n, int32_t cols,
                      int32_t vocab, float* out, void* stream);

/* Replaces evaluation.i2t / t2i's `numpy.dot` + per-row `numpy.argsort` loop
 * (evaluation.py:164-171, 192-199) for the row stripe [row0, row0+nrows) of the N x M score
 * matrix d = A B^T (A [N,D], B [M,D], exact-fp32 MFMA).  The matrix is never materialised:
 *   rank[i - row0] = #{ j != i : d[i,j] > d[i,i] }   (position of i in the descending sort)
 *   top1[i - row0] = argmax_j d[i,j]                 (smallest j on exact ties)
 * for i in the stripe; the diagonal convention requires row0 + nrows <= M. */
size_t cmhse_sim_rank_workspace(int32_t nrows);
int cmhse_sim_rank(const float* A, const float* B, int32_t N, int32_t M, int32_t D, int32_t row0,
                   int32_t nrows, int32_t* rank, int32_t* top1, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Same, with an optional cmhse_timer (or NULL) whose event pair brackets the counting pass (the
 * N x M MFMA contraction with the rank / arg-max epilogue) on `stream` — measurement only. */
int cmhse_sim_rank_ex(const float* A, const float* B, int32_t N, int32_t M, int32_t D,
                      int32_t row0, int32_t nrows, int32_t* rank, int32_t* top1, void* workspace,
                      size_t workspace_bytes, void* stream, void* timer);

/* Top-K retrieval (no reference counterpart: what a user of a trained model asks first — the K
 * best videos for a paragraph, or the reverse).  For each row i of the stripe [row0, row0+nrows)
 * of d = A B^T (A [N,D] queries, B [M,D] gallery, exact-fp32 MFMA whatever the math mode):
 *   index[i - row0, :]  the K columns j with the largest d[i,j], by score descending, then by j
 *                       ascending on exact ties (the top1 rule of cmhse_sim_rank: the order of the
 *                       64-bit key (ordered bits of d[i,j]) << 32 | (0xFFFFFFFF - j), unique per row,
 *                       so the result depends on neither tiling nor scheduling);
 *   scores[i - row0, :] their scores, bit-identical to the same entries of cmhse_cosine_sim(A, B).
 * 1 <= K <= min(M, CMHSE_TOPK_MAX); K == M is a full stable descending sort of the row.  The N x M
 * matrix is never materialised; the workspace holds K keys per row for each of a few column panels,
 * a count fixed by nrows and K (LDS occupancy), not by M — 12 MB at nrows 4917, M 4917 or 10^6, K 50.
 * nrows == 0: nothing is launched (scores, index, workspace may be NULL).  Inputs are assumed finite;
 * otherwise the order is unspecified, but every index written lies in [0, M). */
#define CMHSE_TOPK_MAX 128
size_t cmhse_sim_topk_workspace(int32_t nrows, int32_t M, int32_t K);
int cmhse_sim_topk(const float* A, const float* B, int32_t N, int32_t M, int32_t D, int32_t row0,
                   int32_t nrows, int32_t K, float* scores /*[nrows,K]*/, int32_t* index /*[nrows,K]*/,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Labelled ranking (no reference counterpart: the reference's i2t / t2i, and cmhse_sim_rank with them,
 * can only rank query i against gallery row i).  Queries A [N,D], gallery B [M,D], N and M independent,
 * d = A B^T in exact fp32 (the MFMA k-chain of every scoring call here, whatever the math mode).  Every
 * query i of the stripe [row0, row0+nrows) has a non-empty list P_i of positives, gallery rows in
 * [0, M) (duplicates inside a list are harmless).  With thr[i] = max over p in P_i of d[i,p]:
 *   rank[i - row0]       = #{ j in [0, M) : d[i,j] > thr[i] }   the 0-based position of the best-placed
 *                          positive in the descending sort of row i.  Strict, no column excluded: no
 *                          positive beats thr[i], and a negative that ties it exactly is not counted
 *                          (the optimistic tie rule of cmhse_sim_rank);
 *   top1[i - row0]       = argmax_j d[i,j], smallest j on exact ties (as cmhse_sim_rank);
 *   best_pos[i - row0]   = the p in P_i with d[i,p] == thr[i], the smallest such p on exact ties (the
 *                          64-bit key of cmhse_sim_topk: independent of tiling and scheduling);
 *   best_score[i - row0] = the bits of d[i, best_pos] as the kernel computed them, never recomputed
 *                          (may be NULL).
 * With M >= N and P_i = {i}, rank and top1 equal cmhse_sim_rank's bit for bit.  Query stripes (their
 * labels sliced with them) concatenate bit for bit into the whole call.
 *
 * Labels are CSR relative to the stripe: pos_off[nrows+1] (0 first, strictly increasing: every query
 * has a positive; pos_off[nrows] == n_pairs) and pos_idx[n_pairs]; query row0 + q owns
 * pos_idx[pos_off[q] .. pos_off[q+1]).  Both arrays are passed twice, as cmhse_group_scores takes its
 * plan: the host copies are validated in full (O(n_pairs)) before anything is launched, the kernels
 * read the device copies, which must hold the same values.
 *
 * Returns CMHSE_ERR_ARG, before anything is launched, for: a null A / B / label / output pointer
 * (best_score excepted); N, M or D <= 0; a stripe outside [0, N]; n_pairs < nrows; pos_off_host[0] != 0,
 * a prefix sum that does not increase (an empty list), pos_off_host[nrows] != n_pairs; an index outside
 * [0, M).  CMHSE_ERR_WORKSPACE: workspace unaligned (256 bytes) or smaller than
 * cmhse_sim_rank_labelled_workspace(nrows, n_pairs) (0 for nrows <= 0 or n_pairs < nrows; otherwise
 * nrows thresholds and 2 x nrows keys — it does not grow with n_pairs).  nrows == 0 (with n_pairs == 0):
 * nothing is launched and every pointer but A and B may be NULL.
 *
 * Cost: a threshold pass of ceil(n_pairs / 128) tiles of 128 x 128 x D (the pairs in CSR order, operand
 * A row r = the query of pair r, operand B row c = the gallery row of pair c; the tile's diagonal holds
 * the pairs' scores, each folded into its query's key by a 64-bit atomic max), a launch that decodes
 * the keys, the counting pass of ceil(nrows / 128) x ceil(M / 128) tiles that cmhse_sim_rank runs (one
 * compare term fewer) and its top-1 pass.  With one positive per query that is cmhse_sim_rank's tile
 * work plus one small launch; the thresholds come out of the same MFMA chain as the scores they are
 * compared with, which is what makes the strict compare exact.  Inputs are assumed finite. */
size_t cmhse_sim_rank_labelled_workspace(int32_t nrows, int32_t n_pairs);
int cmhse_sim_rank_labelled(const float* A, const float* B, int32_t N, int32_t M, int32_t D, int32_t row0,
                            int32_t nrows, const int32_t* pos_off_host, const int32_t* pos_idx_host,
                            const int32_t* pos_off, const int32_t* pos_idx, int32_t n_pairs,
                            int32_t* rank /*[nrows]*/, int32_t* top1 /*[nrows]*/,
                            int32_t* best_pos /*[nrows]*/, float* best_score /*[nrows] or NULL*/,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Certified ranking: the ranks of the FLOAT64 scores of the same fp32 rows, at about the cost of
 * cmhse_sim_rank.  A [N,D], B [M,D], the stripe [row0, row0+nrows) with row0 + nrows <= M (the diagonal
 * convention of cmhse_sim_rank).  s64(i,j) is the float64 dot product of the fp32 rows i of A and j of B:
 * exact products, summed in ONE fixed order by ONE routine that serves every pair, (i,i) included (one
 * wave: lane l adds the terms k = l, l + 64, ... ascending by fused multiply-add from 0, then the 64
 * partial sums are added pairwise over lane distances 32, 16, 8, 4, 2, 1).  All outputs int32 [nrows]:
 *   rank_lo[i - row0]  = #{ j != i : s64(i,j) >  s64(i,i) }   the optimistic rule of cmhse_sim_rank, on
 *                        the float64 scores;
 *   rank_hi[i - row0]  = #{ j != i : s64(i,j) >= s64(i,i) }   the pessimistic rank: above rank_lo only on
 *                        exact float64 ties, which bit-identical gallery rows produce (a collapsed model
 *                        has rank_lo 0 and rank_hi M - 1 everywhere);
 *   top1[i - row0]     = cmhse_sim_rank's, by its fp32 rule, unchanged and NOT certified (the certified
 *                        arg-max is cmhse_sim_topk_exact with K = 1);
 *   resolved[i - row0] = the pairs of row i that went through float64: a diagnostic, deterministic
 *                        because the classification is.
 * How: the counting pass of cmhse_sim_rank with a per-row tolerance tol_i = 2 E_i, where E_i bounds
 * |v(i,j) - s64(i,j)| for the fp32 MFMA score v and every j (the fused-multiply-add chain bound
 * gamma_D |a_i| max_j |b_j|, gamma_D = D u / (1 - D u), u = 2^-24, plus the float64 routine's own error and
 * the rounding of the norm and tolerance arithmetic; derived in sim.hip).  v(i,j) - v(i,i) > tol_i: surely
 * above, counted in both ranks; v(i,i) - v(i,j) > tol_i: surely below; anything else is recomputed as
 * s64(i,j) and compared with s64(i,i), inside the tile that found it (no list of pairs, no capacity,
 * no second pass).
 * Properties: the results do not depend on the tolerance as long as it is valid (the tunable
 * "rank_exact_tol_scale" only moves `resolved`), nor on tiling or scheduling (integer counts; one k order
 * per routine); row stripes concatenate bit for bit into the whole call; the math mode does not matter
 * (scoring is exact fp32 whatever the mode, as everywhere else).  Inputs are assumed finite; D < 2^24
 * (CMHSE_ERR_UNSUPPORTED otherwise).
 * cmhse_sim_rank_exact_workspace(nrows) is a function of nrows alone (0 for nrows <= 0; about 32 bytes a
 * row).  Errors as cmhse_sim_rank's, before anything is launched: CMHSE_ERR_ARG for a null pointer, N, M or
 * D <= 0, a stripe outside [0, N] or row0 + nrows > M; CMHSE_ERR_WORKSPACE for a workspace that is
 * unaligned (256 bytes) or too small.  nrows == 0: nothing is launched.
 * Cost: cmhse_sim_rank's two passes, one wave per row of the stripe and of B in front (norms, s64(i,i)),
 * two small launches, and one wave-wide float64 dot product per undecided pair.
 *
 * cmhse_sim_rank_exact_tolerance(D, |a_i|, max_j |b_j|): tol_i as the kernel computes it (before the
 * tunable's factor and the rounding up to fp32); host-only, no GPU.  NaN for D <= 0 or a negative norm,
 * +inf for D >= 2^24. */
size_t cmhse_sim_rank_exact_workspace(int32_t nrows);
double cmhse_sim_rank_exact_tolerance(int32_t D, double norm_a, double norm_b_max);
int cmhse_sim_rank_exact(const float* A, const float* B, int32_t N, int32_t M, int32_t D, int32_t row0,
                         int32_t nrows, int32_t* rank_lo /*[nrows]*/, int32_t* rank_hi /*[nrows]*/,
                         int32_t* top1 /*[nrows]*/, int32_t* resolved /*[nrows]*/, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Certified labelled ranking: cmhse_sim_rank_exact's interval for cmhse_sim_rank_labelled's protocol — the
 * ranks of the FLOAT64 scores against any set of positives per query, any gallery size.  Queries A [N,D],
 * gallery B [M,D], N and M independent, the stripe [row0, row0+nrows).  Labels are CSR relative to the stripe,
 * passed as a host copy and a device copy, exactly as cmhse_sim_rank_labelled takes them, with ONE stricter
 * rule: the list of every query must be STRICTLY ASCENDING (sorted, no duplicate), else CMHSE_ERR_ARG — the
 * pessimistic rank needs the number of DISTINCT positives at the threshold (ops.sim_rank_labelled_exact sorts
 * and de-duplicates for its callers).
 * s64(i,j) is the float64 dot product of cmhse_sim_rank_exact: the ONE routine, its lane order and its
 * butterfly, for every float64 score of the call, the thresholds included.  With P_i the list of query i and
 * thr64(i) = max over p in P_i of s64(i,p), all outputs [nrows]:
 *   rank_lo[i - row0]    = #{ j in [0,M) : s64(i,j) > thr64(i) }   cmhse_sim_rank_labelled's optimistic rule
 *                          on the float64 scores;
 *   rank_hi[i - row0]    = rank_lo + #{ j not in P_i : s64(i,j) == thr64(i) }   the position of the best-placed
 *                          positive if every exact tie with a NEGATIVE goes against it; a positive that ties
 *                          the best positive is never counted.  Above rank_lo only on exact float64 ties (a
 *                          collapsed model: rank_lo 0, rank_hi M - |P_i|);
 *   top1[i - row0]       = cmhse_sim_rank_labelled's, by its fp32 rule, unchanged and NOT certified (the
 *                          certified arg-max is cmhse_sim_topk_exact with K = 1);
 *   best_pos[i - row0]   = the p in P_i with s64(i,p) == thr64(i), the smallest such p;
 *   best_score[i - row0] = thr64(i), float64 (may be NULL);
 *   resolved[i - row0]   = the columns of row i that went through float64 in the counting pass: a diagnostic,
 *                          a function of the inputs alone, >= 1 (the best positive's own column always lies
 *                          inside the tolerance).
 * How: (1) one wave per row of the stripe and of B: |a_i|, zeroed counters, max_j |b_j|, then tol_i = 2 E_i
 * (1 + 2^-18) rounded up to fp32, the tolerance of cmhse_sim_rank_exact; (2) the float64 threshold pass: one
 * wave per (query, positive) pair writes its s64 into a vector of n_pairs doubles, then one wave per query
 * reduces its list to thr64, best_pos and the number of list entries at thr64 — no floating-point atomics,
 * nothing that depends on who arrives first; (3) the counting pass of cmhse_sim_rank_exact, no column excluded,
 * against thr32(i) = float(thr64(i)): fl(v(i,j) - thr32(i)) > tol_i: surely above; < -tol_i: surely below;
 * anything else is recomputed as s64(i,j) and compared with thr64(i) inside the tile that found it.  The
 * tolerance is valid unchanged because |thr32 - thr64| <= u |thr64| (or 2^-150) <= E_i takes the place of the
 * diagonal's |v(i,i) - s64(i,i)| <= E_i (derived in sim.hip); (4) rank_hi = rank_lo + ties - (list entries at
 * thr64), and top1 is decoded.
 * Properties: the results do not depend on the tolerance as long as it is valid (the tunable
 * "rank_exact_tol_scale" only moves `resolved`), nor on tiling, scheduling or math mode; query stripes, with
 * their labels sliced, concatenate bit for bit into the whole call; with M >= N and P_i = {i}, rank_lo and
 * rank_hi equal cmhse_sim_rank_exact's.  Inputs are assumed finite; D < 2^24 (CMHSE_ERR_UNSUPPORTED otherwise).
 * Errors, before anything is launched, with the codes and in the order of cmhse_sim_rank_labelled:
 * CMHSE_ERR_ARG for a null A / B; N, M or D <= 0; a stripe outside [0, N]; (nrows == 0 with n_pairs == 0:
 * nothing is launched and every pointer but A and B may be NULL; nrows == 0 with other n_pairs: CMHSE_ERR_ARG;)
 * a null label pointer or n_pairs < nrows; pos_off_host[0] != 0, pos_off_host[nrows] != n_pairs, a prefix sum
 * that does not increase (an empty list); an index outside [0, M); a list that is not strictly ascending; a
 * null rank_lo / rank_hi / top1 / best_pos / resolved / workspace.  Then CMHSE_ERR_WORKSPACE for a workspace
 * that is unaligned (256 bytes) or smaller than cmhse_sim_rank_labelled_exact_workspace(nrows, n_pairs), then
 * CMHSE_ERR_UNSUPPORTED for D >= 2^24.
 * cmhse_sim_rank_labelled_exact_workspace(nrows, n_pairs): 0 for nrows <= 0 or n_pairs < nrows; otherwise
 * about 36 bytes a row AND 8 bytes a pair — unlike cmhse_sim_rank_labelled's it grows with n_pairs (the
 * float64 score of every pair is kept for the deterministic reduction).
 * Cost: cmhse_sim_rank_exact's without its diagonal pass, plus one wave-wide float64 dot product per pair. */
size_t cmhse_sim_rank_labelled_exact_workspace(int32_t nrows, int32_t n_pairs);
int cmhse_sim_rank_labelled_exact(const float* A, const float* B, int32_t N, int32_t M, int32_t D, int32_t row0,
                                  int32_t nrows, const int32_t* pos_off_host, const int32_t* pos_idx_host,
                                  const int32_t* pos_off, const int32_t* pos_idx, int32_t n_pairs,
                                  int32_t* rank_lo /*[nrows]*/, int32_t* rank_hi /*[nrows]*/,
                                  int32_t* top1 /*[nrows]*/, int32_t* best_pos /*[nrows]*/,
                                  double* best_score /*[nrows] or NULL*/, int32_t* resolved /*[nrows]*/,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* Certified top-K retrieval: the K best columns of every row by the FLOAT64 scores of the same fp32 rows, at
 * about twice the cost of cmhse_sim_topk.  A [N,D] queries, B [M,D] gallery, N and M independent (no diagonal
 * convention), the stripe [row0, row0+nrows).  s64(i,j) is the float64 dot product of cmhse_sim_rank_exact:
 * the ONE routine with its lane order and its butterfly.  For every row i of the stripe:
 *   index[i - row0, :]   the first K columns in the order (s64(i,j) descending, then j ascending): the tie
 *                        rule of cmhse_sim_topk and of top1, applied to the float64 scores.  Two scores that
 *                        compare equal as doubles tie (-0.0 and +0.0 included);
 *   scores[i - row0, :]  those s64 values, float64;
 *   resolved[i - row0]   the columns of row i that went through float64: a diagnostic, >= K, a function of
 *                        the inputs alone.
 * How: (1) cmhse_sim_topk into a private region: v_K(i), the K-th fp32 score of the row; (2) one wave per row
 * of the stripe and of B: |a_i|, max_j |b_j|, and tol_i = 2 E_i (1 + 2^-18) rounded up to fp32, the tolerance
 * of cmhse_sim_rank_exact (cmhse_sim_rank_exact_tolerance); (3) a second tile pass of the same shape whose
 * scores are bit-identical to (1)'s: every column with fl(v_K(i) - v(i,j)) <= tol_i is a candidate, gets its
 * s64 inside the tile that found it, and is merged into the row's list of K (float64 bits, column) pairs in
 * LDS; (4) one wave per row merges the column panels' lists.  No list of pairs, no capacity, no retry.
 * Why it is exact: the K columns of the fp32 list have v >= v_K, so s64 >= v_K - E_i, so the K-th largest
 * s64 of the row is >= v_K - E_i; a member of the float64 top-K has s64 at least that (on a tie at the
 * boundary too), so v >= v_K - 2 E_i: it is a candidate, and the exact top-K of a superset of the top-K is
 * the top-K (derived in topk.hip).
 * Properties: the result does not depend on the tolerance as long as it is valid (the tunable
 * "rank_exact_tol_scale" multiplies it and only moves `resolved`), nor on tiling, panel count or scheduling;
 * row stripes concatenate bit for bit; the math mode does not matter.  Inputs are assumed finite.
 * 1 <= K <= min(M, CMHSE_TOPK_MAX).  Errors, before anything is launched, with the codes and in the order of
 * cmhse_sim_topk: CMHSE_ERR_ARG for a null A / B, N, M or D <= 0, K outside its range, a stripe outside
 * [0, N]; nrows == 0: nothing is launched and every other pointer may be NULL; CMHSE_ERR_ARG for a null
 * scores / index / resolved / workspace; CMHSE_ERR_WORKSPACE for a workspace that is unaligned (256 bytes) or
 * too small; CMHSE_ERR_UNSUPPORTED for D >= 2^24 (the bound needs D u < 1).
 * cmhse_sim_topk_exact_workspace(nrows, M, K) (0 for nrows, M <= 0 or K outside [1, CMHSE_TOPK_MAX]):
 * cmhse_sim_topk_workspace(nrows, M, K) and that call's two outputs (8 bytes x nrows x K), 12 bytes a row of
 * norm and tolerance (v_K is read from the fp32 list in place), and per column panel 12 bytes x nrows x K of
 * pairs and 4 x nrows of counts.  The panel count follows cmhse_sim_topk's rule with this pass's LDS size
 * (64 x K x 12 bytes of lists): fixed by nrows and K, not by M — 30 MB at nrows 4917, M 4917 or 10^6, K 50.
 * The size is NOT monotone in nrows or K (nor is cmhse_sim_topk_workspace): the panel count is a floor,
 * 256 x (workgroups per CU) / row tiles, so a larger stripe or K can need less (K = 1, M = 4917: nrows 5440
 * needs more than nrows 5504).  Size the buffer for the call it serves; a buffer sized for the largest stripe
 * is not thereby large enough for a smaller one. */
size_t cmhse_sim_topk_exact_workspace(int32_t nrows, int32_t M, int32_t K);
int cmhse_sim_topk_exact(const float* A, const float* B, int32_t N, int32_t M, int32_t D, int32_t row0,
                         int32_t nrows, int32_t K, double* scores /*[nrows,K]*/, int32_t* index /*[nrows,K]*/,
                         int32_t* resolved /*[nrows]*/, void* workspace, size_t workspace_bytes, void* stream);

/* Group-wise video <-> paragraph scores and ranking from the low-level rows (the score
 * GroupWiseContrastiveLoss trains on, loss.py:26-41; upstream's validate() has its evaluation
 * commented out, train.py:228-244).  clips [Nc, D] and caps [Ns, D] are encode_data's clip and
 * caption rows (already normalised: nothing is normalised here); video b owns the clip rows
 * [clip_off[b], clip_off[b+1]), paragraph b the caption rows [cap_off[b], cap_off[b+1]).
 *   G[i, j]  over the block (clips of video i) x (captions of paragraph j) of the fp32 scores
 *            clips[r] . caps[c] (exact-fp32 MFMA, each bit-identical to cmhse_cosine_sim's):
 *            CMHSE_GROUP_MAX   the block maximum;
 *            CMHSE_GROUP_MEAN  the scores summed in fp64 sequentially in row-major order (clip-major,
 *                              then caption), divided in fp64 by the count, rounded to fp32 — for
 *                              blocks of at most 256 entries the order of cmhse_groupwise_fwd's
 *                              `reduced`, so bit-identical to it there.
 * The clip x caption matrix never reaches HBM: whole videos are packed into row tiles of at most 128
 * clip rows and whole paragraphs into column tiles of at most 128 caption rows, and each workgroup
 * reduces the blocks of its tile in its epilogue (no atomics, no partials).
 *
 * cmhse_group_plan (host only, no GPU needed): from the host prefix sums clip_off_host[B+1] and
 * cap_off_host[B+1] (0 first, strictly increasing: every count >= 1) fills plan[0, len) and returns
 * len, or CMHSE_ERR_ARG (null pointer, B <= 0, bad prefix sums), CMHSE_ERR_UNSUPPORTED (a video or
 * paragraph of more than 128 rows), CMHSE_ERR_WORKSPACE (plan_cap < CMHSE_GROUP_PLAN_MAX(B)).
 * Layout (int32): B, Nc, Ns, R row tiles, C column tiles, clip_off[B+1], cap_off[B+1], the first
 * video of each row tile [R+1] (ending in B), the first paragraph of each column tile [C+1].
 * The caller uploads plan[0, len) to the device; the calls below take both copies: the host copy is
 * validated in full (O(B)) and sizes the launch, the kernels read the device copy, which must hold
 * the same values.  The count vectors need not be equal (num_caps != num_clips).
 *
 * cmhse_group_scores: G [B, B] row-major (video i, paragraph j).  No workspace.
 * cmhse_group_rank: the ranks of cmhse_sim_rank applied to G with its diagonal —
 *   rank_v2p[i] = #{j != i : G[i,j] > G[i,i]},  top1_v2p[i] = the j of the largest G[i,j], smallest j
 *   on ties; rank_p2v / top1_p2v the same over the columns (j -> i).  G lives in the workspace
 *   (cmhse_group_rank_workspace(B): B^2 floats + per-64-tile partials, 106 MB at B = 4917).
 * Exact fp32 whatever the math mode.  Argument errors are returned before anything is launched. */
#define CMHSE_GROUP_MEAN 0
#define CMHSE_GROUP_MAX 1
#define CMHSE_GROUP_PLAN_MAX(B) (4 * (B) + 9)
#define CMHSE_GROUP_TILE_ROWS 128   /* the most clip / caption rows of a tile, so of a video / paragraph */
int32_t cmhse_group_plan(const int32_t* clip_off_host, const int32_t* cap_off_host, int32_t B,
                         int32_t* plan, int32_t plan_cap);
int cmhse_group_scores(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                       int32_t B, const int32_t* plan_host, const int32_t* plan, int32_t plan_len,
                       int32_t reduce, float* G /*[B,B]*/, void* stream);
size_t cmhse_group_rank_workspace(int32_t B);
int cmhse_group_rank(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                     int32_t B, const int32_t* plan_host, const int32_t* plan, int32_t plan_len,
                     int32_t reduce, int32_t* rank_v2p, int32_t* top1_v2p, int32_t* rank_p2v,
                     int32_t* top1_p2v, void* workspace, size_t workspace_bytes, void* stream);

/* Certified group-wise ranking: the ranks of the FLOAT64 block scores of the same fp32 rows, as an interval, at
 * about the cost of cmhse_group_rank.  Inputs as for cmhse_group_rank (counts 1..128 rows, num_caps != num_clips
 * allowed, both reduce modes).
 * G64(i, j), THE float64 block score — one device routine (exact64.hpp: block64) serves every float64 group
 * score of the call, the diagonal's included:
 *   s64(r, c) = the float64 dot product of cmhse_sim_rank_exact (dot64: its lane order, its butterfly) of clip
 *               row r of video i and caption row c of paragraph j, rows ascending;
 *   CMHSE_GROUP_MAX   G64 = max s64(r, c): nothing is rounded, so the order does not matter;
 *   CMHSE_GROUP_MEAN  acc = 0.0; for r: for c: acc += s64(r, c) — sequential float64, clip-major then caption,
 *                     the order of cmhse_group_scores' fp32 mean — then G64 = acc / double(count).
 * Consequence: two bit-identical groups with their rows in the same order have bit-identical G64 against
 * anything, so they tie exactly.  Under CMHSE_GROUP_MEAN a paragraph whose captions are permuted need not
 * (float64 addition does not associate), nor need groups of equal rows but different counts.
 * Outputs, all int32 [B]; v2p: query = video i, its row of G64; p2v: query = paragraph j, its column:
 *   rank_lo[q]  = #{ k != q : G64(line q)[k] >  G64[q, q] }   the optimistic rule of cmhse_group_rank;
 *   rank_hi[q]  = #{ k != q : G64(line q)[k] >= G64[q, q] }   above rank_lo only on exact float64 ties (a
 *                 collapsed model of equal groups has rank_lo 0 and rank_hi B - 1 everywhere);
 *   top1[q]     = cmhse_group_rank's fp32 arg-max, unchanged and NOT certified;
 *   resolved[q] = the off-diagonal blocks of that query whose comparison went through float64: a function of
 *                 the input (and the tunable below) alone.
 * How: cmhse_group_rank's launches with a tolerance per query.  With E(|a|, |b|) the bound of
 * cmhse_sim_rank_exact on |v - s64| for one fp32 MFMA score, A_i the largest clip norm of video i and Bmax the
 * largest caption norm of the call: |G32[i,j] - G64(i,j)| <= E(A_i, Bmax) under max (a maximum is 1-Lipschitz and
 * rounds nothing), and E plus (u + 2^-38) A_i Bmax under mean (the two float64 summations of at most 2^14 terms
 * and the rounding of the mean to fp32); p2v swaps the roles (B_j, the largest clip norm of the call).  The
 * tolerance is twice that, times 1 + 2^-18, rounded up to fp32 (derived in exact64.hpp).  A difference from the
 * diagonal score beyond it decides the float64 comparison; every other block — two blocks that tie exactly
 * among them — is recomputed with block64 inside the 64 x 64 tile of G that found it, once even when both
 * directions want it (no list of pairs, no capacity, no retry).
 * Properties: the results do not depend on the tolerance as long as it is valid ("rank_exact_tol_scale"
 * multiplies it here too and only moves `resolved`; at 2^20 and D >= 16 every off-diagonal block goes through
 * float64), nor on tiling or scheduling (integer counts).  Inputs are assumed finite; D < 2^24
 * (CMHSE_ERR_UNSUPPORTED otherwise).
 * cmhse_group_rank_exact_workspace(B, Nc, Ns): cmhse_group_rank_workspace(B) plus O(B + Nc + Ns) vectors,
 * 256-byte aligned; 0 for B <= 0, Nc < B or Ns < B.  Errors, before anything is launched: CMHSE_ERR_ARG as
 * cmhse_group_rank's (a group of more than 128 rows is cmhse_group_plan's CMHSE_ERR_UNSUPPORTED), then
 * CMHSE_ERR_WORKSPACE for a workspace that is unaligned (256 bytes) or too small.
 * Cost: cmhse_group_rank's, one wave per clip / caption row in front (norms), one wave per group (G64[i, i]),
 * two small launches, and one block64 per undecided block.
 *
 * cmhse_group_rank_exact_tolerance(D, reduce, A_i, Bmax): the tolerance as the kernel computes it (before the
 * tunable's factor and the rounding up to fp32); host-only, no GPU.  NaN for D <= 0, a bad reduce or a negative
 * norm, +inf for D >= 2^24. */
size_t cmhse_group_rank_exact_workspace(int32_t B, int32_t Nc, int32_t Ns);
double cmhse_group_rank_exact_tolerance(int32_t D, int32_t reduce, double norm_a, double norm_b_max);
int cmhse_group_rank_exact(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                           int32_t B, const int32_t* plan_host, const int32_t* plan, int32_t plan_len,
                           int32_t reduce, int32_t* rank_lo_v2p, int32_t* rank_hi_v2p, int32_t* top1_v2p,
                           int32_t* resolved_v2p, int32_t* rank_lo_p2v, int32_t* rank_hi_p2v, int32_t* top1_p2v,
                           int32_t* resolved_p2v, void* workspace, size_t workspace_bytes, void* stream);

/* Group-wise top-K retrieval: the K best gallery groups of every query group by the block score
 * above, for any video set and any paragraph set (Bv videos of clips, Bp paragraphs of caps: Bv and
 * Bp independent, every count 1..CMHSE_GROUP_TILE_ROWS rows).
 *   CMHSE_GROUP_P2V  every paragraph j is a query, the videos are the gallery: [Bp, K] results;
 *   CMHSE_GROUP_V2P  every video i is a query, the paragraphs are the gallery: [Bv, K] results.
 *   scores[q, :]  the block scores, bit-identical to the reduction cmhse_group_scores computes (in
 *                 the square case the same entries of its G, in both reduce modes: the mean stays
 *                 clip-major, then caption, with the fp64 sum, whichever side is the query);
 *   index[q, :]   their gallery groups, by score descending, then by index ascending on exact ties
 *                 (the 64-bit key of cmhse_sim_topk, unique per query: the result depends on neither
 *                 tiling nor scheduling, and K == gallery size is a full stable sort).
 * 1 <= K <= min(gallery groups, CMHSE_TOPK_MAX).  Exact fp32 whatever the math mode.  Neither the
 * Nc x Ns clip x caption matrix nor the Bq x Bg matrix of block scores is stored: each workgroup holds
 * one query tile and walks a panel of gallery tiles, reducing each tile's blocks in LDS and merging
 * them into per-query sorted lists; a second pass merges the panels' lists.  The panel count fills
 * the CUs once, so the workspace (panels x Bq x K keys) is fixed by the query side and K, not by the
 * gallery (once the gallery has as many tiles as there are panels).  A query subset is a smaller call
 * with its rows and counts sliced: the results of query stripes concatenate bit for bit into the
 * whole call's.
 *
 * cmhse_group_topk_plan (host only, no GPU needed): from the host prefix sums clip_off_host[Bv+1] and
 * cap_off_host[Bp+1] (0 first, strictly increasing) fills plan[0, len) and returns len, or
 * CMHSE_ERR_ARG (null pointer, Bv or Bp <= 0, bad prefix sums, bad direction, K outside
 * [1, min(gallery groups, CMHSE_TOPK_MAX)]), CMHSE_ERR_UNSUPPORTED (a video or paragraph of more than
 * 128 rows), CMHSE_ERR_WORKSPACE (plan_cap < CMHSE_GROUP_TOPK_PLAN_MAX(Bv, Bp)).  Layout (int32):
 * Bv, Bp, Nc, Ns, direction, K, R clip tiles, C caption tiles, clip_off[Bv+1], cap_off[Bp+1], the
 * first video of each clip tile [R+1], the first paragraph of each caption tile [C+1].  The gallery
 * side packs as cmhse_group_plan does (whole groups, <= 128 rows a tile); the query side also caps
 * the groups of a tile at a number derived from K (the LDS its lists take).  As for cmhse_group_scores
 * the caller uploads plan[0, len) and passes both copies; direction and K are recorded in the plan and
 * must equal the call's.
 * cmhse_group_topk_workspace: bytes for the plan (0 for an invalid plan), 256-byte aligned.
 * Argument errors are returned before anything is launched. */
#define CMHSE_GROUP_P2V 0
#define CMHSE_GROUP_V2P 1
#define CMHSE_GROUP_TOPK_PLAN_MAX(Bv, Bp) (2 * (Bv) + 2 * (Bp) + 12)
int32_t cmhse_group_topk_plan(const int32_t* clip_off_host, int32_t Bv, const int32_t* cap_off_host,
                              int32_t Bp, int32_t direction, int32_t K, int32_t* plan, int32_t plan_cap);
size_t cmhse_group_topk_workspace(const int32_t* plan_host, int32_t plan_len);
int cmhse_group_topk(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                     const int32_t* plan_host, const int32_t* plan, int32_t plan_len, int32_t direction,
                     int32_t reduce, int32_t K, float* scores /*[Bq,K]*/, int32_t* index /*[Bq,K]*/,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Certified group-wise top-K retrieval: the K best gallery groups of every query group by the FLOAT64 block
 * scores of the same fp32 rows, at about twice the cost of cmhse_group_topk plus one block64 per candidate.
 * Inputs as for cmhse_group_topk: any video set against any paragraph set (Bv and Bp independent, every count
 * 1..CMHSE_GROUP_TILE_ROWS rows), both directions, both reduce modes.  G64 is THE float64 block score of
 * cmhse_group_rank_exact (exact64.hpp: block64, the same routine, the same bits).  For every query group q:
 *   index[q, :]   the first K gallery groups in the order (G64 descending, then gallery index ascending): the
 *                 tie rule of cmhse_group_topk, applied to the float64 scores.  Two scores that compare equal as
 *                 doubles tie (-0.0 and +0.0 included);
 *   scores[q, :]  those G64 values, float64;
 *   resolved[q]   the gallery groups of query q that went through block64: a diagnostic, >= K, a function of
 *                 the inputs and of the tunable "rank_exact_tol_scale" alone (nothing is skipped in a
 *                 data-dependent way).
 * How: (1) cmhse_group_topk, its kernels unchanged, into a private region of the workspace: G_K(q), the K-th
 * fp32 block score of the query (first, so all it can refuse is refused before anything is launched); (2) one
 * wave per clip and caption row: its norm, the largest norm of each side rounded up to fp32, and per query
 * group tol_q = cmhse_group_rank_exact_tolerance(D, reduce, A_q, Bmax) x "rank_exact_tol_scale" rounded up to
 * fp32 (A_q the largest norm of the query's rows, Bmax the largest of the gallery side: for p2v the paragraph's
 * largest caption norm against the largest clip norm of the call); (3) a second pass of cmhse_group_topk's grid
 * whose fp32 block scores are bit-identical to (1)'s: every gallery group with fl(G_K(q) - G32(q,g)) <= tol_q is
 * a candidate, gets its block64 inside the tile that found it, and is merged into the query's list of K
 * (float64 bits, index) pairs in LDS; (4) one wave per query merges the gallery panels' lists and sums their
 * counts.  No list of pairs in memory, no capacity, no retry; nothing waits on another workgroup.
 * Why it is exact: |G32(q,g) - G64(q,g)| <= E_q for every g (the bound of cmhse_group_rank_exact, row-wise for
 * a video query, column-wise for a paragraph query; tol_q = 2 E_q (1 + 2^-18)).  The K groups of the fp32 list
 * have G32 >= G_K, so the K-th largest G64 of the query is >= G_K - E_q; a member of the float64 top-K has G64 at
 * least that (on a tie at the boundary too), so G32 >= G_K - 2 E_q: it is a candidate, and the exact top-K of a
 * superset of the top-K is the top-K (derived in group.hip).
 * Properties: the results do not depend on the tolerance as long as it is valid (the tunable only moves
 * `resolved`; at 2^20 and D >= 16 every gallery group goes through float64), nor on tiling, panel count,
 * scheduling or math mode; query subsets concatenate bit for bit.  Inputs are assumed finite.
 *
 * cmhse_group_topk_exact_plan (host only): cmhse_group_topk_plan's layout, arguments and errors; the query side
 * is capped by THIS pass's LDS (a list entry is 12 bytes here, 8 there), by the same rule and never above
 * cmhse_group_topk_plan's cap, so the plan serves the nested fp32 call too.  A plan of cmhse_group_topk_plan
 * whose query tiles exceed the cap is refused by the two calls below (workspace 0, CMHSE_ERR_ARG).
 * cmhse_group_topk_exact_workspace: bytes for the plan (0 for an invalid one), 256-byte aligned:
 * cmhse_group_topk_workspace and that call's two outputs (8 bytes x Bq x K), 8 bytes per row of the query side,
 * 4 per query group, and per gallery panel 12 bytes x Bq x K of pairs and 4 x Bq of counts.  The panel count
 * follows cmhse_group_topk's rule with this pass's LDS size: fixed by the query side and K, not by the gallery
 * (once the gallery has as many tiles as there are panels).
 * Errors, before anything is launched, with the codes and in the order of cmhse_group_topk: CMHSE_ERR_ARG for a
 * null pointer (scores / index / resolved / workspace included), Nc, Ns or D <= 0, a bad reduce, a plan that
 * fails cmhse_group_topk's check, disagrees with the call or exceeds this pass's cap; CMHSE_ERR_WORKSPACE for a
 * workspace that is unaligned (256 bytes) or too small; CMHSE_ERR_UNSUPPORTED for D >= 2^24 (the bound needs
 * D u < 1). */
int32_t cmhse_group_topk_exact_plan(const int32_t* clip_off_host, int32_t Bv, const int32_t* cap_off_host,
                                    int32_t Bp, int32_t direction, int32_t K, int32_t* plan, int32_t plan_cap);
size_t cmhse_group_topk_exact_workspace(const int32_t* plan_host, int32_t plan_len);
int cmhse_group_topk_exact(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                           const int32_t* plan_host, const int32_t* plan, int32_t plan_len, int32_t direction,
                           int32_t reduce, int32_t K, double* scores /*[Bq,K]*/, int32_t* index /*[Bq,K]*/,
                           int32_t* resolved /*[Bq]*/, void* workspace, size_t workspace_bytes, void* stream);

/* Labelled group-wise ranking (no reference counterpart): cmhse_sim_rank_labelled's protocol on the block
 * score above — any video set against any paragraph set (Bv videos of clips [Nc, D], Bp paragraphs of caps
 * [Ns, D]: Bv and Bp independent, every count 1..CMHSE_GROUP_TILE_ROWS rows), any set of correct gallery groups
 * per query group, matrix-free.
 *   CMHSE_GROUP_P2V  every paragraph is a query, the videos are the gallery (Bq = Bp, Bg = Bv);
 *   CMHSE_GROUP_V2P  every video is a query, the paragraphs are the gallery (Bq = Bv, Bg = Bp).
 * G(q, g) is the block score of cmhse_group_scores / cmhse_group_topk, bit for bit, in both reduce modes: always
 * the clips x captions tile, reduced clip-major then caption, with the fp64 sum for the mean, whichever side is
 * the query.  Every query group q has a non-empty list P_q of gallery groups in [0, Bg) (duplicates inside a list
 * are harmless).  With thr[q] = max over p in P_q of G(q, p), all outputs [Bq]:
 *   rank[q]       = #{ g in [0, Bg) : G(q, g) > thr[q] }   the 0-based position of the best-placed positive.
 *                   Strict, no gallery group excluded: no positive beats thr[q], and a negative that ties it
 *                   exactly is not counted (the optimistic tie rule of cmhse_sim_rank_labelled);
 *   top1[q]       = argmax_g G(q, g), the smaller g on exact ties (the 64-bit score key of cmhse_group_topk);
 *   best_pos[q]   = the p in P_q with G(q, p) == thr[q], the smallest such p on exact ties;
 *   best_score[q] = the bits of G(q, best_pos[q]) as the kernel computed them, never recomputed (may be NULL).
 * Properties:
 *   - Square case: with Bv == Bp and P_q = {q}, rank and top1 equal cmhse_group_rank's for that direction, bit
 *     for bit (its rank excludes the diagonal, which never beats itself).
 *   - Stripes: a query subset is a smaller call with its rows, counts and labels sliced; the results of query
 *     stripes concatenate bit for bit into the whole call's.
 *   - The result depends on neither tiling, panel count, scheduling nor math mode: counts and 64-bit keys are
 *     integers, and the thresholds come out of the same MFMA chain and the same block reduction as the scores
 *     they are compared with, which is what makes the strict compare exact.  No float atomics anywhere.
 *   - Workspace: one 8-byte key per query group, and per gallery panel one 4-byte count and one 8-byte key per
 *     query group: O(panels x Bq) + O(Bq).  It never holds Bq x Bg or Nc x Ns values; the panel count follows
 *     cmhse_group_topk's rule (it fills the CUs once), so past that count the workspace does not grow with the
 *     gallery.  At Bv = Bp = 4917 (val_1): under 1 MB, against cmhse_group_rank's 106 MB.
 *   - No device memory is written from host memory inside the call: everything the kernels read — offsets,
 *     tiles, labels, pair tiles — arrives in the plan the caller uploads.
 *
 * cmhse_group_rank_labelled_plan (host only, no GPU needed): from the host prefix sums clip_off_host[Bv+1] and
 * cap_off_host[Bp+1] (0 first, strictly increasing) and the labels as CSR over the query groups —
 * pos_off_host[Bq+1] (0 first, strictly increasing: every query has a positive; pos_off_host[Bq] == n_pairs)
 * and pos_idx_host[n_pairs]; query q owns pos_idx_host[pos_off_host[q] .. pos_off_host[q+1]) — fills
 * plan[0, len) and returns len, or
 *   CMHSE_ERR_ARG          a null pointer; Bv or Bp <= 0; a bad direction; bad prefix sums; pos_off_host[0] != 0,
 *                          an empty list, pos_off_host[Bq] != n_pairs; an index outside [0, Bg);
 *   CMHSE_ERR_UNSUPPORTED  a video or paragraph of more than 128 rows (or a plan beyond int32);
 *   CMHSE_ERR_WORKSPACE    plan_cap < CMHSE_GROUP_RANK_LABELLED_PLAN_MAX(Bv, Bp, n_pairs).
 * The labels are validated in full here (O(n_pairs)).  Layout (int32): Bv, Bp, Nc, Ns, direction, R clip tiles,
 * C caption tiles, n_pairs, T pair tiles, the query cap; clip_off[Bv+1], cap_off[Bp+1], the first video of each
 * clip tile [R+1], the first paragraph of each caption tile [C+1], pos_off[Bq+1], pos_idx[n_pairs], the first
 * pair of each pair tile [T+1].  The gallery side packs as cmhse_group_plan does (whole groups, <= 128 rows a
 * tile); the query side also caps the groups of a tile at 72 (the LDS a query group takes here: no K lists, so
 * the cap lies above cmhse_group_topk_plan's).  Pair tiles: the (query, positive) pairs in CSR order, whole
 * pairs packed greedily while the clip rows and the caption rows of a tile both stay <= 128 (a query with many
 * or long positives spans several tiles).  The caller uploads plan[0, len) and passes both copies: the host
 * copy is validated in full (O(Bv + Bp + n_pairs)) and sizes the launches, the kernels read the device copy,
 * which must hold the same values.  The direction is recorded in the plan and must equal the call's.
 * cmhse_group_rank_labelled_workspace: bytes for the plan (0 for an invalid plan), 256-byte aligned.
 *
 * cmhse_group_rank_labelled returns, before anything is launched: CMHSE_ERR_ARG for a null pointer (best_score
 * excepted); Nc, Ns or D <= 0; a bad reduce or direction; a plan that fails the check above or disagrees with
 * the call (Nc, Ns, direction, its length); then CMHSE_ERR_WORKSPACE for a workspace that is unaligned (256
 * bytes) or smaller than cmhse_group_rank_labelled_workspace.
 * Cost: a threshold pass of T tiles of 128 x 128 x D (operand rows gathered by address; each tile's diagonal
 * blocks folded into their queries' keys by a 64-bit atomic max), the counting pass — cmhse_group_topk's grid of
 * query tiles x gallery panels, i.e. the tile work of cmhse_group_scores once — and one small launch.  Inputs
 * are assumed finite.  Exact fp32 whatever the math mode. */
#define CMHSE_GROUP_RANK_LABELLED_PLAN_MAX(Bv, Bp, n_pairs) (3 * (Bv) + 3 * (Bp) + 2 * (n_pairs) + 16)
int32_t cmhse_group_rank_labelled_plan(const int32_t* clip_off_host, int32_t Bv, const int32_t* cap_off_host,
                                       int32_t Bp, int32_t direction, const int32_t* pos_off_host,
                                       const int32_t* pos_idx_host, int32_t n_pairs, int32_t* plan,
                                       int32_t plan_cap);
size_t cmhse_group_rank_labelled_workspace(const int32_t* plan_host, int32_t plan_len);
int cmhse_group_rank_labelled(const float* clips, const float* caps, int32_t Nc, int32_t Ns, int32_t D,
                              const int32_t* plan_host, const int32_t* plan, int32_t plan_len, int32_t direction,
                              int32_t reduce, int32_t* rank /*[Bq]*/, int32_t* top1 /*[Bq]*/,
                              int32_t* best_pos /*[Bq]*/, float* best_score /*[Bq] or NULL*/, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Replaces loss.cosine_sim (loss.py:12-13): scores[n,m] = im s^T, exact fp32. */
int cmhse_cosine_sim(const float* im, const float* s, int32_t n, int32_t m, int32_t D,
                     float* scores, void* stream);

/* Replaces loss.ContrastiveLoss.forward (loss.py:86-117) for im [n,D], s [n,D]:
 *   cost_s = max(0, margin + S - diag_i), cost_im = max(0, margin + S - diag_j), diagonals cleared,
 *   max_violation: row/column maxima instead of all entries; norm: divide by n*n.
 * Writes the scalar loss to *loss (device).  `scores_out` ([n,n], may be NULL -> kept in the
 * workspace) receives the score matrix (needed by the backward pass). */
size_t cmhse_contrastive_workspace(int32_t n);
int cmhse_contrastive_fwd(const float* im, const float* s, int32_t n, int32_t D, float margin,
                          int32_t max_violation, int32_t norm, float* loss, float* scores_out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Batched form of cmhse_contrastive_fwd for evaluation.encode_data's per-loader-batch 'Letest'
 * loss (evaluation.py:129 -> model.py:287-292): block b is the square problem on rows
 * [blk_off[b], blk_off[b+1]) of im and s (blk_off: device int32 [n_blocks+1], block sizes
 * <= max_n); losses[b] receives its loss.  One launch set for all blocks instead of one per
 * loader batch. */
size_t cmhse_contrastive_blocks_workspace(int32_t n_blocks, int32_t max_n);
int cmhse_contrastive_blocks_fwd(const float* im, const float* s, const int32_t* blk_off,
                                 int32_t n_blocks, int32_t max_n, int32_t D, float margin,
                                 int32_t max_violation, int32_t norm, float* losses,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Backward of cmhse_contrastive_blocks_fwd — what loss.backward() (model.py:367) computes through
 * the 4-7 ContrastiveLoss calls of a training step (model.py:333-343) when they are evaluated as
 * blocks of two row-blocked matrices: `scores` is the forward call's workspace (block b's stored
 * n_b x n_b scores at scores + b * max_n * max_n floats), grad_out[b] (device) the upstream gradient
 * of losses[b]; d_im / d_s ([rows, D], same row blocking as im / s) receive the gradients.  One
 * launch set (statistics, coefficient matrices, two batched TN products) for all blocks. */
size_t cmhse_contrastive_blocks_bwd_workspace(int32_t n_blocks, int32_t max_n);
int cmhse_contrastive_blocks_bwd(const float* im, const float* s, const float* scores,
                                 const int32_t* blk_off, int32_t n_blocks, int32_t max_n, int32_t D,
                                 float margin, int32_t max_violation, int32_t norm,
                                 const float* grad_out, float* d_im, float* d_s, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* The contrastive block of one training step (model.py:333-343) in one call: F.normalize of the
 * step's encoder outputs x[e] ([rows[e], D], device, contiguous) and the n_terms losses
 *   values[k] = ContrastiveLoss(normalize(x[term_a[k]]), normalize(x[term_b[k]]))   (loss.py:86-117)
 * plus their weighted total  *total = sum_k weight[k] * values[k]  (fp32, in term order) — the
 * reference's  loss_1 + loss_3 + (loss_5a + loss_5b) / 2 + ...  with weight 1 or 0.5.  Values are
 * those of cmhse_l2norm_rows + cmhse_contrastive_fwd per term, bit for bit (same kernels, the rows
 * normalised straight into the row-blocked operands).  The workspace keeps the normalised rows and
 * the stored scores for cmhse_step_losses_bwd, which must be given the same descriptor and
 * workspace: it writes dx[e] = d total / d x[e] * *grad_total for every e (dx: HOST array of n_emb
 * device pointers, each [rows[e], D]; an embedding no term uses gets zeros).  rows[term_a[k]] must
 * equal rows[term_b[k]].  Five launches each way on `stream`, no host synchronisation. */
#define CMHSE_STEP_LOSS_MAX 8
typedef struct cmhse_step_losses {
  int32_t n_emb, n_terms, D;
  const float* x[CMHSE_STEP_LOSS_MAX];
  int32_t rows[CMHSE_STEP_LOSS_MAX];
  int32_t term_a[CMHSE_STEP_LOSS_MAX], term_b[CMHSE_STEP_LOSS_MAX];
  float weight[CMHSE_STEP_LOSS_MAX];
  float margin;
  int32_t max_violation, norm;
} cmhse_step_losses;
size_t cmhse_step_losses_workspace(const cmhse_step_losses* d);
int cmhse_step_losses_fwd(const cmhse_step_losses* d, float* values, float* total, void* workspace,
                          size_t workspace_bytes, void* stream);
int cmhse_step_losses_bwd(const cmhse_step_losses* d, const float* grad_total, float* const* dx,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- backward pass (what loss.backward(), model.py:367, computes through the operators above) ---- */

/* Parameter gradients of one encoder layer, same shapes as cmhse_gru_weights; overwritten. */
typedef struct cmhse_gru_grads {
  float* dw_ih;  /* [3H, I] */
  float* dw_hh;  /* [3H, H] */
  float* db_ih;  /* [3H] */
  float* db_hh;  /* [3H] */
  float* dw_lin; /* [H, H]  (CMHSE_POOL_ATTN) */
  float* db_lin; /* [H] */
  float* dw_att; /* [H] */
} cmhse_gru_grads;

/* Backward of cmhse_gru_pool_fwd for the same `seqs` / `w` / pooling, given dout = d loss / d out
 * ([S,H], same row indexing as `out`) and the forward's workspace (run with
 * pool_mode | CMHSE_SAVE_FOR_BACKWARD).  Writes the parameter gradients to `grads` and, optionally,
 *   dx_rows      [S] device addresses: d loss / d x of step 0 of (sorted) sequence s goes there, rows
 *                of stride I floats (used for the level-2 encoders, whose inputs are level-1
 *                embeddings, model.py:252-253).  Ordinary rows are written exactly once; the
 *                row of a time-constant input (x_step_floats = 0) receives the SUM over its steps,
 *                accumulated with float atomics: zero it first;
 *   d_emb_table  [vocab, I]: gradient of embed.weight, ACCUMULATED with float atomics (zero it
 *                first); token batches only (model.py:94);
 *   dh0          d loss / d hidden (layers.py:98-100) with the row indexing of `out`: sequence s
 *                at row out_row[s] — [S, H], or [sum_T, H] with CMHSE_POOL_ALL, where out_row[s] is
 *                the sequence's first output row.
 * Any of the three may be NULL; dx_rows and d_emb_table are mutually exclusive. */
size_t cmhse_gru_pool_bwd_workspace(int32_t S, int32_t Tmax, int64_t sum_T, int32_t I, int32_t H,
                                    int32_t pool_mode);
int cmhse_gru_pool_bwd(const cmhse_seq_batch* seqs, const cmhse_gru_weights* w, int32_t pool_mode,
                       const float* dout, const void* fwd_workspace, const cmhse_gru_grads* grads,
                       const uint64_t* dx_rows, float* d_emb_table, float* dh0, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Several INDEPENDENT cmhse_gru_pool_bwd requests in one call (at most CMHSE_MAX_JOBS), the
 * backward counterpart of cmhse_gru_pool_fwd_multi: the BPTT step of every request shares one
 * launch (chains are aligned at their LAST step), so the two towers of a training step
 * (model.py:319-321: clip_enc / txt_enc, then vid_seq_enc / txt_seq_enc) pay one dependent
 * launch per step instead of two.  Results are bit-identical to the separate calls. */
typedef struct cmhse_gru_bwd_job {
  const cmhse_seq_batch* seqs;
  const cmhse_gru_weights* weights;
  int32_t pool_mode;
  const float* dout;
  const void* fwd_workspace;
  const cmhse_gru_grads* grads;
  const uint64_t* dx_rows;
  float* d_emb_table;
  float* dh0;
  void* workspace;
  size_t workspace_bytes;
  void* stream;        /* optional hipStream_t of this request's own launches (see cmhse_gru_job.stream) */
  void* side_stream;   /* optional second hipStream_t (or NULL).  The BPTT chain of a training batch
                          is a sequence of short dependent launches that leaves most of the chip
                          idle; the weight-gradient products (dW_ih, dW_hh, the bias sums, dW_lin)
                          and d(input) are throughput work whose operands — the gate-derivative
                          rows of steps >= t — are final as soon as the chain has passed t.  With a
                          side stream they are launched there chunk of time steps by chunk, each
                          ordered behind the step that completed its rows by an event, and run
                          beside the rest of the chain; the call joins the side stream back into
                          `stream` before it returns.  Results are bit-identical with and without
                          it (the chunks accumulate in the same order either way). */
} cmhse_gru_bwd_job;
int cmhse_gru_pool_bwd_multi(const cmhse_gru_bwd_job* jobs, int32_t n_jobs, void* stream);

/* Backward of F.normalize (model.py:333-343): dx from x [rows, cols] (contiguous) and g = d/dy. */
int cmhse_l2norm_rows_bwd(const float* x, const float* g, float* dx, int32_t rows, int32_t cols,
                          void* stream);

/* Backward of ContrastiveLoss.forward (loss.py:86-117) from the score matrix the forward stored
 * (`scores_out`) and the upstream gradient *grad_out (device scalar): d_im, d_s [n, D]. */
size_t cmhse_contrastive_bwd_workspace(int32_t n);
int cmhse_contrastive_bwd(const float* im, const float* s, const float* scores, int32_t n, int32_t D,
                          float margin, int32_t max_violation, int32_t norm, const float* grad_out,
                          float* d_im, float* d_s, void* workspace, size_t workspace_bytes,
                          void* stream);

/* loss.GroupWiseContrastiveLoss.forward (loss.py:26-71, --weak_low_level_loss): clip x caption
 * scores [n, n], reduced per (video i, video j) block to their max (max_violation) or mean, then
 * the same hinge loss on the reduced [B, B] matrix (norm divides by B*B).  row_off / col_off:
 * device int32 [B+1] prefix sums of num_clips / num_caps.  `reduced` [B,B] and `arg` [B,B] are
 * kept by the caller for cmhse_groupwise_bwd. */
size_t cmhse_groupwise_workspace(int32_t n, int32_t B);
int cmhse_groupwise_fwd(const float* im, const float* s, int32_t n, int32_t D,
                        const int32_t* row_off, const int32_t* col_off, int32_t B, float margin,
                        int32_t max_violation, int32_t norm, float* loss, float* reduced,
                        int32_t* arg, float* scores_out, void* workspace, size_t workspace_bytes,
                        void* stream);
size_t cmhse_groupwise_bwd_workspace(int32_t n, int32_t B);
int cmhse_groupwise_bwd(const float* im, const float* s, int32_t n, int32_t D,
                        const int32_t* row_off, const int32_t* col_off, int32_t B, float margin,
                        int32_t max_violation, int32_t norm, const float* reduced,
                        const int32_t* arg, const float* grad_out, float* d_im, float* d_s,
                        void* workspace, size_t workspace_bytes, void* stream);

/* decoder/loss.py:17-26 EuclideanLoss: loss = mean_r (or sum_r) sqrt(sum_c (a[r,c] - b_r[c])^2).
 * a is [rows, cols] contiguous; row r of b is at b_rows[r] (device addresses) when b_rows != NULL,
 * else b + r*cols.  The backward gives d loss / d a (b is detached upstream, model.py:347,363). */
int cmhse_euclid_fwd(const float* a, const float* b, const uint64_t* b_rows, int32_t rows,
                     int32_t cols, int32_t norm, float* loss, float* row_dist /* [rows] scratch */,
                     void* stream);
int cmhse_euclid_bwd(const float* a, const float* b, const uint64_t* b_rows, int32_t rows,
                     int32_t cols, int32_t norm, const float* grad_out, float* d_a, void* stream);

/* Measurement aid (bench.py's roofline leg): a pair of HIP events owned by the handle.  A timer
 * passed in cmhse_seq_batch.step_timer is recorded before the first and after the last GRU step
 * kernel of that call; cmhse_timer_elapsed_ms waits for the stop event and returns the span. */
void* cmhse_timer_create(void);
void cmhse_timer_destroy(void* timer);
int cmhse_timer_elapsed_ms(void* timer, float* ms_host);
int32_t cmhse_timer_launches(void* timer);   /* step kernels launched inside the bracket */
/* The launches of the LDS-tiled step kernel inside the bracket, each between its own event pair:
 * summed duration, their algorithmic FLOPs (2*3H*(I+H) + 14H per sequence and step), their
 * algorithmic HBM bytes (4I + 8H per sequence and step, the weights once per launch) and count. */
int cmhse_timer_tiled(void* timer, float* ms_host, double* flops_host, double* bytes_host,
                      int32_t* launches_host);

/* The one configuration entry point: kernel-shape crossovers a caller (a test, a benchmark) may
 * move.  They change WHICH kernel shape serves a step, never a result beyond fp32 summation order
 * (and the shapes selected by mid_units / mid_waves are bit-identical to each other).  `value` >= 0
 * sets the tunable, < 0 only reads it; *old_value (if not NULL) receives the previous value.
 *   "tiny_max_seqs"     1024  active sequences at or below which a forward step runs on the
 *                             small-batch kernels instead of the LDS-tiled one
 *   "mid_max_seqs"      1024  ... at or below which it runs on the mid-size kernel (hoisted input
 *                             projection + split-K 16x16x4 tiles); 0 disables that kernel
 *   "mid_units"            0  16 | 8 | 4 forces the mid-size step's hidden units per workgroup
 *   "mid_waves"            0  4 | 8 forces its waves per workgroup
 *   "mid_tall_min_seqs"  129  active sequences from which the mid-size step of a training call
 *                             takes 64 sequences per workgroup instead of 32 (bit-identical)
 *   "tall_tile_min_wgs" 2048  64-row workgroups from which an LDS-tiled launch uses 128-row tiles
 *   "bwd_mid_max_seqs"   512  active sequences at or below which a BPTT step runs on the mid-size
 *                             backward kernel
 *   "bwd_split_min_seqs"  33  active sequences from which (up to bwd_mid_max_seqs) a BPTT step runs
 *                             as two launches with K split over the grid; 0 = never
 *   "bwd_tail_min_steps"   4  steps with at most 32 active sequences at the end of a chain from
 *                             which its BPTT runs them inside ONE resident kernel (a grid barrier
 *                             per step instead of a launch); 0 = never.  The kernel holds H / 16
 *                             workgroups resident (one per CU): at most four such chains at once
 *   "fwd_tail_min_steps"   4  the same for the forward chain of a training call
 *                             (CMHSE_SAVE_FOR_BACKWARD, job on its own stream)
 *   "resident_timeout_ms" 5000  wall time a grid barrier of a resident kernel / a dependency wait of
 *                             the step chain may take before the launch gives up (cmhse_async_status);
 *                             0 = give up at the second clock check of a wait (tests: walks the
 *                             abort path)
 *   "bwd_chunk_rows"    2048  packed rows a weight-gradient chunk spans before its products are
 *                             issued beside the chain (changes the order in which chunks are
 *                             accumulated, i.e. the gradients to fp32 rounding)
 *   "xproj_chunk_rows"  1536  packed rows per chunk of a training chain's hoisted input projection
 *                             beside the chain; 0 = one launch in front of it
 *   "chain_min_steps"      2  consecutive LDS-tiled steps of an inference call from which they run as
 *                             ONE launch (gru_step_chain_kernel: per-row-tile dependencies instead
 *                             of a launch per time step; bit-identical); 0 = never
 *   "early_xproj"          1  the hoisted input projection of an inference call's small-batch steps on
 *                             the call's side stream (tail_stream) before the first step, beside the
 *                             tiled steps; 0 = in order in front of those steps (results identical)
 *   "chain_tall_min_wgs" 256  64-row workgroups per step from which such a chain uses 128-row tiles
 *                             (four times that when a request of the chain has I < H)
 *   "tn_rows_bm"           0  tile height of the weight-gradient products: 128 | 192; 0 = 192 where
 *                             every product's row count (3H, H) is a whole number of them, else 128
 *                             (the row split into parts follows the tile count, i.e. the gradients
 *                             to fp32 rounding; profiles/r04_wgrad_rate.txt)
 *   "pull_waves"          32  single-wave workgroups of one cmhse_pull_steps launch
 *   "tok_table"            1  a token-fed exact inference request with word-steps (sum_T) >= 4 x vocab
 *                             projects the whole vocabulary once (G = emb W_ih^T, one launch in front
 *                             of its first step; requests of a call with the same emb_table and W_ih
 *                             share it) and its steps read x_t W_ih^T from G[token]; 0 = off (results
 *                             identical).  Read when the workspace is sized
 *                             (cmhse_gru_pool_workspace_tok) and when the call starts
 *   "share_prefix"         1  (read by the host glue, cmhse_amd/evaluation.py, not by the library) 1: the
 *                             text tower of a validation pass leaves out every video's first caption whose
 *                             tokens are a prefix of its paragraph's (cmhse_tok_prefix_check) and pools it
 *                             from the paragraph's rows (cmhse_seq_batch.n_alias); 0 = encode every caption
 *                             (results identical)
 *   "rank_exact_tol_scale" 1  integer in [1, 2^20] (anything else: CMHSE_ERR_ARG) that multiplies the
 *                             tolerance of cmhse_sim_rank_exact: more pairs go through float64 (`resolved`
 *                             grows), every other output stays bit for bit; at 2^20 every pair of an input
 *                             with D >= 16 does (tests: the float64 path ranks the whole matrix)
 *   "multi_step_off"       0  (not a crossover, and per DEVICE rather than per context) 1 while the
 *                             multi-step kernels are switched off on the calling thread's current device
 *                             after an acknowledged timeout (cmhse_async_status below); readable, and
 *                             settable either way
 * These are the PROCESS DEFAULTS (atomics): set them between calls, not while calls that size
 * workspaces with them (`*_workspace` reads mid_max_seqs) are in flight on other threads.  A caller
 * that wants its own values — two models tuned differently in one process, a library that must not
 * disturb its host's settings — uses a context instead (below).  Unknown name: CMHSE_ERR_ARG.
 * (Five opt-ins of rounds 4-5 that measured slower than the defaults — a resident BPTT chain, the
 * one-launch BPTT step, attention tiles as chain tasks, a second ticket map, a resident inference
 * tail — left the library in round 6; docs/HISTORY.md and profiles/r04_chain_resident.txt,
 * r05_bptt_one_launch.txt, r05_chain_attention.txt, r05_dual_column_tile.txt, r05_rank_share.txt keep
 * the measurements, the git history the code.) */
int cmhse_tune(const char* name, int32_t value, int32_t* old_value);

/* Tuning contexts (round 5; SURVEY 8b "re-entrant, no global state").  A context is a private copy
 * of the crossovers above, initialised from the process defaults at creation.  cmhse_ctx_enter(ctx)
 * makes it the CALLING THREAD's current context and returns the previous one (NULL = none): every
 * library call that thread makes until it enters another one (cmhse_ctx_enter(prev) to leave) —
 * workspace sizing and launches alike — reads its crossovers from the context, and cmhse_tune /
 * other threads / other contexts do not affect it.  The context must outlive the calls made inside
 * it; host-side only (a few hundred bytes).  cmhse_ctx_tune: cmhse_tune on a context. */
void* cmhse_ctx_create(void);
void cmhse_ctx_destroy(void* ctx);
int cmhse_ctx_tune(void* ctx, const char* name, int32_t value, int32_t* old_value);
void* cmhse_ctx_enter(void* ctx);

/* The kernels that stay resident over several time steps of a chain (the few-sequence tails of a
 * training chain: "*_tail_min_steps") synchronise their workgroups with a grid barrier, which needs
 * all of them on the chip at once; the step chain ("chain_min_steps") waits on per-row-tile counters
 * and needs its workgroups to start in index order.  The launchers check
 * the CU count; what they cannot see — another process holding CUs, a CU mask — ends in a timeout
 * ("resident_timeout_ms", default 5000): the kernel's workgroups all leave, the call's results are
 * invalid, and a word in pinned host memory is raised.  This function returns CMHSE_ERR_TIMEOUT
 * while that word is set for the calling thread's current device (CMHSE_OK otherwise) and clears
 * it when `clear` != 0; cmhse_gru_pool_fwd[_multi] / cmhse_gru_pool_bwd[_multi] check it on entry
 * and return CMHSE_ERR_TIMEOUT without launching.  Clearing a raised status also switches the
 * multi-step kernels off ON THAT DEVICE, for every tuning context and the process defaults alike
 * ("chain_min_steps", "*_tail_min_steps" read as 0 there: one launch per time step, which needs
 * neither co-residency nor in-order workgroup starts) — other devices keep them; setting one of those
 * knobs to a positive value (cmhse_tune / cmhse_ctx_tune) with the device current switches them back
 * on.  The status is asynchronous: it reflects launches that have RUN, so poll it after a stream
 * synchronisation (or once per step, one step late). */
int cmhse_async_status(int32_t clear);

/* Self-test of that barrier and of its failure path (tests): launches `workgroups` (<= 1024)
 * single-wave workgroups that each arrive at `rounds` grid barriers, every barrier expecting
 * `missing` more arrivals than there are workgroups.  workspace: 256 bytes, 256-byte aligned
 * (zeroed by the call); on completion uint32 word [2] = workgroups that passed every barrier, word
 * [3] = workgroups that left through the abort path.  missing = 0 never times out; missing > 0 always
 * does, after "resident_timeout_ms", and raises the status cmhse_async_status reports. */
int cmhse_selftest_grid_sync(void* workspace, int32_t workgroups, int32_t missing, int32_t rounds,
                             void* stream);

/* Text for an error code returned by the functions above (static storage). */
const char* cmhse_strerror(int code);

/* Library / target identification: "cmhse_hip <version> gfx950". */
const char* cmhse_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CMHSE_HIP_H_ */
