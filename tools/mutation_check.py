#!/usr/bin/env python3
"""Mutation check of the parity tests: do they notice a kernel that drops a reference quirk?

  python tools/mutation_check.py build [name ...]   (build container: hipcc, no GPU needed)
      copies cmhse_amd/csrc to build/mutants/<name>/, applies ONE source edit per mutant, and builds
      build/mutants/libcmhse_<name>.so (same ABI; the product sources and library are untouched).
  python tools/mutation_check.py run [name ...]     (GPU box)
      runs the selected GPU tests once per mutant with CMHSE_HIP_LIB pointing at it and reports
      which tests FAILED — a mutant that no test kills is a hole in the suite.  Also runs the same
      selection on the product library (must pass).  `--tests <pytest arguments>` after the names
      replaces the selection, e.g. to show that a mutant survives the tests that were there before
      the ones written to kill it.

Mutants:
  attn_eps_fwd   gru_attention.hpp: the masked softmax's `+ 0.0001f` (layers.py:158-162) -> `+ 0.0f`
  attn_eps_bwd   bwd_pool_kernels.hpp: the same epsilon in the attention backward
  norm_by_n, gru_bhn_outside_r(_tiled), rank_counts_ties, l2norm_eps   (round 6, second batch) see MUTANTS
  bwd_step_combine_4_waves, bwd_step_drops_carry, bwd_gates_dz, bwd_tail_four_blocks   the BPTT step
                 shapes (killed by tests/test_gpu_bptt_shapes.py; the tail one by test_gpu_chain.py's
                 resident-tail test)
  fwd_tail_two_blocks, mid_combine_4_waves, tiny_all_prev_state, tile_all_prev_state, scalar_k_remainder
                 the forward step shapes (killed by tests/test_gpu_fwd_shapes.py; the tail one by
                 test_gpu_chain.py's forward resident-tail test)
  gw_reduce_first_trip, gw_argmax_last_tie, gw_expand_mean_by_width, gw_expand_first_trip, euclid_norm_by_cols
                 the loss kernels at training shapes (killed by tests/test_gpu_loss_shapes.py; of the four
                 group-wise ones only the mean by width is caught by an older test:
                 profiles/loss_shapes_mutation_check.txt)
  bf3_ring_reload_last_but_one, bf3_epilogue_odd_lo, bf3_attn_ring_past_cut, bf3_split_rows_truncates,
  bf3_h0_ignored, bf3_tiled_wgs_counts_bf3
                 the bf16x3 math mode (killed by tests/test_gpu_bf3_shapes.py — the last one changes the
                 exact neighbour's tile height only, which no result can show:
                 profiles/bf3_shapes_mutation_check.txt)
  side_reduce_two_segments, side_reduce_ignores_add, side_tn_reduce_ignores_accumulate, side_attn_du_no_tanh,
  side_colsum_first_slab, side_pool_all_negated
                 what the backward launches beside the BPTT chain (killed by tests/test_gpu_bwd_side_shapes.py;
                 which of them an older test catches: profiles/bwd_side_mutation_check.txt)
  score_deal_tile_g4, score_count_plain_order_swapped, score_group_plain_order_even_columns, score_topk_panel_even_split,
  score_gtopk_panel_even_split, score_topk_list_rezeroed_per_tile, score_gtopk_list_rezeroed_per_tile,
  score_merge_list_not_shifted
                 the tile deal and the panel walk of the scoring kernels (killed by tests/test_gpu_score_shapes.py;
                 which of them an older test catches: profiles/score_shapes_mutation_check.txt)
  attn_pool_first_round, attn_pool_den_first_trip, attn_pool_first_unit_round, attn_bwd_den_first_trip,
  attn_bwd_wave_first_step, colsum_two_slabs
                 the loops that change behaviour only with a sequence's length or past H = 1024 (killed by
                 tests/test_gpu_long_shapes.py; which of them an older test catches:
                 profiles/long_shapes_mutation_check.txt)
  tanh_cancels_near_zero, tanh_ratio_form, sigmoid_clamps_argument, mid_max_tie_later_step, fwd_tail_max_tie_later_step,
  attn_den_clamps_energy, attn_bwd_unit_sum, l2norm_bwd_projects_inside_clamp
                 value-only edits that are wrong only at extreme numbers (killed by tests/test_gpu_value_regimes.py;
                 none of them by an older test: profiles/value_regimes_mutation_check.txt)
  topk_exact_tol_zero, topk_exact_tol_small, topk_exact_tie_larger_column
                 the second pass of the certified top-K (killed by tests/test_gpu_topk_exact.py:
                 profiles/topk_exact_mutation_check.txt)
  ws_rank_not_zeroed, ws_top1key_not_zeroed, ws_labelled_keys_half_zeroed, ws_exact_pre_keeps_resolved,
  ws_exact_norm_max_not_zeroed, ws_topk_exact_norm_max_not_zeroed, ws_group_norm_max_not_zeroed, ws_bwd_carry_not_zeroed,
  ws_bwd_dpool_not_zeroed, ws_bwd_zero_row_not_zeroed, ws_split_k_not_zeroed, ws_bf3_hs_pad_not_zeroed
                 one deleted or narrowed initialisation of a workspace region or of an output that is counted or
                 summed into (killed by tests/test_gpu_dirty_workspace.py: profiles/dirty_workspace_mutation_check.txt).
                 None touches a sync word, a ticket, a barrier counter, the abort word or an address table.  Two change
                 no result (EQUIVALENT): the carry memset is redundant, the own_zero arm of launch_nt_out has no caller.
"""
import os
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, 'build', 'mutants')
RUN_TIMEOUT_S = int(os.environ.get('MUTATION_RUN_TIMEOUT', '1800'))      # one pytest run of `run`

MUTANTS = {
    # value regimes (tests/value_regimes.py): value-only edits that are wrong only at extreme numbers
    # ... the form before the polynomial branch: relative error ~1e-7 / |x| near 0
    'tanh_cancels_near_zero': ('gru_step_tile.hpp', 'return fabsf(x) < kTanhSmall ? poly : big;', 'return big;'),
    # ... (e - 1) / (e + 1): inf * 0 once exp(2x) overflows
    'tanh_ratio_form': ('gru_step_tile.hpp', 'const float big = 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f);',
                        'const float big = (__expf(2.0f * x) - 1.0f) * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f);'),
    # ... a sigmoid that clamps its argument: 1 - 1.1e-7 where the reference gives exactly 1
    'sigmoid_clamps_argument': ('gru_step_tile.hpp', 'return __builtin_amdgcn_rcpf(1.0f + __expf(-x));',
                                'return __builtin_amdgcn_rcpf(1.0f + __expf(-fminf(fmaxf(x, -16.0f), 16.0f)));'),
    # ... the running maximum's tie rule (strict '>': the first maximum wins) where the forward saves the arg-max
    'mid_max_tie_later_step': ('gru_small_batch.hpp', 'if (p.t == 0 || hn > *op) {', 'if (p.t == 0 || hn >= *op) {'),
    'fwd_tail_max_tie_later_step': ('gru_small_batch.hpp', 'if (hn > *op) {      // (t >= 1 here', 'if (hn >= *op) {      // (t >= 1 here'),
    # ... a softmax denominator that clamps its energies / a Jacobian that takes the weights to sum to 1
    'attn_den_clamps_energy': ('gru_attention.hpp', 'part += expf(e);', 'part += expf(fminf(e, 30.0f));'),
    'attn_bwd_unit_sum': ('bwd_pool_kernels.hpp', 'if (lane == 0) q.de[row] = a * (q.de[row] - c);',
                          'if (lane == 0) q.de[row] = a * (q.de[row] - c / (1.0f - 0.0001f / den));'),
    # ... the projection term inside the 1e-12 clamp of F.normalize's backward
    'l2norm_bwd_projects_inside_clamp': ('norm_rows.hpp', 's_dot = nrm < 1e-12f ? 0.f : (', 's_dot = false ? 0.f : ('),
    'attn_eps_fwd': ('gru_attention.hpp', 's_den = d + 0.0001f;', 's_den = d + 0.0f;'),
    'attn_eps_bwd': ('bwd_pool_kernels.hpp', 's_den = d + 0.0001f;', 's_den = d + 0.0f;'),
    # loss.py:114-115: `norm` divides by n * m, not by n
    'norm_by_n': ('loss_kernels.hpp', 'loss = loss / static_cast<float>(static_cast<int64_t>(p.n) * p.n);',
                  'loss = loss / static_cast<float>(p.n);'),
    # nn.GRU: n = tanh(W_in x + b_in + r * (W_hn h + b_hn)) — b_hn INSIDE the reset gate's product
    # (the mid-size step kernel, the one the golden-sized batches run on)
    'gru_bhn_outside_r': ('gru_small_batch.hpp', 'const float ng = tanhf_(e_gx[q][2] + e_b[q][2] + rg * ghn);',
                          'const float ng = tanhf_(e_gx[q][2] + e_b[q][2] + rg * hn_ + e_b[q][3]);'),
    # ... and the LDS-tiled step (batches of more than 1024 sequences)
    'gru_bhn_outside_r_tiled': ('gru_step_tile.hpp', 'const float ng = tanhf_(acc[ms][2][r] + b_in + rg * ghn);',
                                'const float ng = tanhf_(acc[ms][2][r] + b_in + rg * acc[ms][3][r] + b_hn);'),
    # evaluation.py:92-95 / 131-134 via the documented tie rule: strict '>' for the rank
    'rank_counts_ties': ('sim.hip', 'valid && (MODE == kSimLabel || j != gi) && v > dii',
                         'valid && (MODE == kSimLabel || j != gi) && v >= dii'),
    # loss.py:100-103: the diagonal of both cost matrices is masked to zero
    'loss_diag_not_masked': ('loss_kernels.hpp', 'if (j == i) c = 0.f;', ''),
    # loss.py:106-111: max_violation keeps the hardest negative per row / column only
    'max_violation_sums': ('loss_kernels.hpp', 'total += p.max_violation ? static_cast<double>(mx) : sum;', 'total += sum;'),
    # F.normalize's eps (model.py l2norm of the encoder outputs): a zero row stays zero, x / max(|x|, 1e-12)
    'l2norm_eps': ('norm_rows.hpp', 's_inv = 1.0f / fmaxf(sqrtf(t), 1e-12f);', 's_inv = 1.0f / sqrtf(t);'),
    # BPTT step shapes (tests/test_gpu_bptt_shapes.py): value-only edits, no address, grid or barrier moves.
    # The 32 x 32 step tile's LDS combine adds the partials of 4 waves only: wrong for the 8-wave kernels
    'bwd_step_combine_4_waves': ('bwd_step_kernels.hpp', 'for (int w = 0; w < NW; ++w) part += red[w][reg][lb + j];',
                                 'for (int w = 0; w < 4; ++w) part += red[w][reg][lb + j];'),
    # ... its epilogue drops the carried dh_{t+1} z_{t+1} (every gru_bwd_step_kernel instantiation)
    'bwd_step_drops_carry': ('bwd_step_kernels.hpp', '      rec += part;', '      rec = part;'),
    # the split step's gate kernel: dz without the sigmoid's (1 - z) factor
    'bwd_gates_dz': ('bwd_step_kernels.hpp', 'dzp.c = dh * (hp.c - ng.c) * zg.c * (1.0f - zg.c);',
                     'dzp.c = dh * (hp.c - ng.c) * zg.c;'),
    # the resident tail multiplies at most 4 of a wave's 16-k blocks: wrong from KB = 6 (H >= 256) on
    'bwd_tail_four_blocks': ('bwd_step_kernels.hpp', 'if (i >= nmine) continue;   // wave-uniform',
                             'if (i >= nmine || i >= 4) continue;'),
    # forward step shapes (tests/test_gpu_fwd_shapes.py): value-only edits as above.
    # The forward resident tail multiplies at most 2 of a wave's 16-k blocks: wrong from KB = 4 (H > 256) on
    'fwd_tail_two_blocks': ('gru_small_batch.hpp', 'if (i >= nmine) continue;   // wave-uniform',
                            'if (i >= nmine || i >= 2) continue;'),
    # the mid-size step combines one K slice per wave: wrong for its 4-wave forms (two slices per wave)
    'mid_combine_4_waves': ('gru_small_batch.hpp', 'for (int w = 0; w < kMidSlices; ++w)\n          hg[g] +=',
                            'for (int w = 0; w < NW; ++w)\n          hg[g] +='),
    # the latency-shaped step's all-states epilogue stores the previous state (gru_step_tiny_kernel)
    'tiny_all_prev_state': ('gru_small_batch.hpp', '\n    p.out[(static_cast<int64_t>(p.out_row[em]) + p.t) * H + u] = hn;',
                            '\n    p.out[(static_cast<int64_t>(p.out_row[em]) + p.t) * H + u] = hp;'),
    # ... and that of the LDS-tiled step and the step chain (gru_step_tile.hpp)
    'tile_all_prev_state': ('gru_step_tile.hpp', 'out[(static_cast<int64_t>(orow[i]) + t) * H + u] = v;',
                            'out[(static_cast<int64_t>(orow[i]) + t) * H + u] = hp[r4 + i];'),
    # the scalar-load tile loops keep the 4th element of a k group past K (its load is clamped to the
    # row's last element, so the value is that element instead of 0)
    'scalar_k_remainder': ('nt_core.hpp', 'v.w = (valid && k + 3 < klim) ? v.w : 0.f;', 'v.w = valid ? v.w : 0.f;'),
    # loss kernels at training shapes (tests/test_gpu_loss_shapes.py): value-only edits as above.
    # block_reduce_kernel visits a thread's first element only: wrong for blocks of more than 256 elements
    'gw_reduce_first_trip': ('loss_kernels.hpp', 'for (int e = tid; e < cnt; e += kThreads) {', 'if (int e = tid; e < cnt) {'),
    # ... its per-thread scan keeps the LAST of a thread's tied maxima (loss.py:31 torch.max: the first)
    'gw_argmax_last_tie': ('loss_kernels.hpp', 'if (v > best || (v == best && flat < arg)) {',
                           'if (v > best || (v == best && flat > arg)) {'),
    # the block mean's gradient divides by the block's width instead of its element count
    'gw_expand_mean_by_width': ('loss_kernels.hpp', 'g / static_cast<float>(cnt);', 'g / static_cast<float>(w);'),
    # groupwise_expand_kernel writes a thread's first element only
    'gw_expand_first_trip': ('loss_kernels.hpp', 'for (int e = threadIdx.x; e < cnt; e += kThreads) {',
                             'if (int e = threadIdx.x; e < cnt) {'),
    # decoder/loss.py:24: the mean is over the rows
    'euclid_norm_by_cols': ('loss_kernels.hpp', 'if (q.norm) sc /= static_cast<float>(q.rows);',
                            'if (q.norm) sc /= static_cast<float>(q.cols);'),
    # the bf16x3 math mode (tests/test_gpu_bf3_shapes.py): each stays inside its request's workspace.
    # The ring's re-load in the loop never fetches the last chunk: wrong from four chunks of 16 k on
    'bf3_ring_reload_last_but_one': ('nt_core.hpp', 'dma(prev, (c + 2 < last) ? c + 2 : last);',
                                     'dma(prev, (c + 2 < last - 1) ? c + 2 : last - 1);'),
    # the step epilogue's pre-split state row: the odd unit of a pair without its lo half
    'bf3_epilogue_odd_lo': ('gru_step_tile.hpp', 'const uint32_t lo = pack_bf16(hn[r] - f0, o1 - f1);',
                            'const uint32_t lo = pack_bf16(hn[r] - f0, 0.f);'),
    # the projection's ring launch runs past rows_split, over pre-split rows no step has written
    'bf3_attn_ring_past_cut': ('gru.hip', 'const int64_t cut = job.rows_split < lo ? lo : (job.rows_split > hi ? hi : job.rows_split);',
                               'const int64_t cut = hi;'),
    # split_rows_kernel truncates the hi half instead of rounding it to nearest even
    'bf3_split_rows_truncates': ('gru_rows.hpp', '\n    const uint32_t hi = pack_bf16(x0, x1);',
                                 '\n    const uint32_t hi = (__float_as_uint(x0) >> 16) | (__float_as_uint(x1) & 0xffff0000u);'),
    # the ring step skips the h phase of step 0: the caller's initial states enter through z h only
    'bf3_h0_ignored': ('gru_step_tile.hpp', 'if (have_h) nt_phase_bf3_ring<', 'if (have_h && t > 0) nt_phase_bf3_ring<'),
    # the 64-row workgroups of bf16x3 requests count towards the exact requests' tall-tile threshold
    'bf3_tiled_wgs_counts_bf3': ('gru.hip', 'if (jobs[k].kind_count[t] > tiny_max_seqs() && !jobs[k].bf3)',
                                 'if (jobs[k].kind_count[t] > tiny_max_seqs())'),
    # what cmhse_gru_pool_bwd launches beside the chain (tests/test_gpu_bwd_side_shapes.py): value-only edits as above.
    # The ordered split-K reduce adds two segments at most: wrong from three segments (K >= 768) on
    'side_reduce_two_segments': ('bwd_pool_kernels.hpp', 'for (int y = 0; y < splits; ++y) s += part[(static_cast<int64_t>(y) * M + m) * N + n];',
                                 'for (int y = 0; y < splits && y < 2; ++y) s += part[(static_cast<int64_t>(y) * M + m) * N + n];'),
    # ... and stores where the attention backward's dpool += du . W_lin must add: the pooling gradient a g is lost
    'side_reduce_ignores_add': ('bwd_pool_kernels.hpp', 'dst[n] = add ? dst[n] + s : s;', 'dst[n] = s;'),
    # the weight-gradient row split's reduce stores into C on a later chunk: the chunks before it are lost
    'side_tn_reduce_ignores_accumulate': ('tn_rows.hpp', '*dst = q.accumulate ? (*dst + s) : s;', '*dst = s;'),
    # du without the tanh's 1 - v^2
    'side_attn_du_no_tanh': ('bwd_pool_kernels.hpp', 'du[p * H + n] = d * w_att[n] * (1.0f - tv * tv);',
                             'du[p * H + n] = d * w_att[n];'),
    # d att_w from the first slab of 512 packed rows only
    'side_colsum_first_slab': ('bwd_pool_kernels.hpp', 'for (int i = 0; i < slabs; ++i) s += part[static_cast<int64_t>(i) * cols + c];',
                               'for (int i = 0; i < slabs && i < 1; ++i) s += part[static_cast<int64_t>(i) * cols + c];'),
    # all-states pooling hands the chain the negated output gradient
    'side_pool_all_negated': ('bwd_pool_kernels.hpp', 'for (int u = threadIdx.x; u < q.H; u += kThreads) d[u] = g[u];',
                              'for (int u = threadIdx.x; u < q.H; u += kThreads) d[u] = -g[u];'),
    # the tile deal and the panel walk of the scoring kernels (tests/test_gpu_score_shapes.py): index- or value-only
    # edits, each inside the buffers its launch owns, no barrier added or moved.
    # xcd_deal_tile splits a block's group index by 4 whatever G is: wrong for G = 2 and 3 (a row tile past the last
    # one falls into the callers' padding return)
    'score_deal_tile_g4': ('score_tile.hpp', 'const int Q = (q / G) * 8 + x;\n  return {G * (Q / col_tiles) + (q % G), Q % col_tiles};',
                           'const int Q = (q / 4) * 8 + x;\n  return {G * (Q / col_tiles) + (q % 4), Q % col_tiles};'),
    # the plain order of the counting passes (G = 0) swaps row and column tile past the first row of tiles
    'score_count_plain_order_swapped': ('sim.hip', '    i0 = (blockIdx.x / p.n_tiles) * BM;\n  }',
                                        '    i0 = (blockIdx.x / p.n_tiles) * BM;\n    if (COUNT && blockIdx.x >= static_cast<unsigned>(p.n_tiles)) {\n'
                                        '      j0 = (blockIdx.x / p.n_tiles) * BN;\n      i0 = (blockIdx.x % p.n_tiles) * BM;\n    }\n  }'),
    # the plain order of group_sim_kernel (G = 0) visits the even column tiles only
    'score_group_plain_order_even_columns': ('group.hip', '    ct = blockIdx.x % p.col_tiles;', '    ct = (blockIdx.x % p.col_tiles) & ~1;'),
    # the panels of the top-K select kernels hold col_tiles / panels tiles each: the remainder's tiles are never visited
    'score_topk_panel_even_split': ('topk.hip', 'static_cast<int>(static_cast<int64_t>(panel) * p.col_tiles / p.panels);\n'
                                    '  const int t_end = static_cast<int>(static_cast<int64_t>(panel + 1) * p.col_tiles / p.panels);',
                                    'panel * (p.col_tiles / p.panels);\n  const int t_end = (panel + 1) * (p.col_tiles / p.panels);'),
    'score_gtopk_panel_even_split': ('group.hip', 'static_cast<int>(static_cast<int64_t>(panel) * p.g_tiles / p.panels);\n'
                                     '  const int t_end = static_cast<int>(static_cast<int64_t>(panel + 1) * p.g_tiles / p.panels);',
                                     'panel * (p.g_tiles / p.panels);\n  const int t_end = (panel + 1) * (p.g_tiles / p.panels);'),
    # the select kernels forget a row's running list at every tile: a panel keeps its last tile only
    'score_topk_list_rezeroed_per_tile': ('topk.hip', 'score_key_t* lst = lists + row * K;',
                                          'score_key_t* lst = lists + row * K;\n      for (int e = lane; e < K; e += 64) lst[e] = 0ull;'),
    'score_gtopk_list_rezeroed_per_tile': ('group.hip', 'score_key_t* lst = lists + qi * K;',
                                           'score_key_t* lst = lists + qi * K;\n      for (int e = lane; e < K; e += 64) lst[e] = 0ull;'),
    # wave_merge leaves the list entries where they were: harmless into an empty list, wrong into a warm one
    'score_merge_list_not_shifted': ('topk_lists.hpp', 'if (e < K && e + lr[h] < K) lst[e + lr[h]] = lv[h];',
                                     'if (e < K && e + lr[h] < K) lst[e] = lv[h];'),
    # long sequences (tests/test_gpu_long_shapes.py): value-only edits, no address, grid, barrier or wait changes.
    # attn_pool_kernel's weighted sum stops after its first round of 256 staged steps: wrong from 257 steps on
    'attn_pool_first_round': ('gru_attention.hpp', 'for (int t0 = 0; t0 < len; t0 += kThreads) {',
                              'for (int t0 = 0; t0 < len && t0 < kThreads; t0 += kThreads) {'),
    # ... its denominator visits each thread's first step only
    'attn_pool_den_first_trip': ('gru_attention.hpp', 'for (int t = tid; t < len; t += kThreads) {', 'if (int t = tid; t < len) {'),
    # ... its output loop runs once: the units from 1024 on are never written
    'attn_pool_first_unit_round': ('gru_attention.hpp', 'for (int ub = 0; ub < H; ub += 4 * kThreads) {',
                                   'for (int ub = 0; ub < H && ub < 4 * kThreads; ub += 4 * kThreads) {'),
    # attn_pool_bwd_kernel's denominator visits each thread's first step only: wrong from 1025 steps on
    'attn_bwd_den_first_trip': ('bwd_pool_kernels.hpp', 'for (int t = tid; t < len; t += NT) part += expf(energy(t));',
                                'if (int t = tid; t < len) part += expf(energy(t));'),
    # ... its pass 1 takes only each wave's first step into c = sum_t a_t da_t: wrong from 17 steps on
    'attn_bwd_wave_first_step': ('bwd_pool_kernels.hpp', '    c_acc += a * d;', '    if (t == wave) c_acc += a * d;'),
    # d att_w from the first two slabs of 512 packed rows: wrong from 1025 rows on
    'colsum_two_slabs': ('bwd_pool_kernels.hpp', 'for (int i = 0; i < slabs; ++i) s += part[static_cast<int64_t>(i) * cols + c];',
                         'for (int i = 0; i < slabs && i < 2; ++i) s += part[static_cast<int64_t>(i) * cols + c];'),
    # certified top-K (tests/test_gpu_topk_exact.py): value-only edits as above.
    # The second pass takes the columns at or above v_K only: the fp32 list's members, re-sorted in float64
    'topk_exact_tol_zero': ('topk.hip', 'const float tol = s_tol[row];', 'const float tol = 0.f;'),
    # ... or a tolerance a thousand times too small: about one fp32 step of a unit-norm score
    'topk_exact_tol_small': ('topk.hip', 'const float tol = s_tol[row];', 'const float tol = s_tol[row] * 1e-3f;'),
    # equal float64 scores put the LARGER column first
    'topk_exact_tie_larger_column': ('topk_lists.hpp', 'return xb > yb || (xb == yb && xi < yi);',
                                     'return xb > yb || (xb == yb && xi > yi);'),
    # dirty workspaces and outputs (tests/test_gpu_dirty_workspace.py): ONE initialisation deleted or narrowed each; wrong
    # numbers only (counters, keys, sums and norms: no sync word, no address table).
    # cmhse_sim_rank counts into whatever `rank` held
    'ws_rank_not_zeroed': ('sim.hip', 'if (hipMemsetAsync(rank, 0, sizeof(int32_t) * nrows, stream) != hipSuccess) return CMHSE_ERR_LAUNCH;\n'
                           '  if (hipMemsetAsync(p.top1key, 0, sizeof(score_key_t) * nrows, stream) != hipSuccess)',
                           'if (hipMemsetAsync(p.top1key, 0, sizeof(score_key_t) * nrows, stream) != hipSuccess)'),
    # ... and takes its top-1 maximum over whatever the key vector held
    'ws_top1key_not_zeroed': ('sim.hip', 'if (hipMemsetAsync(p.top1key, 0, sizeof(score_key_t) * nrows, stream) != hipSuccess)\n'
                              '    return CMHSE_ERR_LAUNCH;', ''),
    # cmhse_sim_rank_labelled clears the top-1 keys and leaves the threshold keys behind them
    'ws_labelled_keys_half_zeroed': ('sim.hip', 'if (hipMemsetAsync(p.top1key, 0, 2 * sizeof(score_key_t) * nrows, stream) != hipSuccess)',
                                     'if (hipMemsetAsync(p.top1key, 0, sizeof(score_key_t) * nrows, stream) != hipSuccess)'),
    # exact_pre_kernel leaves the diagnostic counter of cmhse_sim_rank_exact as it found it
    'ws_exact_pre_keeps_resolved': ('sim.hip', '      p.s64_diag[r] = sii;\n      p.norm_a[r] = na;\n      p.rank_lo[r] = 0;\n      p.ties[r] = 0;\n'
                                    '      p.resolved[r] = 0;',
                                    '      p.s64_diag[r] = sii;\n      p.norm_a[r] = na;\n      p.rank_lo[r] = 0;\n      p.ties[r] = 0;'),
    # the largest gallery norm of the three certified calls starts from what the word held (atomicMax on the bits)
    'ws_exact_norm_max_not_zeroed': ('sim.hip', 'if (hipMemsetAsync(q.norm_b_max, 0, sizeof(unsigned), stream) != hipSuccess) return CMHSE_ERR_LAUNCH;\n'
                                     '  const int64_t pre_rows = static_cast<int64_t>(nrows) + M;\n  hipLaunchKernelGGL(exact_pre_kernel,',
                                     'const int64_t pre_rows = static_cast<int64_t>(nrows) + M;\n  hipLaunchKernelGGL(exact_pre_kernel,'),
    'ws_topk_exact_norm_max_not_zeroed': ('topk.hip', 'if (hipMemsetAsync(q.norm_b_max, 0, sizeof(unsigned), stream) != hipSuccess) return CMHSE_ERR_LAUNCH;', ''),
    'ws_group_norm_max_not_zeroed': ('group.hip', 'if (hipMemsetAsync(q.norm_max, 0, 2 * sizeof(unsigned), stream) != hipSuccess) return CMHSE_ERR_LAUNCH;', ''),
    # the BPTT's carried dh z starts from what the workspace held (EQUIVALENT: every row is written before it is read)
    'ws_bwd_carry_not_zeroed': ('bwd.hip', '(void)hipMemsetAsync(carry, 0, static_cast<size_t>(S) * H * 4, st);', ''),
    # last-state / max pooling scatter their output gradient into rows that were never cleared
    'ws_bwd_dpool_not_zeroed': ('bwd.hip', '(void)hipMemsetAsync(dpool, 0, static_cast<size_t>(sum_T) * H * 4, st);', '(void)0;'),
    # the row of zeros that stands in for h_{-1} and for padding keeps its old bytes (the barrier counter behind it is still cleared)
    'ws_bwd_zero_row_not_zeroed': ('bwd.hip', '(void)hipMemsetAsync(zero_row, 0, L.tail_sync + 256 - L.zero_row, st);',
                                   '(void)hipMemsetAsync(ws + L.tail_sync, 0, 256, st);'),
    # launch_nt_out's own_zero arm (split == 1) sums into an uncleared C: no caller passes split == 1
    'ws_split_k_not_zeroed': ('bwd.hip', 'if (own_zero) (void)hipMemsetAsync(c, 0, static_cast<size_t>(M) * N * sizeof(float), st);', ''),
    # bf16x3, H % 16 != 0: the chunk padding of the pre-split hidden states keeps its old bytes
    'ws_bf3_hs_pad_not_zeroed': ('gru.hip', 'if (b->H % 16 != 0)   // the epilogue writes whole (hi, lo) pairs; the chunk padding must read 0\n'
                                 '        (void)hipMemsetAsync(wsb + L.hs_s, 0,\n'
                                 '                             static_cast<size_t>(job->rows_split) * split_ld(b->H) * sizeof(float), stream);', ''),
}
# mutants that change no result, with the reason: run and reported, but no test can kill them
EQUIVALENT = {
    'bf3_tiled_wgs_counts_bf3': 'moves an exact request between 64- and 128-row tiles, which give the same bits; the line is '
                                'pinned by tests/test_bf3_shapes_cpu.py (fwd_shapes.TILED_WGS_ALSO)',
    'ws_bwd_carry_not_zeroed': 'every BPTT step kernel reads carry only at rows m < S_next, which the step before it wrote '
                               '(bwd_step_kernels.hpp; the last step has S_next = 0, the resident tail starts from a register): '
                               'the memset in bwd_begin is belt and braces and no result can show that it is gone',
    'ws_split_k_not_zeroed': 'the own_zero arm of launch_nt_out has no caller (tests/test_bwd_side_shapes_cpu.py '
                             'test_the_own_zero_arm_has_no_caller): the deleted memset cannot run',
}
# the tests that must kill them (and pass on the product library)
SELECT = ['tests/test_quirks_tight.py', 'tests/test_gpu_golden.py', 'tests/test_gpu_gru.py', 'tests/test_gpu_scoring.py',
          'tests/test_gpu_bptt_shapes.py', 'tests/test_gpu_fwd_shapes.py', 'tests/test_gpu_chain.py',
          'tests/test_gpu_loss_shapes.py', 'tests/test_gpu_bf3_shapes.py', 'tests/test_gpu_bwd_side_shapes.py',
          'tests/test_gpu_score_shapes.py', 'tests/test_gpu_long_shapes.py', 'tests/test_gpu_topk_exact.py',
          'tests/test_gpu_value_regimes.py', '-k',
          'epsilon or test_layers_vs_golden or test_layer_backward_vs_golden or test_model_vs_golden or norm or '
          'test_gru_pool_vs_oracle or tie or zero or l2norm or test_contrastive_vs_oracle or bptt_step_shape or '
          'mixed_step_shapes or bptt_tail or fwd_step_shape or forward_tail or loss_shapes or bf3_shape or bwd_side_shape or '
          'score_shape or long_shape or outlier_paragraph or topk_exact or value_regime or at_the_clamp or stays_in_its_row']


def build(only=()):
  from cmhse_amd import build as b
  os.makedirs(OUT, exist_ok=True)
  for name, (fname, old, new) in MUTANTS.items():
    if only and name not in only:
      continue
    root = os.path.join(OUT, name)
    shutil.rmtree(root, ignore_errors=True)
    src = os.path.join(root, 'cmhse_amd', 'csrc')          # (the sources include ../../include/cmhse_hip.h)
    shutil.copytree(b.CSRC, src)
    shutil.copytree(os.path.join(REPO, 'include'), os.path.join(root, 'include'))
    text = open(os.path.join(src, fname)).read()
    assert text.count(old) == 1, (name, text.count(old))
    open(os.path.join(src, fname), 'w').write(text.replace(old, new))
    target = os.path.join(OUT, 'libcmhse_%s.so' % name)
    cmd = [b._hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared']
    cmd += list(b.DEVICE_FLAGS) + ['-o', target]
    cmd += [os.path.join(src, s) for s in b.SOURCES]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
      raise SystemExit('hipcc failed for %s:\n%s' % (name, res.stdout[-3000:]))
    shutil.rmtree(root)
    print('built', target)


def run(only=()):
  only = list(only)
  select = SELECT
  if '--tests' in only:
    select = only[only.index('--tests') + 1:]
    only = only[:only.index('--tests')]
  results = {}
  for name in [None] + sorted(m for m in MUTANTS if not only or m in only):
    env = dict(os.environ)
    if name:
      env['CMHSE_HIP_LIB'] = os.path.join(OUT, 'libcmhse_%s.so' % name)
    try:
      res = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider',
                            '--tb=line'] + select, cwd=REPO, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=RUN_TIMEOUT_S)
    except subprocess.TimeoutExpired:
      print('=== %s: no end after %d s — nothing more is started on this GPU' % (name or 'product library', RUN_TIMEOUT_S))
      return 2
    if res.returncode < 0 or res.returncode in (134, 139):      # the process died (abort, segmentation fault): a finding
      print('=== %s: the test process died (rc %d) — nothing more is started on this GPU' % (name or 'product library', res.returncode))
      print(res.stdout[-2000:])
      return 2
    failed = [l for l in res.stdout.splitlines() if l.startswith('FAILED')]
    errors = [l for l in res.stdout.splitlines() if l.startswith('ERROR')]
    tail = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ''
    if errors:      # a mutant that does not even load (stale build, ABI drift) has killed nothing
      print('=== %s: %d collection / setup ERRORS — rebuild the mutants (python tools/mutation_check.py build)' % (name, len(errors)))
      failed = []
    results[name or 'product'] = (res.returncode, failed, tail)
    print('=== %s: rc %d  %s' % (name or 'product library', res.returncode, tail))
    for l in failed:
      print('   ', l[:240])
    for l in res.stdout.splitlines():
      if 'Max absolute difference' in l or 'Mismatched elements' in l:
        print('      ', l.strip())
  for m in results:
    if m in EQUIVALENT:
      print('(%s: an equivalent mutant — %s)' % (m, EQUIVALENT[m]))
  ok = results['product'][0] == 0 and all(results[m][1] for m in results if m != 'product' and m not in EQUIVALENT)
  print('mutation check:', 'every mutant killed, product green' if ok else 'HOLE: see above')
  return 0 if ok else 1


if __name__ == '__main__':
  sys.exit(build(sys.argv[2:]) if sys.argv[1:2] == ['build'] else run(sys.argv[2:]))
