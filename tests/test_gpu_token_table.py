"""The token projection table (tunable tok_table): a token-fed inference request reads the x phase
of its steps from G = emb W_ih^T instead of multiplying; the results must be BIT-identical to the
steps that compute it (tiled per-step kernel, step chain with 64- and 128-row tiles, mid-size tail;
the tiny kernel keeps its own x phase), for every pooling, with and without h0, with out-of-range
token ids and I = 300 (not a multiple of 16)."""
import numpy as np
import pytest
import torch

from cmhse_amd import ops

pytestmark = pytest.mark.gpu


def _requests(dev, seed, specs, V, I):
  """specs: (S, T, H, pool_mode, h0, tokens, full) per request; all token requests share one
  embedding table of V rows and, per H, one set of weights (a caption and a paragraph request)."""
  g = torch.Generator().manual_seed(seed)
  rng = np.random.RandomState(seed)
  keep = []
  table = torch.randn(V, I, generator=g).to(dev)
  keep.append(table)
  shared = {}

  def weights(I_, H, attn):
    key = (I_, H)
    if key not in shared:
      w = dict(w_ih=torch.randn(3 * H, I_, generator=g).mul_(0.1), w_hh=torch.randn(3 * H, H, generator=g).mul_(0.05),
               b_ih=torch.randn(3 * H, generator=g).mul_(0.1), b_hh=torch.randn(3 * H, generator=g).mul_(0.1),
               w_lin=torch.randn(H, H, generator=g).mul_(0.05), b_lin=torch.randn(H, generator=g).mul_(0.1),
               w_att=torch.randn(1, H, generator=g).mul_(0.2))
      shared[key] = {k: v.to(dev) for k, v in w.items()}
    w = shared[key]
    return w if attn else {k: w[k] for k in ('w_ih', 'w_hh', 'b_ih', 'b_hh')}

  reqs = []
  for S, T, H, mode, h0, tokens, full in specs:
    lens = rng.randint(1, T + 1, size=S).astype(np.int64)
    lens[:max(1, full)] = T
    r = dict(weights=weights(I, H, mode == ops.POOL_ATTN), pool_mode=mode, lens=lens, I=I, H=H, device=dev)
    if tokens:
      tok = torch.randint(0, V, (S, T), generator=g)
      # out-of-range ids: clamped to 0 / V - 1 like the embedding lookup of the steps
      flat = tok.view(-1)
      idx = torch.randint(0, flat.numel(), (max(4, flat.numel() // 50),), generator=g)
      flat[idx[0::2]] = -3
      flat[idx[1::2]] = V + 11
      tok = tok.to(dev)
      keep.append(tok)
      r.update(tok_ptrs=ops.padded_row_ptrs(tok), emb_table=table)
    else:
      x = torch.randn(S, T, I, generator=g).to(dev)
      keep.append(x)
      r.update(x_ptrs=ops.padded_row_ptrs(x))
    if h0:
      h = torch.randn(S, H, generator=g).to(dev)
      keep.append(h)
      r.update(h0_ptrs=ops.padded_row_ptrs(h))
    reqs.append(r)
  return reqs, keep


def _run(reqs, table_on):
  with ops.tuned(tok_table=1 if table_on else 0):
    res = ops.gru_pool_fwd_multi(reqs, tail_stream=torch.cuda.Stream(priority=-1))
  torch.cuda.synchronize()
  outs = []
  for r, (out, ctx) in zip(reqs, res):
    outs.append((out.cpu().numpy(), ops.saved_region(ctx, 'hs').cpu().numpy(), ctx['ws'].numel()))
  return outs


CASES = {
    # step chain, 128-row tiles (MSUB 2) at H = 1024, then the mid-size tail; a caption-like and a
    # paragraph-like request share the table beside a feature-fed request
    'chain_h1024_msub2': (dict(chain_tall_min_wgs=1),
                          [(1300, 10, 1024, ops.POOL_ATTN, False, False, 1100),
                           (1400, 6, 1024, ops.POOL_LAST, False, True, 1200),
                           (1200, 14, 1024, ops.POOL_ATTN, True, True, 1100)]),
    # step chain, 64-row tiles
    'chain_h1024_msub1': (dict(chain_tall_min_wgs=0),
                          [(1300, 9, 1024, ops.POOL_MAX, True, True, 1150)]),
    # one launch per time step (no chain), 128-row tiles, then mid
    'per_step': (dict(chain_min_steps=0, tall_tile_min_wgs=64),
                 [(1500, 8, 1024, ops.POOL_ATTN, False, True, 1100),
                  (1300, 7, 1024, ops.POOL_LAST, True, True, 1050)]),
    # H % 32 != 0 (never chained), partial column tiles; every step tiled
    'odd_h': (dict(tiny_max_seqs=0, mid_max_seqs=0),
              [(400, 9, 200, ops.POOL_MAX, False, True, 200),
               (300, 7, 200, ops.POOL_LAST, True, True, 100)]),
    # tiled steps then the tiny kernel (mid-size kernel off): the tail keeps its own x phase
    'tiny_tail': (dict(mid_max_seqs=0),
                  [(1300, 8, 128, ops.POOL_ATTN, True, True, 1100),
                   (1200, 6, 128, ops.POOL_MAX, False, True, 1050)]),
    # mid-size tail from the first step (gx rows from G), with and without h0
    'mid_only': (dict(tiny_max_seqs=0),
                 [(600, 12, 256, ops.POOL_ATTN, False, True, 200),
                  (500, 9, 256, ops.POOL_LAST, True, True, 100),
                  (400, 7, 256, ops.POOL_MAX, True, True, 50)]),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_token_table_is_bit_identical(dev, tune, case):
  knobs, specs = CASES[case]
  tune(**knobs)
  V, I = 97, 300        # word-steps >= 4 x vocab in every token request: the table is on
  reqs, keep = _requests(dev, 7 + len(case), specs, V, I)
  on = _run(reqs, True)
  off = _run(reqs, False)
  for k, (spec, a, b) in enumerate(zip(specs, on, off)):
    if spec[5]:
      assert a[2] > b[2], 'request %d: the table is not on (the test would not test it)' % k
    np.testing.assert_array_equal(a[0], b[0], err_msg='%s request %d: out' % (case, k))
    np.testing.assert_array_equal(a[1], b[1], err_msg='%s request %d: hidden states' % (case, k))
  del keep
