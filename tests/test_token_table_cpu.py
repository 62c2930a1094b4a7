"""CPU-side checks of the token projection table's gate and workspace term
(cmhse_gru_pool_workspace_tok, tunable tok_table): pure host functions, no GPU."""
from cmhse_amd import _lib, ops

VOCAB, I, H = 13058, 300, 1024
TABLE = (VOCAB * 3 * H * 4 + 255) // 256 * 256     # G[vocab, 3H] f32, one 256-byte aligned region


def _sizes(S, Tmax, sum_T, I_, H_, mode, vocab):
  lib = _lib.load()
  return (lib.cmhse_gru_pool_workspace(S, Tmax, sum_T, I_, H_, mode),
          lib.cmhse_gru_pool_workspace_tok(S, Tmax, sum_T, I_, H_, mode, vocab))


def test_table_term_above_the_gate():
  # the bench split's text request: 539 684 word-steps over 13 058 tokens
  base, tok = _sizes(9834, 480, 539684, I, H, 0, VOCAB)
  assert tok - base == TABLE
  assert TABLE == 160456704       # 160 MB
  # exactly at the gate (word-steps == 4 x vocab) and one below
  base, tok = _sizes(4000, 40, 4 * VOCAB, I, H, 0, VOCAB)
  assert tok - base == TABLE
  base, tok = _sizes(4000, 40, 4 * VOCAB - 1, I, H, 0, VOCAB)
  assert tok == base


def test_no_table_outside_the_exact_inference_path():
  # a training batch (32 paragraphs, ~3k word-steps) stays below the gate
  base, tok = _sizes(32, 250, 3000, I, H, _lib.SAVE_FOR_BACKWARD, VOCAB)
  assert tok == base
  base, tok = _sizes(32, 250, 3000, I, H, 0, VOCAB)
  assert tok == base
  # training and bf16x3 calls keep their paths whatever their size
  for mode in (_lib.SAVE_FOR_BACKWARD, _lib.MATH_BF16X3, 1 | _lib.SAVE_FOR_BACKWARD):
    base, tok = _sizes(9834, 480, 539684, I, H, mode, VOCAB)
    assert tok == base, mode
  # no tokens, no dwordx4 shapes, a table whose row offsets would not fit an int32
  assert _sizes(9834, 480, 539684, I, H, 0, 0)[1] == _sizes(9834, 480, 539684, I, H, 0, 0)[0]
  assert _sizes(9834, 480, 539684, 302, H, 0, VOCAB)[1] == _sizes(9834, 480, 539684, 302, H, 0, VOCAB)[0]
  big = 200000
  assert _sizes(90000, 480, 4 * big, I, 4096, 0, big)[1] == _sizes(90000, 480, 4 * big, I, 4096, 0, big)[0]


def test_tunable_switches_the_table_off():
  assert ops.tune('tok_table') == 1          # the default
  with ops.tuned(tok_table=0):
    base, tok = _sizes(9834, 480, 539684, I, H, 0, VOCAB)
    assert tok == base
  base, tok = _sizes(9834, 480, 539684, I, H, 0, VOCAB)
  assert tok - base == TABLE
