"""The planner of the text tower's prefix sharing (evaluation.text_prefix_aliases, pure NumPy): which
first captions leave the level-1 text request and which rows of which paragraph stand in for them; and
the host-side token check (evaluation.text_prefix_flags on host tensors).  No GPU."""
import numpy as np
import pytest
import torch

from cmhse_amd import evaluation, ops, synthetic


def _lengths(spec):
  num_caps = np.asarray(spec.num_clips, dtype=np.int64)
  len_cap = np.asarray(spec.words_per_sent, dtype=np.int64)
  starts = np.cumsum(num_caps) - num_caps
  len_par = np.add.reduceat(len_cap, starts)
  return len_cap, len_par, num_caps, starts


def _check(len_cap, len_par, num_caps, starts, flags):
  kept, (vid, a_len, a_row) = evaluation.text_prefix_aliases(len_cap, len_par, num_caps, flags)
  want = np.ones(len(num_caps), dtype=bool) if flags is None else np.asarray(flags) != 0
  want &= len_par >= len_cap[starts]
  np.testing.assert_array_equal(vid, np.flatnonzero(want))       # sources: the flagged videos' paragraphs
  np.testing.assert_array_equal(a_row, starts[vid])              # rows: their first captions
  np.testing.assert_array_equal(a_len, len_cap[starts[vid]])     # lengths: the captions' own
  assert (a_len <= len_par[vid]).all() and (a_len >= 1).all()
  # kept + aliased = all captions, each once
  both = np.concatenate([kept, a_row])
  np.testing.assert_array_equal(np.sort(both), np.arange(len(len_cap)))
  assert (np.diff(kept) > 0).all()
  return kept, vid, a_len, a_row


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_planner_on_ragged_splits(seed):
  spec = synthetic.ragged_spec(24, seed=seed)
  len_cap, len_par, num_caps, starts = _lengths(spec)
  single = int((num_caps == 1).sum())
  assert 4 <= single <= 7 and (len_cap == 1).any()      # single-caption videos and length-1 items
  kept, vid, a_len, _ = _check(len_cap, len_par, num_caps, starts, None)
  assert len(vid) == 24
  # a single-caption video aliases its whole paragraph
  np.testing.assert_array_equal(a_len[num_caps == 1], len_par[num_caps == 1])
  # flags partly 0: those videos keep their first caption
  flags = np.ones(24, dtype=np.int32)
  flags[::3] = 0
  kept_f, vid_f, _, _ = _check(len_cap, len_par, num_caps, starts, flags)
  assert len(vid_f) == 16 and set(starts[::3]) <= set(kept_f.tolist())
  # a paragraph shorter than the first caption is never aliased, whatever its flag says
  short = len_par.copy()
  short[5] = len_cap[starts[5]] - 1
  _, vid_s, _, _ = _check(len_cap, short, num_caps, starts, None)
  assert 5 not in vid_s.tolist() and len(vid_s) == 23


def test_planner_on_the_full_split():
  spec = synthetic.anet_like_spec(4917, seed=0)
  len_cap, len_par, num_caps, starts = _lengths(spec)
  kept, vid, a_len, _ = _check(len_cap, len_par, num_caps, starts, None)
  assert len(vid) == 4917
  assert int(a_len.sum()) == 75615 and int(a_len.max()) == 91
  assert int(len_cap.sum()) + int(len_par.sum()) == 539684
  # the plan trap: without the first captions the text tower falls to <= 1024 sequences one step earlier,
  # so the reduced request must carry the step plan of the ORIGINAL lengths
  orig = ops.step_counts(np.concatenate([len_cap, len_par]))
  red = ops.step_counts(np.concatenate([len_cap[kept], len_par]))
  assert len(orig) == len(red) and (orig >= red).all()
  assert int((orig > 1024).sum()) == 72 and int((red > 1024).sum()) == 71
  # tiled row-steps and 128-row tiles per column tile of the steps the plan keeps tiled
  assert int(orig[:72].sum()) == 509022 and int(red[:72].sum()) == 433610
  tiles = lambda c: int(((c[:72] + 127) // 128).sum())
  assert tiles(orig) == 4014 and tiles(red) == 3423


def test_planner_rejects_a_broken_contract():
  with pytest.raises(ValueError):
    evaluation.text_prefix_aliases([3, 2], [5], [1], None)       # counts do not add up
  with pytest.raises(ValueError):
    evaluation.text_prefix_aliases([3], [3, 1], [1, 0], None)    # a video without captions


def test_host_token_check():
  spec = synthetic.ragged_spec(24, seed=1)
  batches = synthetic.make_batches(spec, 7, 8, 60, seed=2)
  flags = evaluation.text_prefix_flags([batches[:2], batches[2:]], torch.device('cpu'))
  assert [len(f) for f in flags] == [14, 10] and all(f.all() for f in flags)
  # one token of a paragraph's prefix changed / a paragraph cut below its first caption
  b = list(batches[0])
  pars, len_par = b[3].clone(), b[7].clone()
  pars[2, 0] += 1
  first = np.cumsum(b[9]) - np.asarray(b[9])
  l0 = int(b[5][first[4]])
  len_par[4] = l0 - 1 if l0 > 1 else len_par[4]
  b[3], b[7] = pars, len_par
  got = evaluation.text_prefix_flags([[tuple(b)]], torch.device('cpu'))[0]
  want = np.ones(7, dtype=bool)
  want[2] = False
  want[4] = l0 == 1
  np.testing.assert_array_equal(got, want)
  # Ragged host tensors take the per-video path
  rag = list(batches[1])
  rag[1] = ops.Ragged(torch.cat([rag[1][i, :int(l)] for i, l in enumerate(rag[5])]), rag[5].numpy())
  rag[3] = ops.Ragged(torch.cat([rag[3][i, :int(l)] for i, l in enumerate(rag[7])]), rag[7].numpy())
  assert evaluation.text_prefix_flags([[tuple(rag)]], torch.device('cpu'))[0].all()


def test_the_tunable_lives_in_the_one_table():
  assert ops.tune('share_prefix') == 1          # the default
  with ops.tuned(share_prefix=0):
    assert ops.tune('share_prefix') == 0
    ctx = ops.TuneContext()                     # a context starts from the process values
    assert ctx.tune('share_prefix') == 0
  assert ops.tune('share_prefix') == 1
  with ops.TuneContext(share_prefix=0):         # ... and ops.tune reads the current context
    assert ops.tune('share_prefix') == 0
  assert ops.tune('share_prefix') == 1
