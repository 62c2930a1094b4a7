"""The BPTT shape cases reach the kernels they name (no GPU needed): the dispatch rule of
bwd_steps / bwd_tail as tests/bptt_shapes.py restates it, its crossovers checked against the
sources, applied to the cases of tests/test_gpu_bptt_shapes.py and of test_gpu_chain.py's
resident-tail test.  A moved crossover fails here instead of quietly moving a case off its target."""
import bptt_shapes as bs

ALL_TARGETS = {'Waves4 vec', 'Waves4 scalar', 'Waves8 vec', 'Waves8 scalar', 'Mid16', 'Mid32',
               'Mid32 many row tiles', 'Split', 'Split S_next=0', 'Split splits=1', 'Split <=16 rows',
               'Split ragged column tile', 'Split short last K slice'} | {
               'Tail KB%d MB%d' % (kb, mb) for kb in bs.TAIL_KBS for mb in (1, 2)}


def test_rule_constants_match_the_sources():
  src = bs.source_constants()
  for name, dflt in bs.KNOBS.items():
    assert src[name] == dflt, (name, src[name], dflt)
  assert src['kBwdNw8Max'] == bs.NW8_MAX
  assert src['kTailMaxSeqs'] == bs.TAIL_MAX_SEQS
  assert (src['kRecBM'], src['kRecBN'], src['kRecBK']) == (bs.REC_BM, bs.REC_BN, bs.REC_BK)
  assert src['tail_kbs'] == bs.TAIL_KBS


def test_every_case_reaches_its_targets():
  for name, knobs, S, T, I, H, profile, pool, targets in bs.CASES:
    assert len(profile) == T and profile[0] == S, name
    lens = bs.lens_of(profile)
    assert bs.counts_of(lens) == list(profile), name
    tags = bs.shape_tags(bs.step_shapes(list(profile), H, True, knobs))
    assert targets <= tags, (name, sorted(targets - tags))


def test_tail_cases_run_every_kb_and_mb():
  seen = set()
  for pool, cls, H, S, n_long in bs.TAIL_CASES:
    counts = bs.tail_case_counts(H, S, n_long)
    tail = bs.tail_of(counts, H)
    assert tail is not None, (H, S, n_long)
    seen.add('Tail KB%d MB%d' % tail[1:])
  assert seen == {t for t in ALL_TARGETS if t.startswith('Tail')}, sorted(seen)


def test_the_tables_reach_every_shape():
  reached = set()
  for name, knobs, S, T, I, H, profile, pool, targets in bs.CASES:
    reached |= bs.shape_tags(bs.step_shapes(list(profile), H, True, knobs))
  for pool, cls, H, S, n_long in bs.TAIL_CASES:
    reached |= bs.shape_tags(bs.step_shapes(bs.tail_case_counts(H, S, n_long), H, True))
  assert ALL_TARGETS <= reached, sorted(ALL_TARGETS - reached)


def test_mixed_jobs_share_a_launch_across_shapes():
  """test_gpu_bptt_shapes.MIXED_JOBS: launch i serves step Tmax_k - 1 - i of every job; at i = 0 two
  vec Waves4 jobs of different H share one launch beside a scalar Waves4 job and a Split job."""
  import importlib.util
  import os
  spec = importlib.util.spec_from_file_location(
      '_mixed', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_bptt_shapes.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  jobs = mod.MIXED_JOBS
  assert len({len(p) for _, _, _, p in jobs}) > 1      # chains of different lengths
  first = []
  for cls, I, H, profile in jobs:
    steps = bs.step_shapes(list(profile), H, True)
    assert steps[0]['t'] == len(profile) - 1       # no resident tail: launch 0 is the last step
    first.append((steps[0]['shape'], steps[0]['vec'], H))
  vec4 = [h for s, v, h in first if s == 'Waves4' and v]
  assert len(vec4) >= 2 and len(set(vec4)) == len(vec4), first
  assert ('Waves4', False) in [(s, v) for s, v, _ in first], first
  assert any(s in ('Split', 'Mid16', 'Mid32') for s, _, _ in first), first
