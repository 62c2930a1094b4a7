"""The forward shape cases reach the kernels they name (no GPU needed): the dispatch rule of
step_shape / plan_chain / launch_steps / launch_fwd_tail as tests/fwd_shapes.py restates it, its
crossovers checked against the sources, applied to the cases of tests/test_gpu_fwd_shapes.py and of
test_gpu_chain.py's forward resident-tail test.  A moved crossover fails here instead of quietly
moving a case off its target."""
import fwd_shapes as fs


def test_rule_constants_match_the_sources():
  src = fs.source_constants()
  for name, dflt in fs.KNOBS.items():
    assert src[name] == dflt, (name, src[name], dflt)
  assert (src['kTinyBM'], src['kTinyBU']) == (fs.TINY_BM, fs.TINY_BU)
  assert src['kGruBU'] == fs.GRU_BU
  assert src['kFwdTailMaxSeqs'] == fs.FWD_TAIL_MAX_SEQS
  assert src['kChainMaxStepsWs'] == fs.CHAIN_MAX_STEPS
  assert src['kChipCUs'] == fs.CHIP_CUS
  assert src['fwd_tail_kbs'] == fs.FWD_TAIL_KBS
  assert src['kXprojFirstRows'] == fs.XPROJ_FIRST_ROWS


def test_every_case_reaches_its_targets():
  assert len({c[0] for c in fs.CASES}) == len(fs.CASES)
  for name, knobs, train, tail_stream, jobs, targets in fs.CASES:
    # (a training request's companion stream is stream_set()[2] or [3]: job streams [0] and [1] only)
    assert 1 <= len(jobs) <= (2 if train else 4), name
    assert targets <= fs.ALL_TAGS, (name, sorted(targets - fs.ALL_TAGS))
    for j in jobs:
      assert fs.counts_of(fs.lens_of(j['counts'])) == j['counts'], name
      assert j['save'] == train and (j['stream'] is not None) == train, name
      if j['plan'] is not None:
        assert all(p >= c for p, c in zip(j['plan'], j['counts'])) and len(j['plan']) == len(j['counts'])
    tags = fs.call_tags(jobs, knobs, tail_stream)
    assert targets <= tags, (name, sorted(targets - tags))


def test_tail_cases_run_every_kb_and_mb():
  seen = set()
  for pool, cls, H, S, n_long in fs.FWD_TAIL_CASES:
    launches, = fs.call_steps([fs.fwd_tail_case_job(pool, H, S, n_long)])
    tails = [ln for ln in launches if ln['kind'] == 'tail']
    assert len(tails) == 1, (H, S, n_long)
    seen.add(tails[0]['tag'])
  assert seen == {t for t in fs.ALL_TAGS if t.startswith('FwdTail KB')}, sorted(seen)


def test_the_tables_reach_every_tag():
  reached = set()
  for name, knobs, train, tail_stream, jobs, targets in fs.CASES:
    reached |= fs.call_tags(jobs, knobs, tail_stream)
  for pool, cls, H, S, n_long in fs.FWD_TAIL_CASES:
    reached |= fs.call_tags([fs.fwd_tail_case_job(pool, H, S, n_long)])
  assert reached <= fs.ALL_TAGS, sorted(reached - fs.ALL_TAGS)
  assert set(fs.UNREACHABLE) <= fs.ALL_TAGS and not set(fs.UNREACHABLE) & reached
  assert fs.ALL_TAGS - set(fs.UNREACHABLE) <= reached, sorted(fs.ALL_TAGS - set(fs.UNREACHABLE) - reached)
  # every family sees every pool mode it has an epilogue for (but those named unreachable, with the reason)
  for fam, pools in fs.FAMILY_POOLS.items():
    for p in pools:
      assert '%s %s' % (fam, p) in reached or '%s %s' % (fam, p) in fs.UNREACHABLE, (fam, p)


def test_required_edges_are_in_the_table():
  """The profiles hold the edges where the tiles go wrong: S_t at 16 / 17, 32 / 33, 64k +- 1 and
  128k +- 1, length-1 sequences, a last step with one active sequence; H with half a 64-unit column
  tile on a chain, H % 16 != 0 on the mid-size kernel, and a share whose plan passes 1024 while its
  own counts are 1 to 63."""
  counts, chain_h, mid_h, share = set(), set(), set(), False
  for name, knobs, train, tail_stream, jobs, targets in fs.CASES:
    for j, launches in zip(jobs, fs.call_steps(jobs, knobs, tail_stream)):
      counts |= set(j['counts'])
      assert j['counts'][-1] < j['counts'][0] or len(j['counts']) == 1, name   # sequences of several lengths
      fams = {ln['tag'].split(' ')[0] for ln in launches}
      if fams & {'Chain64', 'Chain128'}:
        chain_h.add(j['H'] % 64)
      if any(t.startswith('Mid') for t in fams):
        mid_h.add(j['H'] % 16)
      if j['plan'] is not None and max(j['plan']) > 1024 and max(j['counts']) <= 63:
        share = share or any(ln['kind'] == 'chain' for ln in launches)
  for c in (16, 17, 32, 33, 63, 65, 127, 129, 255, 257, 1):
    assert c in counts, c
  assert 32 in chain_h and any(h != 0 for h in mid_h) and share
  lens1 = [j for c in fs.CASES for j in c[4] if j['counts'][1:2] and j['counts'][1] < j['counts'][0]]
  assert lens1                                   # length-1 sequences
  assert any(j['counts'][-1] == 1 for c in fs.CASES for j in c[4])
  ige = [c for c in fs.CASES if 'Chain128 vec' in c[5] and all(j['I'] >= j['H'] for j in c[4])]
  ilt = [c for c in fs.CASES if 'Chain128 vec' in c[5] and all(j['I'] < j['H'] for j in c[4])]
  assert ige and ilt
