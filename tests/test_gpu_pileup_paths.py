"""k_pileup and the k_tok_* token aggregation on the directed path cases of
tests/pileup_path_cases.py: every counter (dense, nflag, dflag, read counts,
reference order by first unit, last positions, insertion tokens) through
source 1 against the oracle pileup and against the reference's counters
(tests/golden/pileup_paths.json), at cutoffs 0 and 20, with the launch
geometry each case exists for asserted from mh_test_pileup_info.  Every case
runs twice on one context, in two orders, so nothing kept from a differently
shaped launch (window maps, scratch, token tables, cached block shapes) can
hide."""
import json
import os
from collections import Counter

import numpy as np
import pytest

import oracle
import pileup_path_cases as ppc
from micall_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'pileup_paths.json')) as f:
        return {(c['name'], c['quality_cutoff']): c for c in json.load(f)['cases']}


_WANT = {}


def _oracle(case, q):
    """The oracle pileup of a case, computed once and shared."""
    if (case.name, q) not in _WANT:
        _WANT[(case.name, q)] = oracle.pileup(case.ref_names, case.pairs, q)
    return _WANT[(case.name, q)]


def _refmap(p, ref_names):
    events = {}
    for r, pos, tok, count in p['events']:
        events.setdefault((r, pos), Counter())[tok] += count
    refmap, counts = {}, Counter()
    order = sorted((p['first_unit'][r], r) for r in range(len(ref_names)) if p['first_unit'][r] >= 0)
    for _, r in order:
        counts[ref_names[r]] = int(p['read_counts'][r])
        top = int(p['max_pos'][r])
        pos_nucs = {}
        dense, nflag, dflag = p['dense'][r, :top], p['nflag'][r, :top], p['dflag'][r, :top]
        for i in np.flatnonzero(dense.any(axis=1) | (nflag != 0) | (dflag != 0)).tolist():
            c = Counter({tok: int(dense[i, k]) for k, tok in enumerate('ACGT') if dense[i, k]})
            if nflag[i]:
                c['N'] = -1
            if dflag[i]:
                c['-'] = -2
            pos_nucs[i + 1] = c
        for (er, pos), c in events.items():
            if er == r:
                pos_nucs.setdefault(pos, Counter()).update(c)
        refmap[ref_names[r]] = (pos_nucs, top)
    return refmap, counts


def _run(ctx, case, q, golden=None, only=None):
    ctx.rows_load(*case.args)
    ctx.pileup(1, q, case.ref_lens, only=only)
    p = ctx.pileup_fetch()
    info = ctx.test_pileup_info()
    if only is not None:
        return p, info
    got, got_counts = _refmap(p, case.ref_names)
    want, want_counts = _oracle(case, q)
    assert list(got) == list(want), case.name
    assert got_counts == want_counts, case.name
    for name in want:
        assert got[name][1] == want[name][1], (case.name, name)            # max_pos
        assert got[name][0] == want[name][0], (case.name, name)
    # nothing counted past a reference's last position
    for r in range(len(case.ref_names)):
        top = int(p['max_pos'][r])
        assert not p['dense'][r, top:].any() and not p['nflag'][r, top:].any() and \
            not p['dflag'][r, top:].any(), (case.name, r)
    if golden is not None:
        g = golden[(case.name, q)]
        assert g['sam'] == case.sha()
        assert list(got) == g['order'], case.name
        ppc.assert_equals_stored(ppc.canonical_counters(got), g['counters'], case.name)
    assert info['n_units'] == len(case.pairs)
    return p, info


def _geometry(case, info):
    """The launch shape each case was built for."""
    hit = np.bincount(case.args[1], minlength=len(case.ref_names)) > 0
    win = np.array(info['win_len'])
    if case.name == 'windows_a':
        assert win[0] == case.ref_lens[0] + 64 < case.ref_lens[0] + ppc.SLACK
    if case.name == 'windows_b1':
        assert info['win_words'] == 0 and win[0] == 0
    if case.name == 'windows_b2':
        assert win[0] == 0 and win[1] > 0 and info['win_words'] == 2 * win[1]
    if case.name == 'windows_c':
        assert (hit & (win == 0)).any() and (hit & (win > 0)).any()
        assert not win[~hit].any()
        # most-hit first; the room runs out among the tied references, and
        # there the lower index gets the window
        assert all(win[t] > 0 for t in ppc.WIN_C_TOP)
        with_win = [t for t in ppc.WIN_C_TIED if win[t] > 0]
        assert 0 < len(with_win) < len(ppc.WIN_C_TIED)
        assert with_win == list(ppc.WIN_C_TIED[:len(with_win)])
    if case.name == 'units':
        assert info['n_units'] > info['blocks'] * info['wpb']
    if case.name.startswith('tokens_'):
        assert info['tok_events'] == len(case.pairs)
        assert info['tok_keys'] > 4096
        assert info['tok_insert_blocks'] > 1 and info['tok_count_blocks'] > 1
    if case.name == 'tokens_{}'.format(ppc.TOKENS_PAIRS[1]):
        assert info['tok_keys'] > ppc.TOK_KEYS


def test_every_case_twice_in_two_orders(ctx, golden):
    cases = ppc.cases()
    wpbs, ran = set(), set()
    order = list(range(len(cases)))
    for rnd, idx in enumerate((order, order[::-1])):
        for k in idx:
            case = cases[k]
            for q in (ppc.Q_CUTOFFS if rnd == 0 else ppc.Q_CUTOFFS[::-1]):
                _, info = _run(ctx, case, q, golden)
                _geometry(case, info)
                if case.name.startswith('units_'):
                    wpbs.add(info['wpb'])
                    ran.add(info['n_units'])
    # unit counts around the waves of one block
    assert len(wpbs) == 1
    wpb = wpbs.pop()
    assert wpb <= ppc.MAX_WPB      # the prefixes reach wpb + 1
    assert {1, wpb, wpb + 1} | ({wpb - 1} - {0}) <= ran, (wpb, sorted(ran))


def test_only_subsets_on_rows(ctx):
    """mh_pileup_only on source 1: the counted references' counters are the
    full pileup's, the others' stay empty (windows b and c)."""
    by_name = {c.name: c for c in ppc.cases()}
    for name, only in (('windows_b2', [0]), ('windows_b2', [1]), ('windows_c', [3, 9, 13]),
                       ('windows_c', [4]), ('windows_c', [0, 1, 5, 7, 8, 11, 12, 15])):
        case = by_name[name]
        full, _ = _run(ctx, case, 20)
        part, info = _run(ctx, case, 20, only=only)
        assert [w == -1 for w in info['win_len']] == [r not in only for r in range(len(case.ref_names))]
        for r in range(len(case.ref_names)):
            if r in only:
                for k in ('dense', 'nflag', 'dflag'):
                    assert np.array_equal(part[k][r], full[k][r]), (name, r, k)
                for k in ('read_counts', 'first_unit', 'max_pos'):
                    assert part[k][r] == full[k][r], (name, r, k)
            else:
                assert part['read_counts'][r] == 0 and part['first_unit'][r] < 0 and part['max_pos'][r] == 0
                assert not part['dense'][r].any() and not part['nflag'][r].any() and not part['dflag'][r].any()
        assert sorted(e for e in part['events'] if e[0] in only) == \
            sorted(e for e in full['events'] if e[0] in only)
        assert not [e for e in part['events'] if e[0] not in only]


def test_tokens_with_tiny_buffers(ctx, golden):
    """The token cases again with event, pool and token buffers a test
    imposes, so the grow-and-retry paths run on these shapes."""
    try:
        ctx.test_set_capacities(pileup_events=64, pileup_event_bytes=256, token_bytes=128)
        before = ctx.retry_counts()
        for case in ppc.cases():
            if case.name.startswith('tokens_'):
                _, info = _run(ctx, case, 20, golden)
                _geometry(case, info)
        after = ctx.retry_counts()
        assert after['pileup_events'] > before['pileup_events']
        assert after['token_bytes'] > before['token_bytes']
    finally:
        ctx.test_set_capacities()


def test_refused_inputs(ctx):
    """129 ops, a read past cap and merged insertions past PU_INSBUF are
    refused with their errors; the read past cap leaves no count in the
    next reference's counters, and the context still piles up afterwards."""
    for name, sam, ref_lens, stage, message in ppc.error_cases():
        ref_names, pairs, args = ppc.rows_of(sam)
        if stage == 'rows_load':
            with pytest.raises(_native.NativeError, match=message):
                ctx.rows_load(*args)
            continue
        ctx.rows_load(*args)
        with pytest.raises(_native.NativeError, match=message):
            ctx.pileup(1, 20, ref_lens)
        if name == 'past_cap':
            p = ctx.pileup_fetch(only=[0, 1])
            assert p['read_counts'][1] == 0 and p['max_pos'][1] == 0
            cap = p['cap']
            dense = np.zeros((2, cap, 4), dtype=np.int32)
            nflag = np.zeros((2, cap), dtype=np.uint8)
            dflag = np.zeros((2, cap), dtype=np.uint8)
            rc, fu = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
            mp = np.zeros(2, dtype=np.int32)
            _native.check(_native.lib().mh_pileup_fetch(ctx.h, _native._ptr(dense), _native._ptr(nflag),
                                                        _native._ptr(dflag), _native._ptr(rc),
                                                        _native._ptr(fu), _native._ptr(mp)),
                          'mh_pileup_fetch')
            assert not dense[1].any() and not nflag[1].any() and not dflag[1].any()
            assert dense[0].sum() > 0
    case = ppc.cases()[0]
    _run(ctx, case, 20)


def test_tokens_big_lds_table_full(ctx):
    """k_tok_insert's li < 0 path: more events per block than TOK_LDS_SLOTS,
    nearly all distinct keys; the (position, token, count) set equals
    numpy.unique over the constructed keys."""
    args, ref_lens, (uniq, count) = ppc.tokens_big()
    n_pairs = len(args[0]) // 2
    ctx.rows_load(*args)
    ctx.pileup(1, 20, ref_lens)
    p = ctx.pileup_fetch(events=False)
    info = ctx.test_pileup_info()
    assert info['tok_events'] == n_pairs
    assert info['tok_insert_blocks'] == info['tok_count_blocks'] == ppc.TOK_BLOCKS
    assert info['tok_events'] // info['tok_insert_blocks'] > ppc.TOK_SLOTS
    assert info['tok_keys'] == len(uniq) > ppc.TOK_KEYS
    assert info['tok_keys'] // info['tok_insert_blocks'] > ppc.TOK_SLOTS
    assert p['read_counts'][0] == n_pairs and p['first_unit'][0] == 0
    key, cnt = ppc.tokens_big_keys(p['ev_raw'])
    assert np.array_equal(key, uniq) and np.array_equal(cnt, count)
    # the positions' plain bases: only the second M base of each pair
    assert int(p['dense'].sum()) == n_pairs and p['max_pos'][0] == ppc.TOKENS_BIG_POS + 1


def test_source_0_long_reference_beside_short(ctx):
    """Mapped records (source 0), unpaired and paired, on a 20 000-position
    reference beside a short one: the no-window path under the mapper's
    records, against the oracle pileup of the same records."""
    from micall_amd import projects, synth
    import random
    rng = random.Random(5)
    seeds = projects.load_default().seed_sequences()
    short = seeds['HIV1B-pol-seed']
    big = ''.join(rng.choices('ACGT', k=ppc.BIG_REF))
    refnames, refseqs = ['big', 'HIV1B-pol-seed'], [big, short]
    for paired in (True, False):
        pairs = synth.make_pairs(400, genomes={'big': big, 'HIV1B-pol-seed': short}, genome_seed=31,
                                 read_seed=32, indel_rate=0.01)
        names, seqs, quals = synth.interleave(pairs)
        ctx.index_build(refnames, refseqs, 20)
        ctx.reads_load(seqs, quals, paired)
        ctx.map(_native.params(oracle.LOCAL))
        alns = ctx.fetch()
        lines = ['@HD\tVN:1.0\tSO:unsorted\n'] + ['@SQ\tSN:{}\tLN:0\n'.format(r) for r in refnames]
        for i in range(len(seqs)):
            a = oracle.OgAln.from_buffer_copy(alns[i].tobytes())
            # unpaired: every read its own unit, as the device takes them
            qname = oracle.qname_of(names[i], True) if paired else 'read{}'.format(i)
            lines.append('\t'.join(oracle.sam_fields(a, qname, seqs[i], quals[i], refnames)) + '\n')
        want, want_counts = oracle.pileup(*oracle.matchmaker(lines), 20)
        ctx.pileup(0, 20, [len(s) for s in refseqs])
        info = ctx.test_pileup_info()
        got, got_counts = _refmap(ctx.pileup_fetch(), refnames)
        assert want_counts['big'] > 0 and want_counts['HIV1B-pol-seed'] > 0
        assert info['win_len'][0] == 0 and info['win_len'][1] > 0
        assert list(got) == list(want) and got_counts == want_counts
        for name in want:
            assert got[name] == want[name], (paired, name)
