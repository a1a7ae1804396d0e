"""k_s2a_merge and the grouping kernels behind it (k_s2a_count, k_s2a_verify,
k_s2a_compact, k_s2a_gather; csrc/mh_sam2aln.hip) on the directed texts of
tests/s2a_merge_cases.py: byte-equal to the reference's own outputs
(tests/golden/s2a_merge_paths.json), with the launch shape each case exists
for asserted from mh_test_sam2aln_info.  tests/test_oracle_s2a_merge.py pins
the oracle to the same outputs on the CPU; here it only words a mismatch."""
import pytest

import ins_oracle
import og_sam2aln
import s2a_merge_cases as mc
from micall_amd import _native

pytestmark = pytest.mark.gpu

OUTPUTS = ('aligned', 'insert', 'failed')


@pytest.fixture(scope='module')
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture
def hook(ctx):
    """mh_test_set_sam2aln, put back to the product's values afterwards."""
    yield ctx.test_set_sam2aln
    ctx.test_set_sam2aln()


def _oracle(text, cuts):
    saved = og_sam2aln.Q_CUTOFFS
    og_sam2aln.Q_CUTOFFS = list(cuts)
    try:
        return og_sam2aln.sam2aln(text)
    finally:
        og_sam2aln.Q_CUTOFFS = saved


def _fetch(ctx):
    return tuple(ctx.sam2aln_output(w) for w in OUTPUTS)


def _assert_run(ctx, run, got, what=''):
    """got equals the fixture's three outputs and sam2aln_stats their rows."""
    c, cuts = run
    want = mc.want_of(run)
    hint = None
    for name, text in zip(OUTPUTS, got):
        if not isinstance(want[name], str) and hint is None:
            hint = _oracle(c.text, cuts)
        mc.assert_equals_stored(text, want[name], (c.name, cuts, name, what),
                                hint[OUTPUTS.index(name)] if hint else None)
    st = list(ctx.sam2aln_stats())
    assert st == [len(mc.units_of(c.text)), len(c.units), want['rows'][0], want['rows'][2]], st


def _assert_launch(info, c, cuts):
    """The launch mh_test_sam2aln_info reports is the one the case was sized for."""
    span = max(max(s['span']) for s in c.shapes)
    ops = max(max(s['ops']) for s in c.shapes)
    assert info['span_cap'] == (max(span, 1) + 15) // 16 * 16 and info['ops_cap'] == max(ops, 1)
    assert info['wave_bytes'] == mc.wave_bytes(span, ops)
    assert info['wpb'] == mc.wpb_of(info['wave_bytes'])
    assert info['n_merge'] == len(c.units) and info['n_cut'] == len(cuts)


# ---- every case at every list --------------------------------------------------------
@pytest.mark.parametrize('run', [r for r in mc.runs() if not r[0].raises], ids=mc.run_id)
def test_matches_reference(ctx, run):
    c, cuts = run
    ctx.sam2aln_csv(c.text, q_cutoffs=cuts)
    _assert_run(ctx, run, _fetch(ctx))
    info = ctx.test_sam2aln_info()
    _assert_launch(info, c, cuts)
    assert info['key_bits'] == 64
    assert info['blocks'] == min(-(-len(c.units) // info['wpb']), mc.BLOCK_CAP)
    entries = len(c.units) * len(cuts)
    assert info['tsize'] == max(mc.MIN_TABLE, 1 << (2 * entries - 1).bit_length())
    if hasattr(c, 'wpb'):
        assert info['wpb'] == c.wpb
    if hasattr(c, 'tsize'):
        assert info['tsize'] == c.tsize
    if c.name == 'ops':
        assert info['ops_cap'] == 200 > 128
    if c.name == 'reuse_natural':
        # some wave takes a second unit, at the grid's own stride
        assert info['wpb'] == 1 and info['blocks'] == mc.BLOCK_CAP
        assert info['n_merge'] > info['blocks'] * info['wpb']


def test_table_sizes_sit_either_side_of_the_minimum():
    assert [mc.by_name('table_{}'.format(n)).tsize for n in mc.TABLE_SIZES] == [mc.MIN_TABLE, 2 * mc.MIN_TABLE]


# ---- reuse: one wave, many units in turn -----------------------------------------------
@pytest.mark.parametrize('max_blocks', mc.REUSE_MAX_BLOCKS)
@pytest.mark.parametrize('name', ['reuse', 'reuse_reversed'])
def test_one_wave_merges_many_units_in_turn(ctx, hook, name, max_blocks):
    c = mc.by_name(name)
    hook(max_blocks=max_blocks)
    for cuts in c.lists:
        ctx.sam2aln_csv(c.text, q_cutoffs=cuts)
        _assert_run(ctx, (c, cuts), _fetch(ctx), max_blocks)
        info = ctx.test_sam2aln_info()
        _assert_launch(info, c, cuts)
        assert info['blocks'] == max_blocks and info['wpb'] == mc.WPB
        assert info['n_merge'] >= 5 * info['blocks'] * info['wpb']
    hook()
    ctx.sam2aln_csv(c.text, q_cutoffs=c.lists[0])
    assert ctx.test_sam2aln_info()['blocks'] == -(-len(c.units) // mc.WPB)


# ---- a real file -------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['reuse', 'reuse_reversed', 'edges64'])
def test_through_a_real_file(ctx, tmp_path, name):
    """mh_sam2aln_file_q: remap.csv mmap'd by the library."""
    c = mc.by_name(name)
    path = tmp_path / 'remap.csv'
    path.write_text(c.text)
    for cuts in c.lists:
        with open(path) as f:
            ctx.sam2aln_file(f.fileno(), q_cutoffs=cuts)
        _assert_run(ctx, (c, cuts), _fetch(ctx), 'file')
        _assert_launch(ctx.test_sam2aln_info(), c, cuts)


# ---- refusals ------------------------------------------------------------------------------
def _assert_context_still_serves(ctx):
    run = (mc.by_name('roles'), [15])
    ctx.sam2aln_csv(run[0].text, q_cutoffs=run[1])
    _assert_run(ctx, run, _fetch(ctx), 'after a refusal')


def test_span_past_the_lds_budget_is_refused(ctx):
    c = mc.by_name('wpb_refused')
    with pytest.raises(_native.NativeError, match=c.refused):
        ctx.sam2aln_csv(c.text, q_cutoffs=c.lists[0])
    info = ctx.test_sam2aln_info()
    assert info['wave_bytes'] > mc.LDS and info['wpb'] == 0 and info['blocks'] == 0
    _assert_context_still_serves(ctx)


def test_all_gap_unit_is_refused_as_the_reference_raises(ctx):
    c = mc.by_name('status_allgap')
    want = mc.want_of((c, c.lists[0]))['raises']
    assert want['class'] == 'ZeroDivisionError'
    with pytest.raises(_native.NativeError, match='all gaps') as err:
        ctx.sam2aln_csv(c.text, q_cutoffs=c.lists[0])
    assert 'unit 1 is all gaps' in str(err.value) and want['message'] in str(err.value)
    _assert_context_still_serves(ctx)


# ---- the collision report ---------------------------------------------------------------------
def test_short_key_reports_a_collision(ctx, hook):
    """An 8-bit key: more (reference, cutoff, body) groups than keys, so
    k_s2a_verify must find distinct sequences under one key and the call must
    say so instead of merging them; with the whole hash again, the same
    context gives the reference's output for the same text."""
    c = mc.by_name('distinct')
    cuts = c.lists[-1]
    assert mc.want_of((c, cuts))['rows'][0] > 256
    hook(key_bits=8)
    assert ctx.test_sam2aln_info()['key_bits'] == 8
    with pytest.raises(_native.NativeError, match='collision'):
        ctx.sam2aln_csv(c.text, q_cutoffs=cuts)
    hook()
    ctx.sam2aln_csv(c.text, q_cutoffs=cuts)
    _assert_run(ctx, (c, cuts), _fetch(ctx), 'after a collision')


def test_short_key_reports_a_collision_among_insertions(ctx, hook):
    """The same narrowing reaches the table of conseq_ins.csv (k_s2a_ins_tab
    and its k_s2a_verify): the count is refused, and counted again with the
    whole hash it equals tests/ins_oracle.py."""
    text = mc.ins_collision_text()
    want = ins_oracle.conseq_ins(text, [15])
    assert want.count('\n') - 1 > 256
    ctx.sam2aln_csv(text, q_cutoffs=[15])
    hook(key_bits=8)
    with pytest.raises(_native.NativeError, match='insertion hash collision'):
        ctx.sam2aln_conseq_ins()
    hook()
    assert ctx.sam2aln_conseq_ins() == want


@pytest.mark.parametrize('bits,blocks', [(7, 0), (65, 0), (64, -1)])
def test_hook_refuses_bad_arguments(ctx, bits, blocks):
    with pytest.raises(_native.NativeError, match='mh_test_set_sam2aln'):
        ctx.test_set_sam2aln(bits, blocks)
    assert ctx.test_sam2aln_info()['key_bits'] == 64
