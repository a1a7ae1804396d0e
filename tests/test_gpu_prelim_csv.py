"""Context.rows_load_csv is mh_prelim_parse plus mh_rows_load: on three of the
edge texts of tests/prelim_cases.py it returns what _native.prelim_parse
returns, and a pileup of its rows equals the pileup of the same rows loaded
through Context.rows_load."""
import numpy as np
import pytest

import prelim_cases as pc
from micall_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _pileup(ctx, n_refs):
    ctx.pileup(1, 20, [64] * n_refs)
    return ctx.pileup_fetch()


@pytest.mark.parametrize('name', ['plain', 'inner_newline', 'unknown_rnames'])
def test_rows_load_csv_equals_prelim_parse_and_rows_load(ctx, name):
    text = pc.TEXTS[name]
    args, want = _native.prelim_parse(text, pc.REFNAMES)
    got = ctx.rows_load_csv(text, pc.REFNAMES)
    assert got['n_rows'] == want['n_rows'] > 0 and got['n_units'] == want['n_units'] > 0
    assert np.array_equal(got['info'], want['info'])
    assert got['present'].tolist() == want['present'].tolist() and got['unknown'] == want['unknown']
    n_refs = len(want['present'])
    from_csv = _pileup(ctx, n_refs)
    ctx.rows_load(*args)
    from_rows = _pileup(ctx, n_refs)
    assert from_csv['read_counts'].sum() > 0
    for key in ('dense', 'nflag', 'dflag', 'read_counts', 'first_unit', 'max_pos'):
        assert np.array_equal(from_csv[key], from_rows[key]), (name, key)
    assert from_csv['cap'] == from_rows['cap']
    assert sorted(from_csv['events']) == sorted(from_rows['events'])
