"""Host-side replay of `tests/golden/loss_spellings.json` (no GPU, no built library): every recorded (spelling, keywords) row,
every `parse_*` and every `check_*` gives today what it gave when the file was written by `tests/golden/make_loss_spellings.py`
-- the exact result, or the exception's type and its exact message."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def maker():
    spec = importlib.util.spec_from_file_location('make_loss_spellings', os.path.join(GOLDEN, 'make_loss_spellings.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope='module')
def table():
    with open(os.path.join(GOLDEN, 'loss_spellings.json')) as f:
        return json.load(f)


def differences(table, labels, inputs, cells, replay):
    """The cells whose live outcome is not the recorded one, as readable lines."""
    out = []
    for given, recorded in zip(inputs, cells):
        for label, want, got in zip(labels, recorded, replay(given)):
            if want is not None and table['outcomes'][want] != got:
                out.append(f'{label}{given!r}: recorded {table["outcomes"][want]!r}, now {got!r}')
    return out


def test_the_file_is_the_grid_of_its_generator(maker, table):
    assert table['spellings'] == maker.NAMES + maker.SUMS and table['surfaces'] == maker.SURFACES
    assert json.dumps(table['keywords'], sort_keys=True) == json.dumps(maker.KEYWORD_SETS, sort_keys=True)      # (as text: nan != nan)
    assert len(table['grid_of']) == len(table['spellings']) and all(len(g) == len(table['keywords']) for g in table['grid'])
    assert len(table['spellings']) * len(table['keywords']) >= 1541


def test_every_row_resolves_as_recorded(maker, table):
    rows = [(name, kw) for name in table['spellings'] for kw in table['keywords']]
    cells = [table['rows'][c] for line in table['grid_of'] for c in table['grid'][line]]
    bad = differences(table, table['surfaces'], rows, cells, lambda r: maker.row(*r))
    assert not bad, f'{len(bad)} of {len(cells) * len(table["surfaces"])} differ:\n' + '\n'.join(bad[:20])


def test_every_name_parses_as_recorded(maker, table):
    bad = differences(table, table['parsers'], table['spellings'], table['parse'], maker.parses)
    bad += differences(table, ['parse_suffix'], [tuple(c) for c in table['suffix_calls']], [[c] for c in table['parse_suffix']],
                       lambda c: [maker.outcome(maker.loss_names.parse_suffix, *c)])
    assert not bad, '\n'.join(bad[:20])


def test_every_value_checks_as_recorded(maker, table):
    bad = differences(table, table['checks'], table['check_values'], table['check'], maker.checks)
    bad += differences(table, ['check_window'], [tuple(p) for p in table['window_pairs']], [[c] for c in table['check_window']],
                       lambda p: [maker.outcome(maker.loss_names.check_window, *p)])
    assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('value', [float('inf'), float('-inf'), 10 ** 400])
def test_no_number_escapes_the_whole_number_checks(maker, value):
    """The two inputs the file leaves out.  Before the five checks were one, `check_radius` answered an infinity with
    OverflowError, and the other three an int too large for a float; the documented ValueError is what all of them give."""
    names = maker.loss_names
    for check, keyword, noun, hi in ((names.check_radius, 'radius', 'boundary radius', 16), (names.check_cap, 'cap', 'surface cap', 4095),
                                     (names.check_window, 'window', 'potts window radius', 7), (names.check_depth, 'depth', 'cldice depth', 16)):
        with pytest.raises(ValueError) as e:
            check(value)
        assert str(e.value) == f'{keyword}={value!r}: the {noun} must be a whole number in 1 .. {hi}'
    with pytest.raises(ValueError, match='dilation=.*the potts dilation must be a whole number in 1 .. 4'):
        names.check_window(3, value)
    with pytest.raises(ValueError, match='radius=.*the boundary radius must be a whole number in 1 .. 16'):
        names.resolve_radius('boundary_f', value)
