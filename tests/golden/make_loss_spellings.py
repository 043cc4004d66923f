"""The recorded outcomes of the device losses' spellings (host only; needs neither a GPU nor the built library).

    python tests/golden/make_loss_spellings.py
Runs every (spelling, keywords) row of the grid below through the host surfaces that turn a `loss_func` and its keywords into
what the engine is told, and writes the results, or the exceptions' type names and exact messages, to loss_spellings.json.
tests/test_loss_spellings_host.py replays the file against the live code, so the file is written once, from the code whose
behaviour is to be kept, and not again: a second run reproduces it byte for byte.  Two inputs are left out on purpose, because
the checks of the five knobs answered them differently: `radius=+-inf`, and a whole number too large for a float.  The test file
states what they give.
"""
import collections
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from eosvos_amd import engine, loss_names, loss_sum  # noqa: E402

OUT = os.path.join(HERE, 'loss_spellings.json')
KEYWORDS = ('fraction', 'radius', 'cap', 'window', 'depth')
NAN, INF = float('nan'), float('inf')


def suffixes(base, hi, glued, junk, some):
    """The lowest and highest suffix, one past it, zero, a leading zero, an empty, a glued and a non-digit suffix, and `some`."""
    return [base, f'{base}_1', f'{base}_{hi}', f'{base}_{hi + 1}', f'{base}_0', f'{base}_0{some}', f'{base}_', base + glued,
            f'{base}_{junk}', f'{base}_{some}']


NAMES = (
    ['cross_entropy', 'dice', 'cross_entropy_and_dice', 'class_balanced_cross_entropy', 'lovasz_hinge', 'lovasz_hinge_flat']
    + suffixes('bootstrapped_cross_entropy', 100, '30', 'x', 30)
    + suffixes('boundary_f', 16, '4', 'a', 4) + ['boundary_f_3', 'boundary_f_4_4', 'boundary_f_-4']
    + suffixes('cross_entropy_and_boundary_f', 16, '4', 'a', 3)
    + suffixes('surface', 4095, 's', '6a', 64) + ['surface_8', 'surface_²', 'surface_٣']
    + suffixes('cldice', 16, '5', 'k', 5) + ['cldice_+5', 'cldice_5 ']
    + suffixes('potts', 7, '3', 'r', 3)
    + ['potts_rxd', 'potts_4x4', 'potts_5x4', 'potts_7x2', 'potts_3x4', 'potts_3x5', 'potts_3x0', 'potts_3x', 'potts_3x02',
       'potts_3x2', 'potts_2x2', 'potts_3X2', 'potts_3x2x1']
    + ['focal', 'Dice', 'dice_3', '', None, 5])

SUMS = [
    '0.5*bootstrapped_cross_entropy_30+dice', 'dice+0.5*cldice_5', 'dice+0.5*surface_64', 'cross_entropy+0.1*potts_3x2',
    '0.5*lovasz_hinge+boundary_f_4', 'lovasz_hinge+0.25*cross_entropy_and_boundary_f', '2*dice', '1*cldice',
    'boundary_f+cross_entropy_and_boundary_f_3',
    'bootstrapped_cross_entropy+bootstrapped_cross_entropy_30', 'boundary_f_3+boundary_f_4', 'surface+surface_8',
    'potts_3+potts_3x2', 'cldice+cldice_8', 'lovasz_hinge+lovasz_hinge_flat', 'dice+dice',
    '2*bootstrapped_cross_entropy_30+surface+potts_2x2+cldice_3', 'bootstrapped_cross_entropy_30+boundary_f_4+surface_64+cldice_5',
    'boundary_f+surface+potts+cldice', 'cross_entropy+dice+lovasz_hinge+surface_64+cldice_5',
    'dice+', '+dice', '0*dice', '1e-1*dice', 'dice + cldice', '0.5*focal+dice', 'dice+cldice_17', '.5*dice', '0.5**dice', '0.5*',
    'dice*0.5', '-1*dice']

KEYWORD_SETS = (
    [{}]
    + [{'fraction': v} for v in (0.3, 0.5, 1.5, 0.0, True, 2.5, NAN)]
    + [{'radius': v} for v in (4, 3, 17, 0, True, 2.5, NAN, 4.0)]
    + [{'cap': v} for v in (64, 8, 4096, 0, True, 2.5, NAN)]
    + [{'window': v} for v in (3, 2, 5, 8, 0, True, 2.5, NAN)]
    + [{'depth': v} for v in (5, 4, 17, 0, True, 2.5, NAN, INF)]
    # two bad keywords at once: which error wins is part of the behaviour
    + [{'fraction': 1.5, 'radius': 17}, {'radius': 17, 'cap': 4096}, {'cap': 0, 'window': 8}, {'window': 2.5, 'depth': 17},
       {'fraction': NAN, 'depth': True}, {'radius': 3, 'depth': 4}, {'fraction': 0.5, 'cap': 8}, {'radius': 2.5, 'window': 2},
       {'fraction': 0.5, 'window': 2}, {'cap': NAN, 'depth': 0}]
    + [{'fraction': 0.3, 'radius': 4, 'cap': 64, 'window': 3, 'depth': 5}, {'fraction': 0.3, 'cap': 64, 'window': 2, 'depth': 3}])

# the values the checks see; check_radius skips the infinities
CHECK_VALUES = [1, 2, 7, 8, 16, 17, 100, 4095, 4096, 65536, 0, -1, 0.25, 0.3, 0.5, 1.0, 1.5, 2.5, 4.0, 16.0, 1e-9, 7.6e-6, 0.999999999,
                True, False, NAN, INF, -INF, None, '3', 2 ** 70]
WINDOW_PAIRS = [(w, d) for w in (1, 3, 4, 5, 7, 8, 0, 2.0, 2.5, True, NAN, INF, None) for d in (None, 1, 2, 4, 5, 0, 2.0, 2.5, True, NAN, INF)]
SUFFIX_CALLS = [(n, bases, hi) for bases, hi in ((['ab', 'a'], 9), (['a', 'ab'], 9), (['ab'], 120), ([], 5))
                for n in ('a', 'ab', 'a_9', 'ab_9', 'ab_10', 'ab_120', 'a_b', 'abc', 'b', '', None, 3)]


NAME = '<the spelling>'      # stands for the row's own spelling inside a recorded outcome, so that equal outcomes are stored once


def plain(x, name=None):
    """A result as JSON keeps it: tuples as lists; with `name` (a non-empty string), NAME in its place inside every string."""
    if isinstance(x, (list, tuple)):
        return [plain(v, name) for v in x]
    if isinstance(x, str) and isinstance(name, str) and name:
        assert NAME not in x
        return x.replace(name, NAME)
    return x


def outcome(fn, *args, name=None, **kw):
    """['ok', the result] or ['err', the exception's type name, its exact message], the spelling `name` written as NAME."""
    try:
        return ['ok', plain(fn(*args, **kw), name)]
    except Exception as e:      # noqa: BLE001  (whatever is raised is the record)
        return ['err', type(e).__name__, plain(str(e), name)]


def spec_fields(name, fraction, radius, cap, window, depth):
    s = engine._resolve.__wrapped__(name, fraction, radius, cap, window, depth)
    return [s.n, list(s.kinds), [float(w) for w in s.weights], s.combine, s.fraction, s.radius, s.cap, s.window, s.depth]


def row(name, kw):
    """One (spelling, keywords) row through every surface, in SURFACES' order."""
    five = [kw.get(k) for k in KEYWORDS]
    return [outcome(spec_fields, name, *five, name=name),
            outcome(loss_sum.resolve, name, kw.get('fraction'), kw.get('radius'), per_image=False, name=name),
            outcome(loss_sum.resolve_cap, name, kw.get('cap'), name=name),
            outcome(loss_sum.resolve_window, name, kw.get('window'), name=name),
            outcome(loss_sum.resolve_depth, name, kw.get('depth'), name=name),
            outcome(loss_names.resolve_loss, name, *five, name=name)]


SURFACES = ['engine._resolve', 'loss_sum.resolve', 'loss_sum.resolve_cap', 'loss_sum.resolve_window', 'loss_sum.resolve_depth',
            'loss_names.resolve_loss']
PARSERS = ['parse_bootstrap', 'parse_boundary', 'parse_surface', 'parse_potts', 'parse_cldice']
CHECKS = ['check_fraction', 'q_of', 'check_radius', 'check_cap', 'check_window', 'check_depth']


def parses(name):
    """One spelling through every `parse_*` of `loss_names`, in PARSERS' order, and through `loss_sum.parse`."""
    return [outcome(getattr(loss_names, p), name, name=name) for p in PARSERS] + [outcome(loss_sum.parse, name, name=name)]


def checks(value):
    """One value through every check, in CHECKS' order; None where the pair is left out."""
    return [None if c == 'check_radius' and value in (INF, -INF) else outcome(getattr(loss_names, c), value) for c in CHECKS]


def record():
    """The whole table.  Equal things are stored once: `grid_of` gives each spelling its line of `grid`, a line holds one index
    into `rows` per keyword set, and a row one index into `outcomes` per surface."""
    outcomes, rows, lines, index = [], [], [], {}

    def cell(o, table=outcomes):
        key = (id(table), json.dumps(o, sort_keys=True))
        if key not in index:
            index[key] = len(table)
            table.append(o)
        return index[key]

    spellings = NAMES + SUMS
    return {
        'surfaces': SURFACES, 'parsers': PARSERS + ['loss_sum.parse'], 'checks': CHECKS,
        'spellings': spellings, 'keywords': KEYWORD_SETS,
        'grid_of': [cell([cell([cell(o) for o in row(name, kw)], rows) for kw in KEYWORD_SETS], lines) for name in spellings], 'grid': lines,
        'parse': [[cell(o) for o in parses(name)] for name in spellings],
        'check_values': CHECK_VALUES, 'check': [[o if o is None else cell(o) for o in checks(v)] for v in CHECK_VALUES],
        'window_pairs': WINDOW_PAIRS, 'check_window': [cell(outcome(loss_names.check_window, w, d)) for w, d in WINDOW_PAIRS],
        'suffix_calls': SUFFIX_CALLS, 'parse_suffix': [cell(outcome(loss_names.parse_suffix, *c)) for c in SUFFIX_CALLS],
        'outcomes': outcomes, 'rows': rows}


def text(table):
    """The table as compact JSON with sorted keys, one line per key and, in the long lists, per entry."""
    def compact(v):
        return json.dumps(v, sort_keys=True, separators=(',', ':'))
    lines = []
    for key in sorted(table):
        value = table[key]
        if key in ('grid', 'outcomes'):
            value = '[\n' + ',\n'.join(compact(v) for v in value) + '\n]'
        else:
            value = compact(value)
        lines.append(f'{compact(key)}:{value}')
    return '{\n' + ',\n'.join(lines) + '\n}\n'


if __name__ == '__main__':
    table = record()
    with open(OUT, 'w') as f:
        f.write(text(table))
    kinds = collections.Counter(o[1] if o[0] == 'err' else 'ok' for o in table['outcomes'])
    print(len(table['spellings']), 'spellings x', len(table['keywords']), 'keyword sets;', len(table['rows']), 'distinct rows,',
          len(table['outcomes']), 'distinct outcomes', dict(kinds), os.path.getsize(OUT), 'bytes')
