"""The spelling of one device loss, from its name to what the engine is told.  Host only and a leaf: importing this module needs
neither torch nor the built library, and nothing else of the package.

A loss is a name of LOSS_KINDS, or a base name of one FAMILIES row with an optional suffix.  A family is a loss (or two) with one
knob -- the bootstrap fraction, the boundary radius, the surface cap, the potts window, the cldice depth -- which the suffix or a
keyword of the same meaning carries.  Every step is written once and takes the row: `parse` splits a name, `check` makes a
keyword's value the number the library receives, `resolve_knob` joins the two, `resolve_name` does all of it for one name.  The
names callers know (`parse_boundary`, `check_cap`, `resolve_depth`, `SURFACE_KINDS`, ...) are bindings of these at the end of the file, and
`bootstrap.py`, `boundary.py`, `surface.py`, `potts.py`, `cldice.py` and `engine.py` re-export them; sums of names are
`loss_sum.py`.  A new loss with a knob is one more row here (and its keyword in the engine's signatures)."""
import collections
import functools
import math
import re

import numpy as np

BOOTSTRAP = 'bootstrapped_cross_entropy'
BOUNDARY_F = 'boundary_f'
BOUNDARY_COMBINED = 'cross_entropy_and_boundary_f'
SURFACE = 'surface'
POTTS = 'potts'
CLDICE = 'cldice'
# the kinds without a knob, and bootstrap's 6; the ids are include/eosvos.h's, where 7 and 11 stay unassigned.  The kinds from 8 on
# need the frame's shape or the frames and are in their FAMILIES rows only
LOSS_KINDS = {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2, 'class_balanced_cross_entropy': 3,
              'lovasz_hinge': 4, 'lovasz_hinge_flat': 5,      # these two: networks/loss_lovasz.py:78-111, per_image True / False
              BOOTSTRAP: 6}                                   # the hardest fraction of the pixels per image (bootstrap.py)
MAX_RADIUS, MAX_CAP, MAX_DEPTH = 16, 4095, 16
MAX_WINDOW, MAX_DILATION, MAX_HALO = 7, 4, 16      # the CRF's limits: radius, dilation, radius * dilation
_POTTS_SUFFIX = re.compile(r'_([1-9][0-9]*)(?:x([1-9][0-9]*))?\Z', re.ASCII)
_INF = float('inf')


def _integer(rest, hi):
    """What follows a base name, as the integer of `_<i>`, i in 1 .. hi without a leading zero; None for anything else."""
    digits = rest[1:]
    if rest[0] != '_' or not digits.isascii() or not digits.isdigit() or digits[0] == '0' or not 1 <= int(digits) <= hi:
        return None
    return int(digits)


def _percent(rest):
    """`_<P>`, P a whole percent 1 .. 100 -> the fraction P / 100."""
    percent = _integer(rest, 100)
    return None if percent is None else percent / 100.0


def _window(rest):
    """`_<r>` -> (r, None): the engine's dilation; `_<r>x<d>` -> (r, d).  r in 1 .. 7, d in 1 .. 4, r * d <= 16."""
    m = _POTTS_SUFFIX.match(rest)
    r, d = (int(m.group(1)), None if m.group(2) is None else int(m.group(2))) if m else (0, None)
    if not 1 <= r <= MAX_WINDOW or (d is not None and (not 1 <= d <= MAX_DILATION or r * d > MAX_HALO)):
        return None
    return r, d


def _whole(keyword, noun, hi, value):
    """A keyword's value as the int the library receives: a whole number 1 .. hi, as an int or a float."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or value != value or value in (_INF, -_INF) \
            or value != int(value) or not 1 <= int(value) <= hi:
        raise ValueError(f'{keyword}={value!r}: the {noun} must be a whole number in 1 .. {hi}')
    return int(value)


def check_fraction(fraction):
    """The fraction as the float the library receives: in (0, 1]."""
    f = float(np.float32(fraction))
    if not (0.0 < f <= 1.0) or not (0.0 < float(fraction) <= 1.0):
        raise ValueError(f'fraction={fraction!r}: the bootstrap fraction must be in (0, 1]')
    return f


def q_of(fraction):
    """round(fraction * 65536) of the fp32 fraction (halves away from zero), clamped to [1, 65536]."""
    return min(65536, max(1, int(math.floor(check_fraction(fraction) * 65536.0 + 0.5))))


def check_window(window, dilation=None):
    """The window radius (and with it the dilation) as the ints the library receives: whole numbers, 1 .. 7 and 1 .. 4, their
    product at most 16."""
    r = _whole('window', 'potts window radius', MAX_WINDOW, window)
    if dilation is None:
        return r
    d = _whole('dilation', 'potts dilation', MAX_DILATION, dilation)
    if r * d > MAX_HALO:
        raise ValueError(f'window={window!r}, dilation={dilation!r}: their product must be at most {MAX_HALO}')
    return r, d


def _join_window(name, carried, window):
    """The potts row's `join`: the keyword is the radius alone, and the dilation the name carries bounds it."""
    r, d = carried
    if r is not None and r != window:
        raise ValueError(f"loss_func='{name}' and window={window!r} disagree")
    if d is not None and window * d > MAX_HALO:
        raise ValueError(f"loss_func='{name}' and window={window!r}: radius * dilation must be at most {MAX_HALO}")
    return window, d


# One row per knob, in the order they are consulted.  keyword: the knob's name in every signature and in LossSpec.  kinds: its
# base names and kind ids.  suffix: what follows a base name -> the value it carries, None if it is no spelling of one.  check:
# a keyword's value -> the number the library receives, or ValueError.  setter: the Engine method (and, after `eosvos_`, the
# library's entry point) that applies it.  bare: what a base name without a suffix carries.  join: the row's own rule for a
# keyword beside a suffix, where "equal or they disagree" is not it.
Family = collections.namedtuple('Family', 'keyword kinds suffix check setter bare join', defaults=(None, None))
FAMILIES = (
    Family('fraction', {BOOTSTRAP: LOSS_KINDS[BOOTSTRAP]}, _percent, check_fraction, 'set_loss_bootstrap'),
    Family('radius', {BOUNDARY_F: 8, BOUNDARY_COMBINED: 9}, functools.partial(_integer, hi=MAX_RADIUS),
           functools.partial(_whole, 'radius', 'boundary radius', MAX_RADIUS), 'set_loss_boundary'),
    Family('cap', {SURFACE: 10}, functools.partial(_integer, hi=MAX_CAP),
           functools.partial(_whole, 'cap', 'surface cap', MAX_CAP), 'set_loss_surface'),
    Family('window', {POTTS: 12}, _window, check_window, 'set_loss_potts', bare=(None, None), join=_join_window),
    Family('depth', {CLDICE: 13}, functools.partial(_integer, hi=MAX_DEPTH),
           functools.partial(_whole, 'depth', 'cldice depth', MAX_DEPTH), 'set_loss_cldice'),
)
BY_KEYWORD = {family.keyword: family for family in FAMILIES}
KEYWORDS = tuple(BY_KEYWORD)      # fraction, radius, cap, window, depth


def _split(name, bases, suffix):
    """`parse` for any bases and suffix rule."""
    if isinstance(name, str):
        for base in bases:
            if name.startswith(base):
                rest = name[len(base):]
                value = suffix(rest) if rest else None
                if rest and value is None:
                    raise NotImplementedError(f"loss_func='{name}'")
                return base, value
    return name, None


def parse(family, name):
    """`<base>` -> (base, None); `<base><suffix>` -> (base, the value the suffix carries), for the first of the family's base
    names the name starts with.  A name under no base is returned as (name, None); anything else under a base raises
    NotImplementedError like an unknown loss name."""
    return _split(name, family.kinds, family.suffix)


def parse_suffix(name, bases, hi):
    """`parse` for any `bases`, the suffix an integer 1 .. hi."""
    return _split(name, bases, functools.partial(_integer, hi=hi))


def belongs(family, where):
    """The ValueError for a keyword whose family the spelling does not hold."""
    return ValueError(f"{family.keyword}= belongs to {' / '.join(repr(k) for k in family.kinds)}, {where}")


def resolve_knob(family, name, value=None):
    """What a spelled name and the family's keyword ask of the knob: the suffix carries a value, `value` is the keyword form, for
    this family's names only, and the two may not disagree.  None (for potts, in either place of the pair): the engine's current
    value stays.  A name of another family gives None, or ValueError with a keyword."""
    base, carried = parse(family, name)
    if base not in family.kinds:
        if value is not None:
            raise belongs(family, f"not to '{name}'")
        return None
    if carried is None:
        carried = family.bare
    if value is None:
        return carried if carried is None or family.join else family.check(carried)
    checked = family.check(value)
    if family.join:
        return family.join(name, carried, checked)
    if carried is not None and (q_of(carried) != q_of(checked) if family.keyword == 'fraction' else carried != checked):
        shown = value if family.keyword == 'fraction' else checked      # (a fraction as given: its fp32 form has digits nobody typed)
        raise ValueError(f"loss_func='{name}' and {family.keyword}={shown!r} disagree")
    return checked


def kind_of(name):
    """A spelled name -> (kind id, its family or None).  A bad suffix under a family's base name raises NotImplementedError, any
    other unknown name KeyError."""
    for family in FAMILIES:
        base = parse(family, name)[0]
        if base in family.kinds:
            return family.kinds[base], family
    return LOSS_KINDS[name], None


def resolve_name(name, fraction=None, radius=None, cap=None, window=None, depth=None):
    """A spelled name and the keyword forms -> (kind id, [fraction, radius, cap, window, depth] as `resolve_knob` gives them, in
    FAMILIES' order).  The keywords of the later families are refused first, in the table's order, then the name, then the
    fraction."""
    later = [resolve_knob(family, name, value) for family, value in zip(FAMILIES[1:], (radius, cap, window, depth))]
    return kind_of(name)[0], [resolve_knob(FAMILIES[0], name, fraction)] + later


def resolve_loss(name, fraction=None, radius=None, cap=None, window=None, depth=None):
    """`resolve_name` as (kind id, fraction or None)."""
    kind, knobs = resolve_name(name, fraction, radius, cap, window, depth)
    return kind, knobs[0]


def parse_potts(name):
    """`parse` of the potts row with the pair spread: (name, r or None, d or None)."""
    base, carried = parse(BY_KEYWORD['window'], name)
    return (base, *(carried or (None, None)))


parse_bootstrap, parse_boundary, parse_surface, parse_cldice = (
    functools.partial(parse, BY_KEYWORD[k]) for k in ('fraction', 'radius', 'cap', 'depth'))
check_radius, check_cap, check_depth = (BY_KEYWORD[k].check for k in ('radius', 'cap', 'depth'))
BOUNDARY_KINDS, SURFACE_KINDS, POTTS_KINDS, CLDICE_KINDS = (BY_KEYWORD[k].kinds for k in ('radius', 'cap', 'window', 'depth'))
resolve_radius, resolve_cap, resolve_window, resolve_depth = (
    functools.partial(resolve_knob, BY_KEYWORD[k]) for k in ('radius', 'cap', 'window', 'depth'))
