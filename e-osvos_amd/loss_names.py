"""The spelling of one device loss: the name table, the `_<integer>` suffixes and what a name plus its keyword asks of the
engine.  Host only and a leaf: importing this module needs neither torch nor the built library, and nothing else of the
package.  `bootstrap.py`, `boundary.py` and `engine.py` re-export what callers know under their names; sums of names are
`loss_sum.py`."""
import math
import re

import numpy as np

LOSS_KINDS = {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2, 'class_balanced_cross_entropy': 3,
              'lovasz_hinge': 4, 'lovasz_hinge_flat': 5,      # these two: networks/loss_lovasz.py:78-111, per_image True / False
              'bootstrapped_cross_entropy': 6}                # the hardest fraction of the pixels per image (bootstrap.py)
BOOTSTRAP = 'bootstrapped_cross_entropy'
BOUNDARY_F = 'boundary_f'
BOUNDARY_COMBINED = 'cross_entropy_and_boundary_f'
# the kinds that need the frame's shape (include/eosvos.h; 7 stays unassigned)
BOUNDARY_KINDS = {BOUNDARY_F: 8, BOUNDARY_COMBINED: 9}
MAX_RADIUS = 16
SURFACE = 'surface'
# the distance-weighted surface loss (surface.py); it needs the frame's shape too.  A third table: the two above stay as they are
SURFACE_KINDS = {SURFACE: 10}
MAX_CAP = 4095
POTTS = 'potts'
# the image-aware pairwise loss (potts.py); it reads the frames of the last forward and no target.  A fourth table with id 12: the
# three above stay as they are, and 11 stays unassigned like 7
POTTS_KINDS = {POTTS: 12}
MAX_WINDOW, MAX_DILATION, MAX_HALO = 7, 4, 16      # the CRF's limits: radius, dilation, radius * dilation
CLDICE = 'cldice'
# the topology-aware centreline loss (cldice.py); it needs the frame's shape like the boundary kinds and `surface`.  A fifth table
# with id 13: the four above stay as they are, 7 and 11 stay unassigned and 14 is unknown
CLDICE_KINDS = {CLDICE: 13}
MAX_DEPTH = 16
_POTTS_SUFFIX = re.compile(r'_([1-9][0-9]*)(?:x([1-9][0-9]*))?\Z', re.ASCII)


def parse_suffix(name, bases, hi):
    """`<base>` -> (base, None); `<base>_<i>`, i an integer 1 .. hi without a leading zero -> (base, i), for the first of
    `bases` the name starts with.  A name under no base is returned as (name, None); anything else under a base raises
    NotImplementedError like an unknown loss name."""
    if isinstance(name, str):
        for base in bases:
            if name.startswith(base):
                rest = name[len(base):]
                if rest == '':
                    return base, None
                digits = rest[1:]
                if rest[0] != '_' or not digits.isascii() or not digits.isdigit() or digits[0] == '0' or not 1 <= int(digits) <= hi:
                    raise NotImplementedError(f"loss_func='{name}'")
                return base, int(digits)
    return name, None


def parse_bootstrap(name):
    """`bootstrapped_cross_entropy` -> (NAME, None): the engine's fraction; `bootstrapped_cross_entropy_<P>`, P an integer
    percent 1 .. 100 without a leading zero -> (NAME, P / 100).  A name that does not start with NAME is returned as
    (name, None); anything else under the prefix raises NotImplementedError like an unknown loss name."""
    base, percent = parse_suffix(name, (BOOTSTRAP,), 100)
    return base, (None if percent is None else percent / 100.0)


def parse_boundary(name):
    """`boundary_f` / `cross_entropy_and_boundary_f` -> (name, None): the engine's radius; with `_<r>`, r an integer 1 .. 16
    without a leading zero -> (base name, r).  A name under neither prefix is returned as (name, None); anything else under a
    prefix raises NotImplementedError like an unknown loss name."""
    return parse_suffix(name, (BOUNDARY_COMBINED, BOUNDARY_F), MAX_RADIUS)


def parse_surface(name):
    """`surface` -> (name, None): the engine's cap; `surface_<L>`, L an integer 1 .. 4095 without a leading zero -> (name, L).
    A name that does not start with `surface` is returned as (name, None); anything else under the prefix raises
    NotImplementedError like an unknown loss name."""
    return parse_suffix(name, (SURFACE,), MAX_CAP)


def parse_potts(name):
    """`potts` -> (name, None, None): the engine's window; `potts_<r>` -> (name, r, None): radius r, the engine's dilation;
    `potts_<r>x<d>` -> (name, r, d).  Integers without a leading zero, r in 1 .. 7, d in 1 .. 4, r * d <= 16.  A name that does
    not start with `potts` is returned as (name, None, None); anything else under the prefix raises NotImplementedError like
    an unknown loss name."""
    if not isinstance(name, str) or not name.startswith(POTTS):
        return name, None, None
    if name == POTTS:
        return POTTS, None, None
    m = _POTTS_SUFFIX.match(name[len(POTTS):])
    r, d = (int(m.group(1)), None if m.group(2) is None else int(m.group(2))) if m else (0, None)
    if not 1 <= r <= MAX_WINDOW or (d is not None and (not 1 <= d <= MAX_DILATION or r * d > MAX_HALO)):
        raise NotImplementedError(f"loss_func='{name}'")
    return POTTS, r, d


def parse_cldice(name):
    """`cldice` -> (name, None): the engine's depth; `cldice_<k>`, k an integer 1 .. 16 without a leading zero -> (name, k).  A
    name that does not start with `cldice` is returned as (name, None); anything else under the prefix raises
    NotImplementedError like an unknown loss name."""
    return parse_suffix(name, (CLDICE,), MAX_DEPTH)


def check_fraction(fraction):
    """The fraction as the float the library receives: in (0, 1]."""
    f = float(np.float32(fraction))
    if not (0.0 < f <= 1.0) or not (0.0 < float(fraction) <= 1.0):
        raise ValueError(f'fraction={fraction!r}: the bootstrap fraction must be in (0, 1]')
    return f


def q_of(fraction):
    """round(fraction * 65536) of the fp32 fraction (halves away from zero), clamped to [1, 65536]."""
    return min(65536, max(1, int(math.floor(check_fraction(fraction) * 65536.0 + 0.5))))


def check_radius(radius):
    """The radius as the int the library receives: a whole number 1 .. 16."""
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or radius != radius or radius != int(radius) \
            or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f'radius={radius!r}: the boundary radius must be a whole number in 1 .. {MAX_RADIUS}')
    return int(radius)


def check_cap(cap):
    """The cap as the int the library receives: a whole number 1 .. 4095."""
    if isinstance(cap, bool) or not isinstance(cap, (int, float)) or not math.isfinite(cap) or cap != int(cap) \
            or not 1 <= int(cap) <= MAX_CAP:
        raise ValueError(f'cap={cap!r}: the surface cap must be a whole number in 1 .. {MAX_CAP}')
    return int(cap)


def check_window(window, dilation=None):
    """The window radius (and with it the dilation) as the ints the library receives: whole numbers, 1 .. 7 and 1 .. 4, their
    product at most 16."""
    def whole(v, lo, hi):
        return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v) and v == int(v) and lo <= int(v) <= hi
    if not whole(window, 1, MAX_WINDOW):
        raise ValueError(f'window={window!r}: the potts window radius must be a whole number in 1 .. {MAX_WINDOW}')
    if dilation is None:
        return int(window)
    if not whole(dilation, 1, MAX_DILATION):
        raise ValueError(f'dilation={dilation!r}: the potts dilation must be a whole number in 1 .. {MAX_DILATION}')
    if int(window) * int(dilation) > MAX_HALO:
        raise ValueError(f'window={window!r}, dilation={dilation!r}: their product must be at most {MAX_HALO}')
    return int(window), int(dilation)


def check_depth(depth):
    """The depth (the number of erosions of the soft skeleton) as the int the library receives: a whole number 1 .. 16."""
    if isinstance(depth, bool) or not isinstance(depth, (int, float)) or not math.isfinite(depth) or depth != int(depth) \
            or not 1 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f'depth={depth!r}: the cldice depth must be a whole number in 1 .. {MAX_DEPTH}')
    return int(depth)


def resolve_loss(name, fraction=None, radius=None, cap=None, window=None, depth=None):
    """A spelled loss name -> (kind id, fraction or None).  `bootstrapped_cross_entropy_<P>` carries P percent; `fraction`
    is the keyword form, for that kind only; the two may not disagree.  None: the engine's current fraction stays.  A bad
    spelling under the bootstrap prefix raises NotImplementedError, any other unknown name KeyError.  The kinds that need the
    frame's shape (BOUNDARY_KINDS) are consulted after LOSS_KINDS and give (kind id, None); their radius, from the name
    or `radius=`, is `resolve_radius`'s, which this call checks too.  SURFACE_KINDS is consulted last, in the same way, its cap
    (`resolve_cap`) checked here too.  POTTS_KINDS comes after it, its window (`resolve_window`) checked here too, and
    CLDICE_KINDS after that with its depth (`resolve_depth`)."""
    radius = resolve_radius(name, radius)
    cap = resolve_cap(name, cap)
    window = resolve_window(name, window)
    depth = resolve_depth(name, depth)
    base, f = parse_bootstrap(name)
    if base not in LOSS_KINDS and parse_boundary(name)[0] in BOUNDARY_KINDS:
        if fraction is not None:
            raise ValueError(f"fraction= belongs to '{BOOTSTRAP}', not to '{name}'")
        return BOUNDARY_KINDS[parse_boundary(name)[0]], None
    if base not in LOSS_KINDS and parse_surface(name)[0] in SURFACE_KINDS:
        if fraction is not None:
            raise ValueError(f"fraction= belongs to '{BOOTSTRAP}', not to '{name}'")
        return SURFACE_KINDS[parse_surface(name)[0]], None
    if base not in LOSS_KINDS and parse_potts(name)[0] in POTTS_KINDS:
        if fraction is not None:
            raise ValueError(f"fraction= belongs to '{BOOTSTRAP}', not to '{name}'")
        return POTTS_KINDS[POTTS], None
    if base not in LOSS_KINDS and parse_cldice(name)[0] in CLDICE_KINDS:
        if fraction is not None:
            raise ValueError(f"fraction= belongs to '{BOOTSTRAP}', not to '{name}'")
        return CLDICE_KINDS[CLDICE], None
    kind = LOSS_KINDS[base]
    if fraction is not None:
        if base != BOOTSTRAP:
            raise ValueError(f"fraction= belongs to '{BOOTSTRAP}', not to '{name}'")
        if f is not None and q_of(f) != q_of(fraction):
            raise ValueError(f"loss_func='{name}' and fraction={fraction!r} disagree")
        f = fraction
    return kind, (None if f is None else check_fraction(f))


def resolve_radius(name, radius=None):
    """The window radius a spelled loss name asks for: `boundary_f_<r>` / `cross_entropy_and_boundary_f_<r>` carry r,
    `radius` is the keyword form, for those kinds only; the two may not disagree.  None: the engine's current radius stays."""
    base, r = parse_boundary(name)
    if radius is not None:
        if base not in BOUNDARY_KINDS:
            raise ValueError(f"radius= belongs to {' / '.join(repr(k) for k in BOUNDARY_KINDS)}, not to '{name}'")
        radius = check_radius(radius)
        if r is not None and r != radius:
            raise ValueError(f"loss_func='{name}' and radius={radius!r} disagree")
        r = radius
    return r


def resolve_cap(name, cap=None):
    """The distance cap a spelled loss name asks for: `surface_<L>` carries L, `cap` is the keyword form, for that kind only; the
    two may not disagree.  None: the engine's current cap stays."""
    base, c = parse_surface(name)
    if cap is not None:
        if base not in SURFACE_KINDS:
            raise ValueError(f"cap= belongs to '{SURFACE}', not to '{name}'")
        cap = check_cap(cap)
        if c is not None and c != cap:
            raise ValueError(f"loss_func='{name}' and cap={cap!r} disagree")
        c = cap
    return c


def resolve_window(name, window=None):
    """The window a spelled loss name asks for, as (radius or None, dilation or None), or None for a name that is no `potts`:
    `potts_<r>` / `potts_<r>x<d>` carry r (and d), `window` is the keyword form of r, for that kind only; the two may not
    disagree.  None in a place: the engine's current value stays."""
    base, r, d = parse_potts(name)
    if base not in POTTS_KINDS:
        if window is not None:
            raise ValueError(f"window= belongs to '{POTTS}', not to '{name}'")
        return None
    if window is not None:
        window = check_window(window)
        if r is not None and r != window:
            raise ValueError(f"loss_func='{name}' and window={window!r} disagree")
        if d is not None and window * d > MAX_HALO:
            raise ValueError(f"loss_func='{name}' and window={window!r}: radius * dilation must be at most {MAX_HALO}")
        r = window
    return r, d


def resolve_depth(name, depth=None):
    """The depth a spelled loss name asks for: `cldice_<k>` carries k, `depth` is the keyword form, for that kind only; the two
    may not disagree.  None: the engine's current depth stays."""
    base, k = parse_cldice(name)
    if depth is not None:
        if base not in CLDICE_KINDS:
            raise ValueError(f"depth= belongs to '{CLDICE}', not to '{name}'")
        depth = check_depth(depth)
        if k is not None and k != depth:
            raise ValueError(f"loss_func='{name}' and depth={depth!r} disagree")
        k = depth
    return k
