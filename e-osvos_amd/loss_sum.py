"""Weighted sums of the device losses, `loss_func: 0.5*lovasz_hinge+boundary_f_4`: the spelling, the checks, and the numpy
twin of the combine launch (`loss_sum_kernel` of `csrc/misc_kernels.hip`, the rule of `include/eosvos.h` at
eosvos_set_loss_sum).  Host only; importing this module needs neither torch nor the built library.

    loss_func := term ('+' term)*          at most MAX_TERMS terms, no blanks
    term      := [weight '*'] name         name: any single spelling `compute_loss` accepts, suffixes included
    weight    := digits ['.' digits]       a plain decimal, no sign, no exponent, > 0; absent = 1

A name with neither '+' nor '*' is not a sum: `resolve` takes it as one term of weight 1, and the engine evaluates it by
that kind's own launches, without the combine launch.  With L_i / d_i the loss and the
gradient term i gives alone and w_i its weight as fp32, the sum is
    acc = w_0 * x_0;  acc = acc + w_i * x_i  (i = 1 .. n-1)         x = the loss value, and per element the gradient
every product and every sum an fp32 operation rounded on its own, never a fused multiply-add, so `combine_host` reproduces
the device bit for bit.  The weights are untuned: no J&F figure exists for any sum."""
import re
from fractions import Fraction

import numpy as np

from .loss_names import (BOOTSTRAP, BOUNDARY_KINDS, CLDICE, CLDICE_KINDS, POTTS, POTTS_KINDS, SURFACE, SURFACE_KINDS, parse_boundary,
                         parse_bootstrap, parse_cldice, parse_potts, parse_surface, resolve_loss, resolve_radius)
from .loss_names import resolve_depth as _term_depth
from .loss_names import resolve_cap as _term_cap
from .loss_names import resolve_window as _term_window

MAX_TERMS = 4                           # EOSVOS_LOSS_MAX_TERMS of include/eosvos.h
_WEIGHT = re.compile(r'[0-9]+(\.[0-9]+)?\Z')


def is_sum(name):
    """Whether a `loss_func` is spelled as a sum: it holds a '+' or a '*'."""
    return isinstance(name, str) and ('+' in name or '*' in name)


def _weight(literal):
    """The fp32 value nearest to a decimal literal, as a float; None unless it is finite and > 0."""
    exact = Fraction(literal)
    with np.errstate(over='ignore'):
        best = np.float32(float(literal))
    if not np.isfinite(best):
        return None
    for other in (np.nextafter(best, np.float32(0)), np.nextafter(best, np.float32(np.inf))):      # (the way through a double
        if np.isfinite(other) and abs(Fraction(float(other)) - exact) < abs(Fraction(float(best)) - exact):   # may round twice)
            best = other
    return float(best) if best > 0 else None


def parse(name):
    """A spelled sum -> [(weight, term name), ...] in spelled order; a single name is the sum of one term of weight 1.  The
    weight is the fp32 value nearest to its literal, as a float.  The split happens before any term reaches `bootstrap.parse`
    / `boundary.parse`; each term name is then checked by `loss_names.resolve_loss`.  Anything outside the grammar, an unknown
    term name and a bad suffix under a known prefix raise NotImplementedError like an unknown loss name."""
    bad = NotImplementedError(f"loss_func='{name}'")
    if not isinstance(name, str) or name == '' or any(c.isspace() for c in name):
        raise bad
    pieces = name.split('+')
    if len(pieces) > MAX_TERMS:
        raise bad
    terms = []
    for piece in pieces:
        weight, star, term = piece.rpartition('*')
        w = 1.0
        if star:
            w = _weight(weight) if _WEIGHT.match(weight) else None
        if w is None or term == '' or '*' in weight:
            raise bad
        try:
            resolve_loss(term)
        except (KeyError, NotImplementedError):
            raise bad from None
        terms.append((w, term))
    return terms


def flat_spelling(name):
    """The spelling with every `lovasz_hinge` term as `lovasz_hinge_flat` (`per_image: False`), weights untouched."""
    pieces = []
    for piece in name.split('+'):
        weight, star, term = piece.rpartition('*')
        pieces.append(weight + star + ('lovasz_hinge_flat' if term == 'lovasz_hinge' else term))
    return '+'.join(pieces)


def resolve(name, fraction=None, radius=None, per_image=True):
    """A spelled sum with the keyword forms -> (kinds, weights, term names, fraction or None, radius or None).  `fraction` /
    `radius` belong to the one term of their family: without such a term, or against a disagreeing suffix, ValueError.  The
    returned fraction / radius are what the name or the keyword carries (None: the engine's current value stays).  `per_image`
    False turns a `lovasz_hinge` term into `lovasz_hinge_flat`.  The same kind twice, or both boundary kinds (they share the
    engine's one radius), is a ValueError."""
    terms = [(w, 'lovasz_hinge_flat' if t == 'lovasz_hinge' and not per_image else t) for w, t in parse(name)]
    names = [t for _, t in terms]
    kinds = [resolve_loss(t)[0] for t in names]
    if len(set(kinds)) != len(kinds):
        raise ValueError(f"loss_func='{name}' names a loss twice")
    boundary_terms = [t for t in names if parse_boundary(t)[0] in BOUNDARY_KINDS]
    if len(boundary_terms) > 1:
        raise ValueError(f"loss_func='{name}' holds both boundary kinds; they share the engine's one radius")
    bootstrap_terms = [t for t in names if parse_bootstrap(t)[0] == BOOTSTRAP]
    if fraction is not None and not bootstrap_terms:
        raise ValueError(f"fraction= belongs to '{BOOTSTRAP}', which is no term of '{name}'")
    if radius is not None and not boundary_terms:
        raise ValueError(f"radius= belongs to {' / '.join(repr(k) for k in BOUNDARY_KINDS)}, neither is a term of '{name}'")
    f = resolve_loss(bootstrap_terms[0], fraction)[1] if bootstrap_terms else None
    r = resolve_radius(boundary_terms[0], radius) if boundary_terms else None
    return kinds, [w for w, _ in terms], names, f, r


def resolve_cap(name, cap=None):
    """The distance cap a spelled sum (or single name) carries, or None: `cap` belongs to the one `surface` term, as `fraction`
    and `radius` belong to theirs in `resolve`: without such a term, or against a disagreeing suffix, ValueError; the term named
    twice is a ValueError too.  A `surface` term beside a boundary kind is allowed: the cap and the radius are separate."""
    surface_terms = [t for _, t in parse(name) if parse_surface(t)[0] in SURFACE_KINDS]
    if len(surface_terms) > 1:
        raise ValueError(f"loss_func='{name}' names a loss twice")
    if cap is not None and not surface_terms:
        raise ValueError(f"cap= belongs to '{SURFACE}', which is no term of '{name}'")
    return _term_cap(surface_terms[0], cap) if surface_terms else None


def resolve_window(name, window=None):
    """The window a spelled sum (or single name) carries, as (radius or None, dilation or None), or None without a `potts`
    term: `window` belongs to the one `potts` term as `cap` belongs to `surface` in `resolve_cap`: without such a term, or
    against a disagreeing suffix, ValueError; two `potts` terms (they share the engine's one window) are a ValueError too."""
    potts_terms = [t for _, t in parse(name) if parse_potts(t)[0] in POTTS_KINDS]
    if len(potts_terms) > 1:
        raise ValueError(f"loss_func='{name}' names a loss twice")
    if window is not None and not potts_terms:
        raise ValueError(f"window= belongs to '{POTTS}', which is no term of '{name}'")
    return _term_window(potts_terms[0], window) if potts_terms else None


def resolve_depth(name, depth=None):
    """The depth a spelled sum (or single name) carries, or None: `depth` belongs to the one `cldice` term as `cap` belongs to
    `surface` in `resolve_cap`: without such a term, or against a disagreeing suffix, ValueError; two `cldice` terms (they share
    the engine's one depth) are a ValueError too."""
    cldice_terms = [t for _, t in parse(name) if parse_cldice(t)[0] in CLDICE_KINDS]
    if len(cldice_terms) > 1:
        raise ValueError(f"loss_func='{name}' names a loss twice")
    if depth is not None and not cldice_terms:
        raise ValueError(f"depth= belongs to '{CLDICE}', which is no term of '{name}'")
    return _term_depth(cldice_terms[0], depth) if cldice_terms else None


def combine_host(values, grads, weights):
    """The numpy twin of the combine launch: `values` the terms' loss values, `grads` their gradients (arrays of one shape, or
    None), `weights` their weights -> (loss, gradient or None) as float32, each product and each sum rounded to fp32 on its
    own, in the terms' order."""
    assert 1 <= len(weights) <= MAX_TERMS and len(values) == len(weights)
    w = [np.float32(x) for x in weights]
    with np.errstate(all='ignore'):
        loss = w[0] * np.float32(values[0])
        for i in range(1, len(w)):
            loss = np.float32(loss + np.float32(w[i] * np.float32(values[i])))
        if grads is None:
            return np.float32(loss), None
        assert len(grads) == len(w)
        g = [np.ascontiguousarray(x, dtype=np.float32) for x in grads]
        acc = w[0] * g[0]
        for i in range(1, len(w)):
            acc = acc + w[i] * g[i]
    return np.float32(loss), acc.astype(np.float32, copy=False)
