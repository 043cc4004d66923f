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

from .loss_names import FAMILIES, LOSS_KINDS, belongs, kind_of, resolve_knob

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


def _split(name):
    """A spelled sum -> [(weight, term name, kind id, the term's family or None), ...] in spelled order: `parse`, with what
    `loss_names.kind_of` found when it checked each term."""
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
            terms.append((w, term, *kind_of(term)))
        except (KeyError, NotImplementedError):
            raise bad from None
    return terms


def parse(name):
    """A spelled sum -> [(weight, term name), ...] in spelled order; a single name is the sum of one term of weight 1.  The
    weight is the fp32 value nearest to its literal, as a float.  The split happens before any term reaches `loss_names`; each
    term name is then checked by `loss_names.kind_of`.  Anything outside the grammar, an unknown term name and a bad suffix
    under a known prefix raise NotImplementedError like an unknown loss name."""
    return [(w, term) for w, term, _, _ in _split(name)]


def flat_spelling(name):
    """The spelling with every `lovasz_hinge` term as `lovasz_hinge_flat` (`per_image: False`), weights untouched."""
    pieces = []
    for piece in name.split('+'):
        weight, star, term = piece.rpartition('*')
        pieces.append(weight + star + ('lovasz_hinge_flat' if term == 'lovasz_hinge' else term))
    return '+'.join(pieces)


# `fraction` and `radius` are refused together before either is resolved, as `resolve` has always done; each later knob on its own
_ROUNDS = (FAMILIES[:2],) + tuple((family,) for family in FAMILIES[2:])


def resolve_terms(name, per_image=True, distinct=True, **given):
    """The one resolution of a spelled sum (or single name): split once, then for every family whose keyword is in `given`
    (`cap=None` asks for the cap the spelling carries) its one term's knob.  A keyword belongs to the one term of its family:
    without such a term, or against a disagreeing suffix, ValueError; two terms of one family (they share the engine's one
    value) are a ValueError too, and with `distinct` so is any kind named twice.  `per_image` False turns a `lovasz_hinge` term
    into `lovasz_hinge_flat`.  Returns (kinds, weights, term names, the knobs asked for in FAMILIES' order: what the name or the
    keyword carries; None: the engine's value stays)."""
    terms = [(w, 'lovasz_hinge_flat', LOSS_KINDS['lovasz_hinge_flat'], f) if t == 'lovasz_hinge' and not per_image else (w, t, k, f)
             for w, t, k, f in _split(name)]
    kinds = [k for _, _, k, _ in terms]
    if distinct and len(set(kinds)) != len(kinds):
        raise ValueError(f"loss_func='{name}' names a loss twice")
    mine = {family.keyword: [t for _, t, _, f in terms if f is family] for family in FAMILIES if family.keyword in given}
    knobs = {}
    for families in _ROUNDS:
        families = [family for family in families if family.keyword in given]
        for family in families:
            if len(mine[family.keyword]) > 1:
                raise ValueError(f"loss_func='{name}' holds both boundary kinds; they share the engine's one radius"
                                 if family.keyword == 'radius' else f"loss_func='{name}' names a loss twice")
        for family in families:
            if given[family.keyword] is not None and not mine[family.keyword]:
                raise belongs(family, f"{'neither is a' if len(family.kinds) > 1 else 'which is no'} term of '{name}'")
        for family in families:
            term = mine[family.keyword]
            knobs[family.keyword] = resolve_knob(family, term[0], given[family.keyword]) if term else None
    return kinds, [w for w, _, _, _ in terms], [t for _, t, _, _ in terms], list(knobs.values())


def resolve(name, fraction=None, radius=None, per_image=True):
    """`resolve_terms` for `fraction` and `radius` -> (kinds, weights, term names, fraction or None, radius or None)."""
    kinds, weights, names, knobs = resolve_terms(name, per_image, fraction=fraction, radius=radius)
    return kinds, weights, names, *knobs


def resolve_cap(name, cap=None):
    """The distance cap a spelled sum (or single name) carries, or None.  A `surface` term beside a boundary kind is allowed: the
    cap and the radius are separate."""
    return resolve_terms(name, distinct=False, cap=cap)[3][0]


def resolve_window(name, window=None):
    """The window a spelled sum (or single name) carries, as (radius or None, dilation or None), or None without a `potts` term."""
    return resolve_terms(name, distinct=False, window=window)[3][0]


def resolve_depth(name, depth=None):
    """The depth a spelled sum (or single name) carries, or None."""
    return resolve_terms(name, distinct=False, depth=depth)[3][0]


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
