"""Required nodeAffinity -> the tagged selector rows of one SEL | SELOP_TAGGED | sel_terms(T) call (include/ksched.h, extensions E9 / E10).

Kubernetes' requiredDuringSchedulingIgnoredDuringExecution is a list of nodeSelectorTerms that are ORed; a term is a list of
matchExpressions (key, operator, values) that are ANDed.  The device call takes T rows per pod, one row per term, one entry per key
(`tag << 29 | id`), and ORs the rows.  node_affinity_rows turns the expressions into those rows.  Pure numpy, no GPU, no library call.

What a row cannot say is reported, never hidden: a pod whose expansion needs more than `max_terms` rows, a NotIn of more than one value
that nodes carry, or two expressions of one term on the same key (a range, say) comes back in `overflow` with rows that match NO node,
so that it binds nowhere until the caller answers it with the combining calls (COMBINE_AND / COMBINE_OR / COMBINE_ANDNOT on further
tagged calls -- INTEGRATION.md has the recipes).  matchFields and preferred (weighted) terms are out of scope.
"""
from __future__ import annotations

from itertools import product
from typing import Iterable, Mapping, Optional, Sequence

import numpy as np

from . import _lib as L

OPERATORS = ("In", "NotIn", "Exists", "DoesNotExist", "Gt", "Lt")
_DEAD = object()  # an expression no node can satisfy: its term matches nothing


def _entry(tag: int, ident: int) -> int:
    return (tag << L.SELTAG_SHIFT) | ident


def _numeric_id(key: str, value) -> int:
    """id = value + 1 of a numeric key's value (0 stays "the node does not carry the key"); may be <= 0 for a negative value"""
    try:
        v = int(str(value).strip(), 10)
    except ValueError:
        raise ValueError(f"pod_terms: key {key!r} is numeric, value {value!r} is no integer") from None
    if v + 1 > L.SELTAG_ID_MASK:
        raise ValueError(f"pod_terms: key {key!r}, value {v}: id {v + 1} does not fit a tagged entry's 29 bits")
    return v + 1


def _ids(key: str, values, value_ids: Mapping, numeric: bool):
    """the ids of the values that a node can carry (an unknown value of an interned key, a negative value of a numeric one: dropped)"""
    out = []
    for v in values:
        if numeric:
            ident = _numeric_id(key, v)
            if ident >= 1:
                out.append(ident)
            continue
        ident = value_ids.get(key, {}).get(v)
        if ident is None or int(ident) == 0:
            continue
        if not 0 < int(ident) <= L.SELTAG_ID_MASK:
            raise ValueError(f"value_ids: key {key!r}, value {v!r}: id {ident} does not fit a tagged entry's 29 bits")
        out.append(int(ident))
    return sorted(set(out))


def _expression(key: str, op: str, values, known: bool, value_ids: Mapping, numeric: bool):
    """one matchExpression -> None (constrains nothing), _DEAD (matches no node), "overflow", or a list of alternative entries (an In
    with m values that nodes carry: m of them, one per expanded term; everything else: one)"""
    values = list(values or ())
    if op not in OPERATORS:
        raise ValueError(f"pod_terms: operator {op!r} (expected one of {', '.join(OPERATORS)})")
    if op in ("Gt", "Lt"):
        if not numeric:
            raise ValueError(f"pod_terms: {op} on key {key!r}, which is not one of numeric_keys (its ids are not ordered)")
        if len(values) != 1:
            raise ValueError(f"pod_terms: {op} on key {key!r} takes exactly one value, got {values!r}")
        ident = _numeric_id(key, values[0])
        if not known:
            return _DEAD
        if op == "Gt":  # a node carries a value >= 0: above a negative bound lies every node that carries the key
            return [_entry(L.SELTAG_GT, ident)] if ident >= 1 else [_entry(L.SELTAG_EXISTS, 0)]
        return [_entry(L.SELTAG_LT, ident)] if ident >= 1 else _DEAD
    if op == "Exists":
        return [_entry(L.SELTAG_EXISTS, 0)] if known else _DEAD
    if op == "DoesNotExist":
        return [_entry(L.SELTAG_ABSENT, 0)] if known else None
    ids = _ids(key, values, value_ids, numeric) if known else []
    if op == "In":
        return [_entry(L.SELTAG_EQ, i) for i in ids] if ids else _DEAD
    if not ids:  # NotIn of values no node carries
        return None
    return [_entry(L.SELTAG_NE, ids[0])] if len(ids) == 1 else "overflow"


def _pod_rows(terms, key_index: Mapping, value_ids: Mapping, numeric: set, max_terms: int):
    """a pod's rows: a list of {key column: entry}, [] = matches no node; None = overflow"""
    rows = []
    overflow = False
    for term in terms:
        term = list(term)
        if not term:  # Kubernetes: an empty term matches no objects
            continue
        alts, dead, unsayable = {}, False, False
        for key, op, values in term:
            got = _expression(key, op, values, key in key_index, value_ids, key in numeric)
            if got is None:
                continue
            if got is _DEAD:
                dead = True
                continue
            if got == "overflow" or key_index[key] in alts:
                unsayable = True
                continue
            alts[key_index[key]] = got
        if dead:  # (whatever else the term says: it is ANDed with an expression no node satisfies)
            continue
        size = 1
        for a in alts.values():
            size *= len(a)
        if unsayable or overflow or len(rows) + size > max_terms:
            overflow = True
            continue
        cols = sorted(alts)
        rows.extend(dict(zip(cols, combo)) for combo in product(*(alts[c] for c in cols)))
    return None if overflow else rows


def node_affinity_rows(pod_terms: Sequence[Optional[Iterable]], keys: Sequence[str], value_ids: Mapping[str, Mapping[str, int]],
                       numeric_keys: Iterable[str] = (), max_terms: int = L.MAX_TERMS):
    """(sel, T, overflow): sel a uint32 array [T][len(keys)][p] for `SEL | SELOP_TAGGED | sel_terms(T)`, overflow the sorted pod indices
    whose affinity the rows cannot say.

    pod_terms[i]: None (the pod has no required affinity: every node passes) or the pod's nodeSelectorTerms, a list of terms, each a list
    of (key, operator, values) with Kubernetes' operator names In, NotIn, Exists, DoesNotExist, Gt, Lt.  keys: the snapshot's label keys in
    column order.  value_ids[key][value]: the interned id (1 ... 2^29 - 1) of every value some node carries under an interned key.
    numeric_keys: the keys whose node ids are value + 1 (monotonic, 0 = absent); Gt and Lt apply to them only, and In / NotIn on them
    intern by the same map.

    * In {m values} expands its term into m terms (the product over the term's In expressions: DNF).  A value no node carries matches
      nothing under In (its expanded term is left out) and is dropped under NotIn.  A key that is no column of the snapshot is carried by
      no node: In, Exists, Gt and Lt on it match nothing, NotIn and DoesNotExist everything.
    * An empty list of terms and an empty term match no node (Kubernetes' rule); None matches every node (all zeros).
    * One row holds one entry per key: a NotIn of more than one carried value, and two expressions of one term on the same key, are
      OVERFLOW, as is a pod whose expansion exceeds max_terms rows, and -- with no label keys at all -- every pod that is not None.
      Overflow pods get rows that match NO node (SEL_NEVER) and are listed: handle them with the combining calls.  (With no label keys
      there is no entry to hold SEL_NEVER and the library passes every node to every pod: the list is then the only report.)
    * A pod with fewer than T rows is padded with rows that match nothing (SEL_NEVER in the first key).
    ValueError: an unknown operator, Gt / Lt on a key that is not numeric or without exactly one value, a non-integer value on a numeric
    key, an id at or above 2^29, max_terms outside 1 ... MAX_TERMS."""
    max_terms = int(max_terms)
    if not 1 <= max_terms <= L.MAX_TERMS:
        raise ValueError(f"max_terms: expected 1 ... {L.MAX_TERMS}, got {max_terms}")
    keys = list(keys)
    key_index = {k: i for i, k in enumerate(keys)}
    if len(key_index) != len(keys):
        raise ValueError("keys: a key occurs twice")
    numeric = set(numeric_keys)
    pods = [None if t is None else _pod_rows(list(t), key_index, value_ids, numeric, max_terms) for t in pod_terms]
    overflow = [i for i, t in enumerate(pod_terms) if t is not None and (pods[i] is None or not keys)]
    over = set(overflow)
    T = max([1] + [len(rows) for i, rows in enumerate(pods) if rows and i not in over])
    sel = np.zeros((T, len(keys), len(pods)), dtype=np.uint32)
    if keys:
        for i, rows in enumerate(pods):
            if pod_terms[i] is None:
                continue
            rows = [] if i in over else rows
            for t, row in enumerate(rows):
                for col, e in row.items():
                    sel[t, col, i] = e
            sel[len(rows):, 0, i] = L.SEL_NEVER
    return sel, T, overflow
