"""node_affinity_rows (kube_scheduler_rs_reference_amd/affinity.py) without a GPU: the rows it builds, run through tests/selterms_ref.py,
against a direct string-level evaluation of Kubernetes' rules on label dicts written HERE, independent of the helper -- every operator;
absent labels under NotIn / DoesNotExist / Gt; multi-value In; a DNF product; an empty list; an empty term; None; an unknown value; a key
the snapshot does not have; overflow (a NotIn of two carried values, two expressions on one key, more than max_terms rows), whose rows
match no node and whose pods are listed; the ValueErrors; and one small hand-written fixture, tests/golden/node_affinity_rows.json."""
import json
import os

import numpy as np
import pytest

from kube_scheduler_rs_reference_amd import MAX_TERMS, SEL_NEVER, node_affinity_rows
from tests import selterms_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_affinity_rows.json")


# ---- Kubernetes' rules, on strings -------------------------------------------------------------------------------------------------------
def expression_matches(labels, key, op, values):
    has = key in labels
    if op == "In":
        return has and labels[key] in values
    if op == "NotIn":
        return not has or labels[key] not in values
    if op == "Exists":
        return has
    if op == "DoesNotExist":
        return not has
    if not has:
        return False  # Gt / Lt on a missing label
    try:
        mine, bound = int(labels[key]), int(values[0])
    except ValueError:
        return False
    return mine > bound if op == "Gt" else mine < bound


def pod_matches(labels, terms):
    """required nodeAffinity: no affinity matches; else ANY term whose expressions ALL match; an empty term matches nothing"""
    if terms is None:
        return True
    return any(len(term) > 0 and all(expression_matches(labels, *e) for e in term) for term in terms)


def kubernetes(nodes, pods):
    return np.array([[pod_matches(labels, terms) for labels in nodes] for terms in pods], dtype=bool).reshape(len(pods), len(nodes))


# ---- the snapshot's side: keys, interned ids, label columns ---------------------------------------------------------------------------------
def intern(nodes, keys, numeric):
    value_ids = {k: {v: i + 1 for i, v in enumerate(sorted({n[k] for n in nodes if k in n}))} for k in keys if k not in numeric}
    lab = np.zeros((len(keys), len(nodes)), dtype=np.uint32)
    for j, n in enumerate(nodes):
        for i, k in enumerate(keys):
            if k in n:
                lab[i, j] = int(n[k]) + 1 if k in numeric else value_ids[k][n[k]]
    return value_ids, lab


def rows_bits(nodes, keys, numeric, pods, **kw):
    value_ids, lab = intern(nodes, keys, numeric)
    sel, T, overflow = node_affinity_rows(pods, keys, value_ids, numeric, **kw)
    assert sel.dtype == np.uint32 and sel.shape == (T, len(keys), len(pods)) and 1 <= T <= kw.get("max_terms", MAX_TERMS)
    assert overflow == sorted(overflow)
    return selterms_ref.pass_bits(lab, sel), sel, T, overflow


def test_the_golden_fixture():
    g = json.load(open(GOLDEN))
    pods = [p["terms"] for p in g["pods"]]
    bits, sel, T, overflow = rows_bits(g["nodes"], g["keys"], g["numeric_keys"], pods)
    assert overflow == g["overflow"] and T == g["terms"]
    as_text = lambda row: "".join("1" if b else "0" for b in row)  # noqa: E731
    assert [as_text(r) for r in bits] == [p["rows"] for p in g["pods"]]
    # the fixture's 'kubernetes' strings are this file's rules; they are the rows' answer for every pod that is not overflow
    assert [as_text(r) for r in kubernetes(g["nodes"], pods)] == [p["kubernetes"] for p in g["pods"]]
    for i, p in enumerate(g["pods"]):
        assert (p["rows"] == p["kubernetes"]) or i in overflow
    assert not sel[:, :, 0].any(), "a pod without affinity is all zeros"
    assert (sel[:, 0, 2] == SEL_NEVER).all() and (sel[:, 0, 8] == SEL_NEVER).all(), "an empty list and an overflow pod: NEVER in every term"


def cluster(rng, n):
    zones, disks = ["a", "b", "c", "d"], ["ssd", "hdd", "nvme"]
    nodes = []
    for _ in range(n):
        labels = {}
        if rng.random() < 0.85:
            labels["zone"] = zones[rng.integers(0, 3)]  # ("d" is a value no node carries)
        if rng.random() < 0.6:
            labels["disk"] = disks[rng.integers(0, 3)]
        if rng.random() < 0.5:
            labels["gpu"] = "true"
        if rng.random() < 0.8:
            labels["cores"] = str(int(rng.choice([0, 4, 8, 16, 17, 32, 64])))
        nodes.append(labels)
    return nodes


KEYS, NUMERIC = ["zone", "disk", "gpu", "cores"], ["cores"]


def random_expression(rng):
    key = KEYS[rng.integers(0, 4)]
    if key == "cores":
        op = ["In", "NotIn", "Exists", "DoesNotExist", "Gt", "Lt"][rng.integers(0, 6)]
        values = [str(int(v)) for v in rng.choice([-1, 0, 4, 8, 16, 17, 32, 64, 100], size=1 if op in ("Gt", "Lt", "NotIn") else rng.integers(1, 4), replace=False)]
    else:
        op = ["In", "NotIn", "Exists", "DoesNotExist"][rng.integers(0, 4)]
        pool = {"zone": ["a", "b", "c", "d"], "disk": ["ssd", "hdd", "nvme", "tape"], "gpu": ["true", "false"]}[key]
        values = [str(v) for v in rng.choice(pool, size=1 if op == "NotIn" else rng.integers(1, len(pool) + 1), replace=False)]
    return (key, op, [] if op in ("Exists", "DoesNotExist") else values)


def random_pod(rng):
    kind = rng.integers(0, 10)
    if kind == 0:
        return None
    if kind == 1:
        return []
    terms = []
    for _ in range(rng.integers(1, 4)):
        used, term = set(), []
        for _ in range(rng.integers(0, 4)):  # (0 expressions: an empty term)
            e = random_expression(rng)
            if e[0] not in used:  # (one expression per key and term: what a row can say)
                used.add(e[0])
                term.append(e)
        terms.append(term)
    return terms


def test_random_pods_against_the_rules_on_label_dicts():
    rng = np.random.default_rng(0xE10A)
    nodes = cluster(rng, 70)
    pods = [random_pod(rng) for _ in range(400)]
    want = kubernetes(nodes, pods)
    bits, sel, T, overflow = rows_bits(nodes, KEYS, NUMERIC, pods)
    assert overflow == [], "one expression per key, NotIn of one value, at most 3 terms of at most 3 x 4 values: everything fits"
    assert np.array_equal(bits, want), f"pods {np.nonzero((bits != want).any(axis=1))[0][:5]} differ from Kubernetes' rules"
    # what the cases tell apart: every operator occurs in a pod whose row is neither empty nor full; pods with every node, with none
    count = want.sum(axis=1)
    mixed = (count > 0) & (count < len(nodes))
    ops = {e[1] for i in np.nonzero(mixed)[0] for term in pods[i] for e in term}
    assert ops == {"In", "NotIn", "Exists", "DoesNotExist", "Gt", "Lt"}
    assert (count == 0).any() and (count == len(nodes)).any() and mixed.sum() > 100 and 2 <= T <= MAX_TERMS
    # rows that differ from every single term's row: the OR shows
    singles = [selterms_ref.pass_bits(intern(nodes, KEYS, NUMERIC)[1], sel[t:t + 1]) for t in range(T)]
    assert sum(all(not np.array_equal(bits[i], s[i]) for s in singles) for i in range(len(pods))) > 20


NODES = [{"zone": "a", "cores": "8"}, {"zone": "b", "cores": "16"}, {"zone": "c"}, {"cores": "32"}, {}]


def check(pods, keys=("zone", "cores"), numeric=("cores",), expect_overflow=(), **kw):
    bits, sel, T, overflow = rows_bits(NODES, list(keys), list(numeric), pods, **kw)
    want = kubernetes(NODES, pods)
    assert overflow == list(expect_overflow)
    for i in range(len(pods)):
        if i in overflow:
            assert not bits[i].any(), f"pod {i}: an overflow pod's rows match no node"
        else:
            assert np.array_equal(bits[i], want[i]), f"pod {i}: {bits[i].astype(int)} against {want[i].astype(int)}"
    return bits, sel, T


def test_every_operator_alone():
    bits, sel, T = check([[[("zone", "In", ["a"])]], [[("zone", "NotIn", ["a"])]], [[("zone", "Exists", [])]], [[("zone", "DoesNotExist", [])]],
                          [[("cores", "Gt", ["8"])]], [[("cores", "Lt", ["32"])]], [[("cores", "In", ["16"])]], [[("cores", "NotIn", ["16"])]]])
    assert T == 1
    assert bits.astype(int).tolist() == [[1, 0, 0, 0, 0], [0, 1, 1, 1, 1], [1, 1, 1, 0, 0], [0, 0, 0, 1, 1],
                                         [0, 1, 0, 1, 0], [1, 1, 0, 0, 0], [0, 1, 0, 0, 0], [1, 0, 1, 1, 1]]


def test_absent_labels_pass_notin_and_doesnotexist_and_fail_gt_and_lt():
    bits, _, _ = check([[[("cores", "NotIn", ["8"])]], [[("cores", "DoesNotExist", [])]], [[("cores", "Gt", ["0"])]], [[("cores", "Lt", ["1000"])]],
                        [[("cores", "Gt", ["-5"])]], [[("cores", "Lt", ["-5"])]], [[("cores", "Lt", ["0"])]]])
    assert bits[:, 2].astype(int).tolist() == [1, 1, 0, 0, 0, 0, 0] and bits[:, 4].astype(int).tolist() == [1, 1, 0, 0, 0, 0, 0]
    assert bits[4].astype(int).tolist() == [1, 1, 0, 1, 0], "above a negative bound lies every node that carries the key"


def test_multi_value_in_and_the_dnf_product():
    bits, sel, T = check([[[("zone", "In", ["a", "b", "c"])]],
                          [[("zone", "In", ["a", "b"]), ("cores", "In", ["8", "16", "32"])]],
                          [[("zone", "In", ["a", "b"]), ("cores", "Gt", ["8"])], [("zone", "DoesNotExist", [])]]])
    assert T == 6, "two zones times three core counts"
    assert bits.astype(int).tolist() == [[1, 1, 1, 0, 0], [1, 1, 0, 0, 0], [0, 1, 0, 1, 1]]
    assert ((sel[:, :, 0] != 0).any(axis=1)).sum() == 6 and (sel[3:, 0, 0] == SEL_NEVER).all(), "three rows, then NEVER padding"


def test_empty_list_empty_term_and_none():
    bits, sel, T = check([[], [[]], None, [[], [("zone", "In", ["b"])]], [[], []]])
    assert bits.any(axis=1).tolist() == [False, False, True, True, False] and bits[2].all()
    assert not sel[:, :, 2].any() and (sel[:, 0, 0] == SEL_NEVER).all()


def test_unknown_values_and_unknown_keys():
    check([[[("zone", "In", ["nowhere"])]], [[("zone", "In", ["a", "nowhere"])]], [[("zone", "NotIn", ["nowhere"])]], [[("zone", "NotIn", ["a", "nowhere"])]],
           [[("rack", "In", ["r1"])]], [[("rack", "NotIn", ["r1"]), ("zone", "In", ["c"])]], [[("rack", "Exists", [])]], [[("rack", "DoesNotExist", [])]],
           [[("zone", "In", [])]], [[("zone", "NotIn", [])]]])


def test_overflow_is_reported_and_binds_nowhere():
    many = [[("zone", "In", ["a", "b", "c"]), ("cores", "In", ["8", "16", "32"])], [("zone", "In", ["a", "b"]), ("cores", "In", ["8", "16", "32", "64"])]]  # 9 + 8 rows
    pods = [[[("zone", "NotIn", ["a", "b"])]],                                   # two NE entries on one key
            [[("cores", "Gt", ["4"]), ("cores", "Lt", ["32"])]],                 # a range: two expressions on one key
            many,                                                                # 17 rows
            [[("zone", "In", ["a"])]],                                           # fits
            [[("zone", "NotIn", ["a", "nowhere"])]],                             # one carried value: fits
            [[("zone", "In", ["nowhere"]), ("cores", "Gt", ["4"]), ("cores", "Lt", ["32"])], [("zone", "In", ["b"])]]]  # the unsayable term is dead anyway
    bits, sel, T = check(pods, expect_overflow=[0, 1, 2])
    assert T == 1, "overflow pods do not size the call"
    check(pods[2:3], expect_overflow=[0])
    bits, sel, T = check([[many[0]]], max_terms=9)
    assert T == 9
    check([[many[0]]], max_terms=8, expect_overflow=[0])
    # the true answers of the overflow pods are not empty: the caller must handle them
    assert kubernetes(NODES, pods[:3]).any(axis=1).all()
    # no label keys at all: only "no affinity" can be said, and there is no entry to hold NEVER -- the list is the only report
    sel, T, overflow = node_affinity_rows([None, [[("zone", "DoesNotExist", [])]], []], [], {})
    assert sel.shape == (1, 0, 3) and T == 1 and overflow == [1, 2]


def test_value_errors():
    ids = {"zone": {"a": 1, "big": 1 << 29}}
    for pods, match in (([[[("zone", "Near", ["a"])]]], "operator"),
                        ([[[("zone", "Gt", ["3"])]]], "numeric"),
                        ([[[("cores", "Gt", ["3", "4"])]]], "exactly one"),
                        ([[[("cores", "Gt", ["many"])]]], "no integer"),
                        ([[[("cores", "In", ["8", "x"])]]], "no integer"),
                        ([[[("cores", "Lt", [str((1 << 29) - 1)])]]], "29 bits"),
                        ([[[("zone", "In", ["big"])]]], "29 bits")):
        with pytest.raises(ValueError, match=match):
            node_affinity_rows(pods, ["zone", "cores"], ids, ["cores"])
    assert node_affinity_rows([[[("cores", "Lt", [str((1 << 29) - 2)])]]], ["zone", "cores"], ids, ["cores"])[2] == []
    for bad in (0, 16):
        with pytest.raises(ValueError, match="max_terms"):
            node_affinity_rows([None], ["zone"], ids, max_terms=bad)
    with pytest.raises(ValueError, match="keys"):
        node_affinity_rows([None], ["zone", "zone"], ids)
