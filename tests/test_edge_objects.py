"""CPU: the object layer on the 'scipy' backend against what THE REFERENCE ITSELF returned on the cases of
tests/edge_cases.py, recorded by tests/golden/make_golden_edges.py into g32_edges_d{1..4}.json.gz (17 sets -- empty, open,
flat, infeasible, with bad rows, of more than 32 rows, with scaled rows, far from the origin -- singly and in every ordered
pair) and g33_objects.json.gz (40 random triples).  Every recorded key, one case per dimension and operation, no
difference, nobody excused: same pieces in the same order (rows 1e-9), same booleans, boxes and vertices, same exception
classes.  This is what lets tests/test_edge_objects_gpu.py read a difference on the 'hip' backend as one of the device
routing and not of the host flow.  The last test holds that file's table of excused keys to its cap."""
import logging
import warnings

import pytest

import edge_cases as E


@pytest.fixture(autouse=True)
def _quiet():
    logging.disable(logging.CRITICAL)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (inf - inf in sampled volumes and box comparisons of open sets, as in the reference)
        yield
    logging.disable(logging.NOTSET)


def _edge_params():
    return [(d, what) for d in E.EDGE_DIMS for what, _, _, _ in E.edge_cases(d)[1]]


_references = {}


def _reference(path):
    if path not in _references:
        _references[path] = E.Reference.replay(path)
    return _references[path]


@pytest.mark.parametrize("d,what", _edge_params(), ids=lambda v: str(v).replace(" ", ""))
def test_edge_sets_against_the_reference(d, what):
    import polytope_amd as pc
    reference = _reference(E.EDGE_FIXTURE % d)
    with E.backend("scipy"):
        n, diffs = E.edge_differences(reference, pc, d, only=what)
    print("d = %d %s: %d recorded outcomes, %d differences" % (d, what, n, len(diffs)))
    assert n == len([k for k in reference.keys() if k.startswith("%d %s " % (d, what))]) > 0   # every recorded key of the operation
    assert not diffs, "\n".join("%s: %s" % kv for kv in sorted(diffs.items()))


def test_random_triples_against_the_reference():
    import polytope_amd as pc
    reference = _reference(E.OBJECT_FIXTURE)
    assert reference.recorded_args == E.OBJECT_ARGS
    with E.backend("scipy"):
        n, diffs = E.object_differences(reference, pc, *map(int, E.OBJECT_ARGS))
    print("%d recorded outcomes, %d differences" % (n, len(diffs)))
    assert n == len(reference.keys())
    assert not diffs, "\n".join("%s: %s" % kv for kv in sorted(diffs.items()))


def _path(name):
    import test_edge_objects_gpu as G
    return E.EDGE_FIXTURE % int(name[-1]) if name.startswith("g32") else G.OBJECT_SETS[name][0]


def test_every_recorded_key_has_a_case_and_the_excused_are_few():
    """The cases here and in tests/test_edge_objects_gpu.py cover the fixtures key for key, and that file's table of excused
    keys stays within its cap: at most 0.5 % of a fixture and five per dimension -- a condition, not a measurement."""
    import test_edge_objects_gpu as G
    EXCUSED, OBJECT_SETS = G.EXCUSED, G.OBJECT_SETS
    for d in E.EDGE_DIMS:
        name = "g32_edges_d%d" % d
        keys = set(_reference(_path(name)).keys())
        assert keys == {E.edge_key(d, w, names) for w, _, _, operands in E.edge_cases(d)[1] for names in operands}
        assert set(EXCUSED[name]) <= keys and len(EXCUSED[name]) <= min(5, 0.005 * len(keys))
    for name, (_, args) in OBJECT_SETS.items():
        keys = set(_reference(_path(name)).keys())
        assert keys == {E.object_key(t, w) for t, d, _, _ in E.triples(*map(int, args)) for w, _, _ in E.object_ops(d)}
        assert set(EXCUSED[name]) <= keys and len(EXCUSED[name]) <= 0.005 * len(keys)
        per_d = {}
        for t, d, _, _ in E.triples(*map(int, args)):
            per_d[d] = per_d.get(d, 0) + sum(1 for k in EXCUSED[name] if k.split(" ", 1)[0] == str(t))
        assert all(v <= 5 for v in per_d.values())
    assert all(v[0] in ("T", "H") and (v[0] == "T" or callable(v[2])) for tab in EXCUSED.values() for v in tab.values())
