"""GPU: region_diff_batch (rdiff_batch_kernel, one whole search per wavefront) against the single search
batch.region_diff_search and the single call polytope.region_diff, on the random overlapping boxes of
test_region_diff_library_search_equals_host_loop: leaves problem by problem at batch sizes 1, 3 and 67, the public call
piece for piece, poison in everything the kernel must not read, every status beside healthy neighbours, the fallback of
a problem beyond the caps, and the caller's stream."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rdiff_batch_host as RB  # noqa: E402
import rdiff_host as RH  # noqa: E402

pytestmark = pytest.mark.gpu

N_TRIALS = 24
ABS_TOL = 1e-7


class Case(object):
    pass


def _pieces(D):
    import polytope_amd.polytope as pcm
    ps = list(D.list_poly) if isinstance(D, pcm.Region) else ([] if D.A.size == 0 else [D])
    return [(q.A.copy(), q.b.copy()) for q in ps]


def _same_pieces(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, ((A0, b0), (A1, b1)) in enumerate(zip(got, want)):
        assert A0.shape == A1.shape and RB.hb.same_bits(A0, A1) and RB.hb.same_bits(b0, b1), (what, k)


def _unit(A, b):
    scale = 1 / np.sqrt(np.sum(A * A, 1)).flatten()
    return A * scale[:, None], b * scale


@pytest.fixture(scope="module")
def hip():
    from polytope_amd import solvers
    old, solvers.default_solver = solvers.default_solver, "hip"
    yield
    solvers.default_solver = old


@pytest.fixture(scope="module")
def ref(hip, tmp_path_factory):
    """The 24 cases once: what region_diff prepares for each (the radii of the stacks, the order, the table and its unit
    rows), the leaves of batch.region_diff_search on that table, the number of radii the library search reads (its host
    build without speculation, the radii from cheby_ball_batch), and per dimension the cases packed ragged: minuends of
    3d rows padded to 3d + 3, boxes of 2d rows padded to 2d + 2, one shared cell table."""
    import polytope_amd.polytope as pcm
    from polytope_amd import batch
    L = RH.build(tmp_path_factory.mktemp("rdiff_host_gpu"))
    cases = []
    for trial, (P, cells) in enumerate(RH.random_cases(N_TRIALS)):
        c = Case()
        c.trial, c.P, c.cells, c.d = trial, P.copy(), [q.copy() for q in cells], P.A.shape[1]
        c.Rc = np.array(pcm._radii_stacked(c.P, c.cells), dtype=float)
        c.order = np.argsort(-c.Rc)[:int(np.sum(c.Rc >= ABS_TOL))]
        A, B, mi = RB.numpy_table(c.P.A, c.P.b, [(c.cells[k].A, c.cells[k].b) for k in c.order], ABS_TOL)
        c.m, c.mi = c.P.A.shape[0], mi
        c.An, c.Bn = _unit(A, B)
        assert np.all(mi > 0)
        try:
            leaves, _ = batch.region_diff_search(c.An, c.Bn, c.m, mi, ABS_TOL)
            c.leaves = [(k, tuple(int(v) for v in r)) for k, r in leaves]
        except ValueError as e:
            assert "out of range" in str(e)
            c.leaves = "IndexError"

        def radii_of(lists, c=c):
            lens = np.array([len(w) for w in lists], dtype=np.int32)
            A3, b3 = np.zeros((len(lists), int(lens.max()), c.d)), np.zeros((len(lists), int(lens.max())))
            for t, w in enumerate(lists):
                A3[t, :lens[t]], b3[t, :lens[t]] = c.An[list(w)], c.Bn[list(w)]
            out = batch.cheby_ball_batch(A3, b3, m=lens)
            return [(float(r) if r >= 0 else 0.0) if st == 0 else float("nan") for r, st in zip(out["r"], out["status"])]
        lib = RH.search(L, c.m, mi, ABS_TOL, radii_of, knobs=RH.NO_SPECULATION)
        assert (lib.code == RH.BAD_INDEX) == (c.leaves == "IndexError") and (c.leaves == "IndexError" or lib.leaves == c.leaves)
        c.n_requests = lib.n_requests
        cases.append(c)
    packs = {}
    for d in (2, 3, 4):
        mine = [c for c in cases if c.d == d]
        assert len(mine) == 8 and all(c.m == 3 * d for c in mine)
        K = Case()
        K.cases, K.d, K.m_max, K.mc_max = mine, d, 3 * d + 3, 2 * d + 2
        K.first, table = [], []
        for c in mine:
            K.first.append(len(table))
            table.extend(_unit(q.A, q.b) for q in c.cells)
        K.Nc = len(table)
        K.CA, K.Cb, K.mc = np.zeros((K.Nc, K.mc_max, d)), np.zeros((K.Nc, K.mc_max)), np.zeros(K.Nc, np.int32)
        for k, (cA, cb) in enumerate(table):
            K.mc[k] = cA.shape[0]
            K.CA[k, :K.mc[k]], K.Cb[k, :K.mc[k]] = cA, cb
        packs[d] = K
    R = Case()
    R.cases, R.packs = cases, packs
    return R


def _batch_of(K, which, lists=None):
    """The problems `which` (indices into K.cases) -> A, b, m, cell_off, cell_idx over K's cell table."""
    B = len(which)
    A, b, m = np.zeros((B, K.m_max, K.d)), np.zeros((B, K.m_max)), np.zeros(B, np.int32)
    off, idx = [0], []
    for p, i in enumerate(which):
        c = K.cases[i]
        m[p] = c.m
        A[p, :c.m], b[p, :c.m] = c.An[:c.m], c.Bn[:c.m]
        idx.extend(K.first[i] + (c.order if lists is None else lists[p]))
        off.append(len(idx))
    return A, b, m, np.asarray(off, np.int32), np.asarray(idx, np.int32)


def _leaves(res, p):
    from polytope_amd import batch
    return [(k, tuple(int(v) for v in r)) for k, r in batch.region_diff_leaves(res, p)]


def _check_problem(res, p, c):
    assert list(res["mi"][p][:len(c.mi)]) == list(c.mi), c.trial
    if c.leaves == "IndexError":
        assert res["status"][p] == RB.RD_INDEX, c.trial
        return
    assert res["status"][p] == RB.RD_OK, (c.trial, int(res["status"][p]))
    assert _leaves(res, p) == c.leaves, c.trial
    assert res["count"][p] == len(c.leaves) and res["nrows"][p] == sum(len(r) for _, r in c.leaves)
    assert res["nlp"][p] >= c.n_requests, (c.trial, int(res["nlp"][p]), c.n_requests)


@pytest.mark.parametrize("size", [1, 3, 67])
@pytest.mark.parametrize("d", [2, 3, 4])
def test_leaves_equal_the_single_search(ref, d, size):
    """Case 1: region_diff_search_batch against batch.region_diff_search, problem by problem; one batch per dimension."""
    from polytope_amd import batch
    K = ref.packs[d]
    which = [(i + (size == 1) * 3) % 8 for i in range(size)]
    A, b, m, off, idx = _batch_of(K, which)
    res = batch.region_diff_search_batch(A, b, m, K.CA, K.Cb, K.mc, off, idx, ABS_TOL)
    for p, i in enumerate(which):
        _check_problem(res, p, K.cases[i])
    # src: new row k of a problem is row src % mc_max of cell src // mc_max of the table
    c = K.cases[which[0]]
    for k in range(int(c.mi.sum())):
        s = int(res["src"][0][k])
        assert RB.hb.same_bits(K.CA[s // K.mc_max, s % K.mc_max], c.An[c.m + k]) and K.Cb[s // K.mc_max, s % K.mc_max] == c.Bn[c.m + k]


def _public_against_single(polys, regs, regs_k, what):
    import polytope_amd
    import polytope_amd.polytope as pcm
    info = {}
    got = polytope_amd.region_diff_batch(polys, regs, _info=info)   # (none of cases 0-11 ends with an IndexError)
    assert len(got) == len(polys) and all(s == RB.RD_OK for s in info["status"]), info["status"]
    pieces = 0
    for k, (p, r) in enumerate(zip(polys, regs_k)):
        want = _pieces(pcm.region_diff(p, r, _Rc=info["Rc"][k]))   # (region_diff copies p itself)
        _same_pieces(_pieces(got[k]), want, (what, k))
        pieces += len(want)
    return pieces


@pytest.mark.parametrize("shared", [True, False])
def test_public_call_equals_the_single_calls(ref, shared):
    """Case 2: polytope.region_diff_batch(polys, regs) against [region_diff(p, r, _Rc=Rc_k)], Rc_k from the batched call
    (radii that tie may differ in the last bit between two batches, and the order follows them): the same number of
    pieces, every piece's A and b bitwise equal; cases 0-11, with one Region per polytope (all twelve in one call: a
    launch per dimension) and with one Region shared by all polytopes of a dimension (the cells of that dimension's
    second case)."""
    import polytope_amd.polytope as pcm
    cases = ref.cases[:12]
    assert all(c.leaves != "IndexError" for c in cases)
    if shared:
        pieces = 0
        for d in (2, 3, 4):
            mine = [c for c in cases if c.d == d]
            reg = pcm.Region([q.copy() for q in mine[1].cells])
            pieces += _public_against_single([c.P.copy() for c in mine], reg, [reg] * len(mine), ("shared", d))
    else:
        regs = [pcm.Region([q.copy() for q in c.cells]) for c in cases]
        pieces = _public_against_single([c.P.copy() for c in cases], regs, regs, "own")
    assert pieces > 12


@pytest.mark.parametrize("poison", [float("nan"), 1e300])
def test_padding_and_neighbours(ref, poison):
    """Case 3: rows past m[p] / mc[c], cells nobody lists and cell-table slots behind the last listed cell filled with
    NaN, and with 1e300: the outputs are unchanged; and a problem's result is the same alone and in the middle of a batch."""
    from polytope_amd import batch
    K = ref.packs[3]
    which = [0, 1, 2, 3, 4]
    A, b, m, off, idx = _batch_of(K, which)
    clean = batch.region_diff_search_batch(A, b, m, K.CA, K.Cb, K.mc, off, idx, ABS_TOL)
    spare = 3   # slots behind the table's last cell
    CA, Cb = np.full((K.Nc + spare, K.mc_max, 3), poison), np.full((K.Nc + spare, K.mc_max), poison)
    mc = np.concatenate([K.mc, np.full(spare, K.mc_max, np.int32)])
    listed = np.zeros(K.Nc, bool)
    listed[idx] = True
    for c in np.nonzero(listed)[0]:
        CA[c, :K.mc[c]], Cb[c, :K.mc[c]] = K.CA[c, :K.mc[c]], K.Cb[c, :K.mc[c]]
    assert not listed.all()
    Ap, bp = A.copy(), b.copy()
    for p in range(len(which)):
        Ap[p, m[p]:], bp[p, m[p]:] = poison, poison
    got = batch.region_diff_search_batch(Ap, bp, m, CA, Cb, mc, off, idx, ABS_TOL)
    for key in clean:
        assert np.array_equal(got[key], clean[key]), key
    alone = batch.region_diff_search_batch(Ap[2:3], bp[2:3], m[2:3], CA, Cb, mc, off[2:4] - off[2], idx[off[2]:off[3]], ABS_TOL)
    assert _leaves(alone, 0) == _leaves(clean, 2) and alone["nlp"][0] == clean["nlp"][2] and alone["status"][0] == clean["status"][2]
    _check_problem(clean, 2, K.cases[2])


def _ngon(n):
    t = 2 * np.pi * (np.arange(n) + 0.25) / n
    return np.c_[np.cos(t), np.sin(t)], np.ones(n)


def test_every_status_on_the_device(ref):
    """Case 4: RD_OVERFLOW (p_max = 2), RD_BUDGET (max_lps = 5), RD_LONG (61 rows of the minuend + 4 of the cell),
    RD_UNSUPPORTED (65 cells listed) and RD_COVERED (the minuend listed as a cell), each between two healthy problems whose
    leaves are unchanged (RD_BUDGET and RD_OVERFLOW also once for the whole launch); and the raw wrapper's second launch
    returns the full leaves of a problem that overflowed.  RD_INDEX has no construction: no whole search is known to
    reach it (tests/test_rdiff_search_host.py, test_moves_on_hand_made_states), its moves are held on the CPU."""
    from polytope_amd import batch
    K = ref.packs[2]
    healthy = [i for i, c in enumerate(K.cases) if c.leaves != "IndexError"][:2]
    ha, hb_ = K.cases[healthy[0]], K.cases[healthy[1]]
    # the special problems share the 2-D cell table: cell Nc = the 61-gon's own rows can not be a cell of 2d + 2 rows, so
    # the table here gets rows enough for it
    gA, gb = _ngon(61)
    mc_max, m_max = 61, 61
    Nc = K.Nc + 2
    CA, Cb, mc = np.zeros((Nc, mc_max, 2)), np.zeros((Nc, mc_max)), np.zeros(Nc, np.int32)
    CA[:K.Nc, :K.mc_max], Cb[:K.Nc, :K.mc_max], mc[:K.Nc] = K.CA, K.Cb, K.mc
    boxA, boxb = _unit(np.array([[1.0, 0], [0, 1.0], [-1.0, 0], [0, -1.0]]), np.array([0.3, 0.3, 0.2, 0.2]))
    CA[K.Nc, :4], Cb[K.Nc, :4], mc[K.Nc] = boxA, boxb, 4                  # a box inside the 61-gon
    CA[K.Nc + 1, :ha.m], Cb[K.Nc + 1, :ha.m], mc[K.Nc + 1] = ha.An[:ha.m], ha.Bn[:ha.m], ha.m   # healthy case a itself

    def problems(specials):
        """healthy a, special, healthy b, special, ... healthy a"""
        rows, lists = [], []
        for s in specials:
            rows += [(ha.An[:ha.m], ha.Bn[:ha.m]), s[0]]
            lists += [list(K.first[healthy[0]] + ha.order), s[1]]
        rows.append((hb_.An[:hb_.m], hb_.Bn[:hb_.m]))
        lists.append(list(K.first[healthy[1]] + hb_.order))
        B = len(rows)
        A, b, m = np.zeros((B, m_max, 2)), np.zeros((B, m_max)), np.zeros(B, np.int32)
        for p, (rA, rb) in enumerate(rows):
            m[p] = rA.shape[0]
            A[p, :m[p]], b[p, :m[p]] = rA, rb
        off = np.concatenate([[0], np.cumsum([len(w) for w in lists])]).astype(np.int32)
        return A, b, m, off, np.concatenate(lists).astype(np.int32)
    own = (ha.An[:ha.m], ha.Bn[:ha.m])
    specials = [((gA, gb), [K.Nc]),                                        # RD_LONG: 61 + 4 rows in the first list
                (own, [K.first[healthy[0]] + int(ha.order[0])] * 65),      # RD_UNSUPPORTED: 65 cells
                (own, [K.first[healthy[0]] + int(ha.order[0]), K.Nc + 1])]  # RD_COVERED: the second cell is the minuend
    A, b, m, off, idx = problems(specials)
    res = batch.region_diff_search_batch(A, b, m, CA, Cb, mc, off, idx, ABS_TOL)
    assert [int(s) for s in res["status"][1::2]] == [RB.RD_LONG, RB.RD_UNSUPPORTED, RB.RD_COVERED]
    assert all(int(res["count"][p]) == 0 for p in (1, 3, 5)) and int(res["nlp"][3]) == 0
    assert int(res["mi"][5][1]) == 0 and int(res["mi"][5][0]) == int(ha.mi[0])
    for p in (0, 2, 4):
        _check_problem(res, p, ha)
    _check_problem(res, 6, hb_)
    # RD_BUDGET and RD_OVERFLOW are the whole launch's: the healthy problems here are small enough for both
    A, b, m, off, idx = _batch_of(K, healthy + [healthy[0]])
    full = batch.region_diff_search_batch(A, b, m, K.CA, K.Cb, K.mc, off, idx, ABS_TOL, p_max=256, r_max=8192)
    assert all(int(s) == RB.RD_OK for s in full["status"]) and int(full["count"].min()) > 2 and int(full["nlp"].min()) > 5
    few = batch.region_diff_search_batch(A, b, m, K.CA, K.Cb, K.mc, off, idx, ABS_TOL, p_max=256, r_max=8192, max_lps=5)
    assert all(int(s) == RB.RD_BUDGET for s in few["status"]) and all(int(v) == 5 for v in few["nlp"])
    over = batch.region_diff_search_batch(A, b, m, K.CA, K.Cb, K.mc, off, idx, ABS_TOL, p_max=2, r_max=8192)
    assert all(int(s) == RB.RD_OVERFLOW for s in over["status"])
    for p in range(3):
        assert (int(over["count"][p]), int(over["nrows"][p]), int(over["nlp"][p])) == \
            (int(full["count"][p]), int(full["nrows"][p]), int(full["nlp"][p]))
        assert _leaves(over, p) == _leaves(full, p)[:2]
    # the wrapper's own second launch: a problem with more than 32 pieces between two that fit
    K3 = ref.packs[3]
    big = next(i for i, c in enumerate(K3.cases) if c.leaves != "IndexError" and len(c.leaves) > 32)
    small = next(i for i, c in enumerate(K3.cases) if c.leaves != "IndexError" and len(c.leaves) <= 32)
    which = [small, big, small]
    A, b, m, off, idx = _batch_of(K3, which)
    first = batch.region_diff_search_batch(A, b, m, K3.CA, K3.Cb, K3.mc, off, idx, ABS_TOL, p_max=32, r_max=1024)
    assert [int(s) for s in first["status"]] == [RB.RD_OK, RB.RD_OVERFLOW, RB.RD_OK]
    res = batch.region_diff_search_batch(A, b, m, K3.CA, K3.Cb, K3.mc, off, idx, ABS_TOL)
    for p, i in enumerate(which):
        _check_problem(res, p, K3.cases[i])
    # RD_BUDGET beside healthy neighbours: a budget between what the small and the large problem need
    need = [int(v) for v in res["nlp"]]
    assert need[0] == need[2] < need[1] - 1
    mid = (need[0] + need[1]) // 2
    got = batch.region_diff_search_batch(A, b, m, K3.CA, K3.Cb, K3.mc, off, idx, ABS_TOL, max_lps=mid, p_max=512, r_max=16384)
    assert [int(s) for s in got["status"]] == [RB.RD_OK, RB.RD_BUDGET, RB.RD_OK] and int(got["nlp"][1]) == mid
    for p in (0, 2):
        _check_problem(got, p, K3.cases[small])
    assert _leaves(got, 1) == K3.cases[big].leaves[:int(got["count"][1])]


def test_packed_call_equals_the_public_call(ref):
    """The packed level batch.region_diff_batch against polytope.region_diff_batch (which case 2 holds to the single
    call): per problem, through piece_off, the same number of pieces and every piece's A and b bitwise equal after the
    reduce; status and Rc; the `order` override against region_diff's `_order`; and a problem none of whose cells
    intersects returns its minuend's unit rows as its one piece."""
    import polytope_amd
    import polytope_amd.polytope as pcm
    from polytope_amd import batch
    cases = [c for c in ref.cases[:12] if c.d == 3]
    polys = [c.P.copy() for c in cases]
    regs = [pcm.Region([q.copy() for q in c.cells]) for c in cases]
    # one more problem: the first polytope against two boxes far away from it
    far = pcm.Region([pcm.box2poly([[5.0, 6.0]] * 3), pcm.box2poly([[7.0, 8.0]] * 3)])
    polys.append(cases[0].P.copy())
    regs.append(far)
    info = {}
    want = polytope_amd.region_diff_batch(polys, regs, _info=info)
    # the packed inputs as the public call packs them: the rows of copies of the polytopes, the cells' rows as they are
    copies = [p.copy() for p in polys]
    cells = [q for r in regs for q in r.list_poly]
    B, m_max, mc_max = len(polys), max(p.A.shape[0] for p in copies) + 2, max(q.A.shape[0] for q in cells) + 1
    A, b, m = np.full((B, m_max, 3), np.nan), np.full((B, m_max), np.nan), np.zeros(B, np.int32)
    for k, p in enumerate(copies):
        m[k] = p.A.shape[0]
        A[k, :m[k]], b[k, :m[k]] = p.A, p.b
    CA, Cb, mc = np.full((len(cells), mc_max, 3), np.nan), np.full((len(cells), mc_max), np.nan), np.zeros(len(cells), np.int32)
    for k, q in enumerate(cells):
        mc[k] = q.A.shape[0]
        CA[k, :mc[k]], Cb[k, :mc[k]] = q.A, q.b
    off = np.concatenate([[0], np.cumsum([len(r) for r in regs])])
    idx = np.arange(len(cells))

    def check(got, want, Rcs):
        assert got["piece_off"].shape == (B + 1,) and got["piece_off"][-1] == len(got["m"])
        assert [int(s) for s in got["status"]] == [RB.RD_OK] * B
        for k in range(B):
            lo, hi = int(got["piece_off"][k]), int(got["piece_off"][k + 1])
            mine = [(got["A"][q, :got["m"][q]], got["b"][q, :got["m"][q]]) for q in range(lo, hi)]
            assert all(int(v) in (0, 1) for v in got["kind"][lo:hi])
            if k < B - 1:
                _same_pieces(mine, _pieces(want[k]), ("packed", k))
            assert RB.hb.same_bits(got["Rc"][off[k]:off[k + 1]], Rcs[k])
    got = batch.region_diff_batch(A, b, m, CA, Cb, mc, off, idx)
    check(got, want, info["Rc"])
    # nothing intersects: the minuend's unit rows, one piece, kind 0
    lo, hi = int(got["piece_off"][B - 1]), int(got["piece_off"][B])
    uA, ub = _unit(copies[-1].A, copies[-1].b)
    assert hi - lo == 1 and int(got["kind"][lo]) == 0 and int(got["m"][lo]) == m[B - 1]
    assert RB.hb.same_bits(got["A"][lo, :m[B - 1]], uA) and RB.hb.same_bits(got["b"][lo, :m[B - 1]], ub)
    assert np.all(got["Rc"][off[B - 1]:] == 0) and np.array_equal(_pieces(want[B - 1])[0][0], copies[-1].A)
    # `order`: the reverse of the radius order for problem 1, region_diff's `_order` on the other side
    Rc1 = info["Rc"][1]
    n1 = int(np.sum(Rc1 >= ABS_TOL))
    rev = np.argsort(-Rc1)[:n1][::-1]
    perm = np.concatenate([rev, [j for j in range(len(Rc1)) if j not in set(rev.tolist())]]).astype(int)
    assert n1 > 1
    order = [None] * B
    order[1] = perm
    got2 = batch.region_diff_batch(A, b, m, CA, Cb, mc, off, idx, order=order)
    try:
        single = _pieces(pcm.region_diff(polys[1], regs[1], _Rc=Rc1, _order=perm))
    except IndexError:
        single = None
    if single is None:
        assert int(got2["status"][1]) == RB.RD_INDEX
    else:
        assert int(got2["status"][1]) == RB.RD_OK
        lo, hi = int(got2["piece_off"][1]), int(got2["piece_off"][2])
        _same_pieces([(got2["A"][q, :got2["m"][q]], got2["b"][q, :got2["m"][q]]) for q in range(lo, hi)], single, "order")
    for k in (0, 2):   # the neighbours keep their pieces
        for key in ("A", "b"):
            a0 = got[key][int(got["piece_off"][k]):int(got["piece_off"][k + 1])]
            a1 = got2[key][int(got2["piece_off"][k]):int(got2["piece_off"][k + 1])]
            w = min(a0.shape[1], a1.shape[1])
            assert a0.shape[0] == a1.shape[0] and np.array_equal(a0[:, :w], a1[:, :w])


def test_a_problem_beyond_the_caps_falls_back(ref):
    """Case 5: an RD_LONG problem (a 61-gon minus a box: 65 rows in the first list) through the public call goes through the
    single region_diff and equals it, beside a problem the kernel solves."""
    import polytope_amd
    import polytope_amd.polytope as pcm
    gA, gb = _ngon(61)
    P = pcm.Polytope(gA, gb)
    box = pcm.box2poly([[-0.2, 0.3], [-0.2, 0.3]])
    c = next(c for c in ref.cases if c.d == 2 and c.leaves != "IndexError")
    polys, regs = [c.P.copy(), P.copy()], [pcm.Region([q.copy() for q in c.cells]), pcm.Region([box.copy()])]
    info = {}
    got = polytope_amd.region_diff_batch(polys, regs, _info=info)
    assert info["status"] == [RB.RD_OK, RB.RD_LONG]
    for k in range(2):
        _same_pieces(_pieces(got[k]), _pieces(pcm.region_diff(polys[k], regs[k], _Rc=info["Rc"][k])), k)
    assert len(_pieces(got[1])) > 1


def test_the_call_runs_on_the_callers_stream(ref):
    """Case 6: CUDA tensors in, on a stream of its own.  The tensors hold a decoy batch (other cases, other leaves); on
    the stream: a delay, the copy of the real batch into the tensors, the call, clones of the outputs; only that stream
    is synchronised.  The leaves are those of case 1 -- a launch that went to the default stream would have answered for
    the decoy -- and the outputs are CUDA tensors."""
    import torch
    from polytope_amd import batch
    import test_streams_gpu as TSG
    K = ref.packs[3]
    ok = [i for i, c in enumerate(K.cases) if c.leaves != "IndexError"]
    real_i, decoy_i = ok[:3], ok[3:6]
    assert [K.cases[i].leaves for i in real_i] != [K.cases[i].leaves for i in decoy_i]
    n_idx = max(sum(len(K.cases[i].order) for i in sel) for sel in (real_i, decoy_i))

    def tensors(sel):
        A, b, m, off, idx = _batch_of(K, sel)
        idx = np.concatenate([idx, np.zeros(n_idx - idx.size, np.int32)])   # (both batches in tensors of one size)
        return [torch.as_tensor(a, device="cuda:0") for a in (A, b, m, off, idx)]
    real, live = tensors(real_i), tensors(decoy_i)
    table = [torch.as_tensor(a, device="cuda:0") for a in (K.CA, K.Cb, K.mc)]
    warm = batch.region_diff_search_batch(live[0], live[1], live[2], table[0], table[1], table[2], live[3], live[4], ABS_TOL,
                                          p_max=256, r_max=8192)
    torch.cuda.synchronize()
    assert [_leaves({k: v.cpu().numpy() for k, v in warm.items()}, p) for p in range(3)] == [K.cases[i].leaves for i in decoy_i]
    P = TSG.Prepared()
    P.torch, P.delay, P.probe = torch, TSG.Delay(torch), torch.zeros(1, device="cuda:0")
    P.delay.ms = 20.0
    s = TSG.stream_apart_from(P, torch.cuda.default_stream())
    with torch.cuda.stream(s):
        P.delay()
        for dst, src in zip(live, real):
            dst.copy_(src)
        res = batch.region_diff_search_batch(live[0], live[1], live[2], table[0], table[1], table[2], live[3], live[4],
                                             ABS_TOL, p_max=256, r_max=8192)
        clones = {k: v.clone() for k, v in res.items()}
    s.synchronize()
    assert all(v.is_cuda for v in res.values())
    got = {k: v.cpu().numpy() for k, v in clones.items()}
    for p, i in enumerate(real_i):
        _check_problem(got, p, K.cases[i])
