"""The host-only plan of gls_ilu_attach (csrc/gls_ilu_plan.cpp, exported as gls_ilu_plan): the renumbering, the
ILU(fill) pattern and the probe colouring it computes without a device are identical to what the attach computed
before the plan was split out of it (tests/golden/ilu_plan_parent.json: counts and SHA-256 digests recorded from
gls_ilu_info / gls_ilu_factors on the parent commit), and satisfy the properties the preconditioner's correctness
rests on. Integer equality only."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

SEED = 20200200
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ilu_plan_parent.json")

# (dim, n, k, kp, fill, ordering, block_dofs): the tuples of test_gpu_ilu.py::test_iluk_factors_match_oracle, Q3-Q3
# (the pressure-on-velocity-node map with k == kp), a blocked multicolor order
CAVITIES = [(2, 4, 1, 1, 0, "cm", 0), (2, 4, 1, 1, 1, "cm", 0), (2, 4, 1, 1, 4, "cm", 0), (2, 3, 2, 1, 1, "cm", 0),
            (3, 2, 1, 1, 1, "cm", 0), (3, 2, 2, 2, 2, "cm", 0), (2, 4, 2, 1, 0, "multicolor", 0),
            (3, 2, 2, 2, 0, "multicolor", 200), (2, 6, 1, 1, 1, "cm", 40), (3, 2, 2, 1, 0, "multicolor", 0),
            (2, 4, 1, 1, 1, "multicolor", 0), (2, 3, 3, 3, 0, "cm", 0), (3, 3, 2, 1, 0, "multicolor", 500)]
# the adapted mapped shell with hanging and slip lines (test_gpu_ilu.py's batched-probing problem): (fill, ordering)
SHELLS = [(1, "cm"), (0, "multicolor")]
CASES = [("cavity",) + c for c in CAVITIES] + [("shell", 3, 0, 2, 1, f, o, 0) for f, o in SHELLS]


def case_id(case):
    kind, dim, n, k, kp, fill, order, blk = case
    return "%s-d%d-n%d-q%dq%d-fill%d-%s-blk%d" % (kind, dim, n, k, kp, fill, order, blk)


@functools.lru_cache(maxsize=None)
def problem_and_state(kind, dim, n, k, kp):
    """The oracle problem of a case and a state on it (shared by the cases on the same problem; not modified)."""
    rng = np.random.default_rng(SEED)
    if kind == "cavity":
        from tests.test_gpu_ilu import _cavity
        p = _cavity(dim, n, k, kp, "bdf1", 0.05)
        u, u1 = (p.apply_nonzero_constraints(rng.uniform(-1, 1, p.n_dofs)) for _ in range(2))
        return p, (u, u1)
    from oracle.oracle import MappedProblem
    from tests.test_dist_plan import _adapted_space
    from tests.test_gpu_uforest import dof_lines
    sp_ = _adapted_space(dim, k, kp)
    lines = dof_lines(sp_)
    p = MappedProblem(sp_, viscosity=1.0, scheme="steady")
    p.set_hanging(*lines)
    p.hang_lines = lines
    rot = lambda X: np.stack([-X[:, 1], X[:, 0], 0 * X[:, 0]], 1)  # noqa: E731
    p.set_dirichlet([("function", 0, rot), ("noslip", 1, None), ("slip", 2, None), ("slip", 3, None)])
    return p, (p.apply_nonzero_constraints(0.1 * rng.standard_normal(p.n_dofs)),)


@functools.lru_cache(maxsize=None)
def oracle_pattern(kind, dim, n, k, kp):
    """(row, col) of the nonzeros of the oracle's assembled, constraint-eliminated system matrix."""
    from oracle.oracle import Oracle
    p, state = problem_and_state(kind, dim, n, k, kp)
    A, _ = Oracle(p).matrix_and_rhs(*state)
    A = A.tocsr()
    A.eliminate_zeros()
    A = A.tocoo()
    return A.row.astype(np.int64), A.col.astype(np.int64)


def iluk_graph(B, fill):
    """Ascending keys i * n + j of the ILU(fill) graph of the sparse matrix B: the oracle's iluk_levels. That is a
    Python loop over rows and pivots (minutes on the shell's 16 k DoFs), so fill 0 and 1 are also written as sparse
    products -- level 1 is (i, j) with a k < min(i, j) such that (i, k) and (k, j) are entries -- which are asserted
    equal to iluk_levels wherever that is affordable and stand in for it on the shell."""
    from oracle.oracle import iluk_levels
    n = B.shape[0]
    ref = None
    if n <= 1200 or fill > 1:
        ref = np.array(sorted(i * n + j for i, j in iluk_levels(B, fill)), dtype=np.int64)
        if fill > 1:
            return ref
    G = (B + sp.identity(n)).tocsr()
    G.data[:] = 1.0
    if fill == 1:
        G = G + sp.tril(G, -1) @ sp.triu(G, 1)
    G = G.tocoo()
    keys = np.unique(G.row.astype(np.int64) * n + G.col)
    if ref is not None:
        assert np.array_equal(keys, ref)
    return keys


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def record(n_dofs, nnz, n_probes, perm, rowp, col):
    return dict(n_dofs=int(n_dofs), nnz=int(nnz), n_probes=int(n_probes), perm=digest(perm), rowp=digest(rowp),
                col=digest(col))


@functools.lru_cache(maxsize=None)
def plan_of(case):
    from tests.gpu_util import ilu_plan_for
    kind, dim, n, k, kp, fill, order, blk = case
    p, _ = problem_and_state(kind, dim, n, k, kp)
    return p, ilu_plan_for(p, fill=fill, ordering=order, block_dofs=blk)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_plan_equals_the_parent_commits_attach(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case_id(case)]
    p, P = plan_of(case)
    assert record(p.n_dofs, P["nnz"], P["n_probes"], P["perm"], P["rowp"], P["col"]) == want


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_plan_invariants(case):
    kind, dim, n_, k, kp, fill, order, blk = case
    p, P = plan_of(case)
    n = p.n_dofs
    perm, rowp, col = (P[key].astype(np.int64) for key in ("perm", "rowp", "col"))
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert rowp[0] == 0 and rowp[-1] == P["nnz"] == len(col)
    rows = np.repeat(np.arange(n), np.diff(rowp))
    assert (np.diff(col)[rows[1:] == rows[:-1]] > 0).all()  # rows strictly ascending
    assert np.array_equal(np.unique(rows[col == rows]), np.arange(n))  # every row holds its diagonal
    # the pattern holds the ILU(fill) graph of the oracle's matrix in the plan's numbering (block-Jacobi: of what is
    # left after the couplings between subdomains are dropped)
    ar, ac = oracle_pattern(kind, dim, n_, k, kp)
    pattern = rows * n + col  # ascending: rows in order, each sorted
    br, bc = perm[ar], perm[ac]
    if blk:
        keep = np.isin(br * n + bc, pattern)
        assert (~keep).any()
        br, bc = br[keep], bc[keep]
    B = sp.csr_matrix((np.ones(len(br)), (br, bc)), shape=(n, n))
    assert np.isin(iluk_graph(B, fill), pattern).all()
    assert len(br) <= P["nnz_a"] <= P["nnz"]
    # distance 2: no row of the matrix holds two DoFs of one probe
    probe = P["probe"].astype(np.int64)
    assert probe.min() >= 0 and probe.max() < P["n_probes"]
    key = ar * P["n_probes"] + probe[ac]
    assert len(np.unique(key)) == len(key)
    # multicolor solves: no pattern entry joins two nodes of one colour
    if order == "multicolor":
        nvd = dim * p.n_vnodes
        d = np.arange(n)
        node = np.where(d < nvd, d // dim, (p.n_vnodes if kp != k else 0) + d - nvd)
        old = np.empty(n, dtype=np.int64)
        old[perm] = d
        color = P["color"].astype(np.int64)
        assert np.array_equal(color[old], np.sort(color))  # the colours are the outermost sort key
        if P["mc_solve"]:
            i, j = old[rows], old[col]
            assert not ((color[i] == color[j]) & (node[i] != node[j])).any()
    else:
        assert not P["mc_solve"]
