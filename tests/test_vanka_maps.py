"""CPU: the host-built maps of the cell-Vanka patches (gls_vanka_maps: neighbour lists and per-pair overlap maps)
against the oracle's assembled matrix. On the 3^3 box (Q2-Q1 and Q2-Q2, a cell with all 26 neighbours) and the
cylinder shell at refinement 1, for every cell c: the union over its neighbours c' of the overlap pairs, expanded to
the entries (i, i') they add K_c'[j][j'] to, reproduces the sparsity of R_c A R_c^T from the oracle's COO (taken
without constraints, so that no entry is eliminated); summing the oracle's element matrices through the maps gives
that patch matrix; the multiplicities equal each DoF's cell count."""
import numpy as np
import pytest

from softx_2020_200_amd.native import GLSError, vanka_maps
from tests import vanka_ref as vr


def unconstrained(case):
    import copy
    p = copy.copy(vr.problem(case, "steady"))
    p.constrained = np.zeros_like(p.constrained)
    p.dirichlet = {}
    return p


@pytest.mark.parametrize("case", vr.CASES)
def test_maps_reproduce_patch_sparsity_and_values(case):
    p = unconstrained(case)
    u, u1, u2 = vr.state(case, "steady")
    M = vanka_maps(3, p.k, p.kp, p.cell_vnodes, p.cell_pnodes if p.kp != p.k else None, p.n_vnodes, p.n_pnodes)
    cd = vr.cell_dofs_of(p)
    nd = cd.shape[1]
    assert np.array_equal(M["cell_dofs"], cd)
    assert np.array_equal(M["mult"], np.bincount(cd.reshape(-1), minlength=p.n_dofs))
    K = vr.oracle_element_matrices(p, u, u1, u2)
    A = vr.oracle_matrix(p, u, u1, u2)
    most = 0
    for c in range(p.n_cells):
        nb = M["nb_cell"][M["nb_off"][c]:M["nb_off"][c + 1]]
        assert np.all(np.diff(nb) > 0) and c in nb
        most = max(most, len(nb))
        pat = np.zeros((nd, nd), dtype=bool)
        Ac = np.zeros((nd, nd))
        for pr in range(M["nb_off"][c], M["nb_off"][c + 1]):
            c2 = M["nb_cell"][pr]
            i, j = (M[k][M["ov_off"][pr]:M["ov_off"][pr + 1]].astype(int) for k in ("ov_i", "ov_j"))
            assert np.array_equal(cd[c][i], cd[c2][j]) and len(i) == len(np.intersect1d(cd[c], cd[c2]))
            pat[np.ix_(i, i)] = True
            Ac[np.ix_(i, i)] += K[c2][np.ix_(j, j)]
        ref = A[cd[c]][:, cd[c]]
        struct = np.zeros((nd, nd), dtype=bool)
        struct[ref.nonzero()] = True  # the COO's structure (explicit zeros of a cell's block included)
        assert np.array_equal(pat, struct), c
        ref = ref.toarray()
        assert np.abs(Ac - ref).max() <= 1e-13 * np.abs(ref).max(), c
    if case.startswith("box"):
        assert most == 27


def test_maps_refuse_a_cell_that_holds_a_node_twice():
    from oracle.oracle import StructuredProblem
    p = StructuredProblem(3, 1, k=2, kp=1, periodic=(0,))
    with pytest.raises(GLSError, match="periodic"):
        vanka_maps(3, 2, 1, p.cell_vnodes, p.cell_pnodes, p.n_vnodes, p.n_pnodes)
