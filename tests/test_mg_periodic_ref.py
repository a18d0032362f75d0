"""CPU: the numpy restatement of the periodic V-cycle (tests/vcycle_periodic_ref.py) that tests/test_gpu_mg_periodic.py
compares the device with: its prolongation is the periodic interpolant, and its GMRES counts are the ones written into
the GPU test."""
import numpy as np
import pytest

from tests import vcycle_periodic_ref as pr


@pytest.mark.parametrize("name", list(pr.CASES))
def test_periodic_reference_prolongation_and_gmres_count(name):
    ops = pr.operators(name)
    H = ops["H"]
    P = H["P"][0]
    pf, pc = H["probs"]
    assert P.shape == (pf.n_dofs, pc.n_dofs)
    # a partition of unity with at most 27 dyadic weights per row; every coarse DoF is injected from one fine DoF
    assert np.abs(np.asarray(P.sum(axis=1)).ravel() - 1.0).max() == 0.0 and np.diff(P.indptr).max() == 27
    assert set(np.unique(np.abs(P.data) * 512.0) % 1.0) == {0.0}
    # it reproduces a trigonometric polynomial of the box at the fine nodes to interpolation accuracy, across the seam
    per = pr.CASES[name]["periodic"]
    f = lambda X: np.prod([np.sin(X[:, d]) if d in per else np.sin(0.5 * X[:, d]) ** 2 for d in range(3)], axis=0)
    nvc, nvf = pc.n_vnodes, pf.n_vnodes
    Pp = P[3 * nvf:, 3 * nvc:]
    err = np.abs(Pp @ f(pr.lattice_coords(pc, pc.kp, pc.pshape)) - f(pr.lattice_coords(pf, pf.kp, pf.pshape))).max()
    # quadratic interpolation on equidistant nodes: |f - I f| <= h^3 max|f'''| / (72 sqrt 3) per direction, here
    # h = pi / 2 and |f'''| <= 1 for every factor (|factor| <= 1), three directions; a seam taken wrongly is O(1)
    assert err <= 3.0 * (np.pi / 2) ** 3 / (72.0 * np.sqrt(3.0)), err
    # the seam is used: some fine row couples the last and the first coarse node of a periodic axis
    d = per[0]
    stride = int(np.prod(pc.pshape[:d]))
    ix = (Pp.indices // stride) % pc.pshape[d]
    rows = np.repeat(np.arange(Pp.shape[0]), np.diff(Pp.indptr))
    lo_rows, hi_rows = set(rows[ix == 0]), set(rows[ix == pc.pshape[d] - 1])
    assert lo_rows & hi_rows
    want = {"xyz": 17, "x": 16}[name]
    assert pr.gmres_iterations(name) == want
