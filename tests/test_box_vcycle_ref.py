"""CPU: the numpy restatement of the V-cycle on nested subdivided hyper_rectangles (tests/vcycle_box_ref.py) that
tests/test_gpu_box.py compares the device with: its prolongation is the box's per-axis interpolant (wrapped on the
periodic axis), and its GMRES counts are the ones written into the GPU test."""
import numpy as np
import pytest

from tests import vcycle_box_ref as br

NUMPY_GMRES_ITS = {"open": 25, "x": 32}


@pytest.mark.parametrize("name", list(br.CASES))
def test_box_reference_prolongation_and_gmres_count(name):
    ops = br.operators(name)
    H = ops["H"]
    P = H["P"][0]
    pf, pc = H["probs"]
    per = br.CASES[name]["periodic"]
    assert pf.n_cells == 8 * 4 * 4 and pc.n_cells == 4 * 2 * 2 and P.shape == (pf.n_dofs, pc.n_dofs)
    assert pf.vshape == [16 if 0 in per else 17, 9, 9] and pc.vshape == [8 if 0 in per else 9, 5, 5]
    # a partition of unity with at most 27 dyadic weights per row; every coarse DoF is injected from one fine DoF
    assert np.abs(np.asarray(P.sum(axis=1)).ravel() - 1.0).max() == 0.0 and np.diff(P.indptr).max() == 27
    assert set(np.unique(np.abs(P.data) * 512.0) % 1.0) == {0.0}
    # it reproduces a quadratic of the box exactly (a wrong axis length or count would not) and, across the seam, a
    # trigonometric polynomial of period 2 to interpolation accuracy
    nvc, nvf = pc.n_vnodes, pf.n_vnodes
    Pp = P[3 * nvf:, 3 * nvc:]
    Xc, Xf = br.lattice_coords(br.LEVELS[1], br.K, per), br.lattice_coords(br.LEVELS[0], br.K, per)
    fx = (lambda X: np.sin(np.pi * X[:, 0])) if 0 in per else (lambda X: X[:, 0] * (2.0 - X[:, 0]))
    f = lambda X: fx(X) * (X[:, 1] ** 2 - 0.3 * X[:, 1]) * (1.0 + X[:, 2] - 2.0 * X[:, 2] ** 2)
    err = np.abs(Pp @ f(Xc) - f(Xf)).max()
    # quadratic interpolation on equidistant nodes: |f - I f| <= h^3 max|f'''| / (72 sqrt 3), h = 0.5 and |f'''| <=
    # pi^3 for sin(pi x); the other factors are reproduced exactly and bounded by 0.7 and 1.125; a seam taken wrongly
    # is O(1)
    tol = 0.5 ** 3 * np.pi ** 3 / (72.0 * np.sqrt(3.0)) * 0.7 * 1.125 if 0 in per else 1e-14
    assert err <= tol, (err, tol)
    if per:  # the seam is used: some fine row couples the last and the first coarse node of the periodic axis
        ix = Pp.indices % pc.pshape[0]
        rows = np.repeat(np.arange(Pp.shape[0]), np.diff(Pp.indptr))
        assert set(rows[ix == 0]) & set(rows[ix == pc.pshape[0] - 1])
    its = br.gmres_iterations(name)
    assert its == NUMPY_GMRES_ITS[name], its
    assert its < br.jacobi_gmres_iterations(name)
