"""One-pass device flow diagnostics (gls_flow_diagnostics through GLSContext.flow_diagnostics): the CFL
maximum of the reference's calculate_CFL (postprocessing_cfl.cc:36-87), int 1/2 |u|^2, int 1/2 |curl u|^2 and
the volume with QGauss(k+1), against a numpy restatement written here: the 1D Lagrange basis on the
equidistant lattice a/m (the support points of FE_Q(m) and of the mapping for m <= 2), its tensor product at
the Gauss points, and for mapped cells the MappingQ Jacobian from the cells' support points (J, det J and
J^-1 by numpy, none of the library's per-point geometry); |K| of the CFL's h from the cell extents or, for
mapped cells, the multilinear corner map. The restatement is pinned first against closed forms and against
the oracle's L2 norm (Oracle.l2_error with exact = 0 and the same Gauss rule), then the device is compared
to it at relative 1e-12, the project's FP64 parity level (tests/test_gpu_parity.py)."""
import numpy as np
import pytest

from oracle.oracle import MappedProblem, Oracle, StructuredProblem
from softx_2020_200_amd.native import GLSError, UMesh, hyper_cube
from softx_2020_200_amd.problem import build_context
from tests.gpu_util import context_for, cuda
from tests.test_gpu_uforest import adapted_space, continuous_field, dof_lines
from tests.test_uforest import CASES

SEED = 20200200
DT = 0.0125
TOL = 1e-12


# ---------------------------------------------------------------------------------------------
# numpy restatement
# ---------------------------------------------------------------------------------------------
def lagrange(m, x):
    """V [len(x)][m+1], D: the Lagrange basis on the nodes a/m and its derivative at x"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    xn = np.arange(m + 1) / m
    V, D = np.ones((len(x), m + 1)), np.zeros((len(x), m + 1))
    for a in range(m + 1):
        for j in range(m + 1):
            if j != a:
                V[:, a] *= (x - xn[j]) / (xn[a] - xn[j])
        for l in range(m + 1):
            if l == a:
                continue
            t = np.full(len(x), 1.0 / (xn[a] - xn[l]))
            for j in range(m + 1):
                if j != a and j != l:
                    t *= (x - xn[j]) / (xn[a] - xn[j])
            D[:, a] += t
    return V, D


def tensor_basis(m, dim, X1):
    """phi [nq][nl], dphi [nq][nl][dim] at the tensor points of X1 (x fastest, like the local node order)"""
    n1, m1 = len(X1), m + 1
    V, D = lagrange(m, X1)
    nq, nl = n1 ** dim, m1 ** dim
    phi, dphi = np.ones((nq, nl)), np.ones((nq, nl, dim))
    for q in range(nq):
        iq = [(q // n1 ** d) % n1 for d in range(dim)]
        for a in range(nl):
            ia = [(a // m1 ** d) % m1 for d in range(dim)]
            for d in range(dim):
                phi[q, a] *= V[iq[d], ia[d]]
                for e in range(dim):
                    dphi[q, a, e] *= (D if e == d else V)[iq[d], ia[d]]
    return phi, dphi


def gauss01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def restate(dim, k, cell_vnodes, n_vnodes, sol, dt, cell_h=None, cell_support=None):
    """(out[4], per-cell CFL) of the definition in include/gls_native.h"""
    gx, gw = gauss01(k + 1)
    phi, dphi = tensor_basis(k, dim, gx)
    nq = len(phi)
    W = np.ones(nq)
    for q in range(nq):
        for d in range(dim):
            W[q] *= gw[(q // (k + 1) ** d) % (k + 1)]
    U = np.asarray(sol)[:dim * n_vnodes].reshape(n_vnodes, dim)[np.asarray(cell_vnodes)]  # [nc][nl][c]
    uq = np.einsum("qb,nbc->nqc", phi, U)
    gxi = np.einsum("qba,nbc->nqca", dphi, U)  # d u_c / d xi_a
    if cell_support is None:
        h = np.asarray(cell_h)
        G = gxi / h[:, None, None, :]
        jxw = W[None, :] * np.prod(h, axis=1)[:, None]
        meas = np.prod(h, axis=1)
    else:
        S = np.asarray(cell_support).reshape(len(U), -1, dim)
        J = np.einsum("qba,nbi->nqia", dphi, S)  # d x_i / d xi_a (the mapping degree is k)
        G = np.einsum("nqca,nqai->nqci", gxi, np.linalg.inv(J))
        jxw = np.linalg.det(J) * W[None, :]
        # cell->measure(): the volume of the multilinear cell through the corners (2-point Gauss is exact)
        corner = [sum(((v >> d) & 1) * k * (k + 1) ** d for d in range(dim)) for v in range(2 ** dim)]
        g2, w2 = gauss01(2)
        _, d1 = tensor_basis(1, dim, g2)
        W2 = np.array([np.prod([w2[(q // 2 ** d) % 2] for d in range(dim)]) for q in range(2 ** dim)])
        meas = (np.linalg.det(np.einsum("qba,nbi->nqia", d1, S[:, corner, :])) * W2[None, :]).sum(axis=1)
    ke = 0.5 * (uq ** 2).sum(axis=2)
    en = 0.5 * (G[..., 1, 0] - G[..., 0, 1]) ** 2
    if dim == 3:
        en = en + 0.5 * ((G[..., 2, 1] - G[..., 1, 2]) ** 2 + (G[..., 0, 2] - G[..., 2, 0]) ** 2)
    phic, _ = tensor_basis(k, dim, np.array([0.5]))
    uc = np.einsum("b,nbc->nc", phic[0], U)
    hh = np.sqrt(4.0 * meas / np.pi) / k if dim == 2 else np.cbrt(6.0 * meas / np.pi) / k
    cfl = np.linalg.norm(uc, axis=1) / hh * dt
    return np.array([cfl.max(), (ke * jxw).sum(), (en * jxw).sum(), jxw.sum()]), cfl


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)


def check(ctx, x, ref, tag):
    out = ctx.flow_diagnostics(cuda(x), DT)
    e = rel(out, ref)
    print(tag, "device", out, "restatement", ref, "relative errors", e)
    assert (ref > 0).all()
    assert (e <= TOL).all(), (tag, e)
    return out


# ---------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------
A3 = np.array([[0.3, -1.1, 0.7], [0.5, 0.2, -0.4], [-0.9, 0.6, -0.5]])
B3 = np.array([0.4, -0.3, 0.2])


def curl2(A):
    if A.shape[0] == 2:
        return (A[1, 0] - A[0, 1]) ** 2
    return (A[2, 1] - A[1, 2]) ** 2 + (A[0, 2] - A[2, 0]) ** 2 + (A[1, 0] - A[0, 1]) ** 2


def box_problem(dim, n, k, kp):
    return StructuredProblem(dim, n, k=k, kp=kp, viscosity=0.1)


def box_restate(p, x):
    return restate(p.dim, p.k, p.cell_vnodes, p.n_vnodes, x, DT, cell_h=p.cell_h)


def mapped_restate(p, x):
    return restate(p.dim, p.k, p.cell_vnodes, p.n_vnodes, x, DT, cell_support=p.cell_support)


def mapped_space(dim):
    """the smallest curved Q2 spaces of the suite: a 2D hyper_shell and the 3D cylinder shell of test_gpu_cell_sf"""
    if dim == 2:
        return UMesh(2, "hyper_shell", "0, 0 : 0.25 : 1 : 4 : true").fe_space(2, 2, qmapping_all=True)
    return UMesh(3, "cylinder_shell", "0.5 : 0.25 : 1 : 8 : 2").fe_space(2, 1, qmapping_all=True)


def linear_nodal(p, A, b):
    x = np.zeros(p.n_dofs)
    x[:p.dim * p.n_vnodes] = (p.vnode_coords() @ A.T + b).reshape(-1)
    return x


# ---------------------------------------------------------------------------------------------
# the restatement against closed forms and the oracle (no device)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,k", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_restatement_linear_field_on_the_box(dim, k):
    """u = A x + b on [-1,1]^dim: int 1/2 |u|^2 = 1/2 (tr(A^T A) / 3 + |b|^2) V, int 1/2 |curl u|^2 = 1/2 |omega|^2 V,
    V = 2^dim; the CFL maximum is over the cell centres"""
    A, b = A3[:dim, :dim], B3[:dim]
    p = box_problem(dim, 3, k, 1)
    out, cfl = box_restate(p, linear_nodal(p, A, b))
    V = 2.0 ** dim
    want = np.array([0.0, 0.5 * (np.trace(A.T @ A) / 3 + b @ b) * V, 0.5 * curl2(A) * V, V])
    centres = p.cell_x0 + 0.5 * p.cell_h
    hh = np.sqrt(4 * p.hc ** 2 / np.pi) / k if dim == 2 else np.cbrt(6 * p.hc ** 3 / np.pi) / k
    want[0] = (np.linalg.norm(centres @ A.T + b, axis=1) / hh * DT).max()
    assert (rel(out, want) <= TOL).all(), (out, want)


@pytest.mark.parametrize("dim", [2, 3])
def test_restatement_linear_field_on_mapped_cells(dim):
    """isoparametric Q2 cells hold u = A x exactly: the enstrophy integral is 1/2 |omega|^2 times the volume"""
    p = MappedProblem(mapped_space(dim))
    A = A3[:dim, :dim]
    out, _ = mapped_restate(p, linear_nodal(p, A, np.zeros(dim)))
    assert rel(out[2], 0.5 * curl2(A) * out[3]) <= TOL
    exact = np.pi * (1 - 0.25 ** 2) if dim == 2 else 0.5 * np.pi * (1 - 0.25 ** 2)
    assert abs(out[3] - exact) < 5e-2 * exact  # the Q2 mapping of the annulus: close to, not equal to, pi (ro^2 - ri^2) L


@pytest.mark.parametrize("kind", ["box2", "box3", "mapped2", "mapped3"])
def test_restatement_kinetic_energy_is_the_oracle_l2_norm(kind):
    """Oracle.l2_error(sol, exact = 0)^2 / 2 with QGauss(k+1): int 1/2 |u|^2 by a second route"""
    dim = int(kind[-1])
    if kind.startswith("box"):
        p = box_problem(dim, 3, 2, 1)
        fn = box_restate
    else:
        p = MappedProblem(mapped_space(dim))
        fn = mapped_restate
    x = np.random.default_rng(SEED).uniform(-1, 1, p.n_dofs)
    eu, _ = Oracle(p).l2_error(x, lambda X: np.zeros((len(X), dim + 1)), nq1d_err=p.k + 1)
    out, _ = fn(p, x)
    assert rel(out[1], 0.5 * eu * eu) <= TOL, (out[1], 0.5 * eu * eu)


# ---------------------------------------------------------------------------------------------
# the device against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k,kp", [(1, 1), (2, 1)])
def test_square_17x17(k, kp):
    """289 cells: more than one block, and not a multiple of the block"""
    p = box_problem(2, 17, k, kp)
    assert len(p.cell_vnodes) == 289
    x = np.random.default_rng(SEED).uniform(-1, 1, p.n_dofs)
    out = check(context_for(p), x, box_restate(p, x)[0], "square 17x17 Q%d-Q%d" % (k, kp))
    assert rel(out[3], 4.0) <= TOL


@pytest.mark.gpu
def test_cube_8_bricks_and_per_cell(monkeypatch):
    """3D 8^3 Q2-Q2 on the Morton mesh: the brick context and the per-cell context of the same mesh (the brick
    kernels disabled while it is created) agree with the restatement and with each other"""
    mesh = hyper_cube(3, 8, 2)
    x = np.random.default_rng(SEED).uniform(-1, 1, 3 * mesh["n_vnodes"] + mesh["n_pnodes"])
    ref, _ = restate(3, 2, mesh["cell_vnodes"], mesh["n_vnodes"], x, DT, cell_h=mesh["cell_h"])
    brick = build_context(mesh, viscosity=0.1)
    assert brick.uses_brick_kernels
    monkeypatch.setenv("GLS_DISABLE_BRICK", "1")
    cell = build_context(mesh, viscosity=0.1)
    monkeypatch.delenv("GLS_DISABLE_BRICK")
    assert not cell.uses_brick_kernels
    ob = check(brick, x, ref, "cube 8^3 Q2-Q2 bricks")
    oc = check(cell, x, ref, "cube 8^3 Q2-Q2 per cell")
    assert (rel(ob, oc) <= TOL).all()


@pytest.mark.gpu
def test_cube_3_q2q1():
    p = box_problem(3, 3, 2, 1)
    ctx = context_for(p)
    assert not ctx.uses_brick_kernels
    x = np.random.default_rng(SEED).uniform(-1, 1, p.n_dofs)
    check(ctx, x, box_restate(p, x)[0], "cube 3^3 Q2-Q1")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_mapped_q2(dim):
    p = MappedProblem(mapped_space(dim), viscosity=0.1)
    ctx = context_for(p)
    x = np.random.default_rng(SEED).uniform(-1, 1, p.n_dofs)
    check(ctx, x, mapped_restate(p, x)[0], "mapped Q2 %dD" % dim)
    # u = A x: exact on the isoparametric cells
    A = A3[:dim, :dim]
    out = ctx.flow_diagnostics(cuda(linear_nodal(p, A, np.zeros(dim))), DT)
    assert rel(out[2], 0.5 * curl2(A) * out[3]) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,dim,spec,flat", [CASES[1], CASES[2]], ids=[CASES[1][0], CASES[2][0]])
def test_adapted_meshes_with_hanging_nodes(name, dim, spec, flat):
    """the vector carries the constrained values (a continuous field), as d_present does"""
    _, h = adapted_space(name, dim, spec, 2, 1)
    sp = h.data
    assert sp["vhang"]
    p = MappedProblem(sp, viscosity=0.1)
    lines = dof_lines(sp)
    p.set_hanging(*lines)
    p.hang_lines = lines
    x = continuous_field(sp, np.random.default_rng(SEED))
    check(context_for(p), x, mapped_restate(p, x)[0], "adapted " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [5, 288], ids=["first_block", "last_partial_block"])
def test_cfl_maximum_placed_by_hand(cell):
    """zero field but for the nodes of one cell: the CFL is that cell's, found in the first block and in the
    last, partial one"""
    p = box_problem(2, 17, 1, 1)
    x = np.zeros(p.n_dofs)
    for a, nd in enumerate(p.cell_vnodes[cell]):
        x[2 * nd:2 * nd + 2] = (1.0 + 0.1 * a, -0.5)
    ref, cfl = box_restate(p, x)
    assert int(np.argmax(cfl)) == cell and cfl[cell] > 1.5 * np.delete(cfl, cell).max()
    check(context_for(p), x, ref, "CFL maximum in cell %d" % cell)


@pytest.mark.gpu
def test_zero_field_and_repeatability():
    p = box_problem(3, 3, 2, 2)
    ctx = context_for(p)
    out = ctx.flow_diagnostics(cuda(np.zeros(p.n_dofs)), DT)
    assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 0.0
    assert rel(out[3], 8.0) <= TOL
    x = cuda(np.random.default_rng(SEED).uniform(-1, 1, p.n_dofs))
    a, b = ctx.flow_diagnostics(x, DT), ctx.flow_diagnostics(x, DT)
    assert np.array_equal(a, b)  # bitwise: fixed-order sums, no atomics
    p2 = box_problem(2, 17, 2, 1)  # more than one block
    ctx2 = context_for(p2)
    x2 = cuda(np.random.default_rng(SEED).uniform(-1, 1, p2.n_dofs))
    assert np.array_equal(ctx2.flow_diagnostics(x2, DT), ctx2.flow_diagnostics(x2, DT))


@pytest.mark.gpu
def test_unsupported_degrees_are_an_error():
    """2D Q3-Q3 has no diagnostics kernel: GLS_EINVAL with a message that names the limit, no launch"""
    p = StructuredProblem(2, 2, k=3, kp=3, viscosity=0.1)
    with pytest.raises(GLSError, match="Q3"):
        context_for(p).flow_diagnostics(cuda(np.zeros(p.n_dofs)), DT)
