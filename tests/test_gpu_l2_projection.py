"""The matrix-free mass operator and the L2 projection on the device (gls_projection_plan_create, gls_mass_apply,
gls_mass_diagonal, gls_l2_projection through GLSContext.projection_plan) against the oracle's assembled
L2-projection system (gls_oracle_l2_projection_coo) and its exact sparse solve.

Tolerances. One mass product and the diagonal: 1e-13 of the block's maximum (velocity, pressure) -- a single sum of
at most 27 x 8 products per entry, tighter than the project's 1e-12 operator parity. The projection: 1e-12 of the
oracle solution's maximum per block, the project's oracle parity; Jacobi-PCG to 1e-15 on these matrices measured
1.3e-15 .. 5.7e-15 on the host. Symmetry x . (M z) = z . (M x): 1e-13 of |x| |M z|, the Cauchy-Schwarz scale of the
two sums. The iteration count: at most twice that of a numpy Jacobi-PCG on the oracle's system in this file.

Meshes: a 2D 7 x 5 stretched box (h_x != h_y), the 3D 3^3 cube (27 cells: a partial last block), the 2D periodic
TGV box, the 2D hyper_shell and the 3D cylinder_shell (the library's 3D curved shell; GridGenerator::hyper_shell is
2D only here) with MappingQ2."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.oracle import MappedProblem, Oracle, StructuredProblem, _dp
from softx_2020_200_amd.io import Expr
from softx_2020_200_amd.native import GLSError, hyper_cube
from softx_2020_200_amd.problem import build_context
from tests.gpu_util import context_for, cuda
from tests.test_gpu_flow_diagnostics import mapped_space
from tests.test_gpu_l2_error import node_coordinates, stretched

SEED = 20200200
PAIRS = [(1, 1), (2, 1), (2, 2)]
VARS = {2: "x,y,t", 3: "x,y,z,t"}
SMOOTH = {2: "sin(1.3*x+0.2)*cos(0.7*y); cos(x)*y; exp(0.5*x)-y^2",
          3: "sin(1.3*x+0.2)*cos(0.7*y); cos(x)*y; z*x; exp(0.5*x)-y^2"}


def smooth(X):
    x, y = X[:, 0], X[:, 1]
    cols = [np.sin(1.3 * x + 0.2) * np.cos(0.7 * y), np.cos(x) * y]
    if X.shape[1] == 3:
        cols.append(X[:, 2] * x)
    cols.append(np.exp(0.5 * x) - y ** 2)
    return np.stack(cols, axis=1)


def wall_values(X):
    """the `function` Dirichlet boundary: non-zero, not the projected function's trace"""
    x, y = X[:, 0], X[:, 1]
    cols = [1.0 + 0.5 * x, -0.3 + y * x]
    if X.shape[1] == 3:
        cols.append(0.2 * X[:, 2] + 1.0)
    return np.stack(cols, axis=1)


def stretched_7x5(k, kp):
    """7 x 5 cells of 0.3 x 0.65 (the first five rows of the 7 x 7 lattice, its nodes renumbered without gaps), lower
    corner (0.3, -0.7)"""
    p = stretched(StructuredProblem(2, 7, k=k, kp=kp, viscosity=0.1), (1.05, 2.275), (0.3, -0.7))
    for key in ("cell_x0", "cell_h"):
        setattr(p, key, np.ascontiguousarray(getattr(p, key)[:35]))
    for key, count in (("cell_vnodes", "n_vnodes"), ("cell_pnodes", "n_pnodes")):
        used, compact = np.unique(getattr(p, key)[:35], return_inverse=True)
        setattr(p, key, np.ascontiguousarray(compact.reshape(35, -1).astype(np.int32)))
        setattr(p, count, len(used))
    p.n_dofs = 2 * p.n_vnodes + p.n_pnodes
    p.constrained = np.zeros(p.n_dofs, dtype=np.uint8)
    return p


MESHES = ["box2d-1-1", "box2d-2-1", "box2d-2-2", "cube3-1-1", "cube3-2-1", "cube3-2-2", "tgv2d", "shell2d", "shell3d"]
WALLED = [m for m in MESHES if m != "tgv2d"]  # the periodic box has no boundary


def make_problem(name):
    if name.startswith("box2d"):
        return stretched_7x5(int(name[6]), int(name[8]))
    if name.startswith("cube3"):
        return StructuredProblem(3, 3, k=int(name[6]), kp=int(name[8]), viscosity=0.1)
    if name == "tgv2d":
        return StructuredProblem(2, 5, k=2, kp=1, lo=0.0, hi=2 * np.pi, viscosity=0.1, periodic=(0, 1))
    return MappedProblem(mapped_space(2 if name == "shell2d" else 3), viscosity=0.1)


def boundary_vnodes(p):
    """velocity nodes on the boundary and their coordinates"""
    if isinstance(p, MappedProblem):
        X = p.vnode_coords()
        return np.nonzero(np.asarray(p.vnode_bid) != 0)[0], X
    X = node_coordinates(p)[0]
    lo, hi = X.min(axis=0), X.max(axis=0)
    on = (np.abs(X - lo) < 1e-12).any(axis=1) | (np.abs(X - hi) < 1e-12).any(axis=1)
    return np.nonzero(on)[0], X


def with_walls(p):
    """every velocity component of every boundary node fixed at wall_values (a `function` boundary)"""
    nodes, X = boundary_vnodes(p)
    assert len(nodes)
    vals = wall_values(X[nodes])
    p.constrained[:] = 0
    p.dirichlet = {}
    for n, v in zip(nodes, vals):
        for c in range(p.dim):
            p.constrained[n * p.dim + c] = 1
            p.dirichlet[int(n * p.dim + c)] = float(v[c])
    return p


@functools.lru_cache(maxsize=None)
def reference(name):
    """(problem without constraints, A, rhs of SMOOTH): the oracle's assembled system, computed once per mesh"""
    p = make_problem(name)
    orc = Oracle(p)
    ic = np.ascontiguousarray(smooth(p.qpoints().reshape(-1, p.dim)))
    P = p.struct()
    nd = orc.L.gls_oracle_dofs_per_cell(C.byref(P))
    cap = p.n_cells * nd * nd
    rows, cols, vals = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap)
    nnz, rhs = C.c_longlong(0), np.zeros(p.n_dofs)
    assert orc.L.gls_oracle_l2_projection_coo(C.byref(P), _dp(ic), rows.ctypes.data_as(C.POINTER(C.c_int)),
                                              cols.ctypes.data_as(C.POINTER(C.c_int)), _dp(vals), C.byref(nnz),
                                              _dp(rhs)) == 0
    n = nnz.value
    return p, sp.coo_matrix((vals[:n], (rows[:n], cols[:n])), shape=(p.n_dofs,) * 2).tocsr(), rhs


def blocks(p):
    nvd = p.dim * p.n_vnodes
    return (("velocity", slice(0, nvd)), ("pressure", slice(nvd, p.n_dofs)))


def seeded(n, k=1):
    rng = np.random.default_rng(SEED)
    return [rng.uniform(-1, 1, n) for _ in range(k)]


def jacobi_pcg(A, b, fixed, x0):
    """(x, iterations) of Jacobi-preconditioned CG on the free rows from x0, to |r| <= 1e-15 |b|: the device
    algorithm in numpy on the oracle's matrix"""
    free = ~fixed
    d = A.diagonal()
    x = x0.copy()
    r = np.where(free, b - A @ x, 0.0)
    z = np.where(free, r / d, 0.0)
    pd, rz, bb, it = z.copy(), r @ z, b @ b, 0
    while r @ r > 1e-30 * bb and it < 10000:
        Ap = np.where(free, A @ pd, 0.0)
        alpha = rz / (pd @ Ap)
        x += alpha * pd
        r -= alpha * Ap
        z = np.where(free, r / d, 0.0)
        rz, old = r @ z, rz
        pd = z + (rz / old) * pd
        it += 1
    return x, it


# ---------------------------------------------------------------------------------------------
# 1, 2: the operator and its diagonal
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
def test_mass_apply_against_the_oracle_matrix(name):
    p, A, _ = reference(name)
    plan = context_for(p).projection_plan(p)
    x, z = seeded(p.n_dofs, 2)
    y, ref = plan.mass_apply(cuda(x)).cpu().numpy(), A @ x
    for tag, s in blocks(p):
        err, scale = np.abs(y[s] - ref[s]).max(), np.abs(ref[s]).max()
        print("%s %s: |M x - A x| / max %.2e" % (name, tag, err / scale))
        assert err <= 1e-13 * scale, (name, tag, err, scale)
    mz = plan.mass_apply(cuda(z)).cpu().numpy()
    a, b = x @ mz, z @ y
    print("%s: x.Mz %.17e z.Mx %.17e" % (name, a, b))
    assert abs(a - b) <= 1e-13 * np.linalg.norm(x) * np.linalg.norm(mz), (name, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
def test_diagonal_against_the_oracle_matrix(name):
    p, A, _ = reference(name)
    d, ref = context_for(p).projection_plan(p).diagonal().cpu().numpy(), A.diagonal()
    for tag, s in blocks(p):
        err, scale = np.abs(d[s] - ref[s]).max(), np.abs(ref[s]).max()
        print("%s %s: |d - diag A| / max %.2e" % (name, tag, err / scale))
        assert err <= 1e-13 * scale, (name, tag, err, scale)


# ---------------------------------------------------------------------------------------------
# 3: the projection against the exact solve
# ---------------------------------------------------------------------------------------------
def check_projection(name, p, A, rhs):
    fixed = p.constrained.astype(bool)
    x0 = np.zeros(p.n_dofs)
    for dof, v in p.dirichlet.items():
        x0[dof] = v
    free = np.nonzero(~fixed)[0]
    ref = x0.copy()  # A_ff x_f = b_f - A_fc x_c
    ref[free] = spla.spsolve(A[free][:, free].tocsc(), (rhs - A @ x0)[free])
    _, its = jacobi_pcg(A, rhs, fixed, x0)
    plan = context_for(p).projection_plan(p)
    x = plan.project(Expr(SMOOTH[p.dim], VARS[p.dim]), 0.0).cpu().numpy()
    print("%s: %d fixed DoFs, %d CG iterations (numpy %d), relative residual %.2e" %
          (name, fixed.sum(), plan.iterations, its, plan.relative_residual))
    for tag, s in blocks(p):
        err, scale = np.abs(x[s] - ref[s]).max(), np.abs(ref[s]).max()
        print("%s %s: |x - x_oracle| / max %.2e" % (name, tag, err / scale))
        assert err <= 1e-12 * scale, (name, tag, err, scale)
    assert plan.relative_residual <= 1e-15
    assert 0 < plan.iterations <= 2 * its, (name, plan.iterations, its)
    assert np.array_equal(x[fixed], x0[fixed])  # the Dirichlet values, exactly


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
def test_projection_without_constraints(name):
    p, A, rhs = reference(name)
    check_projection(name, p, A, rhs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WALLED)
def test_projection_with_a_function_boundary(name):
    _, A, rhs = reference(name)
    p = with_walls(make_problem(name))
    assert any(v != 0.0 for v in p.dirichlet.values())
    check_projection(name + " walls", p, A, rhs)


# ---------------------------------------------------------------------------------------------
# 4, 5, 6: properties
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k,kp", PAIRS)
def test_polynomials_of_the_space_are_reproduced(k, kp):
    """degree <= k per variable in the velocity, <= kp in the pressure: the projection is the nodal interpolant"""
    p = stretched_7x5(k, kp)
    u = "1 + 2*x - y + 0.5*x*y" if k == 1 else "1 + 2*x - y + 0.5*x*y - x^2*y + 0.25*x^2*y^2 + y^2"
    v = "x - 3*y + x*y" if k == 1 else "x - 3*y + x*y^2 - 0.5*x^2"
    q = "0.5 - x + 2*y - x*y" if kp == 1 else "0.5 - x + 2*y - x*y + x^2*y^2 - y^2"
    e = Expr("; ".join((u, v, q)), VARS[2])
    Xv, Xp = node_coordinates(p)
    nodal = np.concatenate([e(np.c_[Xv, np.zeros(len(Xv))])[:, :2].reshape(-1), e(np.c_[Xp, np.zeros(len(Xp))])[:, 2]])
    x = context_for(p).projection_plan(p).project(e, 0.0).cpu().numpy()
    for tag, s in blocks(p):
        err, scale = np.abs(x[s] - nodal[s]).max(), np.abs(nodal[s]).max()
        print("Q%d-Q%d %s: |x - interpolant| / max %.2e" % (k, kp, tag, err / scale))
        assert err <= 1e-12 * scale, (k, kp, tag, err, scale)


@pytest.mark.gpu
def test_time_enters_the_function():
    p = stretched_7x5(2, 1)
    plan = context_for(p).projection_plan(p)
    a = plan.project(Expr("cos(x)*exp(-t); sin(y)*t; x*y + t", VARS[2]), 0.3).cpu().numpy()
    b = plan.project(Expr("cos(x)*exp(-0.3); sin(y)*0.3; x*y + 0.3", VARS[2]), 0.0).cpu().numpy()
    c = plan.project(Expr("cos(x)*exp(-t); sin(y)*t; x*y + t", VARS[2]), 0.0).cpu().numpy()
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)


@pytest.mark.gpu
def test_two_calls_are_bitwise_equal():
    for name in ("box2d-2-1", "cube3-2-2", "shell2d"):
        p = with_walls(make_problem(name))
        plan = context_for(p).projection_plan(p)
        e = Expr(SMOOTH[p.dim], VARS[p.dim])
        a, ia = plan.project(e, 0.0).cpu().numpy(), plan.iterations
        b, ib = plan.project(e, 0.0).cpu().numpy(), plan.iterations
        assert np.array_equal(a, b) and ia == ib, name
        x = cuda(seeded(p.n_dofs)[0])
        assert np.array_equal(plan.mass_apply(x).cpu().numpy(), plan.mass_apply(x).cpu().numpy()), name


@pytest.mark.gpu
def test_cube_8_bricks_and_per_cell(monkeypatch):
    """3D 8^3 Q2-Q2 on the Morton mesh: the brick context and the per-cell context of the same mesh give the same
    bits (the layout enters only through the context's cell tables); 512 cells of 27 points: 57 blocks"""
    mesh = hyper_cube(3, 8, 2)
    brick = build_context(mesh, viscosity=0.1)
    assert brick.uses_brick_kernels
    monkeypatch.setenv("GLS_DISABLE_BRICK", "1")
    cell = build_context(mesh, viscosity=0.1)
    monkeypatch.delenv("GLS_DISABLE_BRICK")
    assert not cell.uses_brick_kernels
    e = Expr(SMOOTH[3], VARS[3])
    x = cuda(seeded(3 * mesh["n_vnodes"] + mesh["n_pnodes"])[0])
    pb, pc = brick.projection_plan(mesh), cell.projection_plan(mesh)
    assert np.array_equal(pb.mass_apply(x).cpu().numpy(), pc.mass_apply(x).cpu().numpy())
    a, b = pb.project(e, 0.0).cpu().numpy(), pc.project(e, 0.0).cpu().numpy()
    assert pb.iterations == pc.iterations and pb.relative_residual <= 1e-15
    assert np.array_equal(a, b)
    assert np.abs(a).max() > 0.5


# ---------------------------------------------------------------------------------------------
# 7: refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals():
    """GLS_EINVAL with a message that names the limit: nothing is launched"""
    p3 = StructuredProblem(2, 2, k=3, kp=3, viscosity=0.1)
    with pytest.raises(GLSError, match=r"\(-1\).*Q3"):
        context_for(p3).projection_plan(p3)
    p = StructuredProblem(2, 3, k=2, kp=1, viscosity=0.1)
    ctx = context_for(p)
    plan = ctx.projection_plan(p)
    with pytest.raises(GLSError, match=r"\(-1\).*2 components, expected 3"):
        plan.project(Expr("x; y", VARS[2]), 0.0)
    with pytest.raises(GLSError, match=r"\(-1\).*4 variables, expected 3"):
        plan.project(Expr("x*z; y; t", VARS[3]), 0.0)
    with pytest.raises(GLSError, match=r"\(-1\).*not the context's"):
        ctx.projection_plan(StructuredProblem(2, 4, k=2, kp=1, viscosity=0.1))
    ctx.set_hanging([0], [0, 1], [4], [1.0])
    with pytest.raises(GLSError, match=r"\(-1\).*hanging or slip lines"):
        ctx.projection_plan(p)
    with pytest.raises(GLSError, match=r"\(-1\).*hanging or slip lines"):  # a plan made before the lines
        plan.project(Expr(SMOOTH[2], VARS[2]), 0.0)
