"""The L2 error against an analytical solution on the device (gls_error_plan_create / gls_l2_error through
GLSContext.error_plan) against a numpy restatement of the application's host l2_error(): QGauss(k+2) tables, the
host Expr at the mapped points, plain dense sums, the two-pass pressure mean and the host's volume rule (box
meshes: the sum of JxW; mapped meshes: the sum of the Q1 cell measures).

The states are seeded U(-1, 1). With a near-exact state u_h - u cancels and ulp differences of the exact values
are magnified, so the tolerance is relative to the fields' scale, not to the error:
    |device - restatement| <= 1e-12 sqrt(int |u_h|^2 + int |u|^2)      (and the same form for the pressure),
1e-12 being the project's parity tolerance (DESIGN row a1)."""
import numpy as np
import pytest

from oracle.oracle import MappedProblem, StructuredProblem
from softx_2020_200_amd.io import Expr
from softx_2020_200_amd.native import GLSError, UMesh, hyper_cube
from softx_2020_200_amd.problem import build_context
from tests.gpu_util import context_for, cuda
from tests.test_gpu_flow_diagnostics import gauss01, mapped_space, tensor_basis
from tests.test_gpu_uforest import adapted_space, continuous_field, dof_lines
from tests.test_uforest import CASES

SEED = 20200200
TOL = 1e-12
EXACT = {2: "sin(pi*x) * cos(0.7*y) * exp(-t); -cos(1.3*x) * sin(pi*y) + t; x*y - 0.25 + sin(x + 2*y) * t",
         3: "sin(pi*x) * cos(0.7*y) * exp(-t) + z; -cos(1.3*x) * sin(pi*y) + t*z; x*z - y; x*y*z - 0.25 + sin(x + 2*y - z) * t"}
VARS = {2: "x,y,t", 3: "x,y,z,t"}


def attr(mesh, key):
    return mesh.get(key) if isinstance(mesh, dict) else getattr(mesh, key, None)


def geometry(mesh, X1):
    """(X [nc][nq][dim], det J [nc][nq], Q1 cell measures or None) at the tensor points of X1 (x fastest)"""
    dim, k = attr(mesh, "dim"), attr(mesh, "k")
    nc = len(attr(mesh, "cell_vnodes"))
    n1 = len(X1)
    xi = np.array([[X1[(q // n1 ** d) % n1] for d in range(dim)] for q in range(n1 ** dim)])
    sup = attr(mesh, "cell_support")
    if sup is None:
        x0, h = np.asarray(attr(mesh, "cell_x0")), np.asarray(attr(mesh, "cell_h"))
        return x0[:, None, :] + h[:, None, :] * xi[None, :, :], np.repeat(np.prod(h, axis=1)[:, None], len(xi), axis=1), None
    assert attr(mesh, "map_degree") == k
    S = np.asarray(sup).reshape(nc, -1, dim)
    phi, dphi = tensor_basis(k, dim, X1)
    J = np.einsum("qba,nbi->nqia", dphi, S)
    # cell->measure(): the multilinear cell through the corners (2-point Gauss is exact)
    corner = [sum(((v >> d) & 1) * k * (k + 1) ** d for d in range(dim)) for v in range(2 ** dim)]
    g2, w2 = gauss01(2)
    _, d1 = tensor_basis(1, dim, g2)
    W2 = np.array([np.prod([w2[(q // 2 ** d) % 2] for d in range(dim)]) for q in range(2 ** dim)])
    meas = (np.linalg.det(np.einsum("qba,nbi->nqia", d1, S[:, corner, :])) * W2[None, :]).sum(axis=1)
    return np.einsum("qb,nbi->nqi", phi, S), np.linalg.det(J), meas


def restate(mesh, x, expr, t):
    """(error_u, error_p, scale_u, scale_p): the host routine in numpy"""
    dim, k, kp, nv = attr(mesh, "dim"), attr(mesh, "k"), attr(mesh, "kp"), attr(mesh, "n_vnodes")
    nq1 = k + 2
    gx, gw = gauss01(nq1)
    W = np.array([np.prod([gw[(q // nq1 ** d) % nq1] for d in range(dim)]) for q in range(nq1 ** dim)])
    X, det, meas = geometry(mesh, gx)
    jxw = det * W[None, :]
    cv = np.asarray(attr(mesh, "cell_vnodes"))
    cp = attr(mesh, "cell_pnodes")
    cp = cv if cp is None else np.asarray(cp)
    x = np.asarray(x)
    uq = np.einsum("qb,nbc->nqc", tensor_basis(k, dim, gx)[0], x[:dim * nv].reshape(nv, dim)[cv])
    pq = np.einsum("qb,nb->nq", tensor_basis(kp, dim, gx)[0], x[dim * nv:][cp])
    E = expr(np.concatenate([X.reshape(-1, dim), np.full((X.shape[0] * X.shape[1], 1), float(t))], axis=1))
    ue = E[:, :dim].reshape(uq.shape)
    pe = E[:, dim].reshape(pq.shape) if E.shape[1] > dim else np.zeros_like(pq)
    vol = jxw.sum() if meas is None else meas.sum()
    pint, peint = (pq * jxw).sum(), (pe * jxw).sum()
    eu = (((uq - ue) ** 2).sum(axis=2) * jxw).sum()
    ep = ((((pq - pint / vol) - (pe - peint / vol)) ** 2) * jxw).sum()
    su = np.sqrt(((uq ** 2).sum(axis=2) * jxw).sum() + ((ue ** 2).sum(axis=2) * jxw).sum())
    sp = np.sqrt((pq ** 2 * jxw).sum() + (pe ** 2 * jxw).sum())
    return np.sqrt(eu), np.sqrt(ep), su, sp


def check(ctx, mesh, x, expr, t, tag, tol=TOL, plan=None):
    plan = plan or ctx.error_plan(mesh, expr)
    eu, ep = plan.l2_error(cuda(x), t)
    ru, rp, su, sp = restate(mesh, x, expr, t)
    print("%s: velocity %.17e (restatement %.17e, |diff| / scale %.2e), pressure %.17e (restatement %.17e, "
          "|diff| / scale %.2e)" % (tag, eu, ru, abs(eu - ru) / su, ep, rp, abs(ep - rp) / max(sp, 1e-300)))
    assert abs(eu - ru) <= tol * su, (tag, eu, ru, su)
    assert abs(ep - rp) <= tol * sp, (tag, ep, rp, sp)
    return eu, ep


def seeded(n):
    return np.random.default_rng(SEED).uniform(-1, 1, n)


def exact(dim):
    return Expr(EXACT[dim], VARS[dim])


def stretched(p, s, origin):
    p.cell_x0 = np.asarray(origin) + (np.asarray(p.cell_x0) + 1.0) * np.asarray(s)
    p.cell_h = np.asarray(p.cell_h) * np.asarray(s)
    return p


def stretched_5x3(k, kp):
    """5 x 3 cells of 0.4 x 1.3 (the first three rows of the 5 x 5 lattice, its nodes renumbered without gaps), lower
    corner (0.3, -0.7): non-square cells, a non-zero x0"""
    p = stretched(StructuredProblem(2, 5, k=k, kp=kp, viscosity=0.1), (1.0, 3.25), (0.3, -0.7))
    for key in ("cell_x0", "cell_h"):
        setattr(p, key, np.ascontiguousarray(getattr(p, key)[:15]))
    for key, count in (("cell_vnodes", "n_vnodes"), ("cell_pnodes", "n_pnodes")):
        used, compact = np.unique(getattr(p, key)[:15], return_inverse=True)
        setattr(p, key, np.ascontiguousarray(compact.reshape(15, -1).astype(np.int32)))
        setattr(p, count, len(used))
    p.n_dofs = 2 * p.n_vnodes + p.n_pnodes
    p.constrained = np.zeros(p.n_dofs, dtype=np.uint8)
    return p


def square_17(k, kp):
    return stretched(StructuredProblem(2, 17, k=k, kp=kp, viscosity=0.1), (0.8, 1.3), (0.3, -0.7))


def node_coordinates(mesh):
    """(velocity node coordinates, pressure node coordinates) from the cells' own geometry"""
    out = []
    for m, key in ((attr(mesh, "k"), "cell_vnodes"), (attr(mesh, "kp"), "cell_pnodes")):
        X, _, _ = geometry(mesh, np.arange(m + 1) / m)
        cn = attr(mesh, key)
        cn = np.asarray(attr(mesh, "cell_vnodes") if cn is None else cn)
        n = attr(mesh, "n_vnodes" if key == "cell_vnodes" else "n_pnodes")
        C = np.zeros((n, attr(mesh, "dim")))
        C[cn.reshape(-1)] = X.reshape(-1, X.shape[2])
        out.append(C)
    return out


# ---------------------------------------------------------------------------------------------
# box cells
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k,kp", [(1, 1), (2, 1), (2, 2)])
def test_stretched_5x3(k, kp):
    p = stretched_5x3(k, kp)
    assert len(p.cell_vnodes) == 15
    check(context_for(p), p, seeded(p.n_dofs), exact(2), 0.3, "5x3 Q%d-Q%d" % (k, kp))


@pytest.mark.gpu
@pytest.mark.parametrize("k,kp", [(1, 1), (2, 1)])
def test_square_17x17_several_blocks(k, kp):
    """289 cells of 9 / 16 points: 28 / 16 cells per block, 11 / 19 blocks of partials, a partial last block"""
    p = square_17(k, kp)
    check(context_for(p), p, seeded(p.n_dofs), exact(2), 0.3, "17x17 Q%d-Q%d" % (k, kp))


@pytest.mark.gpu
@pytest.mark.parametrize("k,kp", [(1, 1), (2, 1)])
def test_cube_3(k, kp):
    p = StructuredProblem(3, 3, k=k, kp=kp, viscosity=0.1)
    check(context_for(p), p, seeded(p.n_dofs), exact(3), 0.3, "3^3 Q%d-Q%d" % (k, kp))


@pytest.mark.gpu
def test_cube_q2q2_bricks_and_per_cell(monkeypatch):
    """3D 2^3 Q2-Q2 on the Morton mesh (one brick): the brick context and the per-cell context of the same mesh
    agree with the restatement, and with each other bitwise"""
    mesh = hyper_cube(3, 2, 2)
    x = seeded(3 * mesh["n_vnodes"] + mesh["n_pnodes"])
    brick = build_context(mesh, viscosity=0.1)
    assert brick.uses_brick_kernels
    monkeypatch.setenv("GLS_DISABLE_BRICK", "1")
    cell = build_context(mesh, viscosity=0.1)
    monkeypatch.delenv("GLS_DISABLE_BRICK")
    assert not cell.uses_brick_kernels
    e = exact(3)
    assert check(brick, mesh, x, e, 0.3, "2^3 Q2-Q2 bricks") == check(cell, mesh, x, e, 0.3, "2^3 Q2-Q2 per cell")


# ---------------------------------------------------------------------------------------------
# mapped cells, hanging nodes
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_mapped_q2_shells(dim):
    p = MappedProblem(mapped_space(dim), viscosity=0.1)
    check(context_for(p), p, seeded(p.n_dofs), exact(dim), 0.3, "mapped Q2 %dD" % dim)


@pytest.mark.gpu
def test_adapted_mesh_with_hanging_nodes():
    """the vector carries the constrained values (a continuous field), as the application's does"""
    name, dim, spec, _ = CASES[1]
    _, h = adapted_space(name, dim, spec, 2, 1)
    sp = h.data
    assert sp["vhang"]
    p = MappedProblem(sp, viscosity=0.1)
    lines = dof_lines(sp)
    p.set_hanging(*lines)
    p.hang_lines = lines
    check(context_for(p), p, continuous_field(sp, np.random.default_rng(SEED)), exact(dim), 0.3, "adapted " + name)


# ---------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------
def interpolant_meshes():
    yield "box 2D", stretched_5x3(2, 1)
    yield "box 3D", StructuredProblem(3, 3, k=2, kp=1, viscosity=0.1)
    yield "mapped 2D", MappedProblem(mapped_space(2), viscosity=0.1)
    # Q2 pressure: x is in the pressure space of a curved cell only when it is isoparametric too
    yield "mapped 3D", MappedProblem(UMesh(3, "cylinder_shell", "0.5 : 0.25 : 1 : 8 : 2").fe_space(2, 2, qmapping_all=True),
                                     viscosity=0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["box 2D", "box 3D", "mapped 2D", "mapped 3D"])
def test_interpolant_of_the_exact_solution(tag):
    """u = (y, -x [, 0]), p = x interpolated into the vector: both errors vanish at rounding level, 1e-13 of the
    fields' scale -- wrong points, a wrong det J or a wrong component order would show at the scale itself"""
    p = dict(interpolant_meshes())[tag]
    dim = p.dim
    Xv, Xp = node_coordinates(p)
    x = np.zeros(p.n_dofs)
    U = np.zeros((p.n_vnodes, dim))
    U[:, 0], U[:, 1] = Xv[:, 1], -Xv[:, 0]
    x[:dim * p.n_vnodes] = U.reshape(-1)
    x[dim * p.n_vnodes:] = Xp[:, 0]
    e = Expr("y; -x; x" if dim == 2 else "y; -x; 0; x", VARS[dim])
    eu, ep = context_for(p).error_plan(p, e).l2_error(cuda(x), 0.0)
    _, _, su, sp = restate(p, x, e, 0.0)
    print("%s: velocity error %.3e (scale %.3e), pressure error %.3e (scale %.3e)" % (tag, eu, su, ep, sp))
    assert su > 0.1 and sp > 0.1
    assert eu <= 1e-13 * su and ep <= 1e-13 * sp, (tag, eu, su, ep, sp)


@pytest.mark.gpu
def test_time_enters_the_exact_solution():
    p = stretched_5x3(2, 1)
    e = Expr("exp(-2*nu*t) * cos(x) * sin(y); -exp(-2*nu*t) * sin(x) * cos(y); -0.25 * exp(-4*nu*t) * (cos(2*x) + cos(2*y))",
             VARS[2], "nu=0.35")
    ctx, x = context_for(p), seeded(p.n_dofs)
    plan = ctx.error_plan(p, e)
    a = check(ctx, p, x, e, 0.3, "t = 0.3", plan=plan)
    b = check(ctx, p, x, e, 1.7, "t = 1.7", plan=plan)
    assert a != b


@pytest.mark.gpu
def test_pressure_shift():
    """a constant added to every pressure DoF: the pressure error moves by rounding only (the means are taken out
    before the square, in two passes), the velocity error not at all"""
    p = square_17(2, 1)
    ctx, e, x = context_for(p), exact(2), seeded(p.n_dofs)
    plan = ctx.error_plan(p, e)
    y = x.copy()
    y[2 * p.n_vnodes:] += 1000.0
    (eu0, ep0), (eu1, ep1) = plan.l2_error(cuda(x), 0.3), plan.l2_error(cuda(y), 0.3)
    _, _, _, sp = restate(p, y, e, 0.3)  # the shifted field's scale
    print("pressure error %.17e shifted %.17e scale %.3e" % (ep0, ep1, sp))
    assert eu0 == eu1
    assert abs(ep0 - ep1) <= TOL * sp


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_missing_pressure_component(dim):
    p = stretched_5x3(2, 1) if dim == 2 else StructuredProblem(3, 3, k=1, kp=1, viscosity=0.1)
    velocity = ";".join(EXACT[dim].split(";")[:dim])
    ctx, x = context_for(p), cuda(seeded(p.n_dofs))
    short, full = Expr(velocity, VARS[dim]), Expr(velocity + "; 0", VARS[dim])
    assert short.n_components == dim and full.n_components == dim + 1
    assert ctx.error_plan(p, short).l2_error(x, 0.3) == ctx.error_plan(p, full).l2_error(x, 0.3)


@pytest.mark.gpu
def test_state_in_the_last_cell_of_a_partial_block():
    p = square_17(1, 1)
    cell = 288  # 28 cells per block: the 9th cell of the 11th block
    x = np.zeros(p.n_dofs)
    for a, (nd, pn) in enumerate(zip(p.cell_vnodes[cell], p.cell_pnodes[cell])):
        x[2 * nd:2 * nd + 2] = (1.0 + 0.3 * a, -0.5 + 0.2 * a * a)
        x[2 * p.n_vnodes + pn] = 0.7 - 0.4 * a
    zero = Expr("0; 0; 0", VARS[2])
    eu, ep = check(context_for(p), p, x, zero, 0.0, "one cell, exact solution 0")
    assert eu > 0.1 and ep > 0.01
    check(context_for(p), p, x, exact(2), 0.3, "one cell")


@pytest.mark.gpu
def test_two_calls_are_bitwise_equal():
    for p, dim in ((square_17(2, 1), 2), (StructuredProblem(3, 3, k=2, kp=2, viscosity=0.1), 3)):
        plan = context_for(p).error_plan(p, exact(dim))
        x = cuda(seeded(p.n_dofs))
        assert plan.l2_error(x, 0.3) == plan.l2_error(x, 0.3)  # fixed-order sums, no atomics


@pytest.mark.gpu
def test_refusals():
    """GLS_EINVAL with a message at gls_error_plan_create: nothing is launched"""
    p3 = StructuredProblem(2, 2, k=3, kp=3, viscosity=0.1)
    with pytest.raises(GLSError, match="Q3"):
        context_for(p3).error_plan(p3, exact(2))
    p = StructuredProblem(2, 3, k=2, kp=1, viscosity=0.1)
    ctx = context_for(p)
    with pytest.raises(GLSError, match="2 variables, expected 3"):
        ctx.error_plan(p, Expr("y; -x; x", "x,y"))
    with pytest.raises(GLSError, match="4 variables, expected 3"):
        ctx.error_plan(p, exact(3))
    with pytest.raises(GLSError, match="1 components"):
        ctx.error_plan(p, Expr("y", VARS[2]))
    with pytest.raises(GLSError, match="stack of 17"):
        ctx.error_plan(p, Expr("x + (" * 16 + "x" + ")" * 16 + "; y; 0", VARS[2]))
    with pytest.raises(GLSError, match="not the\\s+context's"):
        ctx.error_plan(StructuredProblem(2, 4, k=2, kp=1, viscosity=0.1), exact(2))
