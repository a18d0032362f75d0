"""The VTU point data evaluated on the device (gls_output_plan_create / gls_output_fields through
GLSContext.output_plan) against the host writer: every test compares plan.fields(sol) with the arrays parsed from an
ASCII file (17 digits: exact) that write_vtu (gls_vtu_write, the literal restatement of the reference's
DataOut::build_patches + post-processors) wrote for the same mesh and the same vector on the host.

Tolerance: the project's device-versus-restatement level, 1e-12 relative in the maximum norm, on seeded U(-1,1)
states (seed 20200200; DESIGN section 2, tests/test_gpu_flow_diagnostics.py). The scales:
  velocity, pressure, velocity_eulerian   their own maximum
  vorticity                               max |grad u| over the patch points
  q_criterion at point p                  0.5 sum_{p' <= p} (|W|^2 + |S|^2) of its cell (q is a difference of two sums;
                                          |W|^2 + |S|^2 = |grad u|^2 in the Frobenius norm)
  points                                  the domain extent
grad u at the patch points, for the scales only, comes from the numpy restatement of the diagnostics test."""
import re

import numpy as np
import pytest

from oracle.oracle import MappedProblem, StructuredProblem
from softx_2020_200_amd.io import write_vtu
from softx_2020_200_amd.native import GLSError, hyper_cube
from softx_2020_200_amd.problem import build_context
from tests.gpu_util import context_for, cuda
from tests.test_gpu_flow_diagnostics import A3, linear_nodal, mapped_space, tensor_basis
from tests.test_gpu_uforest import adapted_space, continuous_field, dof_lines
from tests.test_io import _read_vtu
from tests.test_uforest import CASES

SEED = 20200200
TOL = 1e-12
FIELDS = ("points", "velocity", "pressure", "vorticity", "q_criterion")


# ---------------------------------------------------------------------------------------------
# the host writer's arrays, and grad u at the patch points for the scales
# ---------------------------------------------------------------------------------------------
def read_ascii(path):
    """the Float64 arrays of an ASCII piece (the UInt8 types array is raw bytes there: no XML parser)"""
    text = open(path, "rb").read().decode("latin-1")
    out = {}
    for m in re.finditer(r'<DataArray type="Float64"(?: Name="(\w+)")?(?: NumberOfComponents="(\d+)")? format="ascii">\n'
                         r'(.*?)</DataArray>', text, re.S):
        a = np.array(m.group(3).split(), dtype=np.float64)
        out[m.group(1) or "points"] = a.reshape(-1, int(m.group(2))) if m.group(2) else a
    return out


def host_fields(tmp_path, mesh, x, ns, **kw):
    f = str(tmp_path / ("host_%d.vtu" % len(list(tmp_path.iterdir()))))
    write_vtu(f, mesh, x, subdivision=ns, binary=False, **kw)
    return read_ascii(f)


def attr(mesh, key):
    return mesh[key] if isinstance(mesh, dict) else getattr(mesh, key, None)


def patch_gradients(mesh, x, ns):
    """G [n_cells][npp][c][i] = d u_c / d x_i at the patch points t / ns (x fastest)"""
    dim, k, nv = attr(mesh, "dim"), attr(mesh, "k"), attr(mesh, "n_vnodes")
    _, dphi = tensor_basis(k, dim, np.arange(ns + 1) / ns)
    U = np.asarray(x)[:dim * nv].reshape(nv, dim)[np.asarray(attr(mesh, "cell_vnodes"))]
    gxi = np.einsum("qba,nbc->nqca", dphi, U)
    sup = attr(mesh, "cell_support") if not isinstance(mesh, dict) or "cell_support" in mesh else None
    if sup is None:
        return gxi / np.asarray(attr(mesh, "cell_h"))[:, None, None, :]
    assert attr(mesh, "map_degree") == k
    J = np.einsum("qba,nbi->nqia", dphi, np.asarray(sup).reshape(len(U), -1, dim))
    return np.einsum("nqca,nqai->nqci", gxi, np.linalg.inv(J))


def compare(dev, ref, G, tag):
    """dev (plan.fields) against ref (the host writer) with the scales of the module docstring"""
    assert set(dev) == set(ref) - {"subdomain"}, (sorted(dev), sorted(ref))
    scale = {n: np.abs(ref[n]).max() for n in ("velocity", "pressure", "velocity_eulerian") if n in ref}
    scale["vorticity"] = np.abs(G).max()
    scale["points"] = (ref["points"].max(axis=0) - ref["points"].min(axis=0)).max()
    for n, s in scale.items():
        assert dev[n].shape == ref[n].shape, (tag, n, dev[n].shape, ref[n].shape)
        e = np.abs(dev[n] - ref[n]).max()
        print("%s %-17s max error %.3e scale %.3e" % (tag, n, e, s))
        assert e <= TOL * s, (tag, n, e, s)
    qs = 0.5 * np.cumsum((G ** 2).sum(axis=(2, 3)), axis=1).reshape(-1)
    e = np.abs(dev["q_criterion"] - ref["q_criterion"])
    print("%s %-17s max error / scale %.3e" % (tag, "q_criterion", (e / np.maximum(qs, 1e-300)).max()))
    assert (e <= TOL * qs).all(), (tag, "q_criterion", (e / np.maximum(qs, 1e-300)).max())


def seeded(n):
    return np.random.default_rng(SEED).uniform(-1, 1, n)


def stretched_square(k, kp):
    """17 x 17 cells of 0.8 h x 1.3 h, lower corner (0.3, -0.7): non-square cells, non-zero x0"""
    p = StructuredProblem(2, 17, k=k, kp=kp, viscosity=0.1)
    s = np.array([0.8, 1.3])
    p.cell_x0 = np.array([0.3, -0.7]) + (np.asarray(p.cell_x0) + 1.0) * s
    p.cell_h = np.asarray(p.cell_h) * s
    return p


def run_case(tmp_path, ctx, mesh, x, ns, tag, **kw):
    plan = ctx.output_plan(mesh, ns, **kw)
    dev = plan.fields(cuda(x))
    compare(dev, host_fields(tmp_path, mesh, x, ns, **kw), patch_gradients(mesh, x, ns), tag)
    return dev


# ---------------------------------------------------------------------------------------------
# box cells
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k,kp", [(1, 1), (2, 1), (2, 2)])
def test_square_17x17(tmp_path, k, kp):
    """289 cells, 4 / 9 / 16 points per cell: several blocks, a partial last block, cells that straddle waves"""
    p = stretched_square(k, kp)
    assert len(p.cell_vnodes) == 289
    ctx, x = context_for(p), seeded(p.n_dofs)
    for ns in (1, 2, 3):
        dev = run_case(tmp_path, ctx, p, x, ns, "square Q%d-Q%d subdivision %d" % (k, kp, ns))
        assert dev["vorticity"].shape == (289 * (ns + 1) ** 2,)
        assert np.all(dev["points"][:, 2] == 0.0) and np.all(dev["velocity"][:, 2] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("k,kp", [(2, 1), (1, 1)])
def test_cube_3(tmp_path, k, kp):
    p = StructuredProblem(3, 3, k=k, kp=kp, viscosity=0.1)
    ctx, x = context_for(p), seeded(p.n_dofs)
    for ns in (1, 2):
        run_case(tmp_path, ctx, p, x, ns, "cube 3^3 Q%d-Q%d subdivision %d" % (k, kp, ns))


@pytest.mark.gpu
def test_cube_8_bricks_and_per_cell(tmp_path, monkeypatch):
    """3D 8^3 Q2-Q2 on the Morton mesh: the brick context and the per-cell context of the same mesh agree with the
    host, and with each other bitwise (the layout enters only through the context's cell tables)"""
    mesh = hyper_cube(3, 8, 2)
    x = seeded(3 * mesh["n_vnodes"] + mesh["n_pnodes"])
    brick = build_context(mesh, viscosity=0.1)
    assert brick.uses_brick_kernels
    monkeypatch.setenv("GLS_DISABLE_BRICK", "1")
    cell = build_context(mesh, viscosity=0.1)
    monkeypatch.delenv("GLS_DISABLE_BRICK")
    assert not cell.uses_brick_kernels
    ref, G = host_fields(tmp_path, mesh, x, 2), patch_gradients(mesh, x, 2)
    db, dc = brick.output_plan(mesh, 2).fields(cuda(x)), cell.output_plan(mesh, 2).fields(cuda(x))
    compare(db, ref, G, "cube 8^3 Q2-Q2 bricks")
    compare(dc, ref, G, "cube 8^3 Q2-Q2 per cell")
    for n in FIELDS:
        assert np.array_equal(db[n], dc[n]), n
    assert np.array_equal(db["points"], ref["points"])  # box cells: the host's expression, the host's bits


# ---------------------------------------------------------------------------------------------
# mapped cells, hanging nodes, SRF
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_mapped_q2(tmp_path, dim):
    p = MappedProblem(mapped_space(dim), viscosity=0.1)
    ctx = context_for(p)
    run_case(tmp_path, ctx, p, seeded(p.n_dofs), 2, "mapped Q2 %dD" % dim)
    # u = A x is exact on the isoparametric cells: the constant curl of A at every patch point, and the points
    # are MappingQ2 of the support points
    A = A3[:dim, :dim]
    dev = ctx.output_plan(p, 2).fields(cuda(linear_nodal(p, A, np.zeros(dim))))
    curl = np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]]) if dim == 3 else A[1, 0] - A[0, 1]
    assert np.abs(dev["vorticity"] - curl).max() <= TOL * np.abs(A).max()
    phi, _ = tensor_basis(2, dim, np.arange(3) / 2)
    X = np.einsum("qb,nbi->nqi", phi, np.asarray(p.cell_support).reshape(len(p.cell_vnodes), -1, dim)).reshape(-1, dim)
    assert np.abs(dev["points"][:, :dim] - X).max() <= TOL * (X.max(axis=0) - X.min(axis=0)).max()
    assert np.abs(dev["velocity"][:, :dim] - X @ A.T).max() <= TOL * np.abs(X @ A.T).max()


@pytest.mark.gpu
def test_adapted_mesh_with_hanging_nodes(tmp_path):
    """the vector carries the constrained values (a continuous field), as d_present does"""
    name, dim, spec, _ = CASES[1]
    _, h = adapted_space(name, dim, spec, 2, 1)
    sp = h.data
    assert sp["vhang"]
    p = MappedProblem(sp, viscosity=0.1)
    lines = dof_lines(sp)
    p.set_hanging(*lines)
    p.hang_lines = lines
    run_case(tmp_path, context_for(p), p, continuous_field(sp, np.random.default_rng(SEED)), 2, "adapted " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,omega", [(3, (0.3, -0.2, 0.5)), (2, (0.0, 0.0, 0.5))])
def test_srf_velocity_eulerian(tmp_path, dim, omega):
    p = stretched_square(2, 1) if dim == 2 else StructuredProblem(3, 3, k=2, kp=1, viscosity=0.1)
    x = seeded(p.n_dofs)
    dev = run_case(tmp_path, context_for(p), p, x, 2, "SRF %dD" % dim, srf=True, omega=omega)
    want = dev["velocity"] + np.cross(np.asarray(omega), dev["points"])
    assert np.abs(dev["velocity_eulerian"] - want).max() <= TOL * np.abs(want).max()
    assert "velocity_eulerian" not in context_for(p).output_plan(p, 2).fields(cuda(x))


# ---------------------------------------------------------------------------------------------
# the running sums of q_criterion, repeatability, refusals, the file
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_q_criterion_restarts_at_every_cell(tmp_path):
    """zero but on the nodes of the last cell (in the last, partial block): q is non-zero only where grad u is,
    the last cell and the three neighbours that share its nodes; each of them follows the prefix formula from
    its own first point, nothing is carried in from the cell before it"""
    p = stretched_square(1, 1)
    ns, npp, cell = 3, 16, 288
    x = np.zeros(p.n_dofs)
    for a, nd in enumerate(p.cell_vnodes[cell]):
        x[2 * nd:2 * nd + 2] = (1.0 + 0.3 * a, -0.5 + 0.2 * a * a)
    touched = [c for c in range(289) if set(p.cell_vnodes[c]) & set(p.cell_vnodes[cell])]
    assert len(touched) == 4 and cell in touched
    dev = run_case(tmp_path, context_for(p), p, x, ns, "one cell")
    q = dev["q_criterion"].reshape(289, npp)
    G = patch_gradients(p, x, ns)
    W, S = 0.5 * (G - G.transpose(0, 1, 3, 2)), 0.5 * (G + G.transpose(0, 1, 3, 2))
    w2, s2 = np.cumsum((W ** 2).sum(axis=(2, 3)), axis=1), np.cumsum((S ** 2).sum(axis=(2, 3)), axis=1)
    for c in range(289):
        if c not in touched:
            assert np.all(q[c] == 0.0), c
        else:
            assert np.abs(q[c]).max() > 0.0
            assert (np.abs(q[c] - 0.5 * (w2[c] - s2[c])) <= TOL * 0.5 * (w2[c] + s2[c])).all(), c
    # the first point of a cell holds its own pointwise value
    assert abs(q[cell, 0] - 0.5 * ((W[cell, 0] ** 2).sum() - (S[cell, 0] ** 2).sum())) <= TOL * 0.5 * (G[cell, 0] ** 2).sum()


@pytest.mark.gpu
def test_zero_field_and_repeatability():
    p = StructuredProblem(3, 3, k=2, kp=2, viscosity=0.1)
    plan = context_for(p).output_plan(p, 2)
    z = plan.fields(cuda(np.zeros(p.n_dofs)))
    for n in FIELDS[1:]:
        assert np.all(z[n] == 0.0), n
    x = cuda(seeded(p.n_dofs))
    a, b = plan.fields(x), plan.fields(x)
    for n in FIELDS:
        assert np.array_equal(a[n], b[n]), n  # bitwise: fixed-order sums, no atomics
    p2 = stretched_square(2, 1)  # several blocks
    plan2 = context_for(p2).output_plan(p2, 3)
    x2 = cuda(seeded(p2.n_dofs))
    a, b = plan2.fields(x2), plan2.fields(x2)
    for n in FIELDS:
        assert np.array_equal(a[n], b[n]), n


@pytest.mark.gpu
def test_refusals():
    """GLS_EINVAL with a message at gls_output_plan_create: nothing is launched"""
    p3 = StructuredProblem(2, 2, k=3, kp=3, viscosity=0.1)
    with pytest.raises(GLSError, match="Q3"):
        context_for(p3).output_plan(p3, 1)
    p = StructuredProblem(2, 3, k=2, kp=1, viscosity=0.1)
    ctx = context_for(p)
    with pytest.raises(GLSError, match="not the\\s+context's"):
        ctx.output_plan(StructuredProblem(2, 4, k=2, kp=1, viscosity=0.1), 1)
    with pytest.raises(GLSError, match="not the\\s+context's"):
        ctx.output_plan(StructuredProblem(2, 3, k=2, kp=2, viscosity=0.1), 1)
    with pytest.raises(GLSError, match="subdivision"):
        ctx.output_plan(p, 16)


@pytest.mark.gpu
def test_plan_write_vtu_against_write_vtu(tmp_path):
    """the file of the device path (binary): the connectivity, offsets, types and subdomain arrays are the host
    writer's bytes, the fields are within the tolerance (the points of box cells: equal)"""
    p = stretched_square(2, 1)
    x, ns = seeded(p.n_dofs), 2
    fh, fd = str(tmp_path / "host.vtu"), str(tmp_path / "device.vtu")
    write_vtu(fh, p, x, subdivision=ns, subdomain=3, binary=True)
    context_for(p).output_plan(p, ns).write_vtu(fd, cuda(x), subdomain=3, binary=True)
    (nph, nch, H), (npd, ncd, D) = _read_vtu(fh), _read_vtu(fd)
    assert (nph, nch) == (npd, ncd) == (289 * 9, 289)
    assert list(H) == list(D)  # the same arrays in the same order
    for n in ("connectivity", "offsets", "types", "subdomain", "points"):
        assert H[n].dtype == D[n].dtype and H[n].tobytes() == D[n].tobytes(), n
    compare({n: D[n] for n in FIELDS}, {n: H[n] for n in FIELDS}, patch_gradients(p, x, ns), "file")
