"""numpy restatement (FP64) of the multigrid V-cycle on nested subdivided hyper_rectangles (gls_mg_attach_box), for
tests/test_box_vcycle_ref.py and tests/test_gpu_box.py. The cycle itself is tests/vcycle_ref.py's Cycle; what is
restated here is what the box changes: the levels are oracle.StructuredProblem.from_refined on the arrays of the
library's mesh builder (gls_mesh_hyper_rectangle: per-axis cell counts and sizes, tile-Morton bricks, wrapped node
lattice on a periodic axis), no-slip on the faces of the open directions, and the prolongation evaluates the coarse
Lagrange basis at the fine node coordinates per axis, the coarse node index taken modulo the lattice on a periodic axis.
Nothing is read from the device and none of the library's tap tables are used.

Cases: 8 x 4 x 4 -> 4 x 2 x 2 cells on the box 0 : (2, 1, 1), Q2-Q2, the coarsest level solved directly with the first
pressure DoF pinned; "open" (all six faces walls) and "x" (periodic in x, walls in y and z). State: a smooth field
of period 2 in x with histories of amplitude 0.97 and 0.94; BDF2, nu = 0.01, dt = 0.1; V(1,1), omega 0.9."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import vcycle_ref as vr

P1, P2 = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0)
NU, DT = 0.01, 0.1
SWEEPS, OMEGA = (1, 1), 0.9
K = 2
LEVELS = ((8, 4, 4), (4, 2, 2))
CASES = {"open": dict(periodic=()), "x": dict(periodic=(0,))}


def lattice_shape(cells, deg, periodic):
    return [deg * cells[d] if d in periodic else deg * cells[d] + 1 for d in range(3)]


def lattice_coords(cells, deg, periodic, p1=P1, p2=P2):
    shape = lattice_shape(cells, deg, periodic)
    ijk = np.indices(tuple(shape[::-1])).reshape(3, -1)[::-1].T
    return np.asarray(p1) + ijk * ((np.asarray(p2) - np.asarray(p1)) / (deg * np.asarray(cells)))


def box_problem(cells, k, periodic, p1=P1, p2=P2, scheme="bdf2", time_steps=(DT,) * 4, viscosity=NU, walls=True):
    """the oracle's problem on the mesh builder's arrays: cells in the builder's order, explicit node coordinates, and
    (walls) every velocity component fixed to 0 on the faces of the directions that are not periodic"""
    from oracle.oracle import StructuredProblem
    from softx_2020_200_amd.native import mesh_hyper_rectangle
    mesh = mesh_hyper_rectangle(cells, p1, p2, k, periodic_mask=sum(1 << d for d in periodic))
    mesh["vnode_x"] = lattice_coords(cells, k, periodic, p1, p2)
    p = StructuredProblem.from_refined(mesh, viscosity=viscosity, scheme=scheme, time_steps=time_steps)
    p.cells, p.periodic, p.p1, p.p2 = tuple(cells), tuple(periodic), tuple(p1), tuple(p2)
    p.vshape = lattice_shape(cells, k, periodic)
    p.pshape = lattice_shape(cells, k, periodic)
    assert p.n_vnodes == int(np.prod(p.vshape))
    if walls:
        ijk = np.indices(tuple(p.vshape[::-1])).reshape(3, -1)[::-1].T
        wall = np.zeros(p.n_vnodes, dtype=bool)
        for d in range(3):
            if d not in periodic:
                wall |= (ijk[:, d] == 0) | (ijk[:, d] == p.vshape[d] - 1)
        dofs = (np.nonzero(wall)[0][:, None] * 3 + np.arange(3)[None]).reshape(-1)
        p.constrained[dofs] = 1
        p.dirichlet = {int(d): 0.0 for d in dofs}
    return p


def lattice_prolongation(cells_c, deg, periodic, X, p1=P1, p2=P2):
    """CSR [len(X), coarse nodes]: the degree-deg Lagrange basis of the coarse box's cells at the points X; the coarse
    node of local index a in cell ci is (ci deg + a) modulo the coarse lattice (the modulo acts on periodic axes only)"""
    shape_c = lattice_shape(cells_c, deg, periodic)
    hc = (np.asarray(p2) - np.asarray(p1)) / np.asarray(cells_c)
    t = (np.asarray(X, dtype=np.float64) - np.asarray(p1)) / hc
    ci = np.clip(np.floor(t + 1e-12).astype(np.int64), 0, np.asarray(cells_c) - 1)
    xi = t - ci
    B = [vr.lagrange_1d(deg, xi[:, d]) for d in range(3)]
    loc = np.indices((deg + 1,) * 3).reshape(3, -1)[::-1].T
    rows, cols, vals = [], [], []
    for a in range(loc.shape[0]):
        w = np.prod([B[d][:, loc[a, d]] for d in range(3)], axis=0)
        w[np.abs(w) < 1e-13] = 0.0  # the nested nodes' exact zeros
        node = np.zeros(len(t), dtype=np.int64)
        st = 1
        for d in range(3):
            node += ((ci[:, d] * deg + loc[a, d]) % shape_c[d]) * st
            st *= shape_c[d]
        nz = np.nonzero(w)[0]
        rows.append(nz)
        cols.append(node[nz])
        vals.append(w[nz])
    P = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(len(t), int(np.prod(shape_c)))).tocsr()
    P.sum_duplicates()
    # the weights are the dyadic products of 1, 3/8, 3/4, -1/8 (k = 2) or 1, 1/2 (k = 1): rounded to them exactly
    P.data = np.round(P.data * 512.0) / 512.0
    P.eliminate_zeros()
    P.sort_indices()
    return P


def prolongation(cells_f, cells_c, k, periodic, p1=P1, p2=P2):
    Pv = lattice_prolongation(cells_c, k, periodic, lattice_coords(cells_f, k, periodic, p1, p2), p1, p2)
    P = sp.block_diag([sp.kron(Pv, sp.identity(3)), Pv]).tocsr()
    P.eliminate_zeros()
    P.sort_indices()
    return P


def smooth_state(p, amp):
    """a smooth field of period 2 in x at the nodes, amplitude amp, not constrained (a Jacobian is taken at any state)"""
    x, y, z = p.vnode_coords().T
    a, pi = amp, np.pi
    vel = np.stack([a * np.cos(pi * x) * np.sin(pi * y) * np.cos(pi * z), -a * np.sin(pi * x) * np.cos(pi * y) * np.cos(pi * z),
                    0.3 * a * np.sin(2 * pi * x) * np.sin(pi * y) * np.sin(pi * z)], 1)
    pr = -a * a / 16.0 * (np.cos(2 * pi * x) + np.cos(2 * pi * y)) * (np.cos(2 * pi * z) + 2.0)
    return np.concatenate([vel.reshape(-1), pr])


@functools.lru_cache(maxsize=None)
def operators(name):
    """vcycle_ref.operators' dict for a box case: H (probs, P, inj, con), state, A, D per level"""
    from oracle.oracle import Oracle
    per = CASES[name]["periodic"]
    probs = [box_problem(c, K, per) for c in LEVELS]
    P = [prolongation(LEVELS[0], LEVELS[1], K, per)]
    H = dict(probs=probs, P=P, inj=[vr.injection(P[0])], con=[np.nonzero(p.constrained)[0] for p in probs], key=name)
    st = [tuple(smooth_state(probs[0], a) for a in (1.0, 0.97, 0.94))]
    u, u1, u2 = (a[H["inj"][0]].copy() for a in st[0])
    probs[1].apply_nonzero_constraints(u)
    st.append((u, u1, u2))
    A = [Oracle(p).matrix_and_rhs(*s)[0].tocsr() for p, s in zip(probs, st)]
    for a in A:
        a.sort_indices()
    return dict(H=H, state=st, A=A, D=[a.diagonal() for a in A])


def cycle(name):
    return vr.Cycle(operators(name), [SWEEPS], OMEGA, vr.DIRECT)


@functools.lru_cache(maxsize=None)
def reference(name):
    ops = operators(name)
    z = cycle(name)(vr.rhs_vector(ops["A"][0].shape[0]))
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def coarse_condition(name):
    ops = operators(name)
    return float(np.linalg.cond(vr.pinned_coarse_matrix(ops["A"][-1], ops["H"]["probs"][-1])[0]))


def bound(name):
    """vcycle_ref.bounds' FP64 rule: max(1e-12, kappa eps), kappa = cond of the pinned coarsest matrix"""
    return max(vr.FP64_TOL, coarse_condition(name) * vr.EPS)


def gmres_problem(name):
    """a consistent right-hand side A x_t (an enclosed or periodic box's matrix is singular in the pressure constant)
    for a seeded x_t that vanishes on the constrained rows"""
    ops = operators(name)
    A = ops["A"][0]
    xt = np.random.default_rng(vr.SEED + 2).uniform(-1, 1, A.shape[0])
    xt[ops["H"]["con"][0]] = 0.0
    return A, xt, A @ xt


@functools.lru_cache(maxsize=None)
def gmres_iterations(name, rel=1e-8):
    from tests.vanka_ref import gmres_right
    A, _, b = gmres_problem(name)
    return gmres_right(A, cycle(name), b, rel, restart=30, max_it=200)[1]


@functools.lru_cache(maxsize=None)
def jacobi_gmres_iterations(name, rel=1e-8):
    """the same system with the point-Jacobi preconditioner (what the V-cycle has to beat)"""
    from tests.vanka_ref import gmres_right
    A, _, b = gmres_problem(name)
    d = operators(name)["D"][0]
    return gmres_right(A, lambda v: v / d, b, rel, restart=30, max_it=2000)[1]
