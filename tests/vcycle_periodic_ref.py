"""numpy restatement (FP64) of the multigrid V-cycle on nested PERIODIC hyper_cubes (gls_mg_attach_periodic), for
tests/test_mg_periodic_ref.py and tests/test_gpu_mg_periodic.py. The cycle itself is tests/vcycle_ref.py's Cycle; what
is restated here is what periodicity changes: the levels are oracle.StructuredProblem(..., periodic=...) on the box
0 : 2 pi (wrapped node lattices, make_periodicity_constraints as node identification), no-slip on the faces of the
directions that are not periodic, and the prolongation evaluates the coarse Lagrange basis at the fine node
coordinates with the coarse node index taken modulo the lattice on a periodic axis. Nothing is read from the device
and none of the library's tap tables are used.

Cases (the smallest periodic hierarchy there is: 8^3 -> 4^3 cells, Q2-Q2, the coarsest level solved directly with the
first pressure DoF pinned): "xyz" fully periodic (16384 -> 2048 DoFs), "x" periodic in x with walls in y and z.
State: the Taylor-Green field of apps/cases/tgv3d_q2q2_bdf2.prm at the nodes, with histories of amplitude 0.97 and
0.94; BDF2, nu = 0.01, dt = 0.1; V(1,1), omega 0.9."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import vcycle_ref as vr

LO, HI = 0.0, 2.0 * np.pi
NU, DT = 0.01, 0.1
SWEEPS, OMEGA = (1, 1), 0.9
CASES = {"xyz": dict(n=8, k=2, periodic=(0, 1, 2)), "x": dict(n=8, k=2, periodic=(0,))}
LEVELS = (8, 4)


def level_problem(m, k, periodic):
    from oracle.oracle import StructuredProblem
    p = StructuredProblem(3, m, k=k, kp=k, lo=LO, hi=HI, colorize=True, viscosity=NU, scheme="bdf2",
                          time_steps=(DT,) * 4, periodic=periodic)
    p.set_dirichlet([("noslip", b, None) for b in range(6) if b // 2 not in periodic])
    return p


def lattice_coords(p, deg, shape):
    ijk = np.indices(tuple(shape[::-1])).reshape(3, -1)[::-1].T
    return p.lo + ijk * (p.hc / deg)


def lattice_prolongation(pc, deg, shape_c, X):
    """CSR [len(X), coarse nodes]: the degree-deg Lagrange basis of pc's cells at the points X; the coarse node of
    local index a in cell ci is (ci deg + a) modulo the coarse lattice (the modulo acts on periodic axes only)"""
    t = (np.asarray(X, dtype=np.float64) - pc.lo) / pc.hc
    ci = np.clip(np.floor(t + 1e-12).astype(np.int64), 0, pc.n - 1)
    xi = t - ci
    B = [vr.lagrange_1d(deg, xi[:, d]) for d in range(3)]
    loc = np.indices((deg + 1,) * 3).reshape(3, -1)[::-1].T
    rows, cols, vals = [], [], []
    for a in range(loc.shape[0]):
        w = np.prod([B[d][:, loc[a, d]] for d in range(3)], axis=0)
        w[np.abs(w) < 1e-13] = 0.0  # the nested nodes' exact zeros (the coordinates carry rounding on 0 : 2 pi)
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


def prolongation(pf, pc):
    Pv = lattice_prolongation(pc, pc.k, pc.vshape, lattice_coords(pf, pf.k, pf.vshape))
    Pp = lattice_prolongation(pc, pc.kp, pc.pshape, lattice_coords(pf, pf.kp, pf.pshape))
    P = sp.block_diag([sp.kron(Pv, sp.identity(3)), Pp]).tocsr()
    P.eliminate_zeros()
    P.sort_indices()
    return P


def tgv_state(p, amp):
    """the Taylor-Green field at the nodes, amplitude amp, not constrained (a Jacobian is taken at any state)"""
    x, y, z = lattice_coords(p, p.k, p.vshape).T
    vel = np.stack([amp * np.cos(x) * np.sin(y) * np.cos(z), -amp * np.sin(x) * np.cos(y) * np.cos(z), 0 * x], 1)
    pr = -amp * amp / 16.0 * (np.cos(2 * x) + np.cos(2 * y)) * (np.cos(2 * z) + 2.0)
    return np.concatenate([vel.reshape(-1), pr])


@functools.lru_cache(maxsize=None)
def operators(name):
    """vcycle_ref.operators' dict for a periodic case: H (probs, P, inj, con), state, A, D per level"""
    from oracle.oracle import Oracle
    c = CASES[name]
    probs = [level_problem(m, c["k"], c["periodic"]) for m in LEVELS]
    P = [prolongation(probs[0], probs[1])]
    H = dict(probs=probs, P=P, inj=[vr.injection(P[0])], con=[np.nonzero(p.constrained)[0] for p in probs], key=name)
    st = [tuple(tgv_state(probs[0], a) for a in (1.0, 0.97, 0.94))]
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
def bound(name):
    """vcycle_ref.bounds' FP64 rule: max(1e-12, kappa eps), kappa = cond of the pinned coarsest matrix"""
    ops = operators(name)
    kappa = float(np.linalg.cond(vr.pinned_coarse_matrix(ops["A"][-1], ops["H"]["probs"][-1])[0]))
    return max(vr.FP64_TOL, kappa * vr.EPS)


def gmres_problem(name):
    """a consistent right-hand side A x_t (the periodic box's matrix is singular in the pressure constant) for a
    seeded x_t that vanishes on the constrained rows"""
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
