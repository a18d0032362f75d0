"""numpy / scipy restatement (FP64) of the geometric multigrid V-cycle z = M^-1 v of softx_2020_200_amd/csrc/gls_mg.cpp
(mg_prepare_levels, mg_vcycle), for tests/test_vcycle_ref.py and tests/test_gpu_vcycle_reference.py. It reads nothing
from the device, imports nothing of the library and uses none of its tap tables:

  levels        oracle.StructuredProblem(3, m, k, kp, colorize=True) for m = n, n/2, ..., 2 with the case's boundary
                conditions on every level;
  P_l           (level l+1 -> l) the coarse Lagrange basis evaluated at the fine node coordinates, a scipy CSR matrix,
                built for the velocity lattice (degree k, three interleaved components) and the pressure lattice
                (degree kp), exact zeros dropped; restriction P_l^T; inj[c] = the fine DoF whose row of P_l is e_c;
  state         u, u1, u2 of level l+1 = the level-l vectors at inj, then the coarse Dirichlet values put into u only;
  operator      A_l = Oracle(p_l).matrix_and_rhs(u_l, u1_l, u2_l)[0], D_l its diagonal, con_l the constrained rows;
  cycle         x = 0; pre sweeps x += omega D^-1 (b - A x); r = b - A x; b_c = P^T r, b_c[con_c] = 0; x_c by recursion;
                y = P x_c, y[con] = 0, x += y; post sweeps;
  coarsest      coarse_sweeps damped-Jacobi sweeps from 0 with coarse_omega, or the direct solve as the device defines
                it: row and column of the first pressure DoF replaced by the identity, np.linalg.solve, x[pin] = 0.

fp32=True takes every smoother product A x (sweeps and residuals, all levels) as A.astype(float32) @ x.astype(float32)
and leaves the rest FP64: it measures how large the FP32 rounding of this algorithm is and is never what the device is
compared with. MUTATIONS are wrong variants on purpose; the CPU self-test requires each to move the result by ten
times the bound the GPU test applies. Everything is cached per case: a reference is computed once and never changed."""
import functools

import numpy as np
import scipy.sparse as sp

SEED = 20200200
EPS = 2.2e-16
FP64_TOL = 1e-12  # the project's FP64 parity tolerance (tests/test_gpu_parity.py)
FP32_FACTOR = 4.0  # device FP32 arithmetic against numpy's FP32 figure (tests/test_gpu_vanka.py)
MUTATIONS = ("omega", "tap", "nozero_c", "nopin", "nohist", "noconstrain")
DIM = 3

# name: n, k, kp, variant, fp32, (pre, post) (the device's pre_smooth -1 = no pre-smoothing is pre 0 here), omega,
# level_sweeps, coarse ("direct",) or ("sweeps", count, damping). The smallest sizes at which the paths are live:
# n = 4 has two levels (Q2 2916 -> 500 DoFs, Q1 500 -> 108), n = 8 three (the only way to an intermediate level)
V11, V22, V01 = (1, 1), (2, 2), (0, 1)
DIRECT = ("direct",)
SWEEPS = ("sweeps", 30, 0.7)


def _case(n, k, kp, variant, fp32, sweeps, omega=0.9, level_sweeps=None, coarse=DIRECT, oseen=False, general=False):
    return dict(n=n, k=k, kp=kp, variant=variant, fp32=fp32, sweeps=sweeps, omega=omega, level_sweeps=level_sweeps,
                coarse=coarse, oseen=oseen, general=general)


CASES = {
    "fp64_v11": _case(4, 2, 2, "cavity", False, V11),
    "fp64_v22": _case(4, 2, 2, "cavity", False, V22),
    "fp64_v01": _case(4, 2, 2, "cavity", False, V01),
    "fp64_q1_v11": _case(4, 1, 1, "cavity", False, V11),
    "fp64_3lev": _case(8, 2, 2, "cavity", False, V11),
    "f32_v11": _case(4, 2, 2, "cavity", True, V11),
    "f32_v22": _case(4, 2, 2, "cavity", True, V22),
    "f32_v01": _case(4, 2, 2, "cavity", True, V01),
    "f32_3lev_bench": _case(8, 2, 2, "cavity", True, V11, level_sweeps={-2: (2, 2)}),
    "f32_coarse_sweeps": _case(4, 2, 2, "cavity", True, V11, coarse=SWEEPS),
    "fp64_coarse_sweeps": _case(4, 2, 2, "cavity", False, V11, coarse=SWEEPS),
    "f32_free_face": _case(4, 2, 2, "free_face", True, V11),
    "f32_oseen_const_n4": _case(4, 2, 2, "const", True, V11, oseen=True),
    "f32_oseen_const_n8": _case(8, 2, 2, "const", True, V11, oseen=True),
    "general_q2q1_jacobi": _case(4, 2, 1, "cavity", False, V22, omega=0.6, general=True),
}
CONST_U, CONST_P = (0.3, -0.2, 0.1), 0.7


def level_sizes(n):
    out = [n]
    while out[-1] % 2 == 0 and out[-1] // 2 >= 2:
        out.append(out[-1] // 2)
    return out


def level_sweep_list(case):
    """[(pre, post)] of the smoothing levels (all but the coarsest), with the case's per-level overrides (negative
    indices count from the coarsest level, as GLSContext.attach_multigrid takes them)"""
    L = len(level_sizes(case["n"]))
    out = [tuple(case["sweeps"])] * L
    for lv, s in (case["level_sweeps"] or {}).items():
        out[lv % L] = tuple(s)
    return out[:L - 1]


def applicable_mutations(case):
    """the mutations that can move the case's result: nopin needs the direct coarse solve; the steady constant-state
    case reads no history and its state already carries the boundary values on every level, so nohist and noconstrain
    restate the same cycle there"""
    out = []
    for m in MUTATIONS:
        if m == "nopin" and case["coarse"][0] != "direct":
            continue
        if m in ("nohist", "noconstrain") and case["variant"] == "const":
            continue
        out.append(m)
    return out


# ---------------------------------------------------------------------------------------------------------------
# levels, transfers, states
# ---------------------------------------------------------------------------------------------------------------
def _lid(X):
    return np.stack([np.ones(len(X)), 0 * X[:, 0], 0 * X[:, 0]], 1)


def _const(X):
    return np.tile(np.array(CONST_U), (len(X), 1))


def level_problem(m, k, kp, variant):
    """cavity: the boundary conditions of tests/test_gpu_ilu.py::_cavity (no-slip walls, the lid y = +1 moving in x),
    BDF2 with dt 0.01; free_face: the same without face 0 (x = -1), which carries no Dirichlet rows; const: steady,
    all six faces Dirichlet at the constant velocity CONST_U"""
    from oracle.oracle import StructuredProblem
    scheme = "steady" if variant == "const" else "bdf2"
    p = StructuredProblem(DIM, m, k=k, kp=kp, viscosity=0.01, scheme=scheme, time_steps=(0.01,) * 4, colorize=True)
    if variant == "const":
        p.set_dirichlet([("function", b, _const) for b in range(6)])
    else:
        walls = [b for b in range(6) if b != 3 and not (variant == "free_face" and b == 0)]
        p.set_dirichlet([("noslip", b, None) for b in walls] + [("function", 3, _lid)])
    return p


def lattice_coords(p, deg):
    """coordinates [n, 3] of the degree-deg node lattice of problem p (x fastest)"""
    nx = deg * p.n + 1
    ijk = np.indices((nx,) * DIM).reshape(DIM, -1)[::-1].T
    return p.lo + ijk * (p.hc / deg)


def lagrange_1d(deg, x):
    """the degree-deg Lagrange basis on the equidistant nodes a / deg of [0, 1] at the points x: [len(x), deg + 1]"""
    xn = np.arange(deg + 1) / deg
    V = np.ones((len(x), deg + 1))
    for a in range(deg + 1):
        for b in range(deg + 1):
            if b != a:
                V[:, a] *= (x - xn[b]) / (xn[a] - xn[b])
    return V


def lattice_prolongation(pc, deg, X, tap=False):
    """CSR [len(X), coarse nodes]: the degree-deg Lagrange basis of the coarse problem pc's cells at the points X, in
    the vectorised form of oracle.evaluate_field (a point on a cell boundary takes the cell floor() gives, the last
    cell at the upper end). tap: the mutation, one 1D weight changed (-0.125 -> -0.12 at degree 2, 0.5 -> 0.49 at 1)"""
    n, nx = pc.n, deg * pc.n + 1
    t = (np.asarray(X, dtype=np.float64) - pc.lo) / pc.hc
    ci = np.clip(np.floor(t).astype(np.int64), 0, n - 1)
    xi = t - ci
    B = [lagrange_1d(deg, xi[:, d]) for d in range(DIM)]
    if tap:
        old, new = (-0.125, -0.12) if deg == 2 else (0.5, 0.49)
        assert any((b == old).any() for b in B)
        B = [np.where(b == old, new, b) for b in B]
    loc = np.indices((deg + 1,) * DIM).reshape(DIM, -1)[::-1].T
    rows, cols, vals = [], [], []
    for a in range(loc.shape[0]):
        w = np.prod([B[d][:, loc[a, d]] for d in range(DIM)], axis=0)
        node = np.zeros(len(t), dtype=np.int64)
        st = 1
        for d in range(DIM):
            node += (ci[:, d] * deg + loc[a, d]) * st
            st *= nx
        nz = np.nonzero(w != 0.0)[0]  # exact zeros dropped
        rows.append(nz)
        cols.append(node[nz])
        vals.append(w[nz])
    P = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(t), nx ** DIM))
    P = P.tocsr()
    P.sum_duplicates()
    P.eliminate_zeros()
    P.sort_indices()
    return P


def prolongation(pf, pc, tap=False):
    """P (level pc -> pf) on the DoF numbering [velocity node * 3 + component, 3 n_vnodes + pressure node]"""
    Pv = lattice_prolongation(pc, pc.k, lattice_coords(pf, pf.k), tap)
    Pp = lattice_prolongation(pc, pc.kp, lattice_coords(pf, pf.kp), tap)
    P = sp.block_diag([sp.kron(Pv, sp.identity(DIM)), Pp]).tocsr()
    P.eliminate_zeros()
    P.sort_indices()
    return P


def injection(P):
    """inj[c] = the fine DoF whose row of P is the unit row e_c"""
    nnz = np.diff(P.indptr)
    unit = np.nonzero(nnz == 1)[0]
    unit = unit[P.data[P.indptr[unit]] == 1.0]
    col = P.indices[P.indptr[unit]]
    inj = np.full(P.shape[1], -1, dtype=np.int64)
    inj[col] = unit
    assert (inj >= 0).all() and len(np.unique(col)) == len(col) == P.shape[1], "injection is not a bijection"
    return inj


@functools.lru_cache(maxsize=None)
def hierarchy(n, k, kp, variant):
    """dict: probs (fine first), P and inj per level pair, con per level"""
    probs = [level_problem(m, k, kp, variant) for m in level_sizes(n)]
    P = [prolongation(probs[l], probs[l + 1]) for l in range(len(probs) - 1)]
    return dict(probs=probs, P=P, inj=[injection(p) for p in P], con=[np.nonzero(p.constrained)[0] for p in probs],
                key=(n, k, kp, variant))


def fine_state(p, variant):
    """u, u1, u2 on the fine level: smooth analytic functions of the node coordinates (the histories are other
    functions, not scalings of u). The fine u does not carry the Dirichlet values (a Jacobian is taken at any state,
    as in tests/test_gpu_parity.py): injected from a fine u that did, the coarse u would carry them already on these
    nested lattices and the levels' constraining (mutation noconstrain) could not be seen. The coarse levels' u is
    constrained after the injection, the histories never. const: the constant state, pressure CONST_P"""
    Xv, Xp = lattice_coords(p, p.k), lattice_coords(p, p.kp)
    if variant == "const":
        u = np.concatenate([np.tile(np.array(CONST_U), len(Xv)), np.full(len(Xp), CONST_P)])
        return p.apply_nonzero_constraints(u.copy()), u.copy(), u.copy()
    x, y, z = Xv.T
    px, py, pz = Xp.T

    def field(a, s):
        vel = np.stack([np.sin(a * x + 0.5 * y + s) * np.cos(z), np.cos(x - a * z + s) * np.sin(1.5 * y),
                        0.5 * np.sin(a * (y + z) + s) + 0.3 * np.cos(2 * x)], 1).reshape(-1)
        return np.concatenate([vel, np.cos(a * px + s) * np.sin(py - 0.5 * pz)])
    return field(1.0, 0.0), field(1.3, 0.4), field(0.8, -0.7)


@functools.lru_cache(maxsize=None)
def operators(n, k, kp, variant, mut=None):
    """per level: the state, A (CSR), D, for the hierarchy's fine state; mut nohist / noconstrain alter the coarse
    levels' states (the other mutations do not touch the operators)"""
    from oracle.oracle import Oracle
    H = hierarchy(n, k, kp, variant)
    if mut not in ("nohist", "noconstrain"):
        mut = None
    if mut is not None:
        base = operators(n, k, kp, variant, None)
    st = [fine_state(H["probs"][0], variant)]
    A = []
    for l, p in enumerate(H["probs"]):
        if l > 0:
            u, u1, u2 = (a[H["inj"][l - 1]].copy() for a in st[l - 1])
            if mut == "nohist":
                u1, u2 = np.zeros_like(u1), np.zeros_like(u2)
            if mut != "noconstrain":
                p.apply_nonzero_constraints(u)
            st.append((u, u1, u2))
        if mut is not None and l == 0:
            A.append(base["A"][0])
            continue
        A.append(Oracle(p).matrix_and_rhs(*st[l])[0].tocsr())
    for a in A:
        a.sort_indices()
    return dict(H=H, state=st, A=A, D=[a.diagonal() for a in A])


def rhs_vector(n_dofs):
    """the vector the preconditioner is applied to: seeded U(-1, 1), non-zero on the Dirichlet rows too"""
    return np.random.default_rng(SEED).uniform(-1, 1, n_dofs)


# ---------------------------------------------------------------------------------------------------------------
# the cycle
# ---------------------------------------------------------------------------------------------------------------
def pinned_coarse_matrix(A, p):
    """dense coarsest matrix with the row and column of the first pressure DoF replaced by the identity, and that DoF"""
    pin = DIM * p.n_vnodes
    M = A.toarray()
    M[pin, :] = 0.0
    M[:, pin] = 0.0
    M[pin, pin] = 1.0
    return M, pin


class Cycle:
    """one case's cycle over fixed operators. dtype np.longdouble: every product, sum and division in extended
    precision and the coarse solve refined four times around the FP64 LU (the precision-floor self-test)"""

    def __init__(self, ops, sweeps, omega, coarse=DIRECT, fp32=False, mut=None, dtype=np.float64):
        H = ops["H"]
        self.H, self.A, self.D, self.con = H, ops["A"], ops["D"], H["con"]
        self.P = H["P"]
        if mut == "tap":
            self.P = [prolongation(H["probs"][l], H["probs"][l + 1], tap=True) for l in range(len(self.P))]
        self.sweeps, self.coarse, self.fp32, self.mut, self.dtype = list(sweeps), coarse, fp32, mut, dtype
        self.omega = omega - 0.01 if mut == "omega" else omega
        self.L = len(self.A)
        assert len(self.sweeps) == self.L - 1
        self.A32 = [a.astype(np.float32) for a in self.A] if fp32 else None
        if dtype is not np.float64:
            assert not fp32
            self.A = [a.astype(dtype) for a in self.A]
            self.P = [p.astype(dtype) for p in self.P]
            self.D = [d.astype(dtype) for d in self.D]
        if coarse[0] == "direct":
            self.M, self.pin = pinned_coarse_matrix(ops["A"][-1], H["probs"][-1])

    def Ax(self, l, x):
        if self.fp32:
            return (self.A32[l] @ x.astype(np.float32)).astype(np.float64)
        return self.A[l] @ x

    def sweep(self, l, x, b, omega):
        return x + omega * (b - self.Ax(l, x)) / self.D[l]

    def coarse_solve(self, b):
        if self.coarse[0] == "sweeps":
            _, count, om = self.coarse
            om = om - 0.01 if self.mut == "omega" else om
            x = np.zeros_like(b)
            for _ in range(count):
                x = self.sweep(self.L - 1, x, b, om)
            return x
        if self.mut == "nopin":  # the singular (enclosed flow) or unpinned matrix by least squares
            return np.linalg.lstsq(self.A[-1].toarray().astype(np.float64), b, rcond=None)[0]
        if self.dtype is np.float64:
            x = np.linalg.solve(self.M, b)
        else:
            import scipy.linalg as sla
            lu = sla.lu_factor(self.M)
            Mx = self.M.astype(self.dtype)
            x = sla.lu_solve(lu, b.astype(np.float64)).astype(self.dtype)
            for _ in range(4):
                r = b - Mx @ x
                x = x + sla.lu_solve(lu, r.astype(np.float64)).astype(self.dtype)
        x[self.pin] = 0.0
        return x

    def level(self, l, b):
        if l == self.L - 1:
            return self.coarse_solve(b)
        pre, post = self.sweeps[l]
        x = np.zeros_like(b)
        for _ in range(pre):
            x = self.sweep(l, x, b, self.omega)
        r = b - self.Ax(l, x) if pre > 0 else b.copy()
        bc = self.P[l].T @ r
        if self.mut != "nozero_c":
            bc[self.con[l + 1]] = 0.0
        y = self.P[l] @ self.level(l + 1, bc)
        y[self.con[l]] = 0.0
        x = x + y
        for _ in range(post):
            x = self.sweep(l, x, b, self.omega)
        return x

    def __call__(self, v):
        return self.level(0, np.asarray(v, dtype=self.dtype))


def case_ops(name, mut=None):
    c = CASES[name]
    return operators(c["n"], c["k"], c["kp"], c["variant"], mut if mut in ("nohist", "noconstrain") else None)


@functools.lru_cache(maxsize=None)
def reference(name, fp32=False, mut=None):
    """z = M^-1 v of the case in FP64 (fp32: its FP32 emulation; mut: a wrong variant)"""
    c = CASES[name]
    ops = case_ops(name, mut)
    z = Cycle(ops, level_sweep_list(c), c["omega"], c["coarse"], fp32=fp32, mut=mut)(rhs_vector(ops["A"][0].shape[0]))
    z.setflags(write=False)
    return z


def block_errors(name, z, ref):
    """(velocity, pressure): max |z - ref| / max |ref| over each block"""
    c = CASES[name]
    nv = DIM * (c["k"] * c["n"] + 1) ** DIM
    z, ref = np.asarray(z), np.asarray(ref)
    return tuple(float(np.abs(z[s] - ref[s]).max() / np.abs(ref[s]).max()) for s in (slice(0, nv), slice(nv, None)))


@functools.lru_cache(maxsize=None)
def coarse_condition(name):
    """kappa of the bound: cond of the pinned coarsest matrix on the direct route, 1 on the sweeps route"""
    c = CASES[name]
    if c["coarse"][0] != "direct":
        return 1.0
    ops = case_ops(name)
    return float(np.linalg.cond(pinned_coarse_matrix(ops["A"][-1], ops["H"]["probs"][-1])[0]))


@functools.lru_cache(maxsize=None)
def bounds(name):
    """the per-block bounds (velocity, pressure) the GPU test applies, from the reference alone. FP64 smoothing:
    max(1e-12, kappa eps), the forward error of a backward-stable coarse solve; FP32 smoothing: 4 x the distance of
    the reference's FP32 emulation from the FP64 reference"""
    c = CASES[name]
    if not c["fp32"]:
        b = max(FP64_TOL, coarse_condition(name) * EPS)
        return (b, b)
    e32 = block_errors(name, reference(name, fp32=True), reference(name))
    return tuple(FP32_FACTOR * e for e in e32)


# ---------------------------------------------------------------------------------------------------------------
# the level pieces (one restriction, one prolongation + sweep) on a case's hierarchy
# ---------------------------------------------------------------------------------------------------------------
def piece_vectors(name, l):
    """seeded x, b (level l) and x_c (level l + 1) for the level pieces; x_c vanishes on the coarse constrained rows,
    as every coarse correction of the cycle does"""
    H = case_ops(name)["H"]
    rng = np.random.default_rng(SEED + 1 + l)
    nf, nc = H["P"][l].shape
    x, b, xc = rng.uniform(-1, 1, nf) * 1e-3, rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nc) * 1e-3
    xc[H["con"][l + 1]] = 0.0
    return x, b, xc


def residual_restrict(name, l, x, b, fp32=False):
    """P^T (b - A x) with the constrained coarse rows zeroed"""
    ops = case_ops(name)
    cy = Cycle(ops, [(1, 1)] * (len(ops["A"]) - 1), 0.9, SWEEPS, fp32=fp32)
    bc = cy.P[l].T @ (b - cy.Ax(l, x))
    bc[cy.con[l + 1]] = 0.0
    return bc


def prolong_smooth(name, l, xc, x, b, omega, fp32=False):
    """one sweep from x + P x_c (the constrained rows of P x_c zeroed)"""
    ops = case_ops(name)
    cy = Cycle(ops, [(1, 1)] * (len(ops["A"]) - 1), 0.9, SWEEPS, fp32=fp32)
    y = cy.P[l] @ xc
    y[cy.con[l]] = 0.0
    return cy.sweep(l, x + y, b, omega)
