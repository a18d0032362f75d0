"""numpy restatement of the additive cell-Vanka smoother from the oracle's matrices, for tests/test_vanka_maps.py and
tests/test_gpu_vanka.py (no device code, nothing of the library but the host-only mesh helpers):

  x <- x + omega D_m^-1 sum_c R_c^T A_c^-1 R_c (b - A x),  A_c = R_c A R_c^T

with A the oracle's assembled, constraint-eliminated Jacobian (Oracle.matrix_and_rhs), the two-level cycle the
multigrid runs around it (pre-sweeps from 0, P^T restriction with the constrained coarse rows zeroed, the coarse
matrix with the first pressure DoF pinned solved exactly, prolongation with the constrained fine rows zeroed,
post-sweeps) and a right-preconditioned GMRES. Everything is cached per case: the references are computed once."""
import ctypes as C
import functools

import numpy as np

SEED = 20200200
CASES = ("box-q2q1", "box-q2q2", "shell-q2q1", "periodic-q2q1")
SCHEMES = ("steady", "bdf2")
TS = (0.05, 0.06, 0.05, 0.05)


def shell_level(sp, nu, scheme):
    from oracle.oracle import MappedProblem
    p = MappedProblem(sp, viscosity=nu, scheme=scheme, time_steps=TS)
    bids = int(np.bitwise_or.reduce(sp["vnode_bid"].astype(np.int64)))
    p.set_dirichlet([("noslip", b, None) for b in range(32) if (bids >> b) & 1])
    return p


@functools.lru_cache(maxsize=None)
def shell_hierarchy(scheme="steady"):
    """the cylinder shell 1 : 0.25 : 1 : 8 : 2 at refinement 1 (128 mapped Q2-Q1 cells, 4560 DoFs) above its
    refinement-0 level: (problems, transfer (off, col, w, inject), fine velocity / pressure node coordinates)"""
    from softx_2020_200_amd.native import UMesh
    m = UMesh(3, "cylinder_shell", "1 : 0.25 : 1 : 8 : 2")
    m.refine_global(1)
    hf = m.fe_space_handle(2, 1, qmapping_all=True)
    hc = m.coarsen_to(0).fe_space_handle(2, 1, qmapping_all=True)
    probs = [shell_level(h.data, 1.0, scheme) for h in (hf, hc)]
    assert probs[0].n_cells == 128 and probs[0].n_dofs == 4560, (probs[0].n_cells, probs[0].n_dofs)
    return probs, hf.mg_transfer_from(hc), (np.array(hf.data["vnode_x"]), np.array(hf.data["pnode_x"]))


@functools.lru_cache(maxsize=None)
def problem(case, scheme):
    from oracle.oracle import StructuredProblem
    if case == "shell-q2q1":
        return shell_hierarchy(scheme)[0][0]
    if case == "periodic-q2q1":  # 3 cells wide and periodic in x: the patches wrap around, no cell holds a node twice
        p = StructuredProblem(3, 3, k=2, kp=1, viscosity=0.05, scheme=scheme, time_steps=TS, periodic=(0,), colorize=True)
        p.set_dirichlet([("noslip", b, None) for b in (2, 3, 4, 5)])
        return p
    kp = 1 if case == "box-q2q1" else 2
    p = StructuredProblem(3, 3, k=2, kp=kp, viscosity=0.05, scheme=scheme, time_steps=TS)
    p.set_dirichlet([("noslip", 0, None)])
    return p


@functools.lru_cache(maxsize=None)
def state(case, scheme, seed=SEED):
    """u, u1, u2: seeded U(-1, 1) vectors (the history is read by bdf2 only)"""
    p = problem(case, scheme)
    rng = np.random.default_rng(seed)
    return tuple(rng.uniform(-1, 1, p.n_dofs) for _ in range(3))


@functools.lru_cache(maxsize=None)
def smooth_state(scheme):
    """the shell's smooth rotating state (the CPU experiment's kind of state, profiles/r06_fine_smoother_experiment.txt)
    with the boundary values applied; the history (bdf2) slightly behind it"""
    probs, _, (Xv, Xp) = shell_hierarchy(scheme)
    u = np.concatenate([np.stack([-Xv[:, 1], Xv[:, 0], 0.3 * np.sin(3 * Xv[:, 2])], 1).reshape(-1), np.cos(Xp[:, 0])])
    probs[0].apply_nonzero_constraints(u)
    return u, 0.98 * u, 0.95 * u


def cell_dofs_of(p):
    nv = p.cell_vnodes.shape[1]
    v = (p.cell_vnodes[:, :, None].astype(np.int64) * p.dim + np.arange(p.dim)[None, None, :]).reshape(p.n_cells, nv * p.dim)
    return np.concatenate([v, p.dim * p.n_vnodes + p.cell_pnodes.astype(np.int64)], 1)


def oracle_element_matrices(p, u, u1, u2):
    from oracle.oracle import _dp, lib
    L = lib()
    nd = cell_dofs_of(p).shape[1]
    P = p.struct()
    z = np.zeros(p.n_dofs)
    K = np.zeros((p.n_cells, nd, nd))
    Fe = np.zeros(nd)
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (u, u1, u2)]
    for c in range(p.n_cells):
        assert L.gls_oracle_local_system(C.byref(P), c, _dp(a[0]), _dp(a[1]), _dp(a[2]), _dp(z), _dp(K[c]), _dp(Fe)) == 0
    return K


def oracle_matrix(p, u, u1, u2):
    from oracle.oracle import Oracle
    return Oracle(p).matrix_and_rhs(u, u1, u2)[0].tocsr()


def patches_of(A, cd):
    return np.stack([A[d][:, d].toarray() for d in cd])


@functools.lru_cache(maxsize=None)
def reference(case, scheme, seed=SEED):
    """dict of the case's oracle data at the seeded state (seed None: the shell's smooth state): K, A (csr), cell_dofs,
    mult, patches, their FP64 inverses"""
    p = problem(case, scheme)
    u, u1, u2 = state(case, scheme, seed) if seed is not None else smooth_state(scheme)
    cd = cell_dofs_of(p)
    A = oracle_matrix(p, u, u1, u2)
    Ac = patches_of(A, cd)
    return dict(p=p, K=oracle_element_matrices(p, u, u1, u2), A=A, cell_dofs=cd, mult=np.bincount(cd.reshape(-1), minlength=p.n_dofs),
                patches=Ac, inv=np.linalg.inv(Ac))


def sweep(A, inv, cd, mult, x, b, omega, fp32=False):
    """one sweep; fp32: the inverses and the cell residuals rounded to FP32 and multiplied in FP32, as the device does"""
    r = b - A @ x
    rc = r[cd]
    if fp32:
        e = np.einsum("cij,cj->ci", inv.astype(np.float32), rc.astype(np.float32)).astype(np.float64)
    else:
        e = np.einsum("cij,cj->ci", inv, rc)
    corr = np.zeros_like(x)
    np.add.at(corr, cd.reshape(-1), e.reshape(-1))
    return x + omega * corr / np.maximum(mult, 1)


def inverse_defect(patches, inv32):
    """max |A_c^-1 (FP32) A_c (FP64) - I| over the cells' entries, the product in FP64"""
    n = patches.shape[1]
    return float(np.abs(np.einsum("cij,cjk->cik", inv32.astype(np.float64), patches) - np.eye(n)[None]).max())


@functools.lru_cache(maxsize=None)
def two_level(scheme, seed=None):
    """the shell's two-level data: fine / coarse matrices at the smooth state (or the seeded one) and its injection,
    P, the constrained rows, the coarse inverse with the first pressure DoF pinned"""
    import scipy.sparse as sp
    probs, (off, col, w, inj), _ = shell_hierarchy(scheme)
    pf, pc = probs
    st = state("shell-q2q1", scheme, seed) if seed is not None else smooth_state(scheme)
    ref = reference("shell-q2q1", scheme, seed)
    P = sp.csr_matrix((np.asarray(w), np.asarray(col), np.asarray(off)), shape=(pf.n_dofs, pc.n_dofs))
    sc = [np.asarray(s)[np.asarray(inj)].copy() for s in st]
    pc.apply_nonzero_constraints(sc[0])
    Ac = oracle_matrix(pc, *sc).toarray()
    pin = pc.dim * pc.n_vnodes
    Ac[pin, :] = 0.0
    Ac[:, pin] = 0.0
    Ac[pin, pin] = 1.0
    Aci = np.linalg.inv(Ac)
    Aci[pin, :] = 0.0
    return dict(ref=ref, P=P, Aci=Aci, con_f=np.nonzero(pf.constrained)[0], con_c=np.nonzero(pc.constrained)[0])


def vcycle(T, b, pre, post, omega, fp32=False):
    ref = T["ref"]
    A, inv, cd, mult = ref["A"], ref["inv"], ref["cell_dofs"], ref["mult"]
    x = np.zeros_like(b)
    for _ in range(pre):
        x = sweep(A, inv, cd, mult, x, b, omega, fp32)
    bc = T["P"].T @ (b - A @ x)
    bc[T["con_c"]] = 0.0
    y = T["P"] @ (T["Aci"] @ bc)
    y[T["con_f"]] = 0.0
    x = x + y
    for _ in range(post):
        x = sweep(A, inv, cd, mult, x, b, omega, fp32)
    return x


def gmres_right(A, M, b, rel, restart=30, max_it=200):
    """right-preconditioned restarted GMRES from x = 0 (modified Gram-Schmidt); (x, iterations)"""
    x = np.zeros_like(b)
    tol = rel * np.linalg.norm(b)
    its = 0
    while its < max_it:
        r = b - A @ x
        beta = np.linalg.norm(r)
        if beta <= tol:
            break
        V = [r / beta]
        Z = []
        H = np.zeros((restart + 1, restart))
        done = False
        for j in range(restart):
            Z.append(M(V[j]))
            wv = A @ Z[j]
            for i in range(j + 1):
                H[i, j] = wv @ V[i]
                wv = wv - H[i, j] * V[i]
            H[j + 1, j] = np.linalg.norm(wv)
            V.append(wv / H[j + 1, j])
            its += 1
            e1 = np.zeros(j + 2)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(H[:j + 2, :j + 1], e1, rcond=None)
            if np.linalg.norm(H[:j + 2, :j + 1] @ y - e1) <= tol or its >= max_it:
                done = True
                break
        x = x + sum(yi * zi for yi, zi in zip(y, Z))
        if done:
            break
    return x, its
