"""GPU: the additive cell-Vanka smoother (gls_mg_params.smoother = 3, gls_vanka_*) against the oracle and a numpy
restatement built from the oracle's matrices (tests/vanka_ref.py). Meshes: the 3^3 box with no-slip faces, Q2-Q1 and
Q2-Q2 (one cell with all 26 neighbours), and the cylinder shell 1 : 0.25 : 1 : 8 : 2 at refinement 1 (128 mapped
Q2-Q1 cells, 4560 DoFs), and the 3^3 Q2-Q1 box periodic in x (the patches wrap around; no cell holds a node twice).
States: seeded U(-1, 1), seed 20200200, steady and BDF2.

Bounds measured on the CPU with numpy alone (FP64 inverses of the oracle's patches rounded to FP32), over the eight
mesh / scheme cases:
  * inverse defect max |A_c^-1(FP32) A_c - I| = 4.71e-6 (box Q2-Q2 steady; the others 7.1e-8 .. 1.2e-6): the device
    inverse may pivot differently, 4 x that = 1.9e-5 allowed;
  * one sweep, FP32 patch products against FP64 ones: 9.43e-8 relative (max-norm): 4 x that = 3.8e-7 allowed;
  * GMRES to 1e-8 on the shell's two-level cycle at the seeded state, right-hand side A x_t for a seeded x_t (the
    enclosed flow's matrix is singular in the pressure constant: a random right-hand side is inconsistent and no
    Krylov method reaches 1e-8 on it, numpy stalls at 0.6): numpy needs 15 (V(1,1), omega 0.8) / 10 (V(2,2))
    iterations steady and 13 / 8 with BDF2; + 2 allowed. The CPU experiment
    (profiles/r06_fine_smoother_experiment.txt: 14 and 11, at a smooth rotating state with a Galerkin coarse matrix;
    here the re-discretised coarse level the library builds) agrees; at that smooth state numpy gives the same
    15 / 10 / 13 / 8."""
import os

import numpy as np
import pytest

from gpu_util import context_for, cuda, relerr
from tests import vanka_ref as vr

INV_BOUND = 4 * 4.71e-6
SWEEP_BOUND = 4 * 9.43e-8
GMRES_ITS = {("steady", 1): 15, ("steady", 2): 10, ("bdf2", 1): 13, ("bdf2", 2): 8}

CASE_SCHEMES = [(c, s) for s in vr.SCHEMES for c in vr.CASES]


def ctx_at(case, scheme, seed=vr.SEED):
    p = vr.problem(case, scheme)
    ctx = context_for(p)
    assert not ctx.uses_brick_kernels
    st = [cuda(a) for a in (vr.state(case, scheme, seed) if seed is not None else vr.smooth_state(scheme))]
    ctx.set_state(*st)
    return p, ctx, st


def xb(n, seed=vr.SEED + 1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)


@pytest.mark.gpu
@pytest.mark.parametrize("case,scheme", CASE_SCHEMES)
def test_element_and_patch_matrices_and_inverses(case, scheme):
    """K_c against gls_oracle_local_system and A_c against the oracle's COO restricted to the cell's DoFs (the
    constrained rows included) at 1e-12; A_c^-1 (FP32) A_c against the identity at 4 x numpy's defect"""
    p, ctx, st = ctx_at(case, scheme)
    ref = vr.reference(case, scheme)
    K = ctx.vanka_element_matrices().cpu().numpy()
    eK = relerr(K, ref["K"])
    A, Ai = ctx.vanka_patch_inverses()
    A, Ai = A.cpu().numpy(), Ai.cpu().numpy()
    nd, ld = ctx.vanka_sizes()
    assert nd == ref["cell_dofs"].shape[1] and ld % 4 == 0 and ld >= nd and not Ai[:, :, nd:].any()
    eA = relerr(A, ref["patches"])
    con = p.constrained[ref["cell_dofs"]].astype(bool)
    assert con.any()
    rows = A[con]  # the constrained rows: the diagonal kernel's value on the diagonal, nothing else
    eC = relerr(rows, ref["patches"][con])
    defect = vr.inverse_defect(ref["patches"], Ai[:, :, :nd])
    print("vanka %s %s: K rel err %.2e, A_c %.2e (constrained rows %.2e), inverse defect %.3e (bound %.3e)" %
          (case, scheme, eK, eA, eC, defect, INV_BOUND))
    assert eK <= 1e-12 and eA <= 1e-12 and eC <= 1e-12, (eK, eA, eC)
    assert defect <= INV_BOUND, defect


@pytest.mark.gpu
@pytest.mark.parametrize("case,scheme", CASE_SCHEMES)
def test_one_sweep_matches_restatement_and_repeats_bitwise(case, scheme):
    import torch
    p, ctx, st = ctx_at(case, scheme)
    ref = vr.reference(case, scheme)
    x, b = xb(p.n_dofs)
    want = vr.sweep(ref["A"], ref["inv"], ref["cell_dofs"], ref["mult"], x, b, 0.8)
    B = cuda(b)
    got = ctx.vanka_sweep(cuda(x), B, 0.8)
    again = ctx.vanka_sweep(cuda(x), B, 0.8)
    e = relerr(got.cpu().numpy(), want)
    print("vanka sweep %s %s: rel err %.3e (bound %.3e)" % (case, scheme, e, SWEEP_BOUND))
    assert torch.equal(got, again)
    assert e <= SWEEP_BOUND, e


def attach_shell(scheme, sweeps, omega=0.8, smoother="vanka", coarse_direct=1):
    probs, xfer, _ = vr.shell_hierarchy(scheme)
    ctxs = [context_for(q) for q in probs]
    ctxs[0].attach_multigrid_transfers(ctxs[1:], [xfer], pre_smooth=sweeps, post_smooth=sweeps, omega=omega,
                                       coarse_direct=coarse_direct, smoother=smoother)
    return probs, ctxs


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,sweeps", [("steady", 1), ("steady", 2), ("bdf2", 1), ("bdf2", 2)])
def test_two_level_preconditioner_iteration_count(scheme, sweeps):
    """GMRES to 1e-8 with the V(s,s) cycle (smoother 3, omega 0.8, direct coarse solve) converges, its true residual
    recomputed from the device operator meets the tolerance, and the count is within 2 of the numpy restatement's"""
    probs, ctxs = attach_shell(scheme, sweeps)
    st = [cuda(a) for a in vr.state("shell-q2q1", scheme)]
    ctxs[0].set_state(*st)
    rng = np.random.default_rng(vr.SEED + 2)
    xt = rng.uniform(-1, 1, probs[0].n_dofs)
    xt[np.nonzero(probs[0].constrained)[0]] = 0.0
    rhs = ctxs[0].jacobian_apply(cuda(xt))  # a consistent right-hand side (enclosed flow: the pressure has a gauge)
    x, its, res, ok = ctxs[0].solve_linear(rhs, ctxs[0].zeros(), max_iterations=200, restart=30, relative_residual=1e-8,
                                           minimum_residual=1e-300, true_residual=True)
    true = float((rhs - ctxs[0].jacobian_apply(x)).norm() / rhs.norm())
    print("vanka two-level %s V(%d,%d): GMRES its %d (numpy %d), true rel residual %.2e" %
          (scheme, sweeps, sweeps, its, GMRES_ITS[(scheme, sweeps)], true))
    assert ok and true <= 1e-8 * 1.01, (its, res, true)
    assert its <= GMRES_ITS[(scheme, sweeps)] + 2, its
    ctxs[0].detach_multigrid()
    # detached: the levels carry no smoother state and Jacobi-preconditioned GMRES runs again
    _, its_j, _, _ = ctxs[0].solve_linear(rhs, ctxs[0].zeros(), max_iterations=5, restart=5, relative_residual=1e-8)
    assert its_j == 5


@pytest.mark.gpu
@pytest.mark.parametrize("coarse_direct", [1, -1])
def test_default_omega_is_0p8(coarse_direct):
    """omega = 0 in gls_mg_params takes 0.8 with smoother 3: the preconditioner's action equals the explicit one's,
    with the direct coarse solve and with the coarsest level's Jacobi sweeps (their weight defaults to 0.6 either way)"""
    import torch
    z = []
    for om in (0.0, 0.8):
        probs, ctxs = attach_shell("steady", 1, omega=om, coarse_direct=coarse_direct)
        ctxs[0].set_state(*[cuda(a) for a in vr.smooth_state("steady")])
        z.append(ctxs[0].apply_preconditioner(cuda(xb(probs[0].n_dofs)[1])))
    assert torch.equal(z[0], z[1])


@pytest.mark.gpu
def test_refresh_follows_the_state_and_freeze_keeps_the_snapshot():
    import torch
    case, scheme = "box-q2q1", "bdf2"
    p, ctx, st = ctx_at(case, scheme)
    A0, I0 = ctx.vanka_patch_inverses()
    st2 = [cuda(a) for a in vr.state(case, scheme, vr.SEED + 7)]
    ctx.set_state(*st2)
    A1, I1 = ctx.vanka_patch_inverses()
    assert not torch.equal(I0, I1)
    ref = vr.reference(case, scheme, vr.SEED + 7)
    x, b = xb(p.n_dofs)
    want = vr.sweep(ref["A"], ref["inv"], ref["cell_dofs"], ref["mult"], x, b, 0.8)
    assert relerr(ctx.vanka_sweep(cuda(x), cuda(b), 0.8).cpu().numpy(), want) <= SWEEP_BOUND
    ctx.freeze_jacobian(True)
    ctx.set_state(*st)  # moves the residual only
    A2, I2 = ctx.vanka_patch_inverses()
    assert torch.equal(I1, I2) and torch.equal(A1, A2)
    ctx.freeze_jacobian(False)
    A3, I3 = ctx.vanka_patch_inverses()
    assert torch.equal(I0, I3) and torch.equal(A0, A3)  # rebuilt at the first state: bitwise the first build


def usable(ctx, p):
    """the context still computes after a refusal"""
    import torch
    ctx.set_state(cuda(np.zeros(p.n_dofs)), cuda(np.zeros(p.n_dofs)), cuda(np.zeros(p.n_dofs)))
    assert bool(torch.isfinite(ctx.residual()).all())


@pytest.mark.gpu
def test_refusals_leave_the_context_usable():
    from oracle.oracle import StructuredProblem
    from softx_2020_200_amd.native import GLSError
    # 2D
    p2 = StructuredProblem(2, 3, k=2, kp=1)
    c2 = context_for(p2)
    c2.set_state(cuda(np.zeros(p2.n_dofs)))
    with pytest.raises(GLSError, match=r"\(-1\).*3D only"):
        c2.vanka_sweep(c2.zeros(), c2.zeros() + 1)
    usable(c2, p2)
    # a brick (pencil) context: the Q2-Q2 cube on Morton 2x2x2 bricks
    from tests.test_gpu_parity import _morton_problem
    pb = _morton_problem(2, 2, "steady", 0.1)
    cb = context_for(pb)
    assert cb.uses_brick_kernels
    cb.set_state(cuda(np.zeros(pb.n_dofs)))
    with pytest.raises(GLSError, match=r"\(-1\).*brick \(pencil\) contexts"):
        cb.vanka_patch_inverses()
    usable(cb, pb)
    # a forest context whose sibling groups run the pencil kernel: Q2-Q2 boxes after set_hanging with no lines
    cf = context_for(pb)
    cf.set_hanging(np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    assert not cf.uses_brick_kernels and cf.forest_bricks() > 0
    cf.set_state(cuda(np.zeros(pb.n_dofs)))
    with pytest.raises(GLSError, match=r"\(-1\).*sibling groups run the brick \(pencil\) kernel"):
        cf.vanka_patch_inverses()
    with pytest.raises(GLSError, match=r"\(-1\).*sibling groups run the brick \(pencil\) kernel"):
        cf.vanka_element_matrices()
    usable(cf, pb)
    # an adapted level with hanging lines, as a multigrid level: refused before anything is detached
    from tests.test_gpu_octree_mg import octree_hierarchy
    from tests.test_octree_mg import adapted_tree
    trees, probs, xfer = octree_hierarchy(adapted_tree(3, 2, 2), 2, 1, nu=0.1)
    ctxs = [context_for(q) for q in probs]
    with pytest.raises(GLSError, match=r"\(-1\).*hanging-node or slip lines"):
        ctxs[0].attach_multigrid_transfers(ctxs[1:], xfer, pre_smooth=1, post_smooth=1, omega=0.8, coarse_direct=1,
                                           smoother="vanka")
    usable(ctxs[0], probs[0])
    ctxs[0].attach_multigrid_transfers(ctxs[1:], xfer, pre_smooth=1, post_smooth=1, omega=0.6, coarse_direct=1, smoother="ilu")
    # a replica attach (the smoother is one-rank)
    p, ctx, st = ctx_at("box-q2q1", "steady")
    rep = context_for(p)
    with pytest.raises(GLSError, match=r"\(-1\).*one rank only"):
        ctx.attach_multigrid_replica(rep, np.zeros(p.n_dofs + 1, np.int64), np.zeros(1, np.int32), np.zeros(1), np.zeros(p.n_dofs, np.int64),
                                     smoother="vanka")
    usable(ctx, p)


@pytest.mark.gpu
def test_singular_patch_is_an_error_not_a_fault():
    """nu = 0 at the zero state, steady: no viscous, convective or mass term is left and the stabilisation parameter is
    not finite, so no patch can be inverted: the rebuild returns an error that names the first cell, the sweep and
    the attached hierarchy's preconditioner likewise, and the context computes again with a viscosity"""
    from softx_2020_200_amd.native import GLSError
    p = vr.problem("box-q2q1", "steady")
    ctx = context_for(p)
    z = cuda(np.zeros(p.n_dofs))
    ctx.set_viscosity(0.0)
    ctx.set_state(z, z, z)
    with pytest.raises(GLSError, match=r"patch matrix of cell 0 is singular or not finite \(27 such cells\)"):
        ctx.vanka_patch_inverses()
    with pytest.raises(GLSError, match="singular or not finite"):
        ctx.vanka_sweep(ctx.zeros(), ctx.zeros() + 1.0)
    ctx.set_viscosity(p.viscosity)
    ctx.set_state(*[cuda(a) for a in vr.state("box-q2q1", "steady")])
    ref = vr.reference("box-q2q1", "steady")
    assert relerr(ctx.vanka_patch_inverses()[0].cpu().numpy(), ref["patches"]) <= 1e-12


@pytest.mark.gpu
def test_app_taylor_couette_with_vanka_smoother(tmp_path):
    """configs[3] (the cylinder shell, Q2-Q1, slip end caps, Kelly adaptation) through the application with
    --precond hmg --mg-smoother vanka --mg-sweeps 2: the oracle pipeline checks of tests/test_gpu_app_configs.py (converged residual
    at every cycle's state, error table, Kelly marking); stderr names the smoother on the conforming first mesh and
    the fallback to the default on the adapted ones (hanging lines)"""
    from tests.test_gpu_app_configs import CASES, check_configs3_pipeline, run_app
    prm = open(os.path.join(CASES, "taylor-couette3d_q2q1_kelly.prm")).read()
    out, dumps = run_app(tmp_path, prm, extra=("--precision", "9", "--precond", "hmg", "--mg-smoother", "vanka", "--mg-sweeps", "2"))
    err = (tmp_path / "stderr.txt").read_text()
    print(err[-1500:])
    assert "V(2,2)-cycle with additive cell-Vanka smoothing on the triangulation's refinement hierarchy" in err, err[-1500:]
    assert "--mg-smoother vanka refused" in err and "hanging-node or slip lines" in err, err[-1500:]
    assert "V(2,2)-cycle with ILU(0) smoothing" in err, err[-1500:]  # --mg-sweeps holds for the fallback too
    check_configs3_pipeline(out, dumps, 1e-8)
