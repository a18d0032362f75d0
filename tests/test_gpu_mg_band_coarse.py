"""GPU: the hierarchy multigrid's coarsest-level LU in band storage (gls_mg_params.coarse_direct = 2) against the
FP64 dense LU (coarse_direct = 1) on the same hierarchy: the Q2-Q1 cylinder shell 1 : 0.25 : 1 : 8 : 2 at refinement
1 (4560 DoFs) above its refinement-0 level, ILU(0) smoothing, the coarsest level probed through its ILU CSR. The
band route solves the same pinned matrix rounded to FP32 (check |A x - 1| / |1| printed with GLS_MG_VERBOSE), so the
preconditioned GMRES takes the same number of iterations (+- 1) and reaches the same solution."""
import ctypes

import numpy as np
import pytest

from gpu_util import context_for, cuda
from tests import vanka_ref as vr


def shell(coarse_direct, coarse_ilu=False):
    probs, xfer, _ = vr.shell_hierarchy("steady")
    ctxs = [context_for(q) for q in probs]
    if coarse_ilu:  # an ILU of the level's own: the multigrid probes such a level column by column
        ctxs[1].attach_ilu()
    ctxs[0].attach_multigrid_transfers(ctxs[1:], [xfer], pre_smooth=1, post_smooth=1, omega=0.6,
                                       coarse_direct=coarse_direct, smoother="ilu")
    ctxs[0].set_state(*[cuda(a) for a in vr.state("shell-q2q1", "steady")])
    return probs, ctxs, xfer


def rhs_of(probs, ctx):
    rng = np.random.default_rng(vr.SEED + 2)
    xt = rng.uniform(-1, 1, probs[0].n_dofs)
    xt[np.nonzero(probs[0].constrained)[0]] = 0.0
    return ctx.jacobian_apply(cuda(xt))  # consistent (enclosed flow: the pressure has a gauge)


def library_log(capfd):
    ctypes.CDLL(None).fflush(None)  # the library's printf lines (stdout is a pipe under pytest: block-buffered)
    return capfd.readouterr().out


@pytest.mark.gpu
def test_band_coarse_solve_matches_dense(monkeypatch, capfd):
    out, logs = {}, {}
    for cd in (1, 2):
        monkeypatch.setenv("GLS_MG_VERBOSE", "1")
        probs, ctxs, _ = shell(cd)
        rhs = rhs_of(probs, ctxs[0])
        x8, its, res, ok = ctxs[0].solve_linear(rhs, ctxs[0].zeros(), max_iterations=200, restart=50, relative_residual=1e-8,
                                                minimum_residual=1e-300, true_residual=True)
        monkeypatch.delenv("GLS_MG_VERBOSE")
        logs[cd] = library_log(capfd)
        assert ok and res <= 1e-8 * float(rhs.norm()) * 1.01, (cd, its, res)
        info = ctxs[0].mg_coarse_info()
        # the solutions are compared where test_umesh_multigrid_linear_solve compares them: both at residual 1e-11
        x11, its11, res11, ok11 = ctxs[0].solve_linear(rhs, ctxs[0].zeros(), max_iterations=400, restart=50,
                                                      relative_residual=1e-11, minimum_residual=1e-300, true_residual=True)
        assert ok11 and res11 <= 1e-11 * float(rhs.norm()) * 1.01, (cd, its11, res11)
        out[cd] = (x8.cpu().numpy(), its, x11.cpu().numpy(), its11, info)
    p = probs[0]
    nvd = p.dim * p.n_vnodes
    info = out[2][4]
    band_lines = [l for l in logs[2].splitlines() if "band storage" in l]
    checks = [l for l in logs[2].splitlines() if "band LU" in l and "check" in l]
    d8 = np.abs(out[2][0][:nvd] - out[1][0][:nvd]).max()
    d11 = np.abs(out[2][2][:nvd] - out[1][2][:nvd]).max()
    scale = max(1.0, np.abs(out[1][2][:nvd]).max())
    print("band coarse solve: coarsest %d DoFs %s; GMRES its dense %d / band %d (1e-8), %d / %d (1e-11); velocity "
          "difference %.2e (1e-8) %.2e (1e-11), scale %.2e\n  %s\n  %s" %
          (probs[1].n_dofs, info, out[1][1], out[2][1], out[1][3], out[2][3], d8, d11, scale, band_lines, checks))
    assert band_lines and "band storage" not in logs[1], (band_lines, logs[1][-1000:])
    assert all(w in band_lines[0] for w in ("n=%d" % probs[1].n_dofs, "bl=", "bu=", "nb=", "blocks=", "bytes=")), band_lines
    assert checks, logs[2][-2000:]
    assert info["storage"] == "band" and info["n"] == probs[1].n_dofs and out[1][4]["storage"] == "dense"
    assert info["nb"] >= max(info["bl"], info["bu"], 1) and info["bytes"] == 4 * 3 * info["n"] * info["nb"], info
    assert abs(out[2][1] - out[1][1]) <= 1, (out[1][1], out[2][1])
    assert d11 < 1e-6 * scale, (d11, scale)


@pytest.mark.gpu
def test_band_refused_on_brick_hierarchy_keeps_the_multigrid():
    """gls_mg_attach's nested brick levels are probed by the brick kernel, not through a CSR: coarse_direct = 2 is
    GLS_EINVAL before anything is detached"""
    import torch
    from softx_2020_200_amd import GLSError, hyper_cube
    from softx_2020_200_amd.problem import build_context, dirichlet_from_bcs
    ctxs = []
    for m in (4, 2):
        mesh = hyper_cube(3, m, 2, 2, -1.0, 1.0)
        mask, dofs, vals = dirichlet_from_bcs(mesh, m, -1.0, 1.0, True, [("noslip", b, None) for b in range(6)])
        ctx = build_context(mesh, viscosity=0.01, vnode_mask=mask)
        ctx.set_dirichlet(dofs, vals)
        ctxs.append(ctx)
    assert ctxs[1].uses_brick_kernels
    ctxs[0].set_time("bdf2", (0.01,) * 4)
    rng = np.random.default_rng(vr.SEED)
    U = cuda(0.1 * rng.uniform(-1, 1, ctxs[0].n_dofs))
    ctxs[0].apply_dirichlet(U)
    v = cuda(rng.uniform(-1, 1, ctxs[0].n_dofs))
    ctxs[0].attach_multigrid(ctxs[1:], pre_smooth=1, post_smooth=1, omega=0.9, coarse_direct=1)
    ctxs[0].set_state(U, U, U)
    z1 = ctxs[0].apply_preconditioner(v).clone()
    with pytest.raises(GLSError, match=r"\(-1\).*band storage.*brick"):
        ctxs[0].attach_multigrid(ctxs[1:], pre_smooth=1, post_smooth=1, omega=0.9, coarse_direct=2)
    assert ctxs[0].mg_coarse_info()["storage"] == "dense" and ctxs[0].mg_coarse_info()["n"] == ctxs[1].n_dofs
    z2 = ctxs[0].apply_preconditioner(v)
    assert torch.equal(z1, z2)


@pytest.mark.gpu
def test_band_refused_on_column_probed_level_keeps_the_multigrid():
    """a coarsest level with an ILU of its own is probed one J.v per column: no CSR to fill the panels from"""
    import torch
    from softx_2020_200_amd import GLSError
    probs, ctxs, xfer = shell(1, coarse_ilu=True)
    v = cuda(np.random.default_rng(vr.SEED).uniform(-1, 1, probs[0].n_dofs))
    z1 = ctxs[0].apply_preconditioner(v).clone()
    with pytest.raises(GLSError, match=r"\(-1\).*band storage.*column by column"):
        ctxs[0].attach_multigrid_transfers(ctxs[1:], [xfer], pre_smooth=1, post_smooth=1, omega=0.6, coarse_direct=2,
                                           smoother="ilu")
    assert ctxs[0].mg_coarse_info()["storage"] == "dense"
    z2 = ctxs[0].apply_preconditioner(v)
    assert torch.equal(z1, z2)


def has_ilu(ctx):
    import ctypes as C
    ctx.L.gls_ilu_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    return ctx.L.gls_ilu_info(ctx.h, None, None) >= 0


@pytest.mark.gpu
def test_band_refused_when_the_panels_do_not_fit(monkeypatch):
    """the panels plus the CSR above the memory limit (half of the free device memory; GLS_MG_BAND_MAX_BYTES lowers it
    here): GLS_EINVAL with the byte count and the limit. Panels that cannot fit at any block width are refused before
    the detach (the context keeps its multigrid); the exact count needs the probing ILU and comes after it, and leaves
    nothing half attached. With the cap lifted the band route attaches"""
    import torch
    from softx_2020_200_amd import GLSError
    probs, ctxs, xfer = shell(1)
    v = cuda(np.random.default_rng(vr.SEED).uniform(-1, 1, probs[0].n_dofs))
    z1 = ctxs[0].apply_preconditioner(v).clone()
    monkeypatch.setenv("GLS_MG_BAND_MAX_BYTES", "1000")  # not even the narrowest block
    with pytest.raises(GLSError, match=r"\(-1\).*needs at least \d+ bytes of panels .* above the limit of 1000 "):
        ctxs[0].attach_multigrid_transfers(ctxs[1:], [xfer], pre_smooth=1, post_smooth=1, omega=0.6, coarse_direct=2,
                                           smoother="ilu")
    assert ctxs[0].mg_coarse_info()["storage"] == "dense" and ctxs[0].mg_coarse_info()["n"] == probs[1].n_dofs
    assert torch.equal(z1, ctxs[0].apply_preconditioner(v))
    nb = 512  # the 768-DoF level's bandwidths (337) round up to the minimum block
    panels = 4 * 3 * probs[1].n_dofs * nb
    monkeypatch.setenv("GLS_MG_BAND_MAX_BYTES", str(panels))  # the panels alone fit, the CSR on top does not
    with pytest.raises(GLSError, match=r"\(-1\).*needs %d bytes of panels \+ \d+ of CSR, above the limit of %d " % (panels, panels)):
        ctxs[0].attach_multigrid_transfers(ctxs[1:], [xfer], pre_smooth=1, post_smooth=1, omega=0.6, coarse_direct=2,
                                           smoother="ilu")
    # detached as a whole: no direct solve, no smoother or probing ILU left on either level
    assert ctxs[0].mg_coarse_info()["n"] == 0 and not has_ilu(ctxs[0]) and not has_ilu(ctxs[1])
    monkeypatch.delenv("GLS_MG_BAND_MAX_BYTES")
    ctxs[0].attach_multigrid_transfers(ctxs[1:], [xfer], pre_smooth=1, post_smooth=1, omega=0.6, coarse_direct=2,
                                       smoother="ilu")
    assert ctxs[0].mg_coarse_info()["storage"] == "band" and ctxs[0].mg_coarse_info()["bytes"] == panels


@pytest.mark.gpu
def test_detach_and_reattach_with_band_factorization_in_flight(monkeypatch):
    """the band factorization's check reads the probing ILU's CSR, which belongs to the coarsest level's context and
    is released by gls_mg_detach: the detach (and the one inside every attach) joins the worker and drains its stream
    first. Prepared (gls_mg_residual_restrict queues the factorization, nothing waits for it), then detached;
    attached and prepared again, then attached over it; the last hierarchy solves as a fresh one does. Run with
    GLS_MG_BAND_BLOCK = 384 (the 768-DoF level's bandwidths are 337): n = 2 nb exactly, where the other tests of this
    file take the automatic 512 with a partial last block"""
    import torch
    monkeypatch.setenv("GLS_MG_BAND_BLOCK", "384")
    probs, ctxs, xfer = shell(2)
    assert ctxs[0].mg_coarse_info()["nb"] == 384
    kw = dict(pre_smooth=1, post_smooth=1, omega=0.6, coarse_direct=2, smoother="ilu")
    x = torch.zeros(probs[0].n_dofs, dtype=torch.float64, device="cuda")
    bc = torch.zeros(probs[1].n_dofs, dtype=torch.float64, device="cuda")
    ctxs[0].mg_residual_restrict(0, x, x.clone(), bc)
    ctxs[0].detach_multigrid()
    assert ctxs[0].mg_coarse_info()["n"] == 0 and not has_ilu(ctxs[1])
    ctxs[0].attach_multigrid_transfers(ctxs[1:], [xfer], **kw)
    ctxs[0].mg_residual_restrict(0, x, x.clone(), bc)
    ctxs[0].attach_multigrid_transfers(ctxs[1:], [xfer], **kw)
    rhs = rhs_of(probs, ctxs[0])
    _, its, res, ok = ctxs[0].solve_linear(rhs, ctxs[0].zeros(), max_iterations=200, restart=50, relative_residual=1e-8,
                                           minimum_residual=1e-300, true_residual=True)
    _, fresh, _ = shell(2)
    _, its_f, _, ok_f = fresh[0].solve_linear(rhs_of(probs, fresh[0]), fresh[0].zeros(), max_iterations=200, restart=50,
                                              relative_residual=1e-8, minimum_residual=1e-300, true_residual=True)
    torch.cuda.synchronize()
    assert ok and ok_f and res <= 1e-8 * float(rhs.norm()) * 1.01 and its == its_f, (its, its_f, res)


@pytest.mark.gpu
def test_destroy_with_band_factorization_in_flight():
    """test_destroy_with_coarse_factorization_in_flight on the band route: the hierarchy prepared
    (gls_mg_residual_restrict queues the panels' fill and hands the block LU to the worker thread, without the coarse
    solve that waits for it) and its contexts destroyed at once: the worker is joined and its stream drained before
    the panels are freed, and the process goes on to a fresh context with a finite residual"""
    import torch
    probs, ctxs, _ = shell(2)
    assert ctxs[0].mg_coarse_info()["storage"] == "band"
    x = torch.zeros(probs[0].n_dofs, dtype=torch.float64, device="cuda")
    ctxs[0].mg_residual_restrict(0, x, x.clone(), torch.zeros(probs[1].n_dofs, dtype=torch.float64, device="cuda"))
    for c in ctxs:
        c.close()
    q = vr.problem("box-q2q1", "steady")
    small = context_for(q)
    small.set_state(*[cuda(a) for a in vr.state("box-q2q1", "steady")])
    r = small.residual()
    torch.cuda.synchronize()
    assert r.numel() == q.n_dofs and bool(torch.isfinite(r).all())
