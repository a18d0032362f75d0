"""The passes GMRES and the V-cycle no longer run on their own, against the launches they replace:
- GMRES tests convergence before it projects a column, and the column at which the solve converges is not projected
  (nothing reads v_{j+1} then). GLS_GMRES_FULL_LAST_COLUMN=1 projects and repairs it as before.
- The first damped-Jacobi sweep from 0, x = 0 + omega b / D, is stored by the kernel that writes b (the restriction's
  sum on the coarse levels, the GMRES projection on the fine one). GLS_MG_FIRST_PRODUCER=0 keeps the update launches;
  the values are bitwise the same.
- GMRES takes ||b||^2 from Newton, which formed it from the same vector with the same reduction
  (GLS_GMRES_NO_NORM_REUSE=1: its own dot); bitwise too.
The switches are read per call. Hierarchies: test_gpu_mg_fused_transfers' Q2-Q2 cavities (FP32 Oseen smoothing,
V(1,1), exact LU on 2^3): 8^3 has one level whose b comes from the restriction's sum, 16^3 one that also restricts."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_mg_fused_transfers import _hier

PRODUCER, FULL_LAST, NO_NORM = "GLS_MG_FIRST_PRODUCER", "GLS_GMRES_FULL_LAST_COLUMN", "GLS_GMRES_NO_NORM_REUSE"
SKIP_LINE = "projection is skipped"


def _set(monkeypatch, **env):
    """value None: unset"""
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _flush():
    ctypes.CDLL(None).fflush(None)  # the library's printf lines (stdout is a pipe under pytest: block-buffered)


def _rhs(h):
    ctx = h.attach("v11_oseen")
    return ctx, ctx.residual().clone()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 16])
def test_vcycle_first_sweep_from_producer_is_bitwise(n, monkeypatch):
    h = _hier(n)
    ctx = h.attach("v11_oseen")
    _set(monkeypatch, **{PRODUCER: None})
    z_on = ctx.apply_preconditioner(h.v).cpu().numpy()
    _set(monkeypatch, **{PRODUCER: "0"})
    z_off = ctx.apply_preconditioner(h.v).cpu().numpy()
    assert np.abs(z_off).max() > 0
    assert np.array_equal(z_on, z_off)


def _solve_pair(ctx, b, monkeypatch, **kw):
    out = []
    for prod in (None, "0"):
        _set(monkeypatch, **{PRODUCER: prod, FULL_LAST: "1"})
        x, its, res, ok = ctx.solve_linear(b, max_iterations=200, relative_residual=1e-8, **kw)
        assert ok and its > 0, (prod, its, res)
        out.append((x.cpu().numpy(), its, res))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("repair_all", [False, True], ids=["default", "repair_every_column"])
def test_gmres_first_sweep_from_projection_is_bitwise(repair_all, monkeypatch):
    """x0 stored by the projection (and, with GLS_GMRES_REPAIR_TOL=0, always by the repair pass that follows it)."""
    ctx, b = _rhs(_hier(8))
    _set(monkeypatch, GLS_GMRES_REPAIR_TOL="0" if repair_all else None)
    (x_on, its_on, _), (x_off, its_off, _) = _solve_pair(ctx, b, monkeypatch, restart=30)
    assert its_on == its_off
    assert np.abs(x_off).max() > 0
    assert np.array_equal(x_on, x_off)


@pytest.mark.gpu
def test_gmres_jacobi_long_columns_are_bitwise(monkeypatch):
    """Jacobi preconditioner, restart 12: no V-cycle to hand a sweep to, and the columns with j + 1 > 8 take the
    unfused projection."""
    from softx_2020_200_amd.problem import build_context
    h = _hier(8)
    ctx = build_context(h.mesh, viscosity=0.01, vnode_mask=h.mask)
    ctx.set_dirichlet(h.dofs, h.vals)
    ctx.set_time("bdf2", (0.01,) * 4)
    ctx.set_state(h.state[0], h.state[0], h.state[1])
    b = ctx.residual().clone()
    out = []
    for prod in (None, "0"):
        _set(monkeypatch, **{PRODUCER: prod, FULL_LAST: "1"})
        x, its, res, ok = ctx.solve_linear(b, max_iterations=36, restart=12, relative_residual=1e-8)
        out.append((x.cpu().numpy(), its))
    assert out[0][1] == out[1][1] and out[0][1] > 12, out[0][1]  # at least one restart: every column length ran
    assert np.array_equal(out[0][0], out[1][0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 16])
def test_skipped_last_projection_keeps_the_solve(n, monkeypatch, capfd):
    """The solve that does not project its last column: same iteration count, converged, and the true residual
    ||b - A x|| recomputed from the device operator within test_gpu_linear_methods' bounds."""
    ctx, b = _rhs(_hier(n))
    rel = 1e-8
    tol = rel * float(b.norm())
    got = {}
    _set(monkeypatch, GLS_GMRES_VERBOSE="1")
    for name, full in (("skip", None), ("full", "1")):
        _set(monkeypatch, **{FULL_LAST: full})
        _flush()
        capfd.readouterr()
        x, its, res, ok = ctx.solve_linear(b, max_iterations=200, restart=30, relative_residual=rel)
        _flush()
        out = capfd.readouterr().out
        assert out.count(SKIP_LINE) == (1 if name == "skip" else 0), out[-2000:]
        tr = float((b - ctx.jacobian_apply(x)).norm())
        print("n=%d %s: %d iterations, reported %.3e, true %.3e, tol %.3e" % (n, name, its, res, tr, tol))
        assert ok, (name, its, res)
        assert res <= tol, (name, res, tol)
        assert tr <= 10 * tol and tr <= 10 * max(res, 1e-3 * tol), (name, tr, res, tol)
        got[name] = (x.cpu().numpy(), its)
    assert got["skip"][1] == got["full"][1], (got["skip"][1], got["full"][1])
    d = np.abs(got["skip"][0] - got["full"][0]).max() / np.abs(got["full"][0]).max()
    print("n=%d: max |x_skip - x_full| / max |x_full| = %.3e" % (n, d))


@pytest.mark.gpu
def test_newton_step_counts_and_bitwise_iterate(monkeypatch):
    """One Newton step as the benchmark calls it. Everything on against everything off: the same counts. With the
    last column projected (only the first-sweep and norm hand-overs on): a bitwise equal iterate."""
    h = _hier(8)
    ctx = h.attach("v11_oseen")
    m1, m2 = h.state

    def step(**env):
        _set(monkeypatch, **env)
        present = m1.clone()
        st = ctx.newton(present, m1, m2, tolerance=1e-30, max_iterations=1, lin_max_iterations=200, restart=30,
                        relative_residual=1e-4, minimum_residual=1e-14)
        ctx.set_state(h.state[0], h.state[0], h.state[1])  # the hierarchy's state, for the tests that share it
        return present.cpu().numpy(), st

    x_off, st_off = step(**{PRODUCER: "0", FULL_LAST: "1", NO_NORM: "1"})
    x_on, st_on = step(**{PRODUCER: None, FULL_LAST: None, NO_NORM: None})
    x_bc, st_bc = step(**{PRODUCER: None, FULL_LAST: "1", NO_NORM: None})
    keys = ("newton_iterations", "linear_iterations", "residual_evaluations", "linear_failures")
    print("newton: off %r, on %r" % ({k: st_off[k] for k in keys}, {k: st_on[k] for k in keys}))
    assert st_off["linear_iterations"] > 0 and st_off["linear_failures"] == 0
    for k in keys:
        assert st_on[k] == st_off[k] and st_bc[k] == st_off[k], (k, st_on[k], st_bc[k], st_off[k])
    assert np.array_equal(x_bc, x_off)
    print("newton: max |x_on - x_off| / max |x_off| = %.3e" % (np.abs(x_on - x_off).max() / np.abs(x_off).max()))
