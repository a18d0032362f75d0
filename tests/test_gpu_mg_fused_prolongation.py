"""The V-cycle's prolongation inside the first post-sweep (the FP32 smoother J.v gathers x + P xc, the slab sum forms
the same value at the brick-surface nodes) against the separate two-pass transfer launches it replaces: level by
level with omega = 0 (the sweep then returns x + P xc itself) and omega = 0.9, as a preconditioner, untouched where
it does not apply (FP64 smoothing, no post-smoothing), with a face without Dirichlet rows, bit-reproducible, and at
solver level. GLS_MG_FUSE_PROLONG=0 (read per call) selects the separate launches in the same process.
The hierarchies are those of test_gpu_mg_fused_transfers (Q2-Q2 cavity, nested levels down to 2^3)."""
import numpy as np
import pytest

from tests.test_gpu_mg_fused_transfers import CONFIGS, TOL, _hier

SWITCH = "GLS_MG_FUSE_PROLONG"
PRECOND = ["v11_oseen", "v11_newton", "v22"]  # V(2,2): only the first post-sweep takes the prolongation
assert all(CONFIGS[c][1] >= 1 for c in PRECOND)

_con = {}


def _con_rows(m, skip_face=None):
    """Dirichlet rows of the cavity on m^3 Q2 cells with the hierarchy's boundary conditions"""
    if (m, skip_face) not in _con:
        from softx_2020_200_amd.native import hyper_cube
        from softx_2020_200_amd.problem import dirichlet_from_bcs
        bcs = [("noslip", i, None) for i in range(6) if i != 3 and i != skip_face]
        if skip_face != 3:
            bcs.append(("function", 3, (1.0, 0.0, 0.0)))
        _con[(m, skip_face)] = np.asarray(dirichlet_from_bcs(hyper_cube(3, m, 2, 2, -1.0, 1.0), m, -1.0, 1.0, True, bcs)[1])
    return _con[(m, skip_face)]


def _on_off(h, config, monkeypatch):
    ctx = h.attach(config)
    monkeypatch.delenv(SWITCH, raising=False)
    z_on = ctx.apply_preconditioner(h.v).cpu().numpy()
    monkeypatch.setenv(SWITCH, "0")
    z_off = ctx.apply_preconditioner(h.v).cpu().numpy()
    monkeypatch.delenv(SWITCH)
    return z_on, z_off


def _fused_pairs(h, monkeypatch, on=True):
    """which level pairs take the in-kernel prolongation (gls_mg_prolong_smooth's report)"""
    import torch
    if on:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "0")
    out = []
    for l in range(len(h.ctxs) - 1):
        x = torch.zeros(h.ctxs[l].n_dofs, dtype=torch.float64, device="cuda")
        xc = torch.zeros(h.ctxs[l + 1].n_dofs, dtype=torch.float64, device="cuda")
        out.append(h.ctx.mg_prolong_smooth(l, xc, x, x.clone(), 0.9)[1])
    monkeypatch.delenv(SWITCH, raising=False)
    return out


def _level_vectors(h, l, rng, skip_face=None):
    """random x, b on level l and a random coarse correction that vanishes on the coarse Dirichlet rows"""
    import torch
    f, c = h.ctxs[l], h.ctxs[l + 1]
    x = torch.from_numpy(rng.uniform(-1, 1, f.n_dofs)).cuda()
    b = torch.from_numpy(rng.uniform(-1, 1, f.n_dofs)).cuda()
    xc = rng.uniform(-1, 1, c.n_dofs)
    xc[_con_rows(h.n >> (l + 1), skip_face)] = 0.0
    return x, b, torch.from_numpy(xc).cuda()


def _check_omega0(h, monkeypatch, skip_face=None):
    """omega = 0: the sweep returns x + P xc. Against gls_mg_transfer's prolongation added to x, on every level pair,
    with the switch on (fused) and off (separate): the paths differ by the order of an FP64 sum of <= 27 terms with
    weights <= 1, so 1e-13 of the largest entry."""
    import torch
    ctx = h.attach("v11_oseen")
    rng = np.random.default_rng(11)
    for l in range(len(h.ctxs) - 1):
        x, b, xc = _level_vectors(h, l, rng, skip_face)
        pxc = torch.zeros_like(x)
        ctx.mg_transfer(l, 1, xc, pxc)
        ref = (x + pxc).cpu().numpy()
        assert np.abs(pxc.cpu().numpy()).max() > 0
        for on in (True, False):
            if on:
                monkeypatch.delenv(SWITCH, raising=False)
            else:
                monkeypatch.setenv(SWITCH, "0")
            got, fused = ctx.mg_prolong_smooth(l, xc, x.clone(), b, 0.0)
            monkeypatch.delenv(SWITCH, raising=False)
            assert fused == on, (l, on, fused)
            err = np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max()
            print("n=%d face %r level %d fused %d: omega = 0 vs x + P xc %.3e" % (h.n, skip_face, l, on, err))
            assert err < 1e-13, (l, on, err)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 8, 16])
def test_fused_prolongation_omega0_is_x_plus_pxc(n, monkeypatch):
    """n = 4: every brick on the boundary and the last brick triple short; 8: interior bricks; 16: three pairs."""
    _check_omega0(_hier(n), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 8, 16])
def test_fused_prolongation_sweep_per_level(n, monkeypatch):
    """omega = 0.9: prolongation + one post-sweep, fused against the separate launches of the same entry (the FP32
    cast of x + P xc may differ by one FP32 ulp)."""
    h = _hier(n)
    ctx = h.attach("v11_oseen")
    rng = np.random.default_rng(12)
    for l in range(len(h.ctxs) - 1):
        x, b, xc = _level_vectors(h, l, rng)
        monkeypatch.delenv(SWITCH, raising=False)
        got, fused = ctx.mg_prolong_smooth(l, xc, x.clone(), b, 0.9)
        assert fused
        monkeypatch.setenv(SWITCH, "0")
        sep, fused = ctx.mg_prolong_smooth(l, xc, x.clone(), b, 0.9)
        monkeypatch.delenv(SWITCH)
        assert not fused
        got, sep = got.cpu().numpy(), sep.cpu().numpy()
        assert np.abs(sep - x.cpu().numpy()).max() > 0
        err = np.abs(got - sep).max() / np.abs(sep).max()
        print("n=%d level %d: omega = 0.9 fused vs separate %.3e" % (n, l, err))
        assert err < TOL, (l, err)


@pytest.mark.gpu
@pytest.mark.parametrize("config", PRECOND)
@pytest.mark.parametrize("n", [4, 8, 16])
def test_fused_prolongation_on_vs_off(n, config, monkeypatch):
    h = _hier(n)
    z_on, z_off = _on_off(h, config, monkeypatch)
    assert np.abs(z_off).max() > 0 and np.abs(z_on).max() > 0
    rel = np.abs(z_on - z_off).max() / np.abs(z_off).max()
    print("n=%d %s: max rel difference %.3e" % (n, config, rel))
    assert rel < TOL, rel
    assert _fused_pairs(h, monkeypatch, True) == [True] * (len(h.ctxs) - 1)
    assert _fused_pairs(h, monkeypatch, False) == [False] * (len(h.ctxs) - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("config", [(1, 1, 0, 0), (1, 0, 1, 1)], ids=["fp64_smoothing", "no_post_sweep"])
@pytest.mark.parametrize("n", [4, 8])
def test_other_paths_untouched(n, config, monkeypatch):
    """FP64 smoothing, and FP32 smoothing without a post-sweep: the same launches either way."""
    h = _hier(n)
    z_on, z_off = _on_off(h, config, monkeypatch)
    assert np.abs(z_off).max() > 0
    assert np.array_equal(z_on, z_off)
    assert _fused_pairs(h, monkeypatch, True) == [False] * (len(h.ctxs) - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("config", PRECOND)
@pytest.mark.parametrize("face", [3, 0])
def test_fused_prolongation_with_a_free_face(face, config, monkeypatch):
    """One face of the cube without Dirichlet rows (the lid y = +1, or x = -1): on its edges and corners constrained
    and free rows meet, and P xc has to vanish on the constrained ones without being masked."""
    h = _hier(8, skip_face=face)
    z_on, z_off = _on_off(h, config, monkeypatch)
    assert np.abs(z_off).max() > 0
    rel = np.abs(z_on - z_off).max() / np.abs(z_off).max()
    print("free face %d %s: max rel difference %.3e" % (face, config, rel))
    assert rel < TOL, rel
    if config == PRECOND[0]:
        _check_omega0(h, monkeypatch, skip_face=face)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 16])
def test_fused_prolongation_bit_reproducible(n, monkeypatch):
    h = _hier(n)
    ctx = h.attach("v11_oseen")
    monkeypatch.delenv(SWITCH, raising=False)
    z1 = ctx.apply_preconditioner(h.v).cpu().numpy()
    z2 = ctx.apply_preconditioner(h.v).cpu().numpy()
    assert np.abs(z1).max() > 0
    assert np.array_equal(z1, z2)
    assert _fused_pairs(h, monkeypatch, True) == [True] * (len(h.ctxs) - 1)


@pytest.mark.gpu
def test_solver_converges_with_equal_iterations(monkeypatch):
    """GMRES to rel 1e-4 (the benchmark's solve) on the Newton right-hand side at n = 16: both paths converge to the
    requested true residual in the same number of iterations."""
    h = _hier(16)
    ctx = h.attach("v11_oseen")
    b = ctx.residual().clone()
    rel, res = 1e-4, {}
    for name in ("on", "off"):
        if name == "off":
            monkeypatch.setenv(SWITCH, "0")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        _, its, r, ok = ctx.solve_linear(b, max_iterations=200, restart=30, relative_residual=rel, true_residual=True)
        res[name] = (its, r, ok)
    monkeypatch.delenv(SWITCH, raising=False)
    print("solve: on %r, off %r, tolerance %.3e" % (res["on"], res["off"], rel * float(b.norm())))
    for its, r, ok in res.values():
        assert ok and its > 0 and r <= rel * float(b.norm()), res
    assert res["on"][0] == res["off"][0], res
