"""The V-cycle's residual restricted inside the FP32 smoother J.v (one launch + one sum on the coarse lattice)
against the separate residual / slab sum / two-pass restriction launches it replaces: the same
preconditioner within the FP32 variants' tolerance, bit-reproducible, untouched where it does not apply (FP64 smoothing,
no pre-smoothing), also with a face without Dirichlet rows, at solver level and level by level.
GLS_MG_FUSE_TRANSFER=0 (read per call) selects the separate launches in the same process."""
import numpy as np
import pytest

SWITCH = "GLS_MG_FUSE_TRANSFER"
TOL = 1e-5  # FP32 preconditioner variants (test_fused_jacobi_sweeps_match_unfused's tolerance)
# (pre_smooth, post_smooth, mixed_precision, smoother_operator); pre_smooth -1 = no pre-smoothing
CONFIGS = {"v11_oseen": (1, 1, 1, 1), "v11_newton": (1, 1, 1, 0), "v22": (2, 2, 1, 1), "v01": (-1, 1, 1, 1)}

_cache = {}


class _Hierarchy:
    """The Q2-Q2 cavity on n^3 cells with nested levels down to 2^3 (exact LU there); skip_face: that face of
    the cube carries no Dirichlet rows on any level."""

    def __init__(self, n, skip_face=None):
        import torch
        import bench
        from softx_2020_200_amd.native import hyper_cube
        from softx_2020_200_amd.problem import build_context, dirichlet_from_bcs
        self.n, self.ctxs, m = n, [], n
        while True:
            mesh = hyper_cube(3, m, 2, 2, -1.0, 1.0)
            walls = [i for i in range(6) if i != 3 and i != skip_face]
            bcs = [("noslip", b, None) for b in walls]
            if skip_face != 3:
                bcs.append(("function", 3, (1.0, 0.0, 0.0)))
            mask, dofs, vals = dirichlet_from_bcs(mesh, m, -1.0, 1.0, True, bcs)
            ctx = build_context(mesh, viscosity=0.01, vnode_mask=mask)
            ctx.set_dirichlet(dofs, vals)
            if m == n:
                self.mesh, self.dofs, self.vals, self.mask = mesh, dofs, vals, mask
            self.ctxs.append(ctx)
            if m % 2 or m // 2 < 2:
                break
            m //= 2
        self.ctx = self.ctxs[0]
        self.ctx.set_time("bdf2", (0.01,) * 4)
        m1 = torch.from_numpy(bench.smooth_state(self.mesh, n, 3, self.dofs, self.vals, 0.0)).cuda()
        m2 = torch.from_numpy(bench.smooth_state(self.mesh, n, 3, self.dofs, self.vals, 0.3)).cuda()
        self.state = (m1, m2)
        # seeded, non-zero on the Dirichlet rows too
        self.v = torch.from_numpy(np.random.default_rng(20200200).uniform(-1, 1, self.ctx.n_dofs)).cuda()
        self.config = None

    def attach(self, config):
        if self.config != config:
            pre, post, mp, op = CONFIGS[config] if isinstance(config, str) else config
            self.ctx.attach_multigrid(self.ctxs[1:], pre_smooth=pre, post_smooth=post, omega=0.9, coarse_direct=1,
                                      mixed_precision=mp, smoother_operator=op)
            self.ctx.set_state(self.state[0], self.state[0], self.state[1])
            self.config = config
        return self.ctx


def _hier(n, skip_face=None):
    key = (n, skip_face)
    if key not in _cache:
        _cache[key] = _Hierarchy(n, skip_face)
    return _cache[key]


def _on_off(h, config, monkeypatch):
    ctx = h.attach(config)
    monkeypatch.delenv(SWITCH, raising=False)
    z_on = ctx.apply_preconditioner(h.v).cpu().numpy()
    monkeypatch.setenv(SWITCH, "0")
    z_off = ctx.apply_preconditioner(h.v).cpu().numpy()
    monkeypatch.delenv(SWITCH)
    return z_on, z_off


def _fused_levels(h, monkeypatch, on=True):
    """which level pairs take the in-kernel restriction (gls_mg_residual_restrict's report)"""
    import torch
    if on:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "0")
    out = []
    for l in range(len(h.ctxs) - 1):
        x = torch.zeros(h.ctxs[l].n_dofs, dtype=torch.float64, device="cuda")
        bc = torch.zeros(h.ctxs[l + 1].n_dofs, dtype=torch.float64, device="cuda")
        out.append(h.ctx.mg_residual_restrict(l, x, x.clone(), bc)[1])
    monkeypatch.delenv(SWITCH, raising=False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("n", [4, 8, 16])
def test_fused_restriction_on_vs_off(n, config, monkeypatch):
    """apply_preconditioner with the in-kernel restriction against the separate launches: n = 4 (every brick on
    the boundary), 8 (interior bricks), 16 (three transfer levels); V(1,1) with the Oseen and the Newton smoother
    operator, V(2,2), and V(0,1), where no level pre-smooths and the separate launches stay."""
    h = _hier(n)
    z_on, z_off = _on_off(h, config, monkeypatch)
    assert np.abs(z_off).max() > 0 and np.abs(z_on).max() > 0
    rel = np.abs(z_on - z_off).max() / np.abs(z_off).max()
    print("n=%d %s: max rel difference %.3e" % (n, config, rel))
    assert rel < TOL, rel
    # the switch selects the path on every level pair (what a V-cycle with pre-smoothing takes)
    assert _fused_levels(h, monkeypatch, True) == [True] * (len(h.ctxs) - 1)
    assert _fused_levels(h, monkeypatch, False) == [False] * (len(h.ctxs) - 1)
    if CONFIGS[config][0] < 0:  # no pre-smoothing: the same launches either way
        assert np.array_equal(z_on, z_off)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 16])
def test_fused_restriction_bit_reproducible(n, monkeypatch):
    h = _hier(n)
    ctx = h.attach("v11_oseen")
    monkeypatch.delenv(SWITCH, raising=False)
    z1 = ctx.apply_preconditioner(h.v).cpu().numpy()
    z2 = ctx.apply_preconditioner(h.v).cpu().numpy()
    assert np.abs(z1).max() > 0
    assert np.array_equal(z1, z2)


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("face", [3, 0])
def test_fused_restriction_with_a_free_face(face, config, monkeypatch):
    """One face of the cube without Dirichlet rows (the lid y = +1, or x = -1): constrained and free rows meet on
    its edges and corners, where a constrained fine row must restrict onto constrained coarse rows only."""
    h = _hier(8, skip_face=face)
    free = (h.mask.reshape(17, 17, 17) == 0)  # [z][y][x]
    assert free[1:-1, -1, 1:-1].all() if face == 3 else free[1:-1, 1:-1, 0].all()
    z_on, z_off = _on_off(h, config, monkeypatch)
    assert np.abs(z_off).max() > 0
    rel = np.abs(z_on - z_off).max() / np.abs(z_off).max()
    print("free face %d %s: max rel difference %.3e" % (face, config, rel))
    assert rel < TOL, rel


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 8])
def test_fp64_smoothing_untouched(n, monkeypatch):
    h = _hier(n)
    z_on, z_off = _on_off(h, (1, 1, 0, 0), monkeypatch)
    assert np.abs(z_off).max() > 0
    assert np.array_equal(z_on, z_off)
    assert _fused_levels(h, monkeypatch, True) == [False] * (len(h.ctxs) - 1)


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


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 8, 16])
def test_fused_coarse_rhs_per_level(n, monkeypatch):
    """Level by level: the fused coarse right-hand side against gls_mg_transfer of a synthetic fine residual.
    x = 0: the residual is b itself, so the reference is R b with the constrained coarse rows zeroed (the constrained
    fine rows, which the fused path leaves out, reach constrained coarse rows only). x != 0: against the separate
    launches (smoother residual, transfer, zeroing) of the same entry point, which see the same FP32 partial sums.
    Required: the 1e-5 of the preconditioner tests. The kernel forms b - s and restricts it in FP64, so both
    comparisons differ by the order of FP64 sums of <= 1000 terms only: also held to 1e-12 of the largest entry."""
    import torch
    h = _hier(n)
    ctx = h.attach("v11_oseen")
    rng = np.random.default_rng(7)
    for l in range(len(h.ctxs) - 1):
        f, c = h.ctxs[l], h.ctxs[l + 1]
        b = torch.from_numpy(rng.uniform(-1, 1, f.n_dofs)).cuda()
        x0 = torch.zeros_like(b)
        bc = torch.zeros(c.n_dofs, dtype=torch.float64, device="cuda")
        monkeypatch.delenv(SWITCH, raising=False)
        _, fused = ctx.mg_residual_restrict(l, x0, b, bc)
        assert fused
        got = bc.cpu().numpy().copy()
        ref_t = torch.zeros_like(bc)
        ctx.mg_transfer(l, 0, b, ref_t)
        ref = ref_t.cpu().numpy()
        nvc = round(c.n_dofs / 4)
        con_c = _constrained_rows(n >> (l + 1))
        ref[con_c] = 0.0
        assert (got[con_c] == 0.0).all()
        free_c = np.setdiff1d(np.arange(c.n_dofs), con_c)
        assert nvc * 4 == c.n_dofs and np.abs(ref).max() > 0
        e0 = np.abs(got - ref)[free_c].max() / np.abs(ref).max()
        # x != 0 (non-zero on the constrained rows too): fused against the separate launches
        x = torch.from_numpy(rng.uniform(-1, 1, f.n_dofs) * 1e-3).cuda()
        _, fused = ctx.mg_residual_restrict(l, x, b, bc)
        assert fused
        got = bc.cpu().numpy().copy()
        monkeypatch.setenv(SWITCH, "0")
        _, fused = ctx.mg_residual_restrict(l, x, b, bc)
        monkeypatch.delenv(SWITCH)
        assert not fused
        sep = bc.cpu().numpy()
        e1 = np.abs(got - sep).max() / np.abs(sep).max()
        print("n=%d level %d: x = 0 vs R b %.3e, x != 0 vs separate launches %.3e" % (n, l, e0, e1))
        assert e0 < TOL and e1 < TOL, (l, e0, e1)
        assert e0 < 1e-12 and e1 < 1e-12, (l, e0, e1)


def _constrained_rows(m):
    """Dirichlet rows of the cavity on m^3 Q2 cells (all six faces, every velocity component)"""
    nx = 2 * m + 1
    i = np.arange(nx)
    on = (i == 0) | (i == nx - 1)
    node = on[:, None, None] | on[None, :, None] | on[None, None, :]
    nodes = np.nonzero(node.reshape(-1))[0]
    return (nodes[:, None] * 3 + np.arange(3)[None]).reshape(-1)
