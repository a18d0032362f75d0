"""The pencil kernels' lattice gather on the verified hyper_cube (brick node ids computed from the brick's Morton
coordinates, OpParams::cube_gather) against the index-array gather it replaces: bit for bit the same residual,
diagonal, J.v (FP64 and FP32), V-cycle and fused level-pair transfers, on one brick, 8 bricks and 64 bricks, for the
hot instantiation (bdf2, no forcing) and the GEN one (steady, forcing, SRF source). Operator quantities also against
a GLS_SLAB_CSR=1 context (cube_nb1 == 0: the general path), which neither switch may disturb.

GLS_CUBE_GATHER=0 (read per launch) selects the index arrays. GLS_SLAB_CUBE_V1=1 is set with it: the name reserved
for keeping the present k_slab_sum_cube once that kernel is rewritten ("Lattice gather": the rewrite
was measured not to pay and is not in the tree), so these cases hold then too."""
import contextlib
import os

import numpy as np
import pytest

OLD_PATH = {"GLS_CUBE_GATHER": "0", "GLS_SLAB_CUBE_V1": "1", "GLS_SLAB_CSR": None}
NEW_PATH = {"GLS_CUBE_GATHER": None, "GLS_SLAB_CUBE_V1": None, "GLS_SLAB_CSR": None}
SCHEMES = ("bdf2", "steady")
SHAPES = (2, 4, 8)  # cells per direction: 1 brick; 8 bricks (groups of 3, 3, 2); 64 bricks (22 workgroups, nb1 = 4)
OPERATOR = ("residual", "residual_and_diagonal.r", "residual_and_diagonal.d", "jacobian_diagonal", "jacobian_apply",
            "jacobian_apply_f32")
VCYCLE = ("apply_preconditioner", "mg_residual_restrict", "mg_prolong_smooth")

_cache = {}


@contextlib.contextmanager
def _env(kv):
    """set (value None: unset) the environment variables kv, restore them afterwards"""
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Hierarchy:
    """The Q2-Q2 cavity on n^3 cells with nested levels down to 2^3 (test_gpu_mg_fused_transfers.py's set-up);
    steady: with a forcing term and the SRF source on every level (the GEN instantiations)"""

    def __init__(self, n, scheme):
        import torch
        import bench
        from softx_2020_200_amd.native import hyper_cube
        from softx_2020_200_amd.problem import build_context, dirichlet_from_bcs
        gen = scheme == "steady"
        rng = np.random.default_rng(20200200 + n)
        self.n, self.ctxs, m = n, [], n
        while True:
            mesh = hyper_cube(3, m, 2, 2, -1.0, 1.0)
            bcs = [("noslip", b, None) for b in (0, 1, 2, 4, 5)] + [("function", 3, (1.0, 0.0, 0.0))]
            mask, dofs, vals = dirichlet_from_bcs(mesh, m, -1.0, 1.0, True, bcs)
            force = rng.uniform(-1, 1, (mesh["cell_vnodes"].shape[0], 27, 3)) if gen else None
            ctx = build_context(mesh, viscosity=0.01, vnode_mask=mask, force_q=force, srf=gen,
                                omega=(0.3, -0.2, 0.5) if gen else (0, 0, 0))
            ctx.set_dirichlet(dofs, vals)
            if m == n:
                self.mesh, self.dofs, self.vals = mesh, dofs, vals
            self.ctxs.append(ctx)
            if m % 2 or m // 2 < 2:
                break
            m //= 2
        self.ctx = self.ctxs[0]
        self.ctx.set_time(scheme, (0.01,) * 4)
        m1 = torch.from_numpy(bench.smooth_state(self.mesh, n, 3, self.dofs, self.vals, 0.0)).cuda()
        m2 = torch.from_numpy(bench.smooth_state(self.mesh, n, 3, self.dofs, self.vals, 0.3)).cuda()
        self.state = (m1, m1, m2)
        if len(self.ctxs) > 1:  # V(1,1), FP32 Oseen smoothing, exact coarse solve: the benchmark's cycle
            self.ctx.attach_multigrid(self.ctxs[1:], pre_smooth=1, post_smooth=1, omega=0.9, coarse_direct=1,
                                      mixed_precision=1, smoother_operator=1)
        self.ctx.set_state(*self.state)

    def quantities(self):
        """every quantity from a fresh state (nothing cached from the call before), as numpy arrays"""
        import torch
        ctx, out = self.ctx, {}
        rng = np.random.default_rng(7)
        vec = lambda c, s=1.0: torch.from_numpy(rng.uniform(-1, 1, c.n_dofs) * s).cuda()
        v = vec(ctx)
        fresh = lambda: ctx.set_state(*self.state)
        fresh()
        out["residual"] = ctx.residual().cpu().numpy()
        fresh()
        r, d = ctx.residual_and_diagonal()
        out["residual_and_diagonal.r"], out["residual_and_diagonal.d"] = r.cpu().numpy(), d.cpu().numpy()
        fresh()
        out["jacobian_diagonal"] = ctx.jacobian_diagonal().cpu().numpy()
        fresh()
        out["jacobian_apply"] = ctx.jacobian_apply(v).cpu().numpy()
        fresh()
        out["jacobian_apply_f32"] = ctx.jacobian_apply_f32(v).cpu().numpy()
        if len(self.ctxs) > 1:
            fresh()
            out["apply_preconditioner"] = ctx.apply_preconditioner(v).cpu().numpy()
            c = self.ctxs[1]
            x, b, xc = vec(ctx, 1e-3), vec(ctx), vec(c, 1e-3)
            bc = torch.zeros(c.n_dofs, dtype=torch.float64, device="cuda")
            _, fused_r = ctx.mg_residual_restrict(0, x, b, bc)
            out["mg_residual_restrict"] = bc.cpu().numpy()
            got, fused_p = ctx.mg_prolong_smooth(0, xc, x.clone(), b, 0.9)
            out["mg_prolong_smooth"] = got.cpu().numpy()
            out["fused"] = (bool(fused_r), bool(fused_p))
        return out


def _results(n, scheme):
    """{variant: {quantity: array}}: "new" the default path, "old" the switches set, "csr" / "csr_old" the same two on
    a context built with GLS_SLAB_CSR=1. Computed once per (n, scheme) and shared by the cases"""
    key = (n, scheme)
    if key not in _cache:
        res = {}
        with _env(NEW_PATH):
            res["new"] = _Hierarchy(n, scheme).quantities()
        with _env(OLD_PATH):
            res["old"] = _Hierarchy(n, scheme).quantities()
        with _env(dict(NEW_PATH, GLS_SLAB_CSR="1")):  # read when the context is built: no cube_nb1
            h = _Hierarchy(n, scheme)
        with _env(NEW_PATH):
            res["csr"] = h.quantities()
        with _env(OLD_PATH):
            res["csr_old"] = h.quantities()
        _cache[key] = res
    return _cache[key]


def _same(a, b):
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    diff = np.abs(a - b).max()
    return np.array_equal(a, b), diff


@pytest.mark.gpu
@pytest.mark.parametrize("quantity", OPERATOR)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n", SHAPES)
def test_operator_bitwise(n, scheme, quantity):
    """lattice gather == index-array gather == the GLS_SLAB_CSR=1 context (the slab sums of the cube form and of the
    map run in the same slot order), and the general path gives the same bits with either switch setting"""
    res = _results(n, scheme)
    new = res["new"][quantity]
    for other in ("old", "csr", "csr_old"):
        eq, diff = _same(new, res[other][quantity])
        print("n=%d %s %s: new vs %s max |diff| %.3e" % (n, scheme, quantity, other, diff))
        assert eq, (other, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("quantity", VCYCLE)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n", [4, 8])
def test_vcycle_bitwise(n, scheme, quantity):
    """one V(1,1)-cycle and the two fused transfer entry points for the finest level pair (n = 2 has one level). The
    fused RST / PRO launches run on the hot instantiation; with the SRF source the library keeps the separate launches
    (mg_fused_restrict_ok), whose J.v gathers the same way. The GLS_SLAB_CSR=1 hierarchy takes the separate transfers
    (other FP64 sum order than the fused ones), so it is held to its own bits under the switches only"""
    res = _results(n, scheme)
    eq, diff = _same(res["new"][quantity], res["old"][quantity])
    print("n=%d %s %s: new vs old max |diff| %.3e, fused %r" % (n, scheme, quantity, diff, res["new"]["fused"]))
    assert eq, diff
    if scheme == "bdf2":
        assert res["new"]["fused"] == (True, True) and res["old"]["fused"] == (True, True)
    eq, diff = _same(res["csr"][quantity], res["csr_old"][quantity])
    assert eq, diff
    assert res["csr"]["fused"] == res["csr_old"]["fused"]
