"""GPU: subdivided hyper_rectangles on the brick path (gls_mesh_hyper_rectangle, k_slab_sum_box, gls_mg_attach_box):
operator parity with the oracle on non-cubic boxes, the closed-form slab sums against the index map bit for bit, the
per-axis transfers against numpy interpolation matrices, cells = (n, n, n) against gls_mg_attach and
gls_mg_attach_periodic bit for bit, the V-cycle against the numpy restatement built from the oracle's Jacobians
(tests/vcycle_box_ref.py), and the refusals.

GMRES counts of the numpy cycle (tests/test_box_vcycle_ref.py recomputes them on the CPU): 25 on the open 8 x 4 x 4 ->
4 x 2 x 2 Q2-Q2 box, 32 with x periodic (V(1,1), omega 0.9, direct coarsest solve, BDF2, nu 0.01, dt 0.1, relative
residual 1e-8); the device may take 2 more."""
import contextlib
import os

import numpy as np
import pytest

from tests import vcycle_box_ref as br
from tests import vcycle_ref as vr
from tests.gpu_util import context_for, cuda, relerr

TOL = 1e-12
SEED = 20200200
NUMPY_GMRES_ITS = {"open": 25, "x": 32}


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


# ---------------------------------------------------------------------------------------------------------------
# parity with the oracle
# ---------------------------------------------------------------------------------------------------------------
PARITY_MESHES = {"open_4x2x6": ((4, 2, 6), (0.0, 0.0, 0.0), (2.0, 0.5, 3.0), ()),
                 "pery_2x6x4": ((2, 6, 4), (0.0, 0.0, 0.0), (1.0, 1.5, 3.0), (1,))}


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["steady", "bdf2"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("mesh", list(PARITY_MESHES))
def test_box_residual_jv_diag_against_oracle(mesh, k, scheme):
    """residual, J.v and diagonal on non-cubic cells (hx, hy, hz not all equal) at 1e-12 relative max-norm, seeded
    U(-1, 1) states; the brick kernels and their slab sums ran, the open box by the closed form"""
    from oracle.oracle import Oracle
    cells, p1, p2, per = PARITY_MESHES[mesh]
    p = br.box_problem(cells, k, per, p1, p2, scheme=scheme, time_steps=(0.01, 0.013, 0.011, 0.009),
                       viscosity=1.0 if scheme == "steady" else 0.01)
    assert len({tuple(h) for h in p.cell_h}) == 1 and len(set(p.cell_h[0])) >= 2
    rng = np.random.default_rng(SEED)
    u, u1, u2, v = (rng.uniform(-1, 1, p.n_dofs) for _ in range(4))
    orc = Oracle(p)
    ctx = context_for(p)
    assert ctx.uses_brick_kernels
    kind, nb, tile = ctx.slab_lattice()
    if per:
        assert kind == 0
    else:
        assert (kind, nb, tile) == (2, tuple(c // 2 for c in cells), 1)
    ctx.timing(True)
    ctx.set_state(cuda(u), cuda(u1), cuda(u2))
    r = ctx.residual().cpu().numpy()
    d = ctx.jacobian_diagonal().cpu().numpy()
    jv = ctx.jacobian_apply(cuda(v)).cpu().numpy()
    assert ctx.timing_get(5)[1] >= 2  # the slab sums behind the residual and the J.v
    er, ed, ej = (relerr(r, orc.residual(u, u1, u2)), relerr(d, orc.jacobian_diagonal(u, u1, u2)),
                  relerr(jv, orc.jacobian_apply(u, v, u1, u2)))
    print("box parity %s Q%d %s: residual %.2e diagonal %.2e J.v %.2e" % (mesh, k, scheme, er, ed, ej))
    assert er < TOL and ed < TOL and ej < TOL
    assert np.all(r[p.constrained.astype(bool)] == 0.0)


# ---------------------------------------------------------------------------------------------------------------
# k_slab_sum_box against the index map
# ---------------------------------------------------------------------------------------------------------------
def _slab_quantities(cells, k, csr):
    """operator quantities on the mesh and one V-cycle (FP32 smoothing, Jacobi sweeps on the coarsest level too) on the
    hierarchy 2 cells -> cells, from contexts created with or without GLS_SLAB_CSR=1"""
    from softx_2020_200_amd.problem import BoxProblem
    p2 = (2.0, 0.5, 3.0)
    out = {}
    with _env({"GLS_SLAB_CSR": "1" if csr else None}):
        prob = BoxProblem(cells, (0, 0, 0), p2, k=k)
        fine = BoxProblem(tuple(2 * c for c in cells), (0, 0, 0), p2, k=k, multigrid=True,
                          mg_coarsest=min(cells), pre_smooth=1, post_smooth=1, omega=0.9, coarse_sweeps=3,
                          coarse_direct=-1, mixed_precision=1)
    assert len(fine.levels) == 1 and fine.levels[0].cells == tuple(cells)
    out["lattice"] = [prob.ctx.slab_lattice(), fine.ctx.slab_lattice(), fine.levels[0].ctx.slab_lattice()]
    for tag, pr_ in (("mesh", prob), ("fine", fine)):
        ctx = pr_.ctx
        rng = np.random.default_rng(SEED + sum(cells))
        u, u1, u2, v = (rng.uniform(-1, 1, ctx.n_dofs) for _ in range(4))
        for a in (u, u1, u2):
            a[pr_.dir_dofs] = 0.0
        ctx.set_time("bdf2", (0.01, 0.013, 0.011, 0.009))
        ctx.set_state(cuda(u), cuda(u1), cuda(u2))
        if tag == "mesh":
            out["residual"] = ctx.residual().cpu().numpy()
            out["jv"] = ctx.jacobian_apply(cuda(v)).cpu().numpy()
            out["jv_f32"] = ctx.jacobian_apply_f32(cuda(v)).cpu().numpy()
            rd = ctx.residual_and_diagonal()
            out["rd.r"], out["rd.d"] = rd[0].cpu().numpy(), rd[1].cpu().numpy()
        else:
            # the cube's V-cycle would restrict and prolongate inside its smoother launches, which only the verified
            # cube has (another algorithm, not another slab sum): both sides take the separate transfers here
            with _env({"GLS_MG_FUSE_TRANSFER": "0", "GLS_MG_FUSE_PROLONG": "0"}):
                out["vcycle"] = ctx.apply_preconditioner(cuda(v)).cpu().numpy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cells,k", [((2, 6, 4), 2), ((4, 8, 12), 2), ((8, 8, 4), 2), ((2, 6, 4), 1), ((4, 4, 4), 2)])
def test_closed_form_slab_sums_equal_the_index_map(cells, k):
    """nb = (1, 3, 2), (2, 4, 6), (4, 4, 2) with tiles of 1, 8, 8 bricks (an axis of one brick, an odd brick count,
    Morton inside a tile), their doubles (tiles of 8, 64, 64) as the V-cycle's fine level; (4, 4, 4): the cube's
    kernel (its fused transfers off on both sides, see _slab_quantities). Residual, FP64 and FP32 J.v, the fused
    residual + diagonal and one V-cycle with FP32 damped-Jacobi sweeps (the slab sum's sweep branch) are bitwise those
    of GLS_SLAB_CSR=1 contexts"""
    a, b = _slab_quantities(cells, k, False), _slab_quantities(cells, k, True)
    nb = tuple(c // 2 for c in cells)
    s = 1
    while all(n % (2 * s) == 0 for n in nb):
        s *= 2
    if cells == (4, 4, 4):
        assert a["lattice"] == [(1, (2, 2, 2), 2), (1, (4, 4, 4), 4), (1, (2, 2, 2), 2)]
    else:
        assert a["lattice"] == [(2, nb, s), (2, tuple(2 * n for n in nb), 2 * s), (2, nb, s)]
    assert b["lattice"] == [(0, None, None)] * 3
    for key in ("residual", "jv", "jv_f32", "rd.r", "rd.d", "vcycle"):
        assert np.isfinite(a[key]).all() and np.abs(a[key]).max() > 0, key
        assert np.array_equal(a[key], b[key]), (key, np.abs(a[key] - b[key]).max())


# ---------------------------------------------------------------------------------------------------------------
# transfers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k,cells,periodic", [(2, (8, 4, 12), ()), (2, (16, 4, 8), (0,)), (1, (8, 12, 4), (1,))])
def test_box_transfers_exact(k, cells, periodic):
    """gls_mg_transfer on box hierarchies: prolongation == the Kronecker product of the per-axis interpolation matrices
    (% nc on periodic axes) within 1e-13 max(1, |ref|), restriction its transpose (|<R f, c> - <f, P c>| < 1e-12
    sum |f|): the bounds of test_multigrid_transfers_exact"""
    import torch
    from softx_2020_200_amd.problem import BoxProblem
    from tests.test_gpu_mg_periodic import _interp_1d_periodic
    from tests.test_gpu_solver import _interp_1d
    prob = BoxProblem(cells, (0, 0, 0), (2.0, 1.0, 3.0), k=k, periodic=periodic, multigrid=True, coarse_direct=-1)
    ctx = prob.ctx
    levels = [prob] + prob.levels
    assert len(levels) == 2 and levels[1].cells == tuple(c // 2 for c in cells)
    rng = np.random.default_rng(SEED)
    sf, sc = levels[0].shape, levels[1].shape
    assert len(set(sf)) == 3
    P1 = [_interp_1d_periodic(sf[d], sc[d], k) if d in periodic else _interp_1d(sf[d], sc[d], k) for d in range(3)]
    nfd, ncd = levels[0].n_dofs, levels[1].n_dofs
    c = rng.uniform(-1, 1, ncd)
    f = rng.uniform(-1, 1, nfd)
    out_f = torch.zeros(nfd, dtype=torch.float64, device="cuda")
    out_c = torch.zeros(ncd, dtype=torch.float64, device="cuda")
    ctx.mg_transfer(0, 1, torch.from_numpy(c).cuda(), out_f)
    ctx.mg_transfer(0, 0, torch.from_numpy(f).cuda(), out_c)
    pf, rc = out_f.cpu().numpy(), out_c.cpu().numpy()
    ncn, nfn = int(np.prod(sc)), int(np.prod(sf))
    fields_c = [c[3 * np.arange(ncn) + a] for a in range(3)] + [c[3 * ncn:]]
    fields_f = [pf[3 * np.arange(nfn) + a] for a in range(3)] + [pf[3 * nfn:]]
    for fc, ff in zip(fields_c, fields_f):
        ref = np.einsum("zc,yb,xa,cba->zyx", P1[2], P1[1], P1[0], fc.reshape(sc[2], sc[1], sc[0]),
                        optimize=True).reshape(-1)
        err = np.abs(ff - ref).max()
        assert err < 1e-13 * max(1.0, np.abs(ref).max()), err
    lhs, rhs = np.dot(rc, c), np.dot(f, pf)
    assert abs(lhs - rhs) < 1e-12 * np.abs(f).sum(), (lhs, rhs)


def _hierarchy_bits(prob, n_levels):
    """one V-cycle, both transfers of every level pair and whether the fused restriction ran, as arrays"""
    ctx = prob.ctx
    rng = np.random.default_rng(SEED)
    res = [ctx.apply_preconditioner(cuda(rng.uniform(-1, 1, ctx.n_dofs))).cpu().numpy()]
    levels = ctx._mg_levels
    assert len(levels) == n_levels
    for l in range(len(levels) - 1):
        c, f = rng.uniform(-1, 1, levels[l + 1].n_dofs), rng.uniform(-1, 1, levels[l].n_dofs)
        out_f, out_c = levels[l].zeros(), levels[l + 1].zeros()
        ctx.mg_transfer(l, 1, cuda(c), out_f)
        ctx.mg_transfer(l, 0, cuda(f), out_c)
        res += [out_f.cpu().numpy(), out_c.cpu().numpy()]
        fused = ctx.mg_residual_restrict(l, levels[l].zeros(), levels[l].zeros() + 1.0, levels[l + 1].zeros())[1]
        res.append(np.array([1.0 if fused else 0.0]))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("periodic", [None, (0,)], ids=["open", "x"])
def test_cubic_box_is_the_cube_hierarchy(periodic):
    """gls_mg_attach_box with cells = (n, n, n): mask 0 against gls_mg_attach on the 8^3 Q2 cavity (bench.py's cycle,
    fused transfers included), mask x against gls_mg_attach_periodic on the 16^3 box: bitwise-equal transfers on every
    level pair, the same fused flags, bitwise-equal gls_apply_preconditioner"""
    import torch
    import bench
    from softx_2020_200_amd.problem import CavityProblem, PeriodicBoxProblem
    out = {}
    for tag in ("cube", "box"):
        if periodic is None:
            n = 8
            opts = dict(mg_coarsest=2, pre_smooth=1, post_smooth=1, omega=0.9, mixed_precision=True,
                        level_sweeps={-2: (2, 2)})
            if tag == "box":
                opts["box"] = ((n, n, n), ())
            prob = CavityProblem(dim=3, n=n, k=2, viscosity=0.01, multigrid=True, **opts)
            m1 = torch.from_numpy(bench.smooth_state(prob.mesh, n, 3, prob.dir_dofs, prob.dir_vals, 0.0)).cuda()
            m2 = torch.from_numpy(bench.smooth_state(prob.mesh, n, 3, prob.dir_dofs, prob.dir_vals, 0.3)).cuda()
        else:
            n = 16
            # Jacobi sweeps on the coarsest level (2592 DoFs): its direct solve is not bitwise reproducible from one
            # hierarchy to the next (two gls_mg_attach_periodic hierarchies built the same way differ by 1e-14
            # relative in one V-cycle); the coarse solve is not what is compared here
            opts = dict(pre_smooth=1, post_smooth=1, omega=0.9, coarse_direct=-1, coarse_sweeps=10, mixed_precision=1)
            if tag == "box":
                opts["box"] = ((n, n, n), periodic)
            prob = PeriodicBoxProblem(n=n, k=2, periodic=periodic, multigrid=True, **opts)
            m1, m2 = cuda(prob.taylor_green(0.0)), cuda(prob.taylor_green(0.03))
        prob.ctx.set_time("bdf2", (0.01,) * 4)
        prob.ctx.set_state(m1, m1, m2)
        out[tag] = _hierarchy_bits(prob, 3)
    assert np.abs(out["cube"][0]).max() > 0
    if periodic is None:
        assert out["cube"][3][0] == 1.0  # the open cube's fused restriction is still taken
    for a, b in zip(out["cube"], out["box"]):
        assert np.array_equal(a, b), np.abs(a - b).max()


# ---------------------------------------------------------------------------------------------------------------
# the V-cycle against the numpy restatement
# ---------------------------------------------------------------------------------------------------------------
_dev = {}


def _box_contexts(name):
    """the case's device levels: the reference's oracle problems (already on the mesh builder's arrays)"""
    if name not in _dev:
        per = br.CASES[name]["periodic"]
        ctxs = [context_for(p) for p in br.operators(name)["H"]["probs"]]
        for ctx, p in zip(ctxs, br.operators(name)["H"]["probs"]):
            assert ctx.uses_brick_kernels and ctx.n_dofs == p.n_dofs
        pre, post = br.SWEEPS
        ctxs[0].attach_multigrid(ctxs[1:], pre_smooth=pre, post_smooth=post, omega=br.OMEGA, coarse_direct=1,
                                 mixed_precision=0, box=(br.LEVELS[0], per))
        ctxs[0].set_state(*[cuda(a) for a in br.operators(name)["state"][0]])
        _dev[name] = ctxs
    return _dev[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(br.CASES))
def test_box_vcycle_against_reference(name):
    """one gls_apply_preconditioner against the numpy cycle, per block, with test_gpu_vcycle_reference.py's FP64 bound
    max(1e-12, kappa eps) (kappa 4.2e4 open, 1.9e4 with x periodic: bounds 9.3e-12 and 4.1e-12); then as GMRES
    preconditioner at most 2 iterations more than the numpy cycle, and fewer than Jacobi-GMRES on the same system"""
    ctxs = _box_contexts(name)
    ctx = ctxs[0]
    z_ref = br.reference(name)
    bd = br.bound(name)
    nv = 3 * br.operators(name)["H"]["probs"][0].n_vnodes
    assert not ctx.mg_residual_restrict(0, ctx.zeros(), ctx.zeros() + 1.0, ctxs[1].zeros())[1]
    assert not ctx.mg_prolong_smooth(0, ctxs[1].zeros(), ctx.zeros(), ctx.zeros() + 1.0, 0.9)[1]
    z = ctx.apply_preconditioner(cuda(vr.rhs_vector(ctx.n_dofs))).cpu().numpy()
    assert np.isfinite(z).all()
    errs = []
    for blk, s in (("velocity", slice(0, nv)), ("pressure", slice(nv, None))):
        e = float(np.abs(z[s] - z_ref[s]).max() / np.abs(z_ref[s]).max())
        print("box vcycle %s %s: device error %.3e, bound %.3e" % (name, blk, e, bd))
        errs.append((blk, e))
    for blk, e in errs:
        assert e <= bd, (name, blk, e, bd)
    _, xt, b = br.gmres_problem(name)
    rhs = cuda(b)
    x, its, res, ok = ctx.solve_linear(rhs, ctx.zeros(), max_iterations=200, restart=30, relative_residual=1e-8,
                                       minimum_residual=1e-300, true_residual=True)
    true = float((rhs - ctx.jacobian_apply(x)).norm() / rhs.norm())
    jac = context_for(br.operators(name)["H"]["probs"][0])
    jac.set_state(*[cuda(a) for a in br.operators(name)["state"][0]])
    _, jits, _, jok = jac.solve_linear(rhs, jac.zeros(), max_iterations=2000, restart=30, relative_residual=1e-8,
                                       minimum_residual=1e-300, true_residual=True)
    print("box vcycle %s: GMRES its %d (numpy %d, Jacobi %d), true rel residual %.2e"
          % (name, its, NUMPY_GMRES_ITS[name], jits, true))
    assert ok and true <= 1e-8 * 1.01, (its, res, true)
    assert its <= NUMPY_GMRES_ITS[name] + 2, (its, NUMPY_GMRES_ITS[name])
    assert jok and its < jits, (its, jits)


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_box_attach_refusals_keep_the_hierarchy():
    """GLS_EINVAL naming the level (and axis), and the hierarchy attached before still answers
    gls_apply_preconditioner with the same bits: an odd count, too few cells on a periodic axis, a level of the wrong
    size, a level whose numbering is not the lattice, a distributed level and a distributed context"""
    import softx_2020_200_amd as sx
    from softx_2020_200_amd import GLSError
    from softx_2020_200_amd.dist import Exchanger, attach, partition
    from softx_2020_200_amd.native import mesh_hyper_rectangle
    from softx_2020_200_amd.problem import BoxProblem, build_context
    cells, p1, p2 = (8, 4, 4), (0, 0, 0), (2, 1, 1)
    for per in ((), (0,)):
        prob = BoxProblem(cells, p1, p2, k=2, periodic=per, multigrid=True, pre_smooth=1, post_smooth=1, omega=0.9)
        assert len(prob.levels) == 1
        ctx, lv1 = prob.ctx, prob.levels[0].ctx
        ctx.set_time("bdf2", (0.05,) * 4)
        rng = np.random.default_rng(SEED)
        u = rng.uniform(-1, 1, ctx.n_dofs)
        u[prob.dir_dofs] = 0.0
        u = cuda(u)
        ctx.set_state(u, u, u)
        v = cuda(rng.uniform(-1, 1, ctx.n_dofs))
        z0 = ctx.apply_preconditioner(v).cpu().numpy()
        assert np.isfinite(z0).all() and np.abs(z0).max() > 0

        def refused(levels, box, *words):
            with pytest.raises(GLSError) as e:
                ctx.attach_multigrid(levels, box=box)
            for w in words:
                assert w in str(e.value), str(e.value)
            assert np.array_equal(ctx.apply_preconditioner(v).cpu().numpy(), z0)

        if per:  # a third level would have 2 cells on the periodic axis
            refused([lv1, lv1], (cells, per), "level 2", "axis 0", "at least 4")
            continue
        refused([lv1, lv1], (cells, per), "level 2", "axis 1", "odd")
        refused([lv1], ((8, 4, 6), per), "level 0", "not nested")
        refused([lv1], ((9, 4, 4), per), "level 0", "axis 0", "odd")
        refused([BoxProblem((4, 2, 4), p1, p2, k=2).ctx], (cells, per), "level 1", "not nested")
        mesh = mesh_hyper_rectangle((4, 2, 2), p1, p2, 2)
        bad = dict(mesh)
        cv = mesh["cell_vnodes"].copy()
        cv[mesh["cell_vnodes"] == 1], cv[mesh["cell_vnodes"] == 2] = 2, 1
        bad["cell_vnodes"], bad["cell_pnodes"] = cv, cv.copy()
        refused([build_context(bad, viscosity=0.01)], (cells, per), "level 1", "lattice")
        plan = partition(mesh["cell_vnodes"], mesh["n_vnodes"], 0, 1)
        dctx = sx.GLSContext(3, 2, 2, plan["local_cells"], None, mesh["cell_h"], mesh["n_vnodes"], mesh["n_vnodes"],
                             viscosity=0.01, cell_x0=mesh["cell_x0"])
        attach(dctx, plan, Exchanger(plan, "cuda", backend="gloo"))
        refused([dctx], (cells, per), "level 1", "distributed")
        with pytest.raises(GLSError) as e:
            dctx.attach_multigrid([lv1], box=((4, 2, 2), per))
        assert "distributed" in str(e.value), str(e.value)
        assert np.array_equal(ctx.apply_preconditioner(v).cpu().numpy(), z0)
