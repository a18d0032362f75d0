"""GPU: the nested multigrid on periodic hyper_cubes (gls_mg_attach_periodic): the wrap-aware two-pass transfers against
numpy interpolation matrices, mask 0 against gls_mg_attach bit for bit, the V-cycle against the numpy restatement built
from the oracle's periodic Jacobians (tests/vcycle_periodic_ref.py), Newton with the periodic V-cycle against Newton
with Jacobi, and the refusals.

GMRES counts of the numpy cycle (tests/test_mg_periodic_ref.py recomputes them on the CPU): 17 on the fully periodic
8^3 -> 4^3 Q2-Q2 box, 16 with x periodic and walls in y, z (V(1,1), omega 0.9, direct coarsest solve, BDF2, nu 0.01,
dt 0.1, relative residual 1e-8); the device may take 2 more."""
import copy

import numpy as np
import pytest

from gpu_util import context_for, cuda
from tests import vcycle_periodic_ref as pr
from tests import vcycle_ref as vr

NUMPY_GMRES_ITS = {"xyz": 17, "x": 16}
# what apps/gls_navier_stokes attaches on a periodic hyper_cube
APP_CYCLE = dict(pre_smooth=1, post_smooth=1, omega=0.6, coarse_omega=0.6, coarse_direct=1, mixed_precision=1,
                 smoother_operator=1)


def _interp_1d_periodic(nf, nc, k):
    """Qk interpolation between nested periodic node lattices (nf = 2 nc nodes, numpy, independent of the C++ tap
    tables): fine node i sits at x = i / (2k) coarse cells, in cell floor(x); coarse node indices wrap with % nc"""
    assert nf == 2 * nc
    P = np.zeros((nf, nc))
    for i in range(nf):
        x = i / (2.0 * k)
        cc = int(np.floor(x))
        xi = x - cc
        for q in range(k + 1):
            L = 1.0
            for b in range(k + 1):
                if b != q:
                    L *= (xi * k - b) / (q - b)
            P[i, (cc * k + q) % nc] += L
    return P


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,periodic", [(2, 16, (0, 1, 2)), (2, 32, (0, 1, 2)), (2, 24, (0,)), (2, 24, (2,)),
                                          (1, 32, (0, 1))])
def test_periodic_transfers_exact(k, n, periodic):
    """gls_mg_transfer on periodic hierarchies: prolongation == the Kronecker product of the per-axis interpolation
    matrices (periodic axes wrapped, the others tests/test_gpu_solver.py's open one) within 1e-13 max(1, |ref|) on every
    level pair, restriction its transpose (|<R f, c> - <f, P c>| < 1e-12 sum |f|); sums of <= 125 products, the bounds
    of test_multigrid_transfers_exact"""
    import torch
    from softx_2020_200_amd.problem import PeriodicBoxProblem
    from tests.test_gpu_solver import _interp_1d
    prob = PeriodicBoxProblem(n=n, k=k, periodic=periodic, multigrid=True, coarse_direct=-1)
    ctx = prob.ctx
    levels = [prob] + prob.levels
    assert len(levels) >= 3
    rng = np.random.default_rng(20200200)
    for l in range(len(levels) - 1):
        sf, sc = levels[l].shape, levels[l + 1].shape
        P1 = [_interp_1d_periodic(sf[d], sc[d], k) if d in periodic else _interp_1d(sf[d], sc[d], k) for d in range(3)]
        nfd, ncd = levels[l].n_dofs, levels[l + 1].n_dofs
        c = rng.uniform(-1, 1, ncd)
        f = rng.uniform(-1, 1, nfd)
        out_f = torch.zeros(nfd, dtype=torch.float64, device="cuda")
        out_c = torch.zeros(ncd, dtype=torch.float64, device="cuda")
        ctx.mg_transfer(l, 1, torch.from_numpy(c).cuda(), out_f)
        ctx.mg_transfer(l, 0, torch.from_numpy(f).cuda(), out_c)
        pf, rc = out_f.cpu().numpy(), out_c.cpu().numpy()
        ncn, nfn = int(np.prod(sc)), int(np.prod(sf))
        fields_c = [c[3 * np.arange(ncn) + a] for a in range(3)] + [c[3 * ncn:]]
        fields_f = [pf[3 * np.arange(nfn) + a] for a in range(3)] + [pf[3 * nfn:]]
        for fc, ff in zip(fields_c, fields_f):
            ref = np.einsum("zc,yb,xa,cba->zyx", P1[2], P1[1], P1[0], fc.reshape(sc[2], sc[1], sc[0]),
                            optimize=True).reshape(-1)
            err = np.abs(ff - ref).max()
            assert err < 1e-13 * max(1.0, np.abs(ref).max()), (l, err)
        lhs, rhs = np.dot(rc, c), np.dot(f, pf)
        assert abs(lhs - rhs) < 1e-12 * np.abs(f).sum(), (l, lhs, rhs)


@pytest.mark.gpu
def test_mask_zero_is_gls_mg_attach():
    """gls_mg_attach_periodic(mask 0) and gls_mg_attach on the 16^3 Q2 cavity (bench.py's cycle): bitwise-equal
    transfers on every level pair and bitwise-equal gls_apply_preconditioner"""
    import torch
    import bench
    from softx_2020_200_amd.problem import CavityProblem
    n = 16
    opts = dict(mg_coarsest=2, pre_smooth=1, post_smooth=1, omega=0.9, mixed_precision=True, level_sweeps={-2: (2, 2)})
    out = {}
    for tag, per in (("attach", None), ("periodic0", ())):
        prob = CavityProblem(dim=3, n=n, k=2, viscosity=0.01, multigrid=True, periodic=per, **opts)
        ctx = prob.ctx
        ctx.set_time("bdf2", (0.01,) * 4)
        m1 = torch.from_numpy(bench.smooth_state(prob.mesh, n, 3, prob.dir_dofs, prob.dir_vals, 0.0)).cuda()
        m2 = torch.from_numpy(bench.smooth_state(prob.mesh, n, 3, prob.dir_dofs, prob.dir_vals, 0.3)).cuda()
        ctx.set_state(m1, m1, m2)
        rng = np.random.default_rng(20200200)
        res = [ctx.apply_preconditioner(cuda(rng.uniform(-1, 1, ctx.n_dofs))).cpu().numpy()]
        levels = ctx._mg_levels
        assert len(levels) == 4
        for l in range(len(levels) - 1):
            c, f = rng.uniform(-1, 1, levels[l + 1].n_dofs), rng.uniform(-1, 1, levels[l].n_dofs)
            out_f, out_c = levels[l].zeros(), levels[l + 1].zeros()
            ctx.mg_transfer(l, 1, cuda(c), out_f)
            ctx.mg_transfer(l, 0, cuda(f), out_c)
            res += [out_f.cpu().numpy(), out_c.cpu().numpy()]
            fused = ctx.mg_residual_restrict(l, levels[l].zeros(), levels[l].zeros() + 1.0, levels[l + 1].zeros())[1]
            res.append(np.array([1.0 if fused else 0.0]))
        out[tag] = res
    assert np.abs(out["attach"][0]).max() > 0
    for a, b in zip(out["attach"], out["periodic0"]):
        assert np.array_equal(a, b), np.abs(a - b).max()


_dev = {}


def _periodic_contexts(name):
    """the case's device levels: the reference's oracle problems with the library's Morton-ordered cell arrays"""
    if name not in _dev:
        import softx_2020_200_amd as sx
        c = pr.CASES[name]
        ctxs = []
        for p in pr.operators(name)["H"]["probs"]:
            q = copy.copy(p)
            m = sx.hyper_cube(3, p.n, p.k, p.k, pr.LO, pr.HI, periodic=c["periodic"])
            for key in ("cell_vnodes", "cell_pnodes", "cell_x0", "cell_h"):
                setattr(q, key, np.ascontiguousarray(m[key]))
            ctx = context_for(q)
            assert ctx.uses_brick_kernels and ctx.n_dofs == p.n_dofs
            ctxs.append(ctx)
        pre, post = pr.SWEEPS
        ctxs[0].attach_multigrid(ctxs[1:], pre_smooth=pre, post_smooth=post, omega=pr.OMEGA, coarse_direct=1,
                                 mixed_precision=0, periodic=c["periodic"])
        ctxs[0].set_state(*[cuda(a) for a in pr.operators(name)["state"][0]])
        _dev[name] = ctxs
    return _dev[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pr.CASES))
def test_periodic_vcycle_against_reference(name):
    """one gls_apply_preconditioner against the numpy cycle, per block, with test_gpu_vcycle_reference.py's FP64 bound
    max(1e-12, kappa eps); then as GMRES preconditioner at most 2 iterations more than the numpy cycle"""
    ctxs = _periodic_contexts(name)
    ctx = ctxs[0]
    z_ref = pr.reference(name)
    bd = pr.bound(name)
    nv = 3 * pr.operators(name)["H"]["probs"][0].n_vnodes
    # periodic level pairs take the unfused transfers
    assert not ctx.mg_residual_restrict(0, ctx.zeros(), ctx.zeros() + 1.0, ctxs[1].zeros())[1]
    assert not ctx.mg_prolong_smooth(0, ctxs[1].zeros(), ctx.zeros(), ctx.zeros() + 1.0, 0.9)[1]
    z = ctx.apply_preconditioner(cuda(vr.rhs_vector(ctx.n_dofs))).cpu().numpy()
    assert np.isfinite(z).all()
    errs = []
    for blk, s in (("velocity", slice(0, nv)), ("pressure", slice(nv, None))):
        e = float(np.abs(z[s] - z_ref[s]).max() / np.abs(z_ref[s]).max())
        print("periodic vcycle %s %s: device error %.3e, bound %.3e" % (name, blk, e, bd))
        errs.append((blk, e))
    for blk, e in errs:
        assert e <= bd, (name, blk, e, bd)
    _, xt, b = pr.gmres_problem(name)
    rhs = cuda(b)
    x, its, res, ok = ctx.solve_linear(rhs, ctx.zeros(), max_iterations=200, restart=30, relative_residual=1e-8,
                                       minimum_residual=1e-300, true_residual=True)
    true = float((rhs - ctx.jacobian_apply(x)).norm() / rhs.norm())
    print("periodic vcycle %s: GMRES its %d (numpy %d), true rel residual %.2e" % (name, its, NUMPY_GMRES_ITS[name], true))
    assert ok and true <= 1e-8 * 1.01, (its, res, true)
    assert its <= NUMPY_GMRES_ITS[name] + 2, (its, NUMPY_GMRES_ITS[name])


def _newton_box(n, multigrid):
    import torch
    from softx_2020_200_amd.problem import PeriodicBoxProblem
    prob = PeriodicBoxProblem(n=n, k=2, periodic=(0, 1, 2), viscosity=0.01, multigrid=multigrid,
                              **(APP_CYCLE if multigrid else {}))
    ctx = prob.ctx
    ctx.set_time("bdf2", (0.05,) * 4)
    m1 = torch.from_numpy(prob.taylor_green(0.0)).cuda()
    m2 = torch.from_numpy(prob.taylor_green(0.03)).cuda()
    x = m1.clone()
    st = ctx.newton(x, m1, m2, tolerance=1e-9, max_iterations=8, lin_max_iterations=3000, restart=100,
                    relative_residual=1e-6, minimum_residual=1e-14)
    return x.cpu().numpy(), st, prob


@pytest.mark.gpu
def test_periodic_multigrid_newton_matches_jacobi_and_is_level_independent():
    """Newton (BDF2, dt 0.05, nu 0.01, the Taylor-Green state) on the fully periodic 16^3 Q2-Q2 box with the periodic
    V-cycle (the application's cycle) and with Jacobi-GMRES: both converge, the velocities agree to 1e-7
    (test_multigrid_preconditioner's bounds), the V-cycle needs fewer linear iterations (the ratio is printed and in
    the failure message, not fixed: on a small-dt periodic box Jacobi is already good), and 32^3 needs at most 2 more
    linear iterations than 16^3"""
    xm, sm, prob = _newton_box(16, True)
    assert len(prob.levels) == 2  # 16 -> 8 -> 4
    xj, sj, _ = _newton_box(16, False)
    ratio = sj["linear_iterations"] / max(sm["linear_iterations"], 1)
    print("periodic 16^3 Newton: multigrid %s, Jacobi %s, linear iteration ratio %.2f" % (sm, sj, ratio))
    assert sm["final_residual"] < 1e-9 and sj["final_residual"] < 1e-9, (sm, sj)
    nv = 3 * prob.mesh["n_vnodes"]
    assert np.abs(xm[:nv] - xj[:nv]).max() < 1e-7, (sm, sj)
    assert sm["linear_iterations"] < sj["linear_iterations"], (sm, sj, ratio)
    _, s32, _ = _newton_box(32, True)
    print("periodic 32^3 Newton: multigrid %s" % (s32,))
    assert s32["final_residual"] < 1e-9, s32
    assert s32["linear_iterations"] <= sm["linear_iterations"] + 2, (s32, sm)


@pytest.mark.gpu
def test_periodic_attach_refusals_keep_the_hierarchy():
    """GLS_EINVAL, and the hierarchy attached before still answers gls_apply_preconditioner with the same bits: a level
    whose numbering is not the wrapped lattice (the level is named), a distributed level and a distributed context
    with a non-zero mask"""
    import softx_2020_200_amd as sx
    from softx_2020_200_amd import GLSError
    from softx_2020_200_amd.dist import Exchanger, attach, partition
    from softx_2020_200_amd.problem import PeriodicBoxProblem, build_context
    per = (0, 1, 2)
    prob = PeriodicBoxProblem(n=8, k=2, periodic=per, multigrid=True, pre_smooth=1, post_smooth=1, omega=0.9)
    ctx = prob.ctx
    ctx.set_time("bdf2", (0.05,) * 4)
    u = cuda(prob.taylor_green(0.0))
    ctx.set_state(u, u, u)
    v = cuda(np.random.default_rng(20200200).uniform(-1, 1, ctx.n_dofs))
    z0 = ctx.apply_preconditioner(v).cpu().numpy()
    assert np.isfinite(z0).all() and np.abs(z0).max() > 0

    def still_answers():
        assert np.array_equal(ctx.apply_preconditioner(v).cpu().numpy(), z0)

    # (a) level 1 with two node ids exchanged: the same counts, not the lattice
    mesh = sx.hyper_cube(3, 4, 2, 2, 0.0, 2.0 * np.pi, periodic=per)
    bad = dict(mesh)
    cv = mesh["cell_vnodes"].copy()
    cv[mesh["cell_vnodes"] == 1], cv[mesh["cell_vnodes"] == 2] = 2, 1
    bad["cell_vnodes"], bad["cell_pnodes"] = cv, cv.copy()
    bad_ctx = build_context(bad, viscosity=0.01)
    with pytest.raises(GLSError) as e:
        ctx.attach_multigrid([bad_ctx], periodic=per)
    assert "level 1" in str(e.value) and "lattice" in str(e.value), str(e.value)
    still_answers()
    # (b) a distributed level / context (one rank's partition of the whole mesh; the exchange is never called)
    plan = partition(mesh["cell_vnodes"], mesh["n_vnodes"], 0, 1)
    dctx = sx.GLSContext(3, 2, 2, plan["local_cells"], None, mesh["cell_h"], mesh["n_vnodes"], mesh["n_vnodes"],
                         viscosity=0.01, cell_x0=mesh["cell_x0"])
    attach(dctx, plan, Exchanger(plan, "cuda", backend="gloo"))
    with pytest.raises(GLSError) as e:
        ctx.attach_multigrid([dctx], periodic=per)
    assert "distributed" in str(e.value), str(e.value)
    still_answers()
    with pytest.raises(GLSError) as e:
        dctx.attach_multigrid([prob.levels[0].ctx], periodic=per)
    assert "distributed" in str(e.value), str(e.value)
    still_answers()
