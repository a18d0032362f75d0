"""The multigrid after its move out of gls_api.cpp (gls_mg.cpp, gls_mg_coarse.cpp) against the library before the
move: one V-cycle application and a GMRES solve on every route of the coarsest-level solve, compared with
tests/golden/mg_parent.json (recorded by tests/golden/make_mg_parent.py at the commit before the split). A case
whose two recordings agreed bit for bit is held to the SHA-256 of its result; the others (rocSOLVER / rocBLAS
routes that were not repeatable at the parent itself) to the stored vector within ten times the recordings' own
difference relative to max|z| (floor 1e-14). The GMRES iteration count is the parent's exactly. The FP32 worker
route (n > 8192) is test_gpu_umesh_mg.py::test_large_coarsest_level_fp32_lu's."""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOLVER_ENV = "GLS_MG_COARSE_SOLVER"
# name -> (kind, size, coarse_direct, GLS_MG_COARSE_SOLVER)
CASES = {
    "cavity4_jacobi_sweeps": ("cavity", 4, -1, None),    # damped-Jacobi coarsest sweeps, no dense solve
    "cavity4_lu": ("cavity", 4, 1, None),                # FP64 unpivoted LU, check, explicit inverse
    "cavity8_lu": ("cavity", 8, 1, None),
    "cavity8_lu_pivoted": ("cavity", 8, 1, "lu"),        # FP64 pivoted LU
    "cavity4_gauss_jordan": ("cavity", 4, 1, "gj"),      # the Gauss-Jordan kernel
    "octree_ilu_csr_probe": ("octree", 0, 1, None),      # two general-mesh levels, ILU smoothing, ILU-CSR probe
    "replica_two_level": ("replica", 0, 1, None),        # mg_vcycle_rep2 with the replica solved exactly
}
SOLVE = dict(max_iterations=500, restart=50, relative_residual=1e-8)


def _cavity(n, coarse_direct):
    """the Q2-Q2 bdf2 cavity hierarchy, state and seeded vector of test_gpu_mg_fused_transfers.py"""
    from tests.test_gpu_mg_fused_transfers import _Hierarchy
    h = _Hierarchy(n)
    h.ctx.attach_multigrid(h.ctxs[1:], pre_smooth=1, post_smooth=1, omega=0.9, coarse_direct=coarse_direct,
                           mixed_precision=1, smoother_operator=1)
    h.ctx.set_state(h.state[0], h.state[0], h.state[1])
    return h.ctx, h.v, h


def _general_state(p, Xv, Xp, dim):
    u = np.concatenate([np.stack([np.sin(Xv[:, 0] + Xv[:, d]) for d in range(dim)], 1).reshape(-1), np.cos(Xp[:, 0])])
    p.apply_nonzero_constraints(u)
    return u


def _octree():
    """the smallest adapted forest of test_gpu_octree_mg.py (Q2-Q1, per-cell levels) and its once-coarsened level:
    ILU(0) smoothing on the fine level, the coarse matrix densified from the probing ILU's CSR"""
    import softx_2020_200_amd as sx
    from gpu_util import context_for, cuda
    from tests.test_gpu_octree_mg import level_problem
    from tests.test_octree_mg import adapted_tree
    tree = adapted_tree(3, 2, 2)
    trees = [tree, tree.coarsen_to(tree.max_level - 1)]
    probs = [level_problem(t, 2, 1, 0.1, "bdf1") for t in trees]
    hf, hc = trees[0].mesh_handle(2, 1), trees[1].mesh_handle(2, 1)
    try:
        xfer = [sx.octree_mg_transfer(hf, hc)]
    finally:
        trees[0].free_mesh_handle(hf)
        trees[1].free_mesh_handle(hc)
    assert probs[1].n_dofs <= 8192, probs[1].n_dofs
    ctxs = [context_for(q) for q in probs]
    ctxs[0].attach_multigrid_transfers(ctxs[1:], xfer, pre_smooth=1, post_smooth=1, omega=0.6, coarse_direct=1,
                                       smoother="ilu")
    mesh = trees[0].mesh(2, 1)
    p = probs[0]
    U = cuda(_general_state(p, mesh["vnode_x"], mesh["pnode_x"], 3))
    ctxs[0].apply_dirichlet(U)
    ctxs[0].set_state(U, cuda(np.zeros(p.n_dofs)))
    v = cuda(np.random.default_rng(20200200).uniform(-1, 1, p.n_dofs))
    return ctxs[0], v, ctxs


def _replica():
    """test_gpu_dist_mg.py's two-level case on one process (a one-rank gloo group): the fine level distributed,
    its coarser level the replica, solved exactly (coarse_direct=1)"""
    import tempfile

    import torch.distributed as dist
    from gpu_util import context_for, cuda, vnode_mask_of
    from softx_2020_200_amd.dist import DistributedGeneralProblem, attach_replica_multigrid
    from tests.test_gpu_dist_mg import _levels
    space, probs, xfer, lines, u, dim = _levels(("cylshell", 2, 1, "jacobi", True))
    p = probs[0]
    store = tempfile.NamedTemporaryFile(prefix="gls_mg_split_", delete=False)
    store.close()
    dist.init_process_group("gloo", init_method="file://" + store.name, rank=0, world_size=1)
    dirs = np.array(sorted(p.dirichlet), np.int64)
    dp = DistributedGeneralProblem(space, 0, 1, "cuda", viscosity=0.1, vnode_mask=vnode_mask_of(p),
                                   dirichlet=(dirs, np.array([p.dirichlet[d] for d in dirs])), lines=lines,
                                   force_q=p.force_q)
    c = dp.ctx
    c.set_time(p.scheme, p.time_steps)
    replica = context_for(probs[1])
    attach_replica_multigrid(dp, replica, xfer[0], coarse_direct=1, pre_smooth=2, post_smooth=2, omega=0.6,
                             smoother="jacobi")
    Ud = cuda(dp.local(u))
    c.apply_dirichlet(Ud)
    c.set_state(Ud, cuda(np.zeros(len(dp.plan["l2g_dofs"]))))
    v = cuda(dp.local(np.random.default_rng(20200200).uniform(-1, 1, p.n_dofs)))
    return c, v, (dp, replica, store.name)


def run_case(name):
    """(z = apply_preconditioner(v) as a host array, GMRES iterations of the solve on the residual)"""
    kind, n, coarse_direct, solver = CASES[name]
    old = os.environ.pop(SOLVER_ENV, None)
    if solver:
        os.environ[SOLVER_ENV] = solver  # read at attach (the Gauss-Jordan buffer) and at every preparation
    try:
        ctx, v, keep = _cavity(n, coarse_direct) if kind == "cavity" else _octree() if kind == "octree" else _replica()
        try:
            z = ctx.apply_preconditioner(v).cpu().numpy()
            b = ctx.residual().clone()
            _, its, res, ok = ctx.solve_linear(b, **SOLVE)
            assert ok, (name, its, res)
        finally:
            if kind == "replica":
                import torch.distributed as dist
                del ctx, keep
                dist.destroy_process_group()
    finally:
        os.environ.pop(SOLVER_ENV, None)
        if old is not None:
            os.environ[SOLVER_ENV] = old
    return z, int(its)


def digest(z):
    return hashlib.sha256(np.ascontiguousarray(z).tobytes()).hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_vcycle_and_solve_match_the_parent(name):
    with open(os.path.join(GOLDEN, "mg_parent.json")) as f:
        gold = json.load(f)["cases"][name]
    z, its = run_case(name)
    assert z.shape == (gold["n_dofs"],) and np.abs(z).max() > 0
    if "sha256" in gold:
        print("%s: %d DoFs, GMRES its %d (parent %d), sha256 %s (parent %s)" % (name, z.size, its, gold["gmres_its"],
                                                                               digest(z)[:16], gold["sha256"][:16]))
        assert digest(z) == gold["sha256"]
    else:
        ref = np.load(os.path.join(GOLDEN, "mg_parent.npz"))[name]
        rel = np.abs(z - ref).max() / np.abs(ref).max()
        print("%s: %d DoFs, GMRES its %d (parent %d), max rel difference %.3e (tolerance %.3e)" % (
            name, z.size, its, gold["gmres_its"], rel, gold["tolerance"]))
        assert rel <= gold["tolerance"], (rel, gold["tolerance"])
    assert its == gold["gmres_its"], (its, gold["gmres_its"])
