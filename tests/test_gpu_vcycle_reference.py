"""GPU: the multigrid V-cycle z = M^-1 v (gls_mg_attach / gls_mg_attach_transfers, gls_apply_preconditioner) against
tests/vcycle_ref.py, the numpy FP64 restatement built from the oracle's assembled matrices and a prolongation formed
from node coordinates. Nothing here compares one device path with another, and no bound is a constant of this file.

Metric: the velocity block and the pressure block separately, max |z_dev - z_ref| / max |z_ref| over the block (the
pressure block is some 300 times larger on the cavity: one bound on the whole vector would hide the velocity).
Bounds (vcycle_ref.bounds, from the reference alone):
  * FP64 smoothing: max(1e-12, kappa eps), kappa = cond of the pinned coarsest matrix on the direct route (the forward
    error of a backward-stable solve), 1 on the sweeps route;
  * FP32 smoothing: 4 x the distance of the reference's FP32 emulation from the FP64 reference, per block.
tests/test_vcycle_ref.py shows on the CPU that every wrong variant of the cycle it knows moves the reference by at least
ten times these bounds. A case that names a fused path asserts that the path is taken at its size.

The levels are the reference's own oracle problems; equal-order levels take the library's Morton-ordered cell arrays
(as tests/test_gpu_parity.py::_morton_problem) and must run the brick kernels."""
import copy

import numpy as np
import pytest

from gpu_util import context_for, cuda
from tests import vcycle_ref as vr

_dev = {}


def _device_problem(p):
    """the oracle problem as the device takes it: equal-order levels with the Morton-ordered hyper_cube cell arrays"""
    if p.k != p.kp:
        return p
    import softx_2020_200_amd as sx
    q = copy.copy(p)
    m = sx.hyper_cube(3, p.n, p.k, p.k, -1.0, 1.0)
    for key in ("cell_vnodes", "cell_pnodes", "cell_x0", "cell_h"):
        setattr(q, key, np.ascontiguousarray(m[key]))
    return q


def _contexts(name):
    """the case's device levels (built once per hierarchy and shared), fine first"""
    c = vr.CASES[name]
    key = (c["n"], c["k"], c["kp"], c["variant"])
    if key not in _dev:
        H = vr.hierarchy(*key)
        ctxs = [context_for(_device_problem(p)) for p in H["probs"]]
        for ctx, p in zip(ctxs, H["probs"]):
            assert ctx.uses_brick_kernels == (p.k == p.kp), (p.n, p.k, p.kp)
            assert ctx.n_dofs == p.n_dofs
        _dev[key] = ctxs
    return _dev[key]


def _attach(name):
    """the case's hierarchy attached with the case's parameters at the case's state; (fine context, all contexts)"""
    c = vr.CASES[name]
    ops = vr.case_ops(name)
    H = ops["H"]
    ctxs = _contexts(name)
    pre, post = c["sweeps"]
    kw = dict(pre_smooth=pre if pre > 0 else -1, post_smooth=post, omega=c["omega"], level_sweeps=c["level_sweeps"])
    if c["coarse"][0] == "direct":
        kw.update(coarse_direct=1)
    else:
        kw.update(coarse_direct=-1, coarse_sweeps=c["coarse"][1], coarse_omega=c["coarse"][2])
    if c["general"]:
        xfer = [(P.indptr, P.indices, P.data, inj) for P, inj in zip(H["P"], H["inj"])]
        ctxs[0].attach_multigrid_transfers(ctxs[1:], xfer, smoother="jacobi", mixed_precision=0, **kw)
    else:
        ctxs[0].attach_multigrid(ctxs[1:], mixed_precision=1 if c["fp32"] else 0, smoother_operator=1 if c["oseen"] else 0,
                                 **kw)
    st = ops["state"][0]
    ctxs[0].set_state(*[cuda(a) for a in (st[:1] if c["variant"] == "const" else st)])
    return ctxs[0], ctxs


def _fused_reports(ctxs):
    """per level pair (restriction fused, prolongation fused), as gls_mg_residual_restrict / gls_mg_prolong_smooth
    report them (zero vectors: only the reports are read)"""
    out = []
    for l in range(len(ctxs) - 1):
        x, b = ctxs[l].zeros(), ctxs[l].zeros() + 1.0
        xc, bc = ctxs[l + 1].zeros(), ctxs[l + 1].zeros()
        out.append((ctxs[0].mg_residual_restrict(l, x, b, bc)[1], ctxs[0].mg_prolong_smooth(l, xc, x, b, 0.9)[1]))
    return out


def _judge(tag, got, ref, nv, bounds):
    """print error, bound and ratio per block, then assert"""
    errs = []
    for blk, s, bd in (("velocity", slice(0, nv), bounds[0]), ("pressure", slice(nv, None), bounds[1])):
        e = float(np.abs(got[s] - ref[s]).max() / np.abs(ref[s]).max())
        print("vcycle_reference %s %s: device error %.3e, bound %.3e, ratio %.3f" % (tag, blk, e, bd, e / bd))
        errs.append((blk, e, bd))
    assert np.isfinite(got).all()
    for blk, e, bd in errs:
        assert e <= bd, (tag, blk, e, bd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(vr.CASES))
def test_vcycle_against_reference(name, monkeypatch):
    c = vr.CASES[name]
    for sw in ("GLS_MG_NO_FUSE", "GLS_MG_FUSE_TRANSFER", "GLS_MG_FUSE_PROLONG", "GLS_MG_FIRST_PRODUCER", "GLS_MG_GRAPH"):
        monkeypatch.delenv(sw, raising=False)
    ctx, ctxs = _attach(name)
    z_ref = vr.reference(name)
    bounds = vr.bounds(name)
    nv = 3 * (c["k"] * c["n"] + 1) ** 3
    assert len(ctxs) == (3 if c["n"] == 8 else 2)
    # liveness: the FP32 brick hierarchies fuse restriction and prolongation on every level pair, nothing else does
    fused = _fused_reports(ctxs)
    want = c["fp32"] and not c["general"]
    assert fused == [(want, want)] * (len(ctxs) - 1), (name, fused)
    v = cuda(vr.rhs_vector(ctx.n_dofs))
    z = ctx.apply_preconditioner(v).cpu().numpy()
    _judge(name, z, z_ref, nv, bounds)
    if name == "f32_coarse_sweeps":  # the coarsest level's sweeps as one captured graph, and its replay
        monkeypatch.setenv("GLS_MG_GRAPH", "1")
        for tag in ("graph", "graph-replay"):
            _judge(name + "[%s]" % tag, ctx.apply_preconditioner(v).cpu().numpy(), z_ref, nv, bounds)
        monkeypatch.delenv("GLS_MG_GRAPH")


@pytest.mark.gpu
@pytest.mark.parametrize("l", [0, 1])
def test_level_pieces_against_reference(l, monkeypatch):
    """on the n = 8 FP32 hierarchy, level pair by level pair: the fused residual restriction against
    P^T (b - A x) with the constrained coarse rows zeroed, and the fused prolongation + sweep against one sweep from
    x + P x_c; bounds: 4 x the FP32 emulation's distance for that single operation, per block"""
    name = "f32_3lev_bench"
    for sw in ("GLS_MG_NO_FUSE", "GLS_MG_FUSE_TRANSFER", "GLS_MG_FUSE_PROLONG", "GLS_MG_FIRST_PRODUCER", "GLS_MG_GRAPH"):
        monkeypatch.delenv(sw, raising=False)
    ctx, ctxs = _attach(name)
    probs = vr.case_ops(name)["H"]["probs"]
    x, b, xc = vr.piece_vectors(name, l)
    nvf, nvc = 3 * probs[l].n_vnodes, 3 * probs[l + 1].n_vnodes

    def bound(ref64, ref32, nv):
        return tuple(vr.FP32_FACTOR * float(np.abs(ref32[s] - ref64[s]).max() / np.abs(ref64[s]).max())
                     for s in (slice(0, nv), slice(nv, None)))
    # restriction
    want = vr.residual_restrict(name, l, x, b)
    bd = bound(want, vr.residual_restrict(name, l, x, b, fp32=True), nvc)
    out, fused = ctx.mg_residual_restrict(l, cuda(x), cuda(b), ctxs[l + 1].zeros())
    assert fused
    _judge("%s restrict level %d" % (name, l), out.cpu().numpy(), want, nvc, bd)
    # prolongation + one sweep
    want = vr.prolong_smooth(name, l, xc, x, b, 0.9)
    bd = bound(want, vr.prolong_smooth(name, l, xc, x, b, 0.9, fp32=True), nvf)
    got, fused = ctx.mg_prolong_smooth(l, cuda(xc), cuda(x), cuda(b), 0.9)
    assert fused
    _judge("%s prolong+sweep level %d" % (name, l), got.cpu().numpy(), want, nvf, bd)
