"""Helpers shared by the GPU parity tests: build a product context from an oracle problem."""
import numpy as np


def vnode_mask_of(p):
    """zero_constraints mask of the Dirichlet DoFs (hanging DoFs are passed as lines, not masked)."""
    c = p.constrained[:p.dim * p.n_vnodes].copy()
    if getattr(p, "hang", None) is not None:
        c[np.nonzero(p.hang[0][1:p.dim * p.n_vnodes + 1] > p.hang[0][:p.dim * p.n_vnodes])[0]] = 0
    c = c.reshape(p.n_vnodes, p.dim).astype(np.uint8)
    m = np.zeros(p.n_vnodes, dtype=np.uint8)
    for d in range(p.dim):
        m |= c[:, d] << d
    return m


def discrete_space_of(p):
    """What the product takes from an oracle problem's mesh and constraints: the cells' nodes (pressure nodes None
    when the pressure sits on the velocity nodes), the Dirichlet mask and the lines. context_for builds the device
    context from it and ilu_plan_for the host-only ILU plan."""
    return dict(cell_vnodes=p.cell_vnodes, cell_pnodes=p.cell_pnodes if p.kp != p.k else None,
                vnode_mask=vnode_mask_of(p), lines=getattr(p, "hang_lines", None))


def context_for(p, **kw):
    from softx_2020_200_amd import GLSContext
    mapped = getattr(p, "cell_support", None) is not None
    if mapped:
        kw = dict(kw, map_degree=p.map_degree, cell_support=p.cell_support)
    s = discrete_space_of(p)
    ctx = GLSContext(p.dim, p.k, p.kp, s["cell_vnodes"], s["cell_pnodes"],
                     None if mapped else p.cell_h, p.n_vnodes, p.n_pnodes, viscosity=p.viscosity,
                     cell_x0=None if mapped else p.cell_x0, vnode_mask=s["vnode_mask"],
                     force_q=p.force_q, srf=p.srf, omega=p.omega, **kw)
    ctx.set_time(p.scheme, p.time_steps)
    if s["lines"] is not None:
        ctx.set_hanging(*s["lines"])
    if p.dirichlet:
        dofs = np.array(sorted(p.dirichlet), dtype=np.int64)
        ctx.set_dirichlet(dofs, np.array([p.dirichlet[d] for d in dofs]))
    return ctx


def ilu_plan_for(p, fill=0, ordering="cm", block_dofs=0):
    """The host-only plan (native.ilu_plan) of context_for(p).attach_ilu(fill=, ordering=, block_dofs=): the
    constrained DoFs are the mask's and the lines', as the context derives them (gls_create, gls_set_hanging)."""
    from softx_2020_200_amd.native import ilu_plan
    s = discrete_space_of(p)
    node, comp = np.nonzero((s["vnode_mask"][:, None] >> np.arange(p.dim)) & 1)
    con = node * p.dim + comp
    if s["lines"] is not None:
        con = np.union1d(con, np.asarray(s["lines"][0], dtype=np.int64))
    return ilu_plan(p.dim, p.k, p.kp, p.n_vnodes, p.n_pnodes, s["cell_vnodes"], s["cell_pnodes"], con, s["lines"],
                    fill=fill, ordering=ordering, block_dofs=block_dofs)


def cuda(a):
    import torch
    return torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")


def relerr(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
