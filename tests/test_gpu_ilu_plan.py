"""The host-only ILU plan (native.ilu_plan, tests/test_ilu_plan.py) is what gls_ilu_attach really uses: an attached
context's renumbering, pattern and counts equal the host export's."""
import numpy as np
import pytest

from tests.gpu_util import context_for, cuda, ilu_plan_for
from tests.test_ilu_plan import problem_and_state


@pytest.mark.gpu
@pytest.mark.parametrize("dim,n,k,kp,fill,order,blk", [(2, 4, 1, 1, 1, "cm", 0), (3, 2, 2, 1, 0, "multicolor", 0),
                                                      (3, 2, 2, 2, 0, "multicolor", 200)])
def test_attached_context_uses_the_host_plan(dim, n, k, kp, fill, order, blk):
    p, state = problem_and_state("cavity", dim, n, k, kp)
    ctx = context_for(p)
    ctx.set_time(p.scheme, p.time_steps)
    ctx.set_state(*[cuda(s) for s in state])
    nnz, n_probes = ctx.attach_ilu(1e-5, 1.0, fill=fill, ordering=order, block_dofs=blk)
    perm, F = ctx.ilu_factors()
    P = ilu_plan_for(p, fill=fill, ordering=order, block_dofs=blk)
    assert (nnz, n_probes) == (P["nnz"], P["n_probes"])
    assert np.array_equal(perm, P["perm"])
    assert np.array_equal(F.indptr, P["rowp"]) and np.array_equal(F.indices, P["col"])
