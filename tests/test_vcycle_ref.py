"""CPU self-tests of tests/vcycle_ref.py, the numpy restatement of the multigrid V-cycle that
tests/test_gpu_vcycle_reference.py holds the device to (no GPU, nothing of the library):

  * the prolongation is the coarse Qk interpolant (oracle.evaluate_field), its rows sum to 1, the injection is a
    bijection onto the coarse DoFs;
  * the FP64 cycle stands on its own rounding: in np.longdouble (sparse products in extended precision, the coarse
    solve refined four times around the FP64 LU) it moves by less than 1e-12 per block;
  * the reference can tell a wrong cycle from a right one at the bound the GPU test applies: for every case, every
    applicable mutation (a damping off by 0.01, one interpolation weight, coarse constrained rows not zeroed, no
    pressure pin, no injected history, coarse state not constrained) moves the result, in at least one block, by at
    least ten times that block's bound. A condition on the cases' inputs, not a measurement: the bounds are
    vcycle_ref.bounds (4 x the FP32 emulation's distance, or max(1e-12, kappa eps))."""
import numpy as np
import pytest

from oracle.oracle import evaluate_field
from tests import vcycle_ref as vr


@pytest.mark.parametrize("k,kp", [(1, 1), (2, 2), (2, 1)])
def test_prolongation_is_the_coarse_interpolant(k, kp):
    H = vr.hierarchy(4, k, kp, "cavity")
    pf, pc = H["probs"][:2]
    P, inj = H["P"][0], H["inj"][0]
    assert P.shape == (pf.n_dofs, pc.n_dofs)
    c = np.random.default_rng(vr.SEED).uniform(-1, 1, pc.n_dofs)
    vel, _ = evaluate_field(pc, c, vr.lattice_coords(pf, k))
    _, pre = evaluate_field(pc, c, vr.lattice_coords(pf, kp))
    want = np.concatenate([vel.reshape(-1), pre])
    err = np.abs(P @ c - want).max()
    print("Q%d-Q%d: |P c - evaluate_field| %.2e" % (k, kp, err))
    assert err <= 1e-13
    assert np.abs(np.asarray(P.sum(axis=1)).ravel() - 1.0).max() <= 1e-14
    assert not (P.data == 0.0).any()
    # injection: a bijection onto the coarse DoFs, and P restricted to its rows is the identity
    assert inj.shape == (pc.n_dofs,) and len(np.unique(inj)) == pc.n_dofs and inj.min() >= 0 and inj.max() < pf.n_dofs
    assert abs(P[inj] - np.eye(pc.n_dofs)).max() == 0.0
    # the coarse nodes sit where their injection sources do, component by component
    Xf = np.concatenate([np.repeat(vr.lattice_coords(pf, k), 3, 0), vr.lattice_coords(pf, kp)])
    Xc = np.concatenate([np.repeat(vr.lattice_coords(pc, k), 3, 0), vr.lattice_coords(pc, kp)])
    assert np.array_equal(Xf[inj], Xc)
    nvf, nvc = 3 * pf.n_vnodes, 3 * pc.n_vnodes
    assert np.array_equal(inj[:nvc] % 3, np.arange(nvc) % 3) and (inj[:nvc] < nvf).all() and (inj[nvc:] >= nvf).all()


def test_three_level_hierarchy_and_constrained_rows_nest():
    H = vr.hierarchy(8, 2, 2, "cavity")
    assert [p.n for p in H["probs"]] == [8, 4, 2] and [p.n_dofs for p in H["probs"]] == [19652, 2916, 500]
    for l in range(2):
        con_f = np.zeros(H["probs"][l].n_dofs, bool)
        con_f[H["con"][l]] = True
        # a coarse DoF is constrained exactly where its injection source is
        assert np.array_equal(np.nonzero(con_f[H["inj"][l]])[0], H["con"][l + 1])
    Hf = vr.hierarchy(4, 2, 2, "free_face")
    Xv = vr.lattice_coords(Hf["probs"][0], 2)
    face0 = (Xv[:, 0] == -1.0) & (np.abs(Xv[:, 1]) < 1.0) & (np.abs(Xv[:, 2]) < 1.0)
    assert face0.sum() == 49 and not Hf["probs"][0].constrained[:3 * len(Xv)].reshape(-1, 3)[face0].any()


def test_coarse_state_is_injected_and_only_u_constrained():
    ops = vr.case_ops("fp64_v11")
    H = ops["H"]
    (u, u1, u2), (uc, u1c, u2c) = ops["state"]
    inj, con_c = H["inj"][0], H["con"][1]
    free = np.setdiff1d(np.arange(len(uc)), con_c)
    assert np.array_equal(uc[free], u[inj][free]) and np.array_equal(u1c, u1[inj]) and np.array_equal(u2c, u2[inj])
    want = np.array([H["probs"][1].dirichlet[d] for d in con_c])
    assert np.array_equal(uc[con_c], want) and set(want) == {0.0, 1.0}
    assert not np.array_equal(u[inj][con_c], want)  # the constraining is not vacuous at this state


def test_fp64_cycle_is_at_its_precision_floor():
    """n = 4 Q2-Q2 V(1,1): the cycle in np.longdouble against the FP64 cycle, per block below 1e-12 (measured 1.8e-14
    on both)"""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not extended precision here"
    name = "fp64_v11"
    c = vr.CASES[name]
    ops = vr.case_ops(name)
    v = vr.rhs_vector(ops["A"][0].shape[0])
    zl = vr.Cycle(ops, vr.level_sweep_list(c), c["omega"], c["coarse"], dtype=np.longdouble)(v)
    assert zl.dtype == np.longdouble
    eu, ep = vr.block_errors(name, vr.reference(name).astype(np.longdouble), zl)
    print("FP64 cycle against the longdouble cycle: velocity %.2e, pressure %.2e" % (eu, ep))
    assert eu < 1e-12 and ep < 1e-12, (eu, ep)


def test_case_table_and_applicable_mutations():
    assert len(vr.CASES) == 15
    assert vr.level_sweep_list(vr.CASES["f32_3lev_bench"]) == [(1, 1), (2, 2)]  # bench.py's layout: V(2,2) above the coarsest
    assert vr.level_sweep_list(vr.CASES["fp64_v01"]) == [(0, 1)]
    for name, c in vr.CASES.items():
        muts = vr.applicable_mutations(c)
        assert {"omega", "tap", "nozero_c"} <= set(muts), name
        assert ("nopin" in muts) == (c["coarse"][0] == "direct"), name
        assert ({"nohist", "noconstrain"} <= set(muts)) == (c["variant"] != "const"), name


@pytest.mark.parametrize("name", list(vr.CASES))
def test_bounds_and_discrimination(name):
    c = vr.CASES[name]
    z = vr.reference(name)
    bd = vr.bounds(name)
    nv = 3 * (c["k"] * c["n"] + 1) ** 3
    print("%s: max|z_u| %.3e, max|z_p| %.3e, kappa %.3e, bounds %.3e (velocity) %.3e (pressure)" %
          (name, np.abs(z[:nv]).max(), np.abs(z[nv:]).max(), vr.coarse_condition(name), bd[0], bd[1]))
    assert np.isfinite(z).all() and np.abs(z[:nv]).max() > 0 and np.abs(z[nv:]).max() > 0
    if c["fp32"]:
        # an FP32 bound stays an FP32-sized figure: a few thousand roundings of 6e-8 at the most
        assert all(4 * 6e-8 <= b <= 1e-4 for b in bd), bd
    else:
        assert bd[0] == bd[1] == max(1e-12, vr.coarse_condition(name) * 2.2e-16) and bd[0] <= 1e-9, bd
    missed = []
    for m in vr.applicable_mutations(c):
        d = vr.block_errors(name, vr.reference(name, mut=m), z)
        print("   %-12s moves velocity %.3e (%.1f x bound), pressure %.3e (%.1f x bound)" %
              (m, d[0], d[0] / bd[0], d[1], d[1] / bd[1]))
        if not (d[0] >= 10 * bd[0] or d[1] >= 10 * bd[1]):
            missed.append((m, d))
    assert not missed, (name, bd, missed)
