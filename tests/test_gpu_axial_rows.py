"""GPU: the fast solve kernel (k_solve_lds) streams the axial wave-table row only of the nodes
that need it (axial side drag or end drag: AQ CDQ != 0 or AEND CDEND != 0).

  1. the skip against no skip (rh_set_solver(ctx, 6): every node treated as axial), bit for bit,
     on every instantiation of the kernel;
  2. designs that move the axial set (every node, the rectangular members only, none) against
     the CPU oracle on the same tables;
  3. those designs through the general kernel k_solve_cases, which keeps the three-row arithmetic.
"""
import copy

import numpy as np
import pytest

from conftest import load_design, load_golden, oracle_tables_of, statics_of
from oracle import raft_oracle as O

pytestmark = pytest.mark.gpu
RTOL = 1e-9   # of test_gpu_parity.test_batch_matches_oracle_nw200


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def make_model(design, T, settings=None):
    """A model of a design dict (or a design name) on the statics of golden T."""
    import raft
    d = load_design(design) if isinstance(design, str) else copy.deepcopy(design)
    if settings:
        d["settings"].update(settings)
    m = raft.Model(d, statics=[statics_of(T)])
    f = m.fowtList[0]
    f.setPosition(T["r6"])
    f.calcStatics()
    f.calcHydroConstants()
    return m, f


def random_cases(n, seed, headings=(0, 30, 60, 90)):
    rng = np.random.default_rng(seed)
    return [dict(wave_spectrum="JONSWAP", wave_period=float(rng.uniform(6, 18)), wave_height=float(rng.uniform(1, 10)),
                 wave_heading=float(rng.choice(headings)), wave_gamma=float(rng.choice([0.0, 0.0, 1.0, 3.3])))
            for _ in range(n)]


class solver_mode:
    """rh_set_solver(ctx, which) for the block, the default restored after it."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        from raft import _native as N
        N.check(N.lib().rh_set_solver(N.context(0), self.which), "rh_set_solver")

    def __exit__(self, *exc):
        from raft import _native as N
        N.check(N.lib().rh_set_solver(N.context(0), 0), "rh_set_solver")


# (golden for the statics, design, nw or None for the design's own grid, the kernel it runs)
GRIDS = [("c2_nw200", "VolturnUS-S_example", 77, "<1,128,true>, pad lanes"),
         ("c2_nw200", "VolturnUS-S_example", 200, "<2,128,true>"),
         ("c2_nw200", "VolturnUS-S_example", 333, "<1,512,false>"),
         ("c2_nw200", "VolturnUS-S_example", 513, "<2,512,false,1>, a whole pad wave"),
         ("c2_nw200", "VolturnUS-S_example", 1025, "<2,512,false,2>: two passes"),
         ("c1_OC3spar", "OC3spar", None, "axial nodes in the middle of a member")]


@pytest.mark.parametrize("tag,design,nw,what", GRIDS, ids=[f"{g[1]}-{g[2]}" for g in GRIDS])
def test_skip_against_no_skip_bit_for_bit(tag, design, nw, what):
    """The default kernel against the same kernel with every node in its axial list
    (rh_set_solver(ctx, 6)): what the skip leaves out is multiplied by exact zeros, so every
    output has the same bits."""
    T = load_golden(tag)
    m, f = make_model(design, T, {"min_freq": 0.2 / nw} if nw else None)
    if nw:
        assert m.nw == nw
    else:
        assert m.nw == 80
    cases = random_cases(12, 5)
    want = ("psd", "std", "zeta", "B_drag", "rao", "margin")
    a = m.analyzeCasesBatch(cases, want=want)
    with solver_mode(6):
        b = m.analyzeCasesBatch(cases, want=want)
    for k in ("iters", "status", "Xi", "psd", "std", "rao", "zeta", "B_drag", "margin"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_skip_against_no_skip_fixed_point_form():
    """The same through solve_batch without the response (the C4 fixed-point form)."""
    from raft.solver import CaseSet, solve_batch
    T = load_golden("c2_nw200")
    m, f = make_model("VolturnUS-S_example", T)
    assert m.nw == 200
    cases = random_cases(12, 5)
    cs = CaseSet(np.zeros(len(cases), dtype=np.int32), [c["wave_heading"] for c in cases], ["JONSWAP"] * len(cases),
                 [c["wave_height"] for c in cases], [c["wave_period"] for c in cases],
                 [c["wave_gamma"] for c in cases])
    dd = f.device_design()
    want = ("zeta", "B_drag", "Bmat", "noXi")
    a = solve_batch([dd], cs, m.nIter, m.XiStart, 0.01, want=want).host()
    with solver_mode(6):
        b = solve_batch([dd], cs, m.nIter, m.XiStart, 0.01, want=want).host()
    for k in ("iters", "status", "zeta", "B_drag", "Bmat"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def variant_design(which):
    """VolturnUS-S_example with another set of axial nodes."""
    d = load_design("VolturnUS-S_example")
    for mem in d["platform"]["members"]:
        if which == "all":            # (i) axial side drag on every member: every node is axial
            mem["Cd_q"] = 0.3
        elif which == "pontoons":     # (ii) the axial set is exactly the rectangular members
            if mem["shape"] == "rect":
                mem["Cd_q"] = 0.4
            else:
                mem["CdEnd"] = 0.0
        elif which == "none":         # (iii) no node is axial
            mem["CdEnd"] = 0.0
        else:
            raise ValueError(which)
    return d


_VARIANT = {}


def variant(which):
    """(model, fowt, oracle tables, cases, oracle results) of a variant: computed once, shared."""
    if which not in _VARIANT:
        T0 = load_golden("c2_nw200")
        m, f = make_model(variant_design(which), T0)
        assert m.nw == 200
        T = oracle_tables_of(f)
        cases = random_cases(8, 31)
        ref = [O.solve_dynamics(T, dict(c), int(m.nIter), float(m.XiStart)) for c in cases]
        _VARIANT[which] = (m, f, T, cases, ref)
    return _VARIANT[which]


def test_variants_move_the_axial_set():
    """The designs do what they are meant to (host side, from the oracle's node tables): every
    submerged node axial, only those of the rectangular members, none."""
    for which, expect in (("all", "all"), ("pontoons", "rect"), ("none", "none")):
        m, f, T, cases, ref = variant(which)
        sub = T["node_sub"] != 0
        axial = (T["node_Cd_q"] != 0) | (T["node_Cd_End"] != 0)
        if expect == "all":
            assert np.all(T["node_Cd_q"][sub] != 0)
        elif expect == "rect":
            assert np.all(T["node_Cd_q"][sub & (T["node_circ"] == 0)] != 0)
            assert not np.any(axial[sub & (T["node_circ"] != 0)])
        else:
            assert not np.any(axial[sub])


@pytest.mark.parametrize("which", ["all", "pontoons", "none"])
def test_variant_designs_match_oracle(which):
    """Identical iteration counts and convergence flags, Xi and B_drag within 1e-9 of the oracle."""
    m, f, T, cases, ref = variant(which)
    res = m.analyzeCasesBatch(cases, want=("B_drag",))
    print(which, "iters", res["iters"].tolist(), "oracle", [r["iters"] for r in ref])
    for ic, r in enumerate(ref):
        print(ic, rel(res["Xi"][ic], r["Xi"][0]), rel(res["B_drag"][ic], r["B_drag"]))
    for ic, r in enumerate(ref):
        assert res["iters"][ic] == r["iters"], (ic, res["iters"][ic], r["iters"])
        assert (res["status"][ic] == 1) == r["converged"], ic
        assert rel(res["Xi"][ic], r["Xi"][0]) < RTOL, ic
        assert rel(res["B_drag"][ic], r["B_drag"]) < RTOL, ic


def test_variant_cases_converge_early_and_late():
    """The 8 cases see more than one iteration count on at least one variant, on the device as
    in the oracle (both early and late convergence are exercised)."""
    seen = []
    for w in ("all", "pontoons", "none"):
        m, f, T, cases, ref = variant(w)
        res = m.analyzeCasesBatch(cases)
        seen.append(len(set(res["iters"].tolist())))
        assert len({r["iters"] for r in ref}) == seen[-1]
    assert max(seen) > 1, seen


@pytest.mark.parametrize("which", ["all", "pontoons"])
def test_variant_designs_fast_and_general_agree(which):
    """The default kernel against the general kernel k_solve_cases (rh_set_solver(ctx, 1)) on a
    design with Cd_q != 0: identical iteration counts and statuses, Xi and B_drag within 1e-12
    (as test_gpu_parity.test_fast_and_general_kernels_agree)."""
    m, f, T, cases, ref = variant(which)
    a = m.analyzeCasesBatch(cases, want=("B_drag",))
    with solver_mode(1):
        b = m.analyzeCasesBatch(cases, want=("B_drag",))
    np.testing.assert_array_equal(a["iters"], b["iters"])
    np.testing.assert_array_equal(a["status"], b["status"])
    for ic in range(len(cases)):
        assert rel(a["Xi"][ic], b["Xi"][ic]) < 1e-12, ic
        assert rel(a["B_drag"][ic], b["B_drag"][ic]) < 1e-12, ic
