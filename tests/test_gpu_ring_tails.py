"""GPU: the tails of the wave-table prefetch rings of k_solve_lds.

The node loops of phases A and C run whole ring rounds (4 nodes in phase A, 6 in phase C; the last
round ends in ghost nodes), and the axial rows go through short loops of their own, four at a time.
So the shapes at which they can go wrong are small node counts: every remainder modulo 4 and 6,
rings that never fill, a member of a single node, an axial last node, axial sets of 0, 1 and 5
nodes (one more than a batch of four), on grids that reach every instantiation of the kernel.

The designs are OC3spar / VolturnUS-S_example with members removed, raised or cut into longer
strips.  Each is checked three ways, 8 cases (headings 0 / 30 / 60 / 90):
  1. against the CPU oracle on the model's own tables: identical iteration counts, Xi and B_drag
     within 1e-9 (as test_gpu_axial_rows.test_variant_designs_match_oracle);
  2. against the general kernel k_solve_cases (rh_set_solver(ctx, 1)): identical iteration counts,
     1e-12;
  3. with every node treated as axial (rh_set_solver(ctx, 6)) against the default, at 1e-12 with
     identical iteration counts: phase C adds a member's axial sum SQ cq to F after the members'
     transverse sums, so a member without axial nodes adds +-0 there in that mode and the bits
     may differ only where an exact zero changes sign (bit for bit on every design here).
"""
import copy

import numpy as np
import pytest

from conftest import load_design, load_golden, oracle_tables_of
from oracle import raft_oracle as O
from test_gpu_axial_rows import make_model, random_cases, rel, solver_mode

pytestmark = pytest.mark.gpu
RTOL = 1e-9   # of test_gpu_axial_rows.test_variant_designs_match_oracle


def volturn(members):
    """VolturnUS-S_example with the listed members only, in the listed order, each with overrides."""
    d = load_design("VolturnUS-S_example")
    by_name = {m["name"]: m for m in d["platform"]["members"]}
    out = []
    for name, over in members:
        mem = copy.deepcopy(by_name[name])
        mem.update(over)
        out.append(mem)
    d["platform"]["members"] = out
    return d


def oc3(**over):
    d = load_design("OC3spar")
    d["platform"]["members"][0].update(over)
    return d


RAISED = dict(rA=[0, 0, -1], dlsMax=35)   # a column whose bottom end node alone is under water

# name: (golden of the statics, design, nw, nodes, member starts, axial nodes ('x') in node order)
DESIGNS = {
    "nn1": ("c2_nw200", lambda: volturn([("center_column", RAISED)]), 1000, 1, [0, 1], "x"),
    "nn2": ("c2_nw200", lambda: volturn([("center_column", dict(dlsMax=35))]), 200, 2, [0, 2], "x."),
    "nn3": ("c1_OC3spar", lambda: oc3(dlsMax=200), 500, 3, [0, 3], "x.x"),
    "nn4": ("c2_nw200", lambda: volturn([("pontoon", dict(heading=[60], dlsMax=21))]), 1030, 4, [0, 4], "...."),
    "nn5": ("c2_nw200", lambda: volturn([("center_column", dict(Cd_q=0.3))]), 1000, 5, [0, 5], "xxxxx"),
    "nn6": ("c1_OC3spar", lambda: oc3(dlsMax=30), 200, 6, [0, 6], "x....x"),
    "nn7": ("c2_nw200", lambda: volturn([("center_column", dict(dlsMax=18)), ("outer_column", dict(heading=[60]))]),
            1000, 7, [0, 2, 7], "x.x...."),
    "nn11": ("c2_nw200", lambda: volturn([("pontoon", dict(heading=[60]))]), 100, 11, [0, 11], "..........."),
    "nn12": ("c2_nw200", lambda: volturn([("pontoon", dict(heading=[60])),
                                          ("outer_column", dict(heading=[60], rA=[51.75, 0, -1], dlsMax=35))]),
             500, 12, [0, 11, 12], "...........x"),
    "nn13": ("c2_nw200", lambda: volturn([("center_column", dict(dlsMax=35)), ("pontoon", dict(heading=[60]))]),
             200, 13, [0, 2, 13], "x............"),
    "nn13b": ("c2_nw200", lambda: volturn([("center_column", dict(CdEnd=0.0)),
                                           ("outer_column", dict(heading=[60, 180], CdEnd=0.0, dlsMax=7))]),
              1030, 13, [0, 5, 9, 13], "............."),
}
_CACHE = {}


def setup(name):
    """(model, cases, oracle results) of a design: computed once, shared by the three checks."""
    if name not in _CACHE:
        tag, make, nw, nn, mstart, axial = DESIGNS[name]
        T0 = load_golden(tag)
        d = make()
        d["settings"]["min_freq"] = d["settings"]["max_freq"] / nw
        m, f = make_model(d, T0)
        assert m.nw == nw
        h = f.host_tables()
        assert h["nn"] == nn and h["mstart"].tolist() == mstart, (h["nn"], h["mstart"])
        off, shape = h["layout"]["node"]
        tab = h["packed"][off:off + int(np.prod(shape))].reshape(shape)   # prep.node_table's columns
        ax = (tab[15] * tab[19] != 0) | (tab[18] * tab[22] != 0)          # a_q Cd_q, a_end Cd_End
        assert "".join("x" if x else "." for x in ax) == axial
        T = oracle_tables_of(f)
        cases = random_cases(8, 17)
        ref = [O.solve_dynamics(T, dict(c), int(m.nIter), float(m.XiStart)) for c in cases]
        _CACHE[name] = (m, cases, ref)
    return _CACHE[name]


def test_designs_cover_the_ring_tails():
    """Host side: the node counts cover every remainder modulo 4 and 6 and rings that never fill; a
    member of a single node, an axial last node, axial sets of 0, 1 and 5 nodes, every grid."""
    nns = sorted({v[3] for v in DESIGNS.values()})
    assert nns == [1, 2, 3, 4, 5, 6, 7, 11, 12, 13]
    assert {n % 4 for n in nns} == {0, 1, 2, 3} and {n % 6 for n in nns} == {0, 1, 2, 3, 4, 5}
    assert any(1 in np.diff(v[4]).tolist() for v in DESIGNS.values())
    assert any(v[5].endswith("x") for v in DESIGNS.values())
    assert {0, 1, 5} <= {v[5].count("x") for v in DESIGNS.values()}
    assert {v[2] for v in DESIGNS.values()} == {100, 200, 500, 1000, 1030}


@pytest.mark.parametrize("name", list(DESIGNS))
def test_ring_tails_match_oracle(name):
    m, cases, ref = setup(name)
    res = m.analyzeCasesBatch(cases, want=("B_drag",))
    print(name, "iters", res["iters"].tolist(), "oracle", [r["iters"] for r in ref])
    for ic, r in enumerate(ref):
        print(ic, rel(res["Xi"][ic], r["Xi"][0]), rel(res["B_drag"][ic], r["B_drag"]))
    for ic, r in enumerate(ref):
        assert res["iters"][ic] == r["iters"], (ic, res["iters"][ic], r["iters"])
        assert (res["status"][ic] == 1) == r["converged"], ic
        assert rel(res["Xi"][ic], r["Xi"][0]) < RTOL, ic
        assert rel(res["B_drag"][ic], r["B_drag"]) < RTOL, ic


@pytest.mark.parametrize("name", list(DESIGNS))
def test_ring_tails_fast_and_general_agree(name):
    m, cases, ref = setup(name)
    a = m.analyzeCasesBatch(cases, want=("B_drag",))
    with solver_mode(1):
        b = m.analyzeCasesBatch(cases, want=("B_drag",))
    np.testing.assert_array_equal(a["iters"], b["iters"])
    np.testing.assert_array_equal(a["status"], b["status"])
    for ic in range(len(cases)):
        print(name, ic, rel(a["Xi"][ic], b["Xi"][ic]), rel(a["B_drag"][ic], b["B_drag"][ic]))
        assert rel(a["Xi"][ic], b["Xi"][ic]) < 1e-12, ic
        assert rel(a["B_drag"][ic], b["B_drag"][ic]) < 1e-12, ic


@pytest.mark.parametrize("name", list(DESIGNS))
def test_ring_tails_every_node_axial(name):
    m, cases, ref = setup(name)
    want = ("psd", "std", "zeta", "B_drag", "rao")
    a = m.analyzeCasesBatch(cases, want=want)
    with solver_mode(6):
        b = m.analyzeCasesBatch(cases, want=want)
    np.testing.assert_array_equal(a["iters"], b["iters"])
    np.testing.assert_array_equal(a["status"], b["status"])
    for k in ("Xi", "psd", "std", "rao", "zeta", "B_drag"):
        print(name, k, "bit for bit" if np.array_equal(a[k], b[k]) else rel(a[k], b[k]))
        assert rel(a[k], b[k]) < 1e-12, k
