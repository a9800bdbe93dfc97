"""GPU: phase B's sums and the prologue's axial list of k_solve_lds, at the node counts where their
batches end.

Phase B reads a node's 3 LW wave partials before it adds them, keeps the node's Bmat in registers for
its 36 translate entries (t3to6_fma: the multiply-adds written outright), and sums the per-node B_drag
entries sixteen at a time, every read of a batch issued before its adds, with one guarded batch of up to
fifteen for the rest; the adds stay in wave and node order.  The prologue builds
the axial-node list on wave 0 from a ballot per 64 nodes and a running count.  The shapes at which these
can go wrong are node counts around the batch size and a list that spans two ballot chunks:

  * nn = 16: one whole batch and an empty tail; nn = 15: the longest tail; nn = 8: half a batch
    (tests/test_gpu_ring_tails.py has nn = 1..7 and 11..13, tails only; the parity tests have nn = 53,
    three batches and a tail of 5);
  * nn = 71: four batches and a tail of 7, a second ballot chunk, and axial nodes on both sides of
    node 64 (node 0, nodes 44..64 of a pontoon with Cd_q = 0.4, a column's end node at 66).

Each design runs on one grid per kernel: nw = 200 (128 threads x 2 bins, node-serial B_drag: its phase
B is unchanged, its prologue the new one), nw = 300 (512 threads x 1 bin) and nw = 700 (512 threads x
2 bins, the bench's kernel).  The fast kernel is the one dispatched as long as its LDS need (lds_bytes
below, solve_lds_smem of rh_solve.hip) stays within 160 KB, which the test asserts.

Checks, 4 cases on two headings each:
  1. against the CPU oracle on the model's own tables: identical iteration counts, Xi and B_drag within
     1e-9 (the tolerance of test_gpu_ring_tails.test_ring_tails_match_oracle);
  2. against the general kernel (rh_set_solver(ctx, 1)): identical iteration counts and statuses, 1e-12;
  3. bit for bit between the default, every node axial (rh_set_solver(ctx, 6)) and one phase-C sweep
     per bin (rh_set_solver(ctx, 8)).  The last is a second compilation of the two-bin kernel that keeps
     phase B in its plain form, so on nw = 700 it also holds the batched phase B against the plain one.
"""
import numpy as np
import pytest

from conftest import load_golden, oracle_tables_of
from oracle import raft_oracle as O
from test_gpu_axial_rows import make_model, random_cases, rel, solver_mode
from test_gpu_ring_tails import volturn

pytestmark = pytest.mark.gpu
RTOL = 1e-9   # of test_gpu_ring_tails.test_ring_tails_match_oracle
LDS_MAX = 160 * 1024

# name: (design, nodes, member starts, axial nodes ('x') in node order)
DESIGNS = {
    "nn8": (lambda: volturn([("outer_column", dict(heading=[60, 180], dlsMax=7))]), 8, [0, 4, 8], "x...x..."),
    "nn15": (lambda: volturn([("pontoon", dict(heading=[60])), ("outer_column", dict(heading=[60], dlsMax=7))]),
             15, [0, 11, 15], "...........x..."),
    "nn16": (lambda: volturn([("pontoon", dict(heading=[60])), ("outer_column", dict(heading=[60]))]),
             16, [0, 11, 16], "...........x...."),
    "nn71": (lambda: volturn([("center_column", {}), ("pontoon", dict(heading=[60, 180], dlsMax=2.5)),
                              ("pontoon", dict(heading=[300], dlsMax=2.0, Cd_q=0.4)),
                              ("outer_column", dict(heading=[60]))]),
             71, [0, 5, 24, 43, 66, 71], "x" + "." * 43 + "x" * 21 + ".x...."),
}
# nw: (threads, bins per thread, node-serial B_drag) of the kernel the grid runs
GRIDS = {200: (128, 2, True), 300: (512, 1, False), 700: (512, 2, False)}
SETUPS = [(name, nw) for name in DESIGNS for nw in GRIDS]
_CACHE = {}


def lds_bytes(nn, nm, nb, lt, ser):
    """solve_lds_smem (rh_solve.hip) for one pass."""
    lw = lt // 64
    red = 27 if ser and nn * 3 * lw < 27 else nn * 3 * lw
    doubles = (12 * lt * nb + red + (0 if ser else nn * 36) + nn * 9 + (nn + 1) * 6 + (nn + 1) + nm * 18
               + 2 * lt * nb + 36 + 108 + lw * 6 + 36 + lw)
    return 8 * doubles + 4 * (nm + 6)


def setup(name, nw):
    """(model, cases, oracle results) of a design on a grid: computed once, shared by the checks."""
    if (name, nw) not in _CACHE:
        make, nn, mstart, axial = DESIGNS[name]
        T0 = load_golden("c2_nw200")
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
        lt, nb, ser = GRIDS[nw]
        need = lds_bytes(nn, len(mstart) - 1, nb, lt, ser)
        print(name, nw, "LDS need", need, "of", LDS_MAX)
        assert need <= LDS_MAX, need   # beyond it rh_solve_cases falls to the general kernel
        T = oracle_tables_of(f)
        cases = random_cases(4, 23, headings=(0, 60))
        ref = [O.solve_dynamics(T, dict(c), int(m.nIter), float(m.XiStart)) for c in cases]
        _CACHE[(name, nw)] = (m, cases, ref)
    return _CACHE[(name, nw)]


def test_designs_cover_the_batches():
    """Host side: whole batches with an empty tail, a tail, and a list that crosses node 64."""
    nns = {v[1] for v in DESIGNS.values()}
    assert {8, 15, 16} <= nns and any(65 <= n <= 128 for n in nns)
    big = next(v for v in DESIGNS.values() if v[1] > 64)
    assert big[3][0] == "x" and big[3][62:65] == "xxx" and "x" in big[3][65:]   # 62, 63 | 64, 66
    assert {GRIDS[nw] for nw in GRIDS} == {(128, 2, True), (512, 1, False), (512, 2, False)}
    assert any(256 < nw <= 512 for nw in GRIDS) and any(512 < nw <= 1024 for nw in GRIDS)
    assert len({c["wave_heading"] for c in random_cases(4, 23, headings=(0, 60))}) == 2


@pytest.mark.parametrize("name,nw", SETUPS)
def test_phase_b_matches_oracle(name, nw):
    m, cases, ref = setup(name, nw)
    res = m.analyzeCasesBatch(cases, want=("B_drag",))
    print(name, nw, "iters", res["iters"].tolist(), "oracle", [r["iters"] for r in ref])
    for ic, r in enumerate(ref):
        print(ic, rel(res["Xi"][ic], r["Xi"][0]), rel(res["B_drag"][ic], r["B_drag"]))
    for ic, r in enumerate(ref):
        assert r["converged"], ic
        assert res["iters"][ic] == r["iters"], (ic, res["iters"][ic], r["iters"])
        assert res["status"][ic] == 1, ic
        assert rel(res["Xi"][ic], r["Xi"][0]) < RTOL, ic
        assert rel(res["B_drag"][ic], r["B_drag"]) < RTOL, ic


@pytest.mark.parametrize("name,nw", SETUPS)
def test_phase_b_fast_and_general_agree(name, nw):
    m, cases, ref = setup(name, nw)
    a = m.analyzeCasesBatch(cases, want=("B_drag",))
    with solver_mode(1):
        b = m.analyzeCasesBatch(cases, want=("B_drag",))
    np.testing.assert_array_equal(a["iters"], b["iters"])
    np.testing.assert_array_equal(a["status"], b["status"])
    for ic in range(len(cases)):
        print(name, nw, ic, rel(a["Xi"][ic], b["Xi"][ic]), rel(a["B_drag"][ic], b["B_drag"][ic]))
        assert rel(a["Xi"][ic], b["Xi"][ic]) < 1e-12, ic
        assert rel(a["B_drag"][ic], b["B_drag"][ic]) < 1e-12, ic


@pytest.mark.parametrize("name,nw", SETUPS)
def test_phase_b_selectors_bit_for_bit(name, nw):
    m, cases, ref = setup(name, nw)
    want = ("psd", "std", "zeta", "B_drag", "rao")
    a = m.analyzeCasesBatch(cases, want=want)
    for mode in (6, 8):
        with solver_mode(mode):
            b = m.analyzeCasesBatch(cases, want=want)
        for k in ("iters", "status", "Xi", "psd", "std", "rao", "zeta", "B_drag"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{k}, rh_set_solver {mode}")
