"""GPU: the fixed point with the LU's updates as four FMAs (rh::msub, csrc/rh_device.h).

The fused update rounds twice per component where sub(a, mul(l, u)) rounded three times, so last bits of Xi
move, the same way in every kernel that shares the header.  16 seeded JONSWAP sea states on OC3spar (the
smallest golden design, 26 nodes) on three grids: nw = 65, one bin per thread with a ragged last wave
(k_solve_lds<1, 128, true>); 513, two bins per thread with bin 1 in one lane only; 1000, the bench grid
(both k_solve_lds<2, 512, false, 1>).  Per grid:

  1. the default kernel against the general one (rh_set_solver(ctx, 1)): equal `iters` and `status`, Xi
     within 1e-12 per case, the bar of test_gpu_parity.test_fast_and_general_kernels_agree;
  2. the default kernel against oracle/raft_oracle.py on the same tables: equal iteration counts, Xi within
     1e-9 per case (norm-relative), the project's parity bar;
  3. the default kernel against one phase-C sweep per bin (rh_set_solver(ctx, 8)), bit for bit.
"""
import numpy as np
import pytest

from conftest import load_golden, oracle_tables_of
from oracle import raft_oracle as O
from test_gpu_axial_rows import make_model, random_cases, rel, solver_mode

pytestmark = pytest.mark.gpu

GRIDS = [65, 513, 1000]
NCASE = 16
WANT = ("psd", "std", "zeta", "rao")
_SHARED = {}


def shared(nw):
    """(model, cases, the default kernel's results) of a grid: computed once, left unchanged."""
    if nw not in _SHARED:
        m, f = make_model("OC3spar", load_golden("c1_OC3spar"), {"min_freq": 0.4 / nw})
        assert m.nw == nw and f.device_design().nn == 26
        cases = random_cases(NCASE, 1300 + nw)
        _SHARED[nw] = (m, f, cases, m.analyzeCasesBatch(cases, want=WANT))
    return _SHARED[nw]


@pytest.mark.parametrize("nw", GRIDS)
def test_default_and_general_kernels_agree(nw):
    m, f, cases, a = shared(nw)
    with solver_mode(1):
        b = m.analyzeCasesBatch(cases, want=WANT)
    worst = max(rel(a["Xi"][ic], b["Xi"][ic]) for ic in range(NCASE))
    print(f"nw={nw} iters {a['iters'].tolist()} worst Xi difference default / general {worst:.2e}")
    np.testing.assert_array_equal(a["iters"], b["iters"])
    np.testing.assert_array_equal(a["status"], b["status"])
    for ic in range(NCASE):
        assert rel(a["Xi"][ic], b["Xi"][ic]) < 1e-12, ic


@pytest.mark.parametrize("nw", GRIDS)
def test_default_kernel_matches_oracle(nw):
    m, f, cases, a = shared(nw)
    T = oracle_tables_of(f)
    ref = [O.solve_dynamics(T, dict(c), int(m.nIter), float(m.XiStart)) for c in cases]
    errs = [rel(a["Xi"][ic], r["Xi"][0]) for ic, r in enumerate(ref)]
    print(f"nw={nw} iters {a['iters'].tolist()} oracle {[r['iters'] for r in ref]} worst Xi error {max(errs):.2e}")
    for ic, r in enumerate(ref):
        assert a["iters"][ic] == r["iters"], (ic, a["iters"][ic], r["iters"])
        assert (a["status"][ic] == 1) == r["converged"], ic
        assert errs[ic] < 1e-9, (ic, errs[ic])


@pytest.mark.parametrize("nw", GRIDS)
def test_default_against_one_sweep_per_bin_bit_for_bit(nw):
    m, f, cases, a = shared(nw)
    with solver_mode(8):
        b = m.analyzeCasesBatch(cases, want=WANT)
    assert np.all(np.isfinite(a["Xi"].view(np.float64)))
    for k in ("Xi", "psd", "rao", "std", "zeta", "iters", "status"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
