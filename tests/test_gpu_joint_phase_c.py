"""GPU: the two-bin fast kernel k_solve_lds<2, 512, false, 1> forms the excitation of both bins of a
thread in one phase-C node sweep and parks bin 1's in global memory across bin 0's solve.  Per bin
the operations and their order are those of one sweep per bin, so every output has the same bits.

  1. the default against one sweep per bin (rh_set_solver(ctx, 8): k_solve_lds_split), bit for bit,
     on the grids where the 512-thread, two-bin kernel can go wrong, for a design with one ghost node
     in the joint ring's last round (VolturnUS-S: 53 nodes) and one with axial nodes in the middle of
     a member (OC3spar: 26 nodes);
  2. the same with every node in the axial list (6 against 9: the widened axial loop);
  3. a solve that stops at the iteration cap and one that converges before it;
  4. the default against the general kernel k_solve_cases;
  5. calls with fext and F_wave, and without the Xi output (the excitation is then parked in the
     case's Xi_last rows, not in its Xi rows).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_axial_rows import make_model, random_cases, rel, solver_mode

pytestmark = pytest.mark.gpu

SPLIT, ALL_AXIAL, ALL_AXIAL_SPLIT, GENERAL = 8, 6, 9, 1
DESIGNS = {"VolturnUS-S_example": ("c2_nw200", 0.2, 53), "OC3spar": ("c1_OC3spar", 0.4, 26)}
# nw: 513 = bin 1 exists for one lane only (waves 1-7 skip its solve); 577 = a partial wave in bin 1;
# 1000 = the bench grid; 1024 = no pad lanes
GRIDS = [513, 577, 1000, 1024]
WANT = ("psd", "std", "zeta", "rao")
KEYS = ("Xi", "psd", "rao", "std", "zeta", "iters", "status")
_MODELS = {}


def model(design, nw):
    """(model, fowt) of a design on a grid of nw bins: built once, shared."""
    if (design, nw) not in _MODELS:
        tag, max_freq, nn = DESIGNS[design]
        m, f = make_model(design, load_golden(tag), {"min_freq": max_freq / nw})
        assert m.nw == nw
        assert f.device_design().nn == nn
        _MODELS[(design, nw)] = (m, f)
    return _MODELS[(design, nw)]


def cases8(seed):
    """8 sea states over headings 0 / 30 / 60 / 90 with gamma from {0, 1, 3.3}."""
    cs = random_cases(8, seed)
    for i, c in enumerate(cs):   # every heading and every gamma is there whatever the draw
        c["wave_heading"] = float((0, 30, 60, 90)[i % 4])
        c["wave_gamma"] = float((0.0, 1.0, 3.3)[i % 3])
    return cs


def same_bits(a, b, keys):
    for k in keys:
        assert torch.equal(torch.from_numpy(np.ascontiguousarray(a[k])), torch.from_numpy(np.ascontiguousarray(b[k]))), k


@pytest.mark.parametrize("nw", GRIDS)
@pytest.mark.parametrize("design", list(DESIGNS))
def test_joint_against_split_bit_for_bit(design, nw):
    m, f = model(design, nw)
    cases = cases8(nw)
    a = m.analyzeCasesBatch(cases, want=WANT)
    with solver_mode(SPLIT):
        b = m.analyzeCasesBatch(cases, want=WANT)
    assert np.all(np.isfinite(a["Xi"].view(np.float64)))
    same_bits(a, b, KEYS)


@pytest.mark.parametrize("nw", GRIDS)
@pytest.mark.parametrize("design", list(DESIGNS))
def test_all_axial_joint_against_split_bit_for_bit(design, nw):
    """Every node in the axial list, in both forms; and the default against it (what the skip
    leaves out is multiplied by exact zeros)."""
    m, f = model(design, nw)
    cases = cases8(nw + 1)
    with solver_mode(ALL_AXIAL):
        a = m.analyzeCasesBatch(cases, want=WANT)
    with solver_mode(ALL_AXIAL_SPLIT):
        b = m.analyzeCasesBatch(cases, want=WANT)
    c = m.analyzeCasesBatch(cases, want=WANT)
    same_bits(a, b, KEYS)
    same_bits(a, c, KEYS)


@pytest.mark.parametrize("design", list(DESIGNS))
def test_iteration_cap_and_early_convergence(design):
    """nIter = 1: every case stops at the cap (the stores of the last allowed iteration);
    nIter = 25: cases converge before it."""
    m, f = model(design, 1000)
    cases = cases8(7)
    keep = m.nIter
    try:
        m.nIter = 1
        a = m.analyzeCasesBatch(cases, want=WANT)
        with solver_mode(SPLIT):
            b = m.analyzeCasesBatch(cases, want=WANT)
        from raft import _native as N
        assert np.any(a["status"] == N.RH_CASE_NOT_CONVERGED), (a["iters"], a["status"])
        same_bits(a, b, KEYS)
        m.nIter = 25
        a = m.analyzeCasesBatch(cases, want=WANT)
        with solver_mode(SPLIT):
            b = m.analyzeCasesBatch(cases, want=WANT)
        print(design, "iters", a["iters"].tolist())
        assert np.any((a["status"] == N.RH_CASE_CONVERGED) & (a["iters"] < 26)), (a["iters"], a["status"])
        same_bits(a, b, KEYS)
    finally:
        m.nIter = keep


@pytest.mark.parametrize("nw", [513, 1000])
def test_joint_and_general_kernels_agree(nw):
    """Identical iteration counts and statuses, Xi within 1e-12 (norm-relative), as
    test_gpu_parity.test_fast_and_general_kernels_agree."""
    m, f = model("VolturnUS-S_example", nw)
    cases = cases8(nw + 2)
    a = m.analyzeCasesBatch(cases, want=WANT)
    with solver_mode(GENERAL):
        b = m.analyzeCasesBatch(cases, want=WANT)
    np.testing.assert_array_equal(a["iters"], b["iters"])
    np.testing.assert_array_equal(a["status"], b["status"])
    for ic in range(len(cases)):
        assert rel(a["Xi"][ic], b["Xi"][ic]) < 1e-12, ic


def _case_set(cases):
    from raft.solver import CaseSet
    return CaseSet(np.zeros(len(cases), dtype=np.int32), [c["wave_heading"] for c in cases], ["JONSWAP"] * len(cases),
                   [c["wave_height"] for c in cases], [c["wave_period"] for c in cases],
                   [c["wave_gamma"] for c in cases])


@pytest.mark.parametrize("nw", [513, 1000])
def test_fext_and_f_wave(nw):
    """An external force per case and the F_wave output: the excitation stored is that of the final
    iteration, from the same registers as before (bin 1's after its read-back)."""
    from raft.solver import solve_batch
    m, f = model("VolturnUS-S_example", nw)
    cases = cases8(nw + 3)
    dd = f.device_design()
    g = torch.Generator().manual_seed(nw)
    fext = (1e5 * torch.randn(len(cases), 6, nw, 2, generator=g, dtype=torch.float64)).to(dd.device)
    fext = torch.view_as_complex(fext).contiguous()
    want = ("psd", "std", "zeta", "rao", "B_drag")
    res = []
    for mode in (0, SPLIT):
        fw = torch.full((len(cases), 6, nw), complex(np.nan, np.nan), dtype=torch.complex128, device=dd.device)
        with solver_mode(mode):
            r = solve_batch([dd], _case_set(cases), m.nIter, m.XiStart, 0.01, want=want, fext=fext, F_wave=fw).host()
        r["F_wave"] = fw.cpu().numpy()
        res.append(r)
    assert np.all(np.isfinite(res[0]["F_wave"].view(np.float64)))
    same_bits(res[0], res[1], KEYS + ("B_drag", "F_wave"))


@pytest.mark.parametrize("nw", [513, 1000])
def test_no_xi_output(nw):
    """The fixed-point form without the response ("noXi"): bin 1's excitation waits in the case's
    Xi_last rows."""
    from raft.solver import solve_batch
    m, f = model("VolturnUS-S_example", nw)
    cases = cases8(nw + 4)
    dd = f.device_design()
    want = ("zeta", "B_drag", "Bmat", "noXi")
    res = []
    for mode in (0, SPLIT):
        fw = torch.full((len(cases), 6, nw), complex(np.nan, np.nan), dtype=torch.complex128, device=dd.device)
        with solver_mode(mode):
            r = solve_batch([dd], _case_set(cases), m.nIter, m.XiStart, 0.01, want=want, F_wave=fw).host()
        assert "Xi" not in r
        r["F_wave"] = fw.cpu().numpy()
        res.append(r)
    assert np.all(np.isfinite(res[0]["F_wave"].view(np.float64)))
    same_bits(res[0], res[1], ("iters", "status", "zeta", "B_drag", "Bmat", "F_wave"))
