"""CPU: the grid pairs and long-double references of tests/test_gpu_force2nd.py
(tests/helpers/force2nd_cases.py) are what they claim to be, and the double-precision oracle
(oracle/qtf_oracle.py, scipy's RegularGridInterpolator and numpy.interp) meets the criteria the device
tests assert at a quarter of their bounds.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import force2nd_cases as F2   # noqa: E402

from oracle import qtf_oracle as Q   # noqa: E402

U = F2.U


def test_grid_pairs_are_what_they_claim():
    P = F2.pairs()
    w2, w = P["1"]
    assert len(w) == 70 and len(w2) == 19 and np.all(np.isin(w2, w)) and w[0] < w2[0] and w[-1] > w2[-1]
    w2, w = P["2"]
    assert len(w) == 300 and len(w2) == 43 and not np.isin(w, w2).any()
    assert not np.isin(w[1:] - w[0], w2 - w2[0]).any()
    assert len(P["3a"][0]) == 2 and len(P["3a"][1]) == 2 and len(P["3b"][1]) == 40
    w2, w = P["4"]
    assert w2[0] < w[0] and w[-1] < w2[-1]
    w2, w = P["5"]
    assert w[-1] < w2[0]
    for name in P:
        x = F2.inputs(name)
        assert not np.allclose(x.Q[0], np.conj(np.swapaxes(x.Q[0], 0, 1)))
        assert x.S.min() >= 0.1 and x.S.max() <= 2.0


@pytest.mark.parametrize("name", list(F2.pairs()))
def test_force_reference_against_oracle(name):
    x = F2.inputs(name)
    worst = [0.0, 0.0]
    for iq in range(2):
        fm_ref, f_ref, fm_scale = F2.force_reference(x.Q[iq], x.w2, x.w, x.S[iq], x.dw)
        fm, f = Q.hydro_force_2nd(x.Q[iq][:, :, None, :], x.w2, x.w, x.S[iq], x.dw)
        rf, rm = F2.force_ratios(f"pair {name}", x.nw, fm_ref, f_ref, fm_scale, fm, f)
        worst = [max(worst[0], rf), max(worst[1], rm)]
        if name == "5":
            assert not f_ref.any() and not fm_ref.any()
        if name == "4":
            assert np.all(f_ref[:, :-1] != 0)
    print(f"pair {name}: oracle f {worst[0]:.3f}, f_mean {worst[1]:.3f} of the bound; "
          f"{int((f_ref != 0).sum())} of {f_ref.size} bins non-zero")
    assert worst[0] <= 0.25 and worst[1] <= 0.25, worst


@pytest.mark.parametrize("name", F2.SPECTRUM_PAIRS)
def test_spectrum_reference_against_oracle(name):
    x = F2.inputs(name)
    fm_ref, f_ref, Sf_ref, fm_scale = F2.spectrum_reference(x.Q[0], x.w2, x.w, x.S[0], x.dw)
    fm, f = Q.hydro_force_2nd_spectrum(x.Q[0][:, :, None, :], x.w2, x.w, x.S[0], x.dw)
    assert not f.imag.any() and not Sf_ref[:, 0].any()
    rf, rm = F2.force_ratios(f"pair {name} spectrum", x.n2, fm_ref, f_ref, fm_scale, fm, f.real, extra=4)
    print(f"pair {name} spectrum: oracle f {rf:.3f}, f_mean {rm:.3f} of the bound")
    assert rf <= 0.25 and rm <= 0.25, (rf, rm)
