"""CPU: the inputs and long-double references of tests/test_gpu_wave_tables.py and
tests/test_gpu_sea_state.py (tests/helpers/wave_cases.py) are what they claim to be, and the criteria
the device tests assert can be met: the double-precision oracle (oracle/raft_oracle.py) is compared
with each reference in the same measure, and has to stay well inside the bound.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wave_cases as W   # noqa: E402

from oracle import raft_oracle as O   # noqa: E402

U, LD = W.U, W.LD


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


def test_wave_design_hits_every_edge():
    d = W.WaveDesign(21, 130)
    kh = d.k * d.depth
    assert (kh < 1).any() and (kh > 710).any()
    assert ((kh > 89.3) & (kh <= 89.4)).any() and ((kh > 89.4) & (kh < 89.5)).any()
    assert np.isinf(np.sinh(kh.max()))                       # the finite-depth formulas would be inf / inf
    assert d.r[0, 2] == -0.01 and d.r[1, 2] == -150.0 and np.all(d.r[:, 2] < 0)
    assert (np.abs(d.r[:, None, 2]) * d.k[None, :]).max() <= 600.0
    assert np.abs(d.r[:, :2]).max() > 500 and np.abs(d.r[:, :2]).max() <= 1000
    assert np.all(d.r != d.r_rel)
    assert 0 < d.mcf.sum() < d.nn and (d.a_i > 0).any() and (d.a_i < 0).any()
    for n in range(d.nn):                                     # orthonormal, not axis-aligned, Imat not symmetric
        F = np.stack([d.q[n], d.p1[n], d.p2[n]])
        assert np.allclose(F @ F.T, np.eye(3), atol=1e-14) and np.abs(F).max() < 0.9999
        assert not np.allclose(d.Imat[n], d.Imat[n].T)
    h = d.host_tables()
    from raft import _native as N
    off, shape = h["layout"]["node"]
    node = h["packed"][off:off + int(np.prod(shape))].reshape(shape)
    assert np.array_equal(node[N.NF["I00"] + 3 * 1 + 2], d.Imat[:, 1, 2])
    for f in ("AQ", "AP1", "AP2", "AEND", "CDQ", "CDP1", "CDP2", "CDEND"):
        assert not node[N.NF[f]].any()


@pytest.mark.parametrize("shape", W.SHAPES, ids=str)
def test_wave_reference_against_oracle(shape):
    """The double oracle against the long-double reference in the device tests' measure: uhat and kproj
    within 1.5 A u s (0.375 of the bound), finer below a quarter of its bound; every reference a normal
    number and finite on the k h > 710 bins."""
    nn, nw, nh = shape
    d = W.WaveDesign(nn, nw)
    betas = W.HEADINGS[:nh]
    ref = W.wave_reference(d, betas)
    for a in (ref.uhat, ref.kproj, ref.finer):
        assert np.all(np.isfinite(a))
    u, kp, F = W.oracle_tables(d, betas)
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(kp)) and np.all(np.isfinite(F))
    ru, rk, rf = W.table_ratios(ref, u, kp, F, nn)
    print(f"oracle vs long double {shape}: uhat {4 * ru:.2f} A u, kproj {4 * rk:.2f} A u, finer {rf:.3f} of its bound")
    assert 4 * ru <= 1.5 and 4 * rk <= 1.5, (ru, rk)
    assert rf < 0.25, rf


@pytest.mark.parametrize("nw", [1, 255, 257])
def test_jonswap_reference_against_oracle(nw):
    """jonswap_ld against O.jonswap: the two agree to rounding (e_np, the figure the device bound is a
    multiple of), and the jump of G at Tp / sqrt(Hs) = 3.6 is orders of magnitude above the bound."""
    refs = W.sea_reference(nw, 0.0117)
    low = 0
    for (Hs, Tp, gam, what), (S, zeta, keep, e_np) in zip(W.sea_cases(), refs):
        print(f"nw={nw} Hs={Hs} Tp={float(Tp)!r} gamma={gam}: e_np = {e_np / U:.1f} u, {int((~keep).sum())} bins <= 1e-300")
        assert e_np < 1e-11, (what, e_np)
        assert np.all(O.jonswap(W.sea_grid(nw), Hs, Tp, Gamma=gam)[~keep] <= 1e-290)
        low += int((~keep).sum())
    # w = 0.02 lies far below every peak: exp(-1.25 fp4) underflows there in any format, so such bins exist
    # on this grid (about half of it for the short periods) and the device tests hold them to <= 1e-290
    print(f"nw={nw}: {low} bins at or below 1e-300 in all")
    assert low >= len(refs)
    if nw > 1:
        on, off = refs[0], refs[1]                          # (4, 7.2) and (4, nextafter(7.2))
        keep = on[2] & off[2]
        jump = float((np.abs(on[0] - off[0])[keep] / on[0][keep]).max())
        assert jump > 1e-4 > 1e6 * 8 * max(on[3], off[3], 4 * U), jump


def test_gamma_branch_arguments_are_exact():
    for Hs, Tp, _, _ in W.sea_cases()[:5]:
        assert float(LD(Tp) / np.sqrt(LD(Hs))) == Tp / np.sqrt(Hs)
    assert 7.2 / np.sqrt(4.0) == 3.6 and np.nextafter(7.2, 8.0) / 2.0 > 3.6
    assert 10.0 / np.sqrt(4.0) == 5.0 and np.nextafter(10.0, 9.0) / 2.0 < 5.0


@pytest.mark.parametrize("shape", W.STAT_SHAPES, ids=str)
def test_statistics_references_against_oracle(shape):
    """get_psd / get_rms in double against the long-double references, at a quarter of the device bounds."""
    ncase, nrow, nw = shape
    dw = 0.0371
    X = W.stat_inputs(ncase, nrow, 6, nw)
    psd, std = W.motion_reference(X, dw)
    bound = (nrow * nw + 16) * U
    for ic in range(ncase):
        x = X[ic].copy()
        x[:, 3:] *= O.RAD2DEG
        for c in range(6):
            assert np.all(np.abs(O.get_psd(x[:, c], dw) - psd[ic, c]) <= 0.25 * bound * psd[ic, c])
            assert abs(O.get_rms(x[:, c]) - std[ic, c]) <= 0.25 * bound * std[ic, c]
    w = np.linspace(0.05, 3.0, nw)
    for ndof in (6, 12):
        X = W.stat_inputs(ncase, nrow, ndof, nw)
        for nch in (1, 5):
            coef = W.channel_coef(nch, ndof)
            pairs = np.stack([coef[:, 0], coef[:, 1]], axis=-1).reshape(-1, 2)
            assert (~pairs.any(axis=1)).any() or ndof * nch < 4
            assert ((pairs[:, 0] == 0) & (pairs[:, 1] != 0)).any()
            psd, std, psd_abs, std_abs = W.channel_reference(X, w, coef, dw)
            bound = (2 * ndof + nrow * nw + 16) * U
            for ic in range(ncase):
                for k in range(nch):
                    xk = np.einsum("d,rdb->rb", coef[k, 0], X[ic]) + w ** 2 * np.einsum("d,rdb->rb", coef[k, 1], X[ic])
                    assert np.all(np.abs(O.get_psd(xk, dw) - psd[ic, k]) <= 0.25 * bound * psd_abs[ic, k])
                    assert abs(O.get_rms(xk) - std[ic, k]) <= 0.25 * bound * std_abs[ic, k]
