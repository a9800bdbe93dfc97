"""Inputs, long-double references and criteria for the direct tests of the second-order force kernels
(tests/test_gpu_force2nd.py; checked on the CPU by tests/test_force2nd_cases.py).

References: oracle/qtf_oracle.py hydro_force_2nd (bilinear resample of the QTF to (w, w), z[y, x]
orientation, 0 strictly outside the QTF grid, difference-frequency diagonals) and
hydro_force_2nd_spectrum, in NumPy longdouble of the double inputs.  The QTF is random complex and
NOT Hermitian, so a swapped y/x index shows; spectra are drawn from U(0.1, 2).  u = 2^-53.

Criteria: f is 4 dw times the square root of a sum of non-negative terms: per element
|dev - ref| <= (nw + 32) u |ref|, identical zero pattern, last bin exactly 0.  f_mean can cancel:
|dev - ref| <= (nw + 32) u 2 dw sum_i |S0_i Re Q_ii|.  Spectrum mode: Sf like f with n2 in place of
nw (Sf[d][0] exactly 0), f within the sum of that and 4 u.
"""
import types

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53


def pairs():
    """name -> (w2 [n2], w [nw]): the grid pairs."""
    w1 = 0.05 + 0.03 * np.arange(70)
    out = {
        # bitwise coincident: probes exactly on w2[0], on inner nodes and on w2[-1]; w runs past both ends
        "1": (w1[5:60:3].copy(), w1),
        # no coincidences; nw > 256: the strided loop takes two trips
        "2": (np.linspace(0.31, 2.03, 43) + 1e-3 / np.pi, np.linspace(0.1, 2.5, 300)),
        # the smallest legal sizes
        "3a": (np.array([0.5, 1.5]), np.array([0.7, 1.2])),
        "3b": (np.array([0.5, 1.5]), np.linspace(0.2, 1.8, 40)),
        # w wholly inside w2: no zeros
        "4": (np.linspace(0.1, 3.0, 25), np.linspace(0.5, 2.5, 50)),
        # disjoint: every f and f_mean exactly 0
        "5": (np.linspace(3.0, 4.0, 10), np.linspace(0.1, 2.0, 30)),
    }
    return out


SPECTRUM_PAIRS = ["1", "2", "4", "5"]


def inputs(name, nq=2, nspec=3):
    """QTFs [nq][n2][n2][6] complex (not Hermitian), spectra [nspec][nw], the grids and dw."""
    w2, w = pairs()[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 77)
    n2, nw = len(w2), len(w)
    Q = (rng.standard_normal([nq, n2, n2, 6]) + 1j * rng.standard_normal([nq, n2, n2, 6])) * 1e4
    S = rng.uniform(0.1, 2.0, [nspec, nw])
    return types.SimpleNamespace(w2=w2, w=w, n2=n2, nw=nw, Q=Q, S=S, dw=float(w[1] - w[0]))


def _cells(g, x):
    """RegularGridInterpolator(linear): i = searchsorted(g, x) - 1 clipped to [0, n - 2], the weight t in
    long double, and inside = not strictly outside the grid."""
    i = np.clip(np.searchsorted(g, x, side="left") - 1, 0, len(g) - 2)
    gl = g.astype(LD)
    t = (x.astype(LD) - gl[i]) / (gl[i + 1] - gl[i])
    return i, t, (x >= g[0]) & (x <= g[-1])


def resample(Q, w2, w):
    """Qi [nw][nw][6] (y = w_i, x = w_j) in clongdouble, 0 outside."""
    i, t, ok = _cells(w2, w)
    Ql = Q.astype(CLD)
    ty, tx = t[:, None, None], t[None, :, None]
    iy, ix = i[:, None], i[None, :]
    v = (Ql[iy, ix] * ((1 - ty) * (1 - tx)) + Ql[iy, ix + 1] * ((1 - ty) * tx) + Ql[iy + 1, ix] * (ty * (1 - tx))
         + Ql[iy + 1, ix + 1] * (ty * tx))
    return np.where((ok[:, None] & ok[None, :])[:, :, None], v, CLD(0))


def force_reference(Q, w2, w, S0, dw):
    """hydro_force_2nd in long double: (f_mean [6], f [6][nw], scale of f_mean [6])."""
    nw = len(w)
    Qi = resample(Q, w2, w)
    S = S0.astype(LD)
    f = np.zeros([6, nw], dtype=LD)
    m2 = Qi.real ** 2 + Qi.imag ** 2
    for mu in range(1, nw):
        i = np.arange(nw - mu)
        f[:, mu - 1] = 4 * np.sqrt(((S[i] * S[i + mu])[:, None] * m2[i, i + mu]).sum(axis=0)) * LD(dw)
    d = np.arange(nw)
    fm = 2 * (S[:, None] * Qi[d, d].real).sum(axis=0) * LD(dw)
    fm_scale = 2 * np.abs(S[:, None] * Qi[d, d].real).sum(axis=0) * LD(dw)
    return fm, f, fm_scale


def _interp0(x, xp, fp):
    """np.interp(x, xp, fp, left=0, right=0) in long double (xp increasing)."""
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, len(xp) - 2)
    v = fp[j] + (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j])
    v = np.where(x == xp[-1], fp[-1], v)
    return np.where((x < xp[0]) | (x > xp[-1]), LD(0), v)


def spectrum_reference(Q, w2, w, S0, dw):
    """hydro_force_2nd_spectrum in long double: (f_mean [6], f [6][nw], Sf [6][n2], scale of f_mean)."""
    n2, nw = len(w2), len(w)
    w2l, wl = w2.astype(LD), w.astype(LD)
    S = _interp0(w2l, wl, S0.astype(LD))
    d1 = w2l[1] - w2l[0]
    Ql = Q.astype(CLD)
    m2 = Ql.real ** 2 + Ql.imag ** 2
    Sf = np.zeros([6, n2], dtype=LD)
    for mu in range(1, n2):
        i = np.arange(n2 - mu)
        Sf[:, mu] = 8 * ((S[i] * S[i + mu])[:, None] * m2[i, i + mu]).sum(axis=0) * d1
    d = np.arange(n2)
    fm = 2 * (S[:, None] * Ql[d, d].real).sum(axis=0) * d1
    fm_scale = 2 * np.abs(S[:, None] * Ql[d, d].real).sum(axis=0) * d1
    f = np.zeros([6, nw], dtype=LD)
    # the abscissas of the second resample are differences of doubles, formed in double by the oracle and
    # the device alike (one correctly rounded subtraction each, so the same doubles): they are inputs of
    # the interpolation here.  Taken exactly instead, their rounding moves a probe by u x against knots
    # dx apart, an error of (x / dx) u in f that no criterion on the sums covers.
    x, mu = (w - w[0]).astype(LD), (w2 - w2[0]).astype(LD)
    for k in range(6):
        v = np.sqrt(2 * _interp0(x, mu, Sf[k]) * LD(dw))
        f[k, :-1] = v[1:]
    return fm, f, Sf, fm_scale


def force_ratios(label, n, fm_ref, f_ref, fm_scale, fm, f, extra=0.0):
    """Worst |x - ref| / bound of f and f_mean with n terms per sum ((n + 32 + extra) u); the zero
    pattern of f must be the reference's and its last bin exactly 0."""
    f, fm = np.asarray(f), np.asarray(fm)
    assert np.array_equal(f == 0, f_ref == 0), f"{label}: zero pattern of f"
    assert np.all(f[:, -1] == 0), f"{label}: last bin"
    nz = f_ref != 0
    rf = float((np.abs(f.astype(LD) - f_ref)[nz] / ((n + 32 + extra) * U * f_ref[nz])).max()) if nz.any() else 0.0
    if np.all(fm_scale == 0):
        assert np.all(fm == 0), f"{label}: f_mean must be exactly 0"
        rm = 0.0
    else:
        rm = float((np.abs(fm.astype(LD) - fm_ref) / ((n + 32) * U * fm_scale)).max())
    return rf, rm
