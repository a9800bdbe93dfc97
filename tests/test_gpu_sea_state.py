"""GPU: the sea state (rh_sea_state / k_sea_state and the solve kernels' own sea_amplitude) and the small
statistics kernels (rh_motion_stats, rh_channel_stats) against long-double references.

Cases, references and criteria are tests/helpers/wave_cases.py (checked on the CPU by
tests/test_wave_cases.py).  Sea state: the IEC gamma branches on and next to their boundaries
(Tp / sqrt(Hs) = 3.6 and 5 exactly, one ulp off, interior), given gammas, and the codes unit, constant
and none mixed into the same call; w = linspace(0.02, 3, nw), nw in {1, 255, 257}.  JONSWAP bins: with
e_np the worst relative error of the double oracle against the long-double reference over the bins
whose reference exceeds 1e-300, the device's S is within 8 max(e_np, 4 u) and its zeta within half of
that plus 2 u; the bins at or below 1e-300 (w = 0.02 is far below every peak, where exp(-1.25 fp4)
underflows in any format; about half the grid for the short periods) come out at or below 1e-290.
unit, constant, none and zeta = sqrt(2 S dw) are exact.  The jump of G at 3.6 is 5.6e-4 relative.

Statistics: |dev - ref| <= (nrow nw + 16) u |ref| for the motion statistics (rotations in degrees);
the channel combination can cancel: (2 ndof + nrow nw + 16) u times the same expression of |a|, |c|
and |Xi|.  Each call once with psd = NULL and once with std = NULL.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wave_cases as W   # noqa: E402

pytestmark = pytest.mark.gpu
U, LD = W.U, W.LD
_REF = {}


def dev():
    import torch
    return torch.device("cuda", 0)


def tens(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def sea_ref(nw, dw):
    if (nw, dw) not in _REF:
        _REF[(nw, dw)] = W.sea_reference(nw, dw)
    return _REF[(nw, dw)]


def mixed_cases():
    """(spectrum code, Hs, Tp, gamma, index into sea_cases() or None): the JONSWAP cases with a unit, a
    constant and a none case among them."""
    from raft import _native as N
    C = N.SPECTRUM_CODES
    js = [(C["JONSWAP"], Hs, Tp, g, i) for i, (Hs, Tp, g, _) in enumerate(W.sea_cases())]
    return [(C["unit"], 2.5, 9.0, 0.0, None)] + js[:4] + [(C["constant"], 3.7, 9.0, 2.0, None)] + js[4:] + \
        [(C["none"], 5.0, 9.0, 0.0, None)]


@pytest.mark.parametrize("want_S", [True, False])
@pytest.mark.parametrize("nw", [1, 255, 257])
def test_sea_state_mixed_cases(nw, want_S):
    import torch
    from raft import _native as N
    w = W.sea_grid(nw)
    dw = float(w[1] - w[0]) if nw > 1 else 0.05
    cases = mixed_cases()
    nc = len(cases)
    spec = tens([c[0] for c in cases], torch.int32)
    Hs, Tp, gam = (tens([c[i] for c in cases]) for i in (1, 2, 3))
    S = torch.full([nc, nw], -1.0, dtype=torch.float64, device=dev()) if want_S else None
    zeta = torch.full([nc, nw], -1.0, dtype=torch.float64, device=dev())
    st = N.stream_handle(torch, dev())
    wt = tens(w)
    args = (nw, N.ptr(wt), dw, N.ptr(spec), N.ptr(Hs), N.ptr(Tp), N.ptr(gam), N.ptr(S), N.ptr(zeta), st)
    assert N.lib().rh_sea_state(N.context(0), 0, *args) == N.RH_OK           # ncase = 0: nothing to do
    torch.cuda.synchronize()
    assert bool((zeta == -1.0).all())
    N.check(N.lib().rh_sea_state(N.context(0), nc, *args), "rh_sea_state")
    torch.cuda.synchronize()
    zeta = zeta.cpu().numpy()
    S = S.cpu().numpy() if want_S else None
    refs = sea_ref(nw, dw)
    for ic, (code, hs, tp, g, j) in enumerate(cases):
        if j is None:
            exact = {N.SPECTRUM_CODES["unit"]: 1.0, N.SPECTRUM_CODES["constant"]: hs, N.SPECTRUM_CODES["none"]: 0.0}[code]
            if want_S:
                assert np.all(S[ic] == exact), (ic, code)
            assert np.all(zeta[ic] == np.sqrt(2.0 * exact * dw)), (ic, code)
            continue
        if want_S:
            assert np.array_equal(zeta[ic], np.sqrt(2.0 * S[ic] * dw)), ("zeta = sqrt(2 S dw)", ic)
        label = f"rh_sea_state nw={nw} Hs={hs} Tp={float(tp)!r} gamma={g}"
        eS, ez = W.check_sea(label, refs[j], S[ic] if want_S else None, zeta[ic])
        print(f"{label}: e_np {refs[j][3] / U:.1f} u, device S {eS / U:.1f} u, zeta {ez / U:.1f} u, "
              f"{int(refs[j][2].sum())} bins compared")


@pytest.mark.parametrize("nw", [255, 1000])
def test_solve_kernel_zeta(nw):
    """rh_solve_cases' own zeta output (sea_amplitude inside the one-bin and the two-bin solve kernel,
    which do not call rh_sea_state) for the same JONSWAP cases, by the same criterion."""
    from raft.prep import DeviceDesign
    from raft.solver import CaseSet, solve_batch
    from test_gpu_lu import Tables
    w = W.sea_grid(nw)
    eye = np.eye(6)
    dd = DeviceDesign(Tables(w, 1e4 * eye, 1e3 * eye, 1e4 * eye), device=0)
    sc = W.sea_cases()
    n = len(sc)
    cs = CaseSet(np.zeros(n, dtype=np.int32), [0.0] * n, ["JONSWAP"] * n, [c[0] for c in sc], [c[1] for c in sc],
                 [c[2] for c in sc])
    r = solve_batch([dd], cs, 0, 0.1, 0.01, want=("zeta",)).host()
    refs = sea_ref(nw, dd.dw)
    for ic, (hs, tp, g, _) in enumerate(sc):
        label = f"rh_solve_cases zeta nw={nw} Hs={hs} Tp={float(tp)!r} gamma={g}"
        _, ez = W.check_sea(label, refs[ic], None, r["zeta"][ic])
        print(f"{label}: e_np {refs[ic][3] / U:.1f} u, device zeta {ez / U:.1f} u")


# ------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("shape", W.STAT_SHAPES, ids=str)
def test_motion_stats(shape):
    import torch
    from raft import _native as N
    ncase, nrow, nw = shape
    dw = 0.0371
    X = W.stat_inputs(ncase, nrow, 6, nw)
    psd_ref, std_ref = W.motion_reference(X, dw)
    Xt = tens(X)
    st = N.stream_handle(torch, dev())
    psd = torch.full([ncase, 6, nw], -1.0, dtype=torch.float64, device=dev())
    std = torch.full([ncase, 6], -1.0, dtype=torch.float64, device=dev())
    N.check(N.lib().rh_motion_stats(N.context(0), ncase, nrow, nw, dw, N.ptr(Xt), N.ptr(psd), None, st), "rh_motion_stats")
    N.check(N.lib().rh_motion_stats(N.context(0), ncase, nrow, nw, dw, N.ptr(Xt), None, N.ptr(std), st), "rh_motion_stats")
    torch.cuda.synchronize()
    bound = (nrow * nw + 16) * U
    rp = float((np.abs(psd.cpu().numpy().astype(LD) - psd_ref) / (bound * psd_ref)).max())
    rs = float((np.abs(std.cpu().numpy().astype(LD) - std_ref) / (bound * std_ref)).max())
    print(f"rh_motion_stats {shape}: worst ratio to the bound: psd {rp:.3f}, std {rs:.3f}")
    assert rp <= 1.0 and rs <= 1.0, (shape, rp, rs)


@pytest.mark.parametrize("nch", [1, 5])
@pytest.mark.parametrize("ndof", [6, 12])
@pytest.mark.parametrize("shape", W.STAT_SHAPES, ids=str)
def test_channel_stats(shape, ndof, nch):
    import torch
    from raft import _native as N
    ncase, nrow, nw = shape
    dw = 0.0371
    w = np.linspace(0.05, 3.0, nw)
    X = W.stat_inputs(ncase, nrow, ndof, nw)
    coef = W.channel_coef(nch, ndof)
    psd_ref, std_ref, psd_abs, std_abs = W.channel_reference(X, w, coef, dw)
    Xt, wt, ct = tens(X), tens(w), tens(coef)
    st = N.stream_handle(torch, dev())
    psd = torch.full([ncase, nch, nw], -1.0, dtype=torch.float64, device=dev())
    std = torch.full([ncase, nch], -1.0, dtype=torch.float64, device=dev())
    for p, s in ((psd, None), (None, std)):
        N.check(N.lib().rh_channel_stats(N.context(0), ncase, nrow, ndof, nw, dw, N.ptr(wt), N.ptr(Xt), nch, N.ptr(ct),
                                         N.ptr(p), N.ptr(s), st), "rh_channel_stats")
    torch.cuda.synchronize()
    bound = (2 * ndof + nrow * nw + 16) * U
    rp = float((np.abs(psd.cpu().numpy().astype(LD) - psd_ref) / (bound * psd_abs)).max())
    rs = float((np.abs(std.cpu().numpy().astype(LD) - std_ref) / (bound * std_abs)).max())
    print(f"rh_channel_stats {shape} ndof={ndof} nch={nch}: worst ratio to the bound: psd {rp:.3f}, std {rs:.3f}")
    assert rp <= 1.0 and rs <= 1.0, (shape, ndof, nch, rp, rs)
