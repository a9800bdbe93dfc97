"""GPU: the dense complex solves under every response -- rh::lu_solve<6>, rh::lu_factor<6> /
rh::lu_apply<6> and the two-FOWT block solve -- on adversarial systems, one arbitrary matrix per bin,
through every entry point that reaches them.

The inputs, their lane layout and the references are tests/helpers/lu_cases.py (checked on the CPU by
tests/test_lu_cases.py): pivot patterns that exchange every pair of rows, waves of 64 bins in which no
lane, every lane, or every other lane exchanges at each step, ties, bad scaling, ill conditioning,
exactly singular systems, and for two FOWTs weak, zero and singular first blocks.

A design with mb_per_bin = 1, C = 0, M_b = -Re Z_b / w_b^2, B_b = Im Z_b / w_b and one node without
drag area puts Z_b in bin b; the grid w cycles through powers of two, so the device's Z is the
intended matrix bit for bit (asserted through the Z output, within 2 ulp).  Spectrum 'none' makes the
excitation fext, and without drag every iteration solves the same system: Xi = Z^-1 fext.

Criteria (u = 2^-53; eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), residual in mpmath):
  GEPP paths (every 6 x 6 solve, the LDS kernel k_system_solve): per system
      eta <= 8 max(worst eta of numpy.linalg.solve on that family, u);
      on family C also forward error <= 64 kappa_inf u on a subsample;
  block paths (k_system_solve_reg<2>, k_array_resp<2>): the same on B-P and on B-W with kappa = 1,
      eta <= 8 u kappa_2(A) on B-W (A = Z1 + K11);
  NaN rule: no regular system gives a NaN, every singular one gives NaN in all its rows -- for the
      block paths a singular first block (B-0) counts as singular, while the LDS kernel, which pivots
      across the blocks, solves B-0 to the GEPP criterion.
The worst eta per family and path is printed next to numpy's (pytest -s); DESIGN.md section
"Accuracy of the dense solves" holds the table of one run.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lu_cases as L   # noqa: E402

pytestmark = pytest.mark.gpu
U = L.U
_CACHE = {}


# ------------------------------------------------------------------------------ designs
def grid(nw):
    """Powers of two, so that -w^2 (Re Z / -w^2) and w (Im Z / w) give Z back exactly."""
    return 2.0 ** ((np.arange(nw) % 4) - 1.0)


class Tables:
    """What prep.DeviceDesign reads of a FOWT: the grid, one submerged node without drag area or
    inertia (unit axes, so every node formula stays finite and contributes exact zeros) and the
    linear matrices, per bin ([nw][6][6]) or frequency independent ([6][6])."""

    def __init__(self, w, M, B, C):
        self.w, self.nw, self.dw = w, len(w), 0.125
        self.depth, self.rho_water, self.g = 200.0, 1025.0, 9.81
        self.M, self.B, self.C = M, B, C

    def host_tables(self):
        from raft import _native as N
        node = np.zeros([N.NF_COUNT, 1])
        for f, v in (("RZ", -10.0), ("XZ", -10.0), ("QZ", 1.0), ("P1X", 1.0), ("P2Y", 1.0), ("CIRC", 1.0)):
            node[N.NF[f], 0] = v
        memb = np.zeros([N.MF_COUNT, 1])
        memb[2, 0] = memb[6, 0] = memb[13, 0] = 1.0      # q, p1, p2
        memb[10, 0], memb[15, 0] = -10.0, 10.0           # rA x p1, rA x p2 for rA = (0, 0, -10)
        memb[18:21, 0] = 1.0
        parts = [("w", self.w), ("k", self.w * self.w / self.g), ("node", node), ("memb", memb),
                 ("M", self.M), ("B", self.B), ("C", self.C)]
        layout, off = {}, 0
        for name, a in parts:
            layout[name] = (off, a.shape)
            off += a.size
        packed = np.concatenate([np.ascontiguousarray(a, dtype=float).ravel() for _, a in parts])
        return dict(packed=packed, layout=layout, imat=None, mstart=np.array([0, 1], dtype=np.int32), nn=1, nm=1,
                    per_bin=self.M.ndim == 3)


def design_of(A):
    """A DeviceDesign whose impedance in bin b is A[b]."""
    from raft.prep import DeviceDesign
    w = grid(len(A))
    M = -A.real / (w * w)[:, None, None]
    B = A.imag / w[:, None, None]
    assert np.array_equal(-(w * w)[:, None, None] * M, A.real) and np.array_equal(w[:, None, None] * B, A.imag)
    return DeviceDesign(Tables(w, M, B, np.zeros([6, 6])), device=0)


def dev():
    import torch
    return torch.device("cuda", 0)


def tens(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


class general_solver:
    """rh_set_solver(ctx, 1) for the block (the general case kernel, the LDS system solve)."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        from raft import _native as N
        N.check(N.lib().rh_set_solver(N.context(0), 1 if self.on else 0), "rh_set_solver")

    def __exit__(self, *exc):
        from raft import _native as N
        N.check(N.lib().rh_set_solver(N.context(0), 0), "rh_set_solver")


# ------------------------------------------------------------------------------ shared inputs
def cases6(nw):
    """Three one-design cases on a grid: layout variant 0 (the quiet, busy and mixed waves), variant 2
    (every family, every exact pair) and variant 1 with family Z in three bins, the last bin among
    them.  With numpy's eta per system and its worst per family over the two regular ones."""
    if ("c6", nw) not in _CACHE:
        s0, s2 = L.layout(nw, 0), L.layout(nw, 2)
        sz = L.with_singular(L.layout(nw, 1), sorted({min(5, nw - 1), min(70, nw - 1), nw - 1}))
        for s in (s0, s2, sz):
            s.eta_np, s.worst = L.numpy_eta(s)
        worst = {}
        for s in (s0, s2, sz):
            for f, v in s.worst.items():
                worst[f] = max(worst.get(f, 0.0), v)
        _CACHE[("c6", nw)] = ([s0, s2, sz], worst)
    return _CACHE[("c6", nw)]


def cases12(nw):
    if ("c12", nw) not in _CACHE:
        out = []
        worst = {}
        for case in range(3):
            Z, K, F, s = L.systems12(nw, case)
            s.eta_np, s.worst = L.numpy_eta(s)
            for f, v in s.worst.items():
                worst[f] = max(worst.get(f, 0.0), v)
            out.append((Z, K, F, s))
        _CACHE[("c12", nw)] = (out, worst)
    return _CACHE[("c12", nw)]


def check_gepp(label, s, X, worst, A=None, singular=None, forward=True):
    """The GEPP criterion and the NaN rule for one case: X [n][nw] against the systems s (A overrides
    the matrices, e.g. with the device's own Z)."""
    A = s.A if A is None else A
    sing = s.singular if singular is None else singular
    X = np.asarray(X).T                                     # [nw][n]
    assert np.all(np.isnan(X[sing].real)) and np.all(np.isnan(X[sing].imag)), f"{label}: a singular bin without NaN"
    reg = np.nonzero(~sing)[0]
    assert np.all(np.isfinite(X[reg])), f"{label}: NaN or inf in a regular bin"
    eta = np.full(s.nw, np.nan)
    for b in reg:
        eta[b] = L.backward_error(A[b], s.b[b], X[b])
    print(L.table_row(label, s, eta, {f: worst[f] for f in set(s.fam[reg])}))
    bound = L.gepp_bound(worst)
    for b in reg:
        assert eta[b] <= bound[s.fam[b]], (label, b, s.fam[b], s.name[b], eta[b], bound[s.fam[b]])
    if forward:
        for b in [b for b in reg if s.fam[b] == "C"][:16]:
            kinf = np.linalg.cond(A[b], np.inf)
            fe = L.forward_error(A[b], s.b[b], X[b])
            assert fe <= 64 * kinf * U, (label, b, fe, kinf)
    return eta


def check_block(label, s, X, worst, lds):
    """12 x 12: the block criteria (or, lds, the GEPP criterion with B-0 solved) and the NaN rule."""
    X = np.asarray(X).T
    nan_expected = s.singular if lds else (s.singular | (s.fam == "B-0"))
    assert np.all(np.isnan(X[nan_expected].real)), f"{label}: a singular system without NaN"
    reg = np.nonzero(~nan_expected)[0]
    assert np.all(np.isfinite(X[reg])), f"{label}: NaN or inf in a regular system"
    eta = np.full(s.nw, np.nan)
    for b in reg:
        eta[b] = L.backward_error(s.A[b], s.b[b], X[b])
    print(L.table_row(label, s, eta, {f: worst[f] for f in set(s.fam[reg])}))
    bound = L.gepp_bound(worst)
    for b in reg:
        f = s.fam[b]
        if f == "B-W" and not lds:
            assert eta[b] <= 8 * U * s.kappaA[b], (label, b, eta[b], s.kappaA[b])
            if s.kappaA[b] >= 1.5:
                continue
        assert eta[b] <= bound[f], (label, b, f, s.name[b], eta[b], bound[f])
    return eta


# ------------------------------------------------------------------------------ rh_solve_cases
@pytest.mark.parametrize("nw", [192, 640, 1088])
def test_solve_cases_on_adversarial_bins(nw):
    """nw = 192: one bin per thread; 640: two bins per thread, ragged; 1088: beyond the single-pass
    fast path.  Each on the automatic kernel and on the general one (rh_set_solver(ctx, 1))."""
    from raft import _native as N
    from raft.solver import CaseSet, solve_batch
    ss, worst = cases6(nw)
    dds = [design_of(s.A) for s in ss]
    fext = tens(np.stack([s.b.T for s in ss]))              # [3][6][nw]
    cs = CaseSet(np.arange(3, dtype=np.int32), [0.0] * 3, ["none"] * 3, [0.0] * 3, [10.0] * 3, [0.0] * 3)
    res = []
    for general in (False, True):
        with general_solver(general):
            r = solve_batch(dds, cs, 10, 0.1, 0.01, want=("Z", "psd", "std"), fext=fext).host()
        res.append(r)
        label = f"rh_solve_cases nw={nw} {'general' if general else 'auto'}"
        assert list(r["status"]) == [N.RH_CASE_CONVERGED, N.RH_CASE_CONVERGED, N.RH_CASE_SINGULAR], (label, r["status"])
        for ic in (0, 1):
            Zd = r["Z"][ic].reshape(nw, 6, 6)
            for part in ("real", "imag"):
                got, want = getattr(Zd, part), getattr(ss[ic].A, part)
                assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want))), (label, ic, part)
            check_gepp(f"{label} case {ic}", ss[ic], r["Xi"][ic], worst, A=Zd)
            assert np.all(np.isfinite(r["psd"][ic])) and np.all(np.isfinite(r["std"][ic]))
        for k in ("Xi", "psd", "std"):                      # the singular case: no response at all
            assert np.all(np.isnan(r[k][2].real)), (label, k)
    np.testing.assert_array_equal(res[0]["iters"], res[1]["iters"])
    np.testing.assert_array_equal(res[0]["status"], res[1]["status"])


# ------------------------------------------------------------------------------ rh_bin_step
def test_bin_step_cuts_a_wave():
    """One design per call, [bin_lo, bin_hi) = [0, 100) and [100, 192): wave 1 is cut in two, and the
    second launch's lanes are shifted by 36 bins against the layout's waves."""
    import torch
    from raft import _native as N
    nw = 192
    ss, worst = cases6(nw)
    ctx, lib = N.context(0), N.lib()
    for ic, s in enumerate(ss):
        dd = design_of(s.A)
        dd.ensure_headings([0.0])
        d = dd.struct()
        st = N.stream_handle(torch, dev())
        zeta, sums = tens(np.zeros(nw)), tens(np.zeros(3))
        fext = tens(s.b.T)
        Xi = torch.zeros([6, nw], dtype=torch.complex128, device=dev())
        XL = torch.full([6, nw], 0.1 + 0j, dtype=torch.complex128, device=dev())
        Bm, Bd = tens(np.ones(9)), tens(np.ones(36))
        flags = []
        for lo, hi in ((0, 100), (100, nw)):
            fl = torch.zeros([3], dtype=torch.int32, device=dev())
            N.check(lib.rh_bin_step(ctx, ctypes.byref(d), 0, N.ptr(zeta), N.ptr(fext), N.ptr(sums), 0.01, lo, hi,
                                    N.ptr(Bm), N.ptr(Bd), N.ptr(Xi), N.ptr(XL), N.ptr(fl), st), "rh_bin_step")
            flags.append(fl.cpu().numpy())
        X = Xi.cpu().numpy()
        assert np.all(Bd.cpu().numpy() == 0.0)
        for (lo, hi), fl in zip(((0, 100), (100, nw)), flags):
            assert fl[2] == int(s.singular[lo:hi].any()), (ic, lo, hi, fl)
            assert fl[1] == 0, (ic, fl)
        # the singular bins are reported through flags[2]; the regular ones meet the criterion
        keep = ~s.singular
        X[:, ~keep] = L.NAN
        check_gepp(f"rh_bin_step nw={nw} case {ic}", s, X, worst)


# ------------------------------------------------------------------------------ rh_heading_response_ext
@pytest.mark.parametrize("nw", [65, 192])
def test_heading_response_on_adversarial_bins(nw):
    import torch
    from raft import _native as N
    ss, worst = cases6(nw)
    dds = [design_of(s.A) for s in ss]
    for dd in dds:
        dd.ensure_headings([0.0])
    arr = (N.RhDesign * 3)(*[dd.struct() for dd in dds])
    i32 = torch.int32
    didx, head = tens(np.arange(3), i32), tens(np.zeros(3), i32)
    zeta, Bd, Bm = tens(np.zeros([3, nw])), tens(np.zeros([3, 36])), tens(np.zeros([3, 1, 9]))
    fext = tens(np.stack([s.b.T for s in ss]))
    Xi = torch.ones([3, 6, nw], dtype=torch.complex128, device=dev())       # stale finite memory
    N.check(N.lib().rh_heading_response_ext(N.context(0), arr, 3, 3, N.ptr(didx), N.ptr(head), N.ptr(zeta), N.ptr(Bd),
                                            N.ptr(Bm), 0, N.ptr(fext), N.ptr(Xi), N.stream_handle(torch, dev())),
            "rh_heading_response_ext")
    X = Xi.cpu().numpy()
    for ic, s in enumerate(ss):
        check_gepp(f"rh_heading_response_ext nw={nw} case {ic}", s, X[ic], worst)
    assert ss[2].singular.sum() >= 1


# ------------------------------------------------------------------------------ rh_system_solve(_batch)
@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("nw", [1, 65, 192])
def test_system_solve_one_fowt(nw, lds):
    """nf = 1: k_system_solve_reg<1>, or the LDS elimination with N = 6; three cases in one batch."""
    import torch
    from raft import _native as N
    ss, worst = cases6(nw)
    Z = tens(np.stack([s.A.reshape(1, nw, 36) for s in ss]))              # [3][1][nw][36]
    F = tens(np.stack([s.b.T for s in ss]))
    X = torch.ones([3, 6, nw], dtype=torch.complex128, device=dev())
    with general_solver(lds):
        N.check(N.lib().rh_system_solve_batch(N.context(0), 3, 1, nw, N.ptr(Z), None, N.ptr(F), N.ptr(X),
                                              N.stream_handle(torch, dev())), "rh_system_solve_batch")
        X = X.cpu().numpy()
    for ic, s in enumerate(ss):
        check_gepp(f"rh_system_solve nf=1 nw={nw} {'lds' if lds else 'reg'} case {ic}", s, X[ic], worst)


@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("nw", [1, 65, 192])
def test_system_solve_two_fowts(nw, lds):
    """nf = 2: the block solve k_system_solve_reg<2> against its envelope, the LDS 12 x 12 elimination
    against the GEPP criterion.  Each case has its own K (rh_system_solve); one batch of two cases
    shares case 0's K (rh_system_solve_batch)."""
    import torch
    from raft import _native as N
    cs, worst = cases12(nw)
    st = N.stream_handle(torch, dev())
    label = f"rh_system_solve nf=2 nw={nw} {'lds' if lds else 'block'}"
    with general_solver(lds):
        for case, (Z, K, F, s) in enumerate(cs):
            Zt, Kt, Ft = tens(Z.reshape(2, nw, 36)), tens(K), tens(F.T)
            X = torch.ones([12, nw], dtype=torch.complex128, device=dev())
            N.check(N.lib().rh_system_solve(N.context(0), 2, nw, N.ptr(Zt), N.ptr(Kt), N.ptr(Ft), N.ptr(X), st),
                    "rh_system_solve")
            check_block(f"{label} case {case}", s, X.cpu().numpy(), worst, lds)
        # a batch of two cases that share case 0's K: its systems twice, the second time with other
        # right-hand sides (the case offset of Z, F and Xi)
        Z0, K0, F0, s0 = cs[0]
        F1 = L._cplx(np.random.default_rng(5), nw, 12)
        s1 = L.Systems(s0.A, F1, s0.fam, s0.name, s0.singular)
        s1.kappaA = s0.kappaA
        Zt = tens(np.stack([Z0.reshape(2, nw, 36)] * 2))
        Ft = tens(np.stack([F0.T, F1.T]))
        X = torch.ones([2, 12, nw], dtype=torch.complex128, device=dev())
        N.check(N.lib().rh_system_solve_batch(N.context(0), 2, 2, nw, N.ptr(Zt), N.ptr(tens(K0)), N.ptr(Ft), N.ptr(X), st),
                "rh_system_solve_batch")
        X = X.cpu().numpy()
    check_block(f"{label} batch case 0", s0, X[0], worst, lds)
    check_block(f"{label} batch case 1", s1, X[1], worst, lds)


# ------------------------------------------------------------------------------ rh_array_solve_stats(_ext)
def array_solve(designs, nf, ncase, didx, Bd, K, K_stride, F, ext):
    """F [ncase][6 nf][nw] in, (Xi, psd, std) out."""
    import torch
    from raft import _native as N
    nw = F.shape[-1]
    arr = (N.RhDesign * len(designs))(*[d.struct() for d in designs])
    X = tens(F)
    psd = torch.ones([ncase * nf, 6, nw], dtype=torch.float64, device=dev())
    std = torch.ones([ncase * nf, 6], dtype=torch.float64, device=dev())
    di, Bdt, Kt = tens(didx, torch.int32), tens(Bd), (None if K is None else tens(K))
    st = N.stream_handle(torch, dev())
    dw = designs[0].dw
    if ext:
        N.check(N.lib().rh_array_solve_stats_ext(N.context(0), arr, len(designs), nf, ncase, N.ptr(di), N.ptr(Bdt), N.ptr(Kt),
                                                 K_stride, N.ptr(X), dw, N.ptr(psd), N.ptr(std), st),
                "rh_array_solve_stats_ext")
    else:
        N.check(N.lib().rh_array_solve_stats(N.context(0), arr, len(designs), nf, ncase, N.ptr(di), N.ptr(Bdt), N.ptr(Kt),
                                             N.ptr(X), dw, N.ptr(psd), N.ptr(std), st), "rh_array_solve_stats")
    return X.cpu().numpy(), psd.cpu().numpy(), std.cpu().numpy()


def check_stats(label, X, psd, std, dw):
    """psd = 0.5 |x|^2 / dw and std = sqrt(0.5 sum |x|^2), rotations in degrees, of the returned rows:
    finite where the rows are, NaN where a bin is (psd) and for the whole entry (std)."""
    nf = X.shape[0] // 6
    for f in range(nf):
        x = X[6 * f:6 * f + 6].copy()
        x[3:] *= 180.0 / np.pi
        m2 = np.abs(x) ** 2
        bad = np.isnan(m2)
        assert np.array_equal(np.isnan(psd[f]), bad), label
        np.testing.assert_allclose(psd[f][~bad], (0.5 * m2 / dw)[~bad], rtol=1e-14, err_msg=label)
        if bad.any():
            assert np.all(np.isnan(std[f])), label
        else:
            np.testing.assert_allclose(std[f], np.sqrt(0.5 * m2.sum(axis=1)), rtol=1e-13, err_msg=label)


@pytest.mark.parametrize("nw", [200, 300])
def test_array_solve_one_fowt(nw):
    """k_array_resp<1, MULTI = nw > 256>: a design per case, F in Xi on entry."""
    ss, worst = cases6(nw)
    dds = [design_of(s.A) for s in ss]
    F = np.stack([s.b.T for s in ss])
    X, psd, std = array_solve(dds, 1, 3, np.arange(3), np.zeros([3, 36]), None, 0, F, ext=False)
    for ic, s in enumerate(ss):
        label = f"rh_array_solve_stats nf=1 nw={nw} case {ic}"
        check_gepp(label, s, X[ic], worst)
        check_stats(label, X[ic], psd[ic:ic + 1], std[ic:ic + 1], dds[0].dw)
    assert np.all(np.isfinite(std[:2])) and np.all(np.isnan(std[2]))


@pytest.mark.parametrize("nw", [200, 300])
def test_array_solve_two_fowts(nw):
    """k_array_resp<2, MULTI>: three cases, each with its own K through K_stride (padded to 150
    doubles) and its own pair of mb_per_bin = 1 designs."""
    cs, worst = cases12(nw)
    dds = [design_of(Z[f]) for Z, _, _, _ in cs for f in range(2)]
    stride = 150
    K = np.full([3, stride], 1e300)
    for ic, (_, Kc, _, _) in enumerate(cs):
        K[ic, :144] = Kc.ravel()
    F = np.stack([Fc.T for _, _, Fc, _ in cs])
    X, psd, std = array_solve(dds, 2, 3, np.arange(6), np.zeros([6, 36]), K, stride, F, ext=True)
    for ic, (_, _, _, s) in enumerate(cs):
        label = f"rh_array_solve_stats_ext nf=2 nw={nw} case {ic}"
        check_block(label, s, X[ic], worst, lds=False)
        check_stats(label, X[ic], psd[2 * ic:2 * ic + 2], std[2 * ic:2 * ic + 2], dds[0].dw)
    assert np.all(np.isfinite(std[:2])) and np.all(np.isnan(std[2:]))


@pytest.mark.parametrize("nf", [1, 2])
def test_array_solve_frequency_independent_design(nf):
    """The mb_per_bin = 0 branch of zload: Z_b = (-w_b^2 M + C) + K_ff + i w_b (B + B_drag) from scaled
    random M, B, C, a drag damping and a full random K, on a plain grid, nw = 300.  The reference matrix
    is formed in numpy in the device's order of operations (it may differ from the device's by the
    contraction of w2 * M + C into one FMA: one rounding of a component, below u in eta)."""
    from raft.prep import DeviceDesign
    nw = 300
    rng = np.random.default_rng(40 + nf)
    w = np.linspace(0.05, 3.0, nw)
    mats = [[rng.standard_normal([6, 6]) * 10 ** rng.uniform(-1, 1, [6, 1]) for _ in range(3)] for _ in range(nf)]
    dds = [DeviceDesign(Tables(w, M, B, C), device=0) for M, B, C in mats]
    Bd = rng.standard_normal([nf, 36])
    K = rng.standard_normal([6 * nf, 6 * nf])
    F = L._cplx(rng, 6 * nf, nw)
    Zf = []
    for f, (M, B, C) in enumerate(mats):
        re = (-(w * w))[:, None, None] * M + C + K[6 * f:6 * f + 6, 6 * f:6 * f + 6]
        Zf.append(re + 1j * (w[:, None, None] * (B + Bd[f].reshape(6, 6))))
    A = np.zeros([nw, 6 * nf, 6 * nf], dtype=complex)
    A[:] = K
    for f in range(nf):
        A[:, 6 * f:6 * f + 6, 6 * f:6 * f + 6] = Zf[f]
    s = L.Systems(A, F.T.copy(), ["M"] * nw, ["mb_per_bin = 0"] * nw)
    s.eta_np, worst = L.numpy_eta(s)
    X, psd, std = array_solve(dds, nf, 1, np.arange(nf), Bd, K, 0, F[None], ext=False)
    label = f"rh_array_solve_stats nf={nf} mb_per_bin=0"
    if nf == 1:
        check_gepp(label, s, X[0], worst, forward=False)
    else:
        s.fam = np.array(["B-W"] * nw)
        s.kappaA = np.array([np.linalg.cond(Zf[0][b]) for b in range(nw)])
        check_block(label, s, X[0], {"B-W": worst["M"]}, lds=False)
    check_stats(label, X[0], psd, std, dds[0].dw)
    assert np.all(np.isfinite(std))
