"""GPU: the Borgman drag linearisation of every solve path, element by element against a long-double
reference: the per-node sums of |v_rel|^2, the node matrices Bmat, the translated B_drag and the drag
excitation, from
  rh_solve_cases with nIter = 0 (one pass linearises at Xi_init; B_drag, Bmat and F_wave are then pure
    functions of the linearisation): k_solve_lds 1 x 128 (nw = 33, 97), 2 x 128 (200), 1 x 512 (257),
    2 x 512 joint and split phase C (513, 1000), two passes (1025, 2048; nn = 77 at nw = 600) and the
    general kernel k_solve_cases (rh_set_solver 1; nn = 212 at nw = 600), solver modes 0, 6, 8, 9, 1;
  rh_linearize (k_lin_sums + k_lin_bdrag + k_drag_exc), nw = 2, 63, 257;
  rh_lin_partial_sums + rh_bin_step over the bin ranges [0, 100), [100, 100), [100, 193), [193, 257);
  rh_drag_excitation, rh_wave_excitation and rh_array_response with a random, non-symmetric Bmat.

Designs, reference and criteria are tests/helpers/drag_cases.py (checked on the CPU by
tests/test_drag_cases.py): members with every pattern of the axial set, circular and rectangular
nodes, one-node and two-node members and one longer than a wave, node counts 1, 4, 5, 11, 40, 76 and the
two at which the dispatch changes kernel (77, 212); heading index 1; a JONSWAP, a unit, a still-water
and a second JONSWAP case per call.  zeta (the kernel's own output where it has one), uhat and finer
(rh_wave_tables on the same design) enter the reference as data.  Every element of every output is
held to its bound; the still-water case is exactly +0 everywhere.  The worst ratio to each bound is
printed (pytest -s); DESIGN.md "Accuracy of the drag linearisation" holds the table of one run.

The dispatch has no grid that reaches k_solve_lds 1 x 256 (nw <= 256 runs on 128 threads whenever the
node tables fit, and they fit whenever the 256-thread layout does), rh_linearize and the other
single-design entry points refuse nw = 1 (the solve entry points need nw >= 2), and no grid beyond
2048 bins is accepted; Xi_init is an argument of the call, not of a case, so the XiStart start is a call
of its own.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import drag_cases as D   # noqa: E402

pytestmark = pytest.mark.gpu
U, LD, CLD = D.U, D.LD, D.CLD
GUARD = 96
HEAD = 1
_DES, _REF = {}, {}
KEYS = ("Bmat", "B_drag", "F_wave")


def dev():
    import torch
    return torch.device("cuda", 0)


def tens(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def bits(a):
    return np.ascontiguousarray(a).view(np.float64 if a.dtype.kind in "fc" else a.dtype)


class solver:
    """rh_set_solver(ctx, mode) for the block."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from raft import _native as N
        N.check(N.lib().rh_set_solver(N.context(0), self.mode), "rh_set_solver")

    def __exit__(self, *exc):
        from raft import _native as N
        N.check(N.lib().rh_set_solver(N.context(0), 0), "rh_set_solver")


def design(name, nw):
    """(DragDesign, DeviceDesign with both headings tabulated, uhat [nn][3][nw] and finer [6][nw] of
    heading HEAD on the host)."""
    if (name, nw) not in _DES:
        import torch
        from raft.hydro_math import DEG2RAD
        from raft.prep import DeviceDesign
        d = D.DragDesign(name, nw)
        dd = DeviceDesign(d, device=0)
        assert dd.ensure_headings([h * DEG2RAD for h in D.HEADINGS_DEG]) == [0, 1]
        torch.cuda.synchronize()
        _DES[(name, nw)] = (d, dd, dd.uhat[HEAD].cpu().numpy(), dd.finer[HEAD].cpu().numpy())
    return _DES[(name, nw)]


def reference(name, nw, ic, Xi, zeta, fext=None, tag=""):
    """drag_reference of one case, computed once per (design, grid, case, tag) and zeta."""
    key = (name, nw, ic, tag)
    hit = _REF.get(key)
    if hit is None or not np.array_equal(hit[0], zeta):
        d, _, uhat, finer = design(name, nw)
        ref = D.drag_reference(d, Xi, zeta, uhat, finer, fext)
        hit = _REF[key] = (zeta.copy(), ref, D.bounds(ref))
    return hit[1], hit[2]


def solve(names, nw, design_idx, case_ids, mode=0, xi_init=True, fext=None):
    """rh_solve_cases with nIter = 0 on the cases case_ids of D.drag_cases() (heading index HEAD), Bmat in a
    NaN-filled buffer with a tail: host arrays, the Xi the pass linearised at, and the raw Bmat buffer."""
    import torch
    from raft.solver import CaseSet, solve_batch
    dds = [design(n, nw)[1] for n in names]
    cases = [D.drag_cases()[i] for i in case_ids]
    nc = len(cases)
    cs = CaseSet(np.asarray(design_idx, dtype=np.int32), [D.HEADINGS_DEG[HEAD]] * nc, [c[0] for c in cases],
                 [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    nnmax = max(dd.nn for dd in dds)
    Xi0 = D.motions(nw)[list(case_ids)] if xi_init else np.full([nc, 6, nw], D.XI_START + 0j)
    raw = torch.full([nc * nnmax * 9 + GUARD], float("nan"), dtype=torch.float64, device=dev())
    Fw = torch.full([nc, 6, nw], complex(float("nan"), float("nan")), dtype=torch.complex128, device=dev())
    with solver(mode):
        r = solve_batch(dds, cs, 0, D.XI_START, 0.01, want=("zeta", "B_drag", "Bmat"), fext=tens(fext) if fext is not None else None,
                        Xi_init=tens(Xi0) if xi_init else None, first_iter=0, F_wave=Fw,
                        out=dict(Bmat=raw[:nc * nnmax * 9].view(nc, nnmax, 3, 3)))
        torch.cuda.synchronize()
    assert list(r._keep[1]["head_host"]) == [HEAD] * nc
    out = r.host()
    out["F_wave"], out["raw"], out["Xi0"] = Fw.cpu().numpy(), raw.cpu().numpy(), Xi0
    return out


def check_case(label, name, nw, ic, out, row, fext=None, tag=""):
    """One case of a solve against the reference: the ratios of Bmat, B_drag and F_wave to their bounds (the
    still-water case: exactly +0, asserted here), one linear solve, a regular status, a finite response."""
    from raft import _native as N
    d = design(name, nw)[0]
    assert out["iters"][row] == 1 and out["status"][row] in (N.RH_CASE_CONVERGED, N.RH_CASE_NOT_CONVERGED), (label, ic)
    assert np.all(np.isfinite(out["Xi"][row].real)) and np.all(np.isfinite(out["Xi"][row].imag)), (label, ic)
    got = dict(Bmat=out["Bmat"][row, :d.nn], B_drag=out["B_drag"][row], F_wave=out["F_wave"][row])
    if ic == D.STILL and fext is None:
        assert np.all(out["zeta"][row] == 0)
        for k, a in got.items():
            assert D.plus_zero(a), (label, "still water", k)
        return {}
    ref, bd = reference(name, nw, ic, out["Xi0"][row], out["zeta"][row], fext, tag)
    return {k: D.worst(got[k], getattr(ref, k), getattr(bd, k)) for k in KEYS}


def check_solve(label, name, nw, out, case_ids, fext=None, tag=""):
    worst = {}
    for row, ic in enumerate(case_ids):
        for k, v in check_case(label, name, nw, ic, out, row, None if fext is None else fext[row], tag).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{label}: worst ratio to the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (label, k, v)


def same_bits(label, a, b, keys=KEYS + ("zeta",)):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), (label, k)
    assert np.array_equal(a["raw"].view(np.int64), b["raw"].view(np.int64)), (label, "Bmat buffer")


ALL = (0, 1, 2, 3)


def run_modes(name, nw, modes):
    """Mode 0 against the reference; 6, 8, 9 the same bits and the same bounds; 1 (the general kernel) the
    bounds."""
    d = design(name, nw)[0]
    kern = D.solve_kernel(nw, d.nn, d.nm)
    base = None
    for mode in modes:
        out = solve([name], nw, [0] * 4, ALL, mode)
        label = f"rh_solve_cases {name} nn={d.nn} nw={nw} solver {mode} ({'general' if mode == 1 else kern})"
        assert np.all(np.isnan(out["raw"][4 * d.nn * 9:])), (label, "the tail behind Bmat was written")
        check_solve(label, name, nw, out, ALL)
        if mode == 0:
            base = out
        elif mode != 1:
            same_bits(label, out, base)


# ------------------------------------------------------------------------------ rh_solve_cases
@pytest.mark.parametrize("nw", [33, 97, 200, 257, 513, 1000, 1025, 2048])
def test_solve_default_design(nw):
    modes = [0, 6] + ([8, 9] if 512 < nw <= 1024 else []) + ([1] if nw in (33, 257, 1000, 2048) else [])
    run_modes("default", nw, modes)


@pytest.mark.parametrize("nw", [33, 97, 200, 257])
@pytest.mark.parametrize("name", D.SMALL)
def test_solve_small_designs(name, nw):
    run_modes(name, nw, [0, 6] + ([1] if nw == 33 else []))


@pytest.mark.parametrize("nw", [513, 1000])
def test_solve_forty_nodes_two_bins(nw):
    run_modes("nn40", nw, [0, 6, 8, 9])


@pytest.mark.parametrize("name", D.LARGE)
def test_solve_large_designs(name):
    """nn = 77: a grid of 512 < nw <= 1024 no longer fits the one-pass kernel and runs the two-pass one with
    an empty second pass; nn = 212: beyond the two-pass kernel too, the general kernel."""
    d = design(name, 600)[0]
    assert D.solve_kernel(600, d.nn, d.nm) == ("two-pass" if name == "nn77" else "general")
    run_modes(name, 600, [0, 6, 1])


@pytest.mark.parametrize("nw", [97, 1000])
def test_solve_with_external_force(nw):
    """fext enters F_wave as an addend and nothing else."""
    rng = np.random.default_rng(nw)
    fext = (rng.standard_normal([4, 6, nw]) + 1j * rng.standard_normal([4, 6, nw])) * 1e3
    out = solve(["default"], nw, [0] * 4, ALL, 0, fext=fext)
    check_solve(f"rh_solve_cases default nw={nw} with fext", "default", nw, out, ALL, fext, "fext")
    same_bits("fext", out, solve(["default"], nw, [0] * 4, ALL, 0), ("Bmat", "B_drag", "zeta"))


@pytest.mark.parametrize("nw", [257, 513])
def test_solve_from_xistart(nw):
    """Xi_init = NULL: the pass linearises at XiLast = XiStart = 0.1 in every DOF and bin."""
    ids = (0, 3)
    out = solve(["default"], nw, [0, 0], ids, 0, xi_init=False)
    check_solve(f"rh_solve_cases default nw={nw} from XiStart", "default", nw, out, ids, tag="xistart")


@pytest.mark.parametrize("nw", [97, 513])
def test_two_designs_in_one_call(nw):
    """Designs of different nn and nm in one launch: each case's outputs are the bits of the call with its
    design alone; the rows nn <= n < nn_max of the smaller design's cases and the tail stay NaN."""
    names = ["nn11", "default"]
    didx, ids = [0, 1, 1, 0], ALL
    both = solve(names, nw, didx, ids)
    nnmax = 76
    alone = [solve([n], nw, [0] * 4, ids) for n in names]
    for row, di in enumerate(didx):
        d = design(names[di], nw)[0]
        one = alone[di]
        for k in ("B_drag", "F_wave", "zeta", "Xi"):
            assert np.array_equal(bits(both[k][row]), bits(one[k][row])), (nw, row, k)
        assert np.array_equal(bits(both["Bmat"][row, :d.nn]), bits(one["Bmat"][row]))
        assert np.all(np.isnan(both["Bmat"][row, d.nn:])), (nw, row, "rows beyond nn were written")
        for k, v in check_case(f"two designs nw={nw}", names[di], nw, ids[row], both, row).items():
            assert v <= 1.0, (nw, row, k, v)
    assert np.all(np.isnan(both["raw"][4 * nnmax * 9:]))


# ------------------------------------------------------------------------------ rh_linearize
@pytest.mark.parametrize("nw", [2, 63, 257])
@pytest.mark.parametrize("name", list(D.DESIGNS))
def test_linearize(name, nw):
    import torch
    from raft import _native as N
    d, dd, _, _ = design(name, nw)
    ds = dd.struct()
    zeta, Xi = D.sea_zeta(d), D.motions(nw)
    st = N.stream_handle(torch, dev())
    worst = {}
    for ic in (0, 1, D.STILL):
        Bd = torch.full([36 + GUARD], float("nan"), dtype=torch.float64, device=dev())
        Bm = torch.full([d.nn * 9 + GUARD], float("nan"), dtype=torch.float64, device=dev())
        Fd = torch.full([6 * nw + GUARD], complex(float("nan"), 0.0), dtype=torch.complex128, device=dev())
        xt, zt = tens(Xi[ic]), tens(zeta[ic])
        N.check(N.lib().rh_linearize(N.context(0), ctypes.byref(ds), HEAD, N.ptr(xt), N.ptr(zt), N.ptr(Bd), N.ptr(Bm),
                                     N.ptr(Fd), st), "rh_linearize")
        torch.cuda.synchronize()
        Bd, Bm, Fd = Bd.cpu().numpy(), Bm.cpu().numpy(), Fd.cpu().numpy()
        assert np.all(np.isnan(Bd[36:])) and np.all(np.isnan(Bm[d.nn * 9:])) and np.all(np.isnan(Fd[6 * nw:].real))
        got = dict(Bmat=Bm[:d.nn * 9].reshape(d.nn, 3, 3), B_drag=Bd[:36].reshape(6, 6), F_drag=Fd[:6 * nw].reshape(6, nw))
        if ic == D.STILL:
            for k, a in got.items():
                assert D.plus_zero(a), (name, nw, "still water", k)
            continue
        ref, bd = reference(name, nw, ic, Xi[ic], zeta[ic], tag="host zeta")
        for k, a in got.items():
            worst[k] = max(worst.get(k, 0.0), D.worst(a, getattr(ref, k), getattr(bd, k)))
    print(f"rh_linearize {name} nn={d.nn} nw={nw}: worst ratio to the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (name, nw, k, v)


# ------------------------------------------------------------------------------ the bin-sharded path
RANGES = ((0, 100), (100, 100), (100, 193), (193, 257))


@pytest.mark.parametrize("name", ["default", "nn11"])
def test_partial_sums_and_bin_step(name):
    import torch
    from raft import _native as N
    nw = 257
    d, dd, _, _ = design(name, nw)
    ds = dd.struct()
    zeta, Xi = D.sea_zeta(d), D.motions(nw)
    st, ctx, lib = N.stream_handle(torch, dev()), N.context(0), N.lib()
    for ic in (0, D.STILL):
        zt, xt = tens(zeta[ic]), tens(Xi[ic])
        still = ic == D.STILL
        if not still:
            ref, bd = reference(name, nw, ic, Xi[ic], zeta[ic], tag="host zeta")
        total = np.zeros([d.nn, 3])
        rs = 0.0
        for lo, hi in RANGES:
            s = torch.full([d.nn * 3 + GUARD], float("nan"), dtype=torch.float64, device=dev())
            N.check(lib.rh_lin_partial_sums(ctx, ctypes.byref(ds), HEAD, N.ptr(xt), N.ptr(zt), lo, hi, N.ptr(s), st),
                    "rh_lin_partial_sums")
            s = s.cpu().numpy()
            assert np.all(np.isnan(s[d.nn * 3:]))
            part = s[:d.nn * 3].reshape(d.nn, 3)
            if still or lo == hi:
                assert D.plus_zero(part), (name, lo, hi)
            else:
                rs = max(rs, D.worst(part, ref.tb[:, :, lo:hi].sum(axis=2), D.bounds(ref, lo, hi).sums))
            total = total + part                                      # the caller's all-reduce
        if not still:
            rs = max(rs, D.worst(total, ref.sums, bd.sums))
        first, rb, tt = None, {}, tens(total)
        for lo, hi in RANGES:
            Bm = torch.full([d.nn * 9 + GUARD], float("nan"), dtype=torch.float64, device=dev())
            Bd = torch.full([36 + GUARD], float("nan"), dtype=torch.float64, device=dev())
            X = torch.zeros([6, nw], dtype=torch.complex128, device=dev())
            XL = xt.clone()
            fl = torch.zeros([3], dtype=torch.int32, device=dev())
            N.check(lib.rh_bin_step(ctx, ctypes.byref(ds), HEAD, N.ptr(zt), None, N.ptr(tt), 0.01, lo, hi, N.ptr(Bm),
                                    N.ptr(Bd), N.ptr(X), N.ptr(XL), N.ptr(fl), st), "rh_bin_step")
            Bm, Bd, fl = Bm.cpu().numpy(), Bd.cpu().numpy(), fl.cpu().numpy()
            assert np.all(np.isnan(Bm[d.nn * 9:])) and np.all(np.isnan(Bd[36:])) and fl[1] == 0 and fl[2] == 0
            got = dict(Bmat=Bm[:d.nn * 9].reshape(d.nn, 3, 3), B_drag=Bd[:36].reshape(6, 6))
            if first is None:
                first = got
            for k, a in got.items():
                assert np.array_equal(bits(a), bits(first[k])), (name, lo, hi, k, "differs between the ranges")
                if still:
                    assert D.plus_zero(a), (name, "still water", k)
                else:
                    rb[k] = max(rb.get(k, 0.0), D.worst(a, getattr(ref, k), getattr(bd, k)))
        if not still:
            print(f"rh_lin_partial_sums + rh_bin_step {name} nw={nw}: worst ratio to the bound: sums {rs:.3f}, " +
                  ", ".join(f"{k} {v:.3f}" for k, v in rb.items()))
            assert rs <= 1.0 and all(v <= 1.0 for v in rb.values()), (name, rs, rb)


# ------------------------------------------------------------------------------ excitation of a given Bmat
@pytest.mark.parametrize("nw", [63, 257])
@pytest.mark.parametrize("name", ["default", "nn11"])
def test_excitation_of_a_random_bmat(name, nw):
    """rh_drag_excitation (k_drag_exc) and rh_wave_excitation (k_heading_resp) with node matrices of nine
    independent entries; second case of each call: still water with Bmat = 0."""
    import torch
    from raft import _native as N
    d, dd, uhat, finer = design(name, nw)
    ds = dd.struct()
    st, ctx, lib = N.stream_handle(torch, dev()), N.context(0), N.lib()
    zeta = D.sea_zeta(d)[[0, D.STILL]]
    Bm = np.stack([D.random_bmat(d.nn), np.zeros([d.nn, 3, 3])])
    e = D.excitation_reference(d, Bm[0], np.zeros([d.nn, 3, 3], dtype=LD), np.abs(Bm[0]).astype(LD), zeta[0], uhat, finer)
    node = D.C_NODE * (d.nn + 16) * U
    b_drag, b_wave = node * e.G_abs, node * (e.G_abs + e.G_lin)
    zt, bt = tens(zeta), tens(Bm)
    Fd = torch.full([2, 6 * nw + GUARD], complex(float("nan"), 0.0), dtype=torch.complex128, device=dev())
    for i in range(2):
        N.check(lib.rh_drag_excitation(ctx, ctypes.byref(ds), HEAD, N.ptr(zt[i]), N.ptr(bt[i]), N.ptr(Fd[i]), st),
                "rh_drag_excitation")
    Fd = Fd.cpu().numpy()
    assert np.all(np.isnan(Fd[:, 6 * nw:].real))
    Fd = Fd[:, :6 * nw].reshape(2, 6, nw)
    arr = (N.RhDesign * 1)(ds)
    didx, head = tens([0, 0], torch.int32), tens([HEAD, HEAD], torch.int32)
    Fw = torch.full([2 * 6 * nw + GUARD], complex(float("nan"), 0.0), dtype=torch.complex128, device=dev())
    N.check(lib.rh_wave_excitation(ctx, arr, 1, 2, N.ptr(didx), N.ptr(head), N.ptr(zt), N.ptr(bt), N.ptr(Fw), st),
            "rh_wave_excitation")
    Fw = Fw.cpu().numpy()
    assert np.all(np.isnan(Fw[12 * nw:].real))
    Fw = Fw[:12 * nw].reshape(2, 6, nw)
    rd, rw = D.worst(Fd[0], e.F_drag, b_drag), D.worst(Fw[0], e.F_wave, b_wave)
    print(f"random Bmat {name} nn={d.nn} nw={nw}: worst ratio to the bound: rh_drag_excitation {rd:.3f}, "
          f"rh_wave_excitation {rw:.3f}")
    assert rd <= 1.0 and rw <= 1.0, (name, nw, rd, rw)
    for what, a in (("rh_drag_excitation", Fd[1]), ("rh_wave_excitation", Fw[1])):
        assert D.plus_zero(a), (name, nw, "still water", what)


@pytest.mark.parametrize("nw", [63, 257, 600])
@pytest.mark.parametrize("name", ["default", "nn11"])
def test_array_response_excitation(name, nw):
    """k_array_exc, the excitation rh_array_response forms for itself (tests/test_gpu_sweep.py ties it to
    the other two only through a response, at 1e-12 of a norm).  It takes the three coefficients e^T Bmat e
    out of the node matrices, so Bmat is the reference's own, rounded to double; one FOWT, no array
    stiffness and B_drag = 0 make Z the design's diagonal impedance, and F = Z Xi recovers the excitation.
    Second case: still water with Bmat = 0."""
    import torch
    from raft import _native as N
    d, dd, uhat, finer = design(name, nw)
    st, ctx, lib = N.stream_handle(torch, dev()), N.context(0), N.lib()
    zeta = D.sea_zeta(d)[[0, D.STILL]]
    ref, _ = reference(name, nw, 0, D.motions(nw)[0], zeta[0], tag="host zeta")
    Bm = np.stack([ref.Bmat.astype(np.float64), np.zeros([d.nn, 3, 3])])
    e = D.excitation_reference(d, Bm[0], np.zeros([d.nn, 3, 3], dtype=LD), ref.B_abs, zeta[0], uhat, finer)
    node = D.C_NODE * (d.nn + 16) * U
    arr = (N.RhDesign * 1)(dd.struct())
    didx, head = tens([0, 0], torch.int32), tens([HEAD, HEAD], torch.int32)
    zt, bt, bd0 = tens(zeta), tens(Bm), tens(np.zeros([2, 36]))
    X = torch.full([2 * 6 * nw + GUARD], complex(float("nan"), 0.0), dtype=torch.complex128, device=dev())
    N.check(lib.rh_array_response(ctx, arr, 1, 1, 2, N.ptr(didx), N.ptr(head), N.ptr(zt), N.ptr(bd0), N.ptr(bt), None,
                                  N.ptr(X), st), "rh_array_response")
    X = X.cpu().numpy()
    assert np.all(np.isnan(X[12 * nw:].real))
    X = X[:12 * nw].reshape(2, 6, nw)
    # Z = -w^2 M + i w B + C of the diagonal M, B, C, in long double; the device's own rounding of Z and of
    # the division moves Z Xi by at most 8 u (w^2 |M| + |C| + w |B|) |Xi|
    w = d.w.astype(LD)
    m, b, c = (np.diag(a).astype(LD)[:, None] for a in (d.M, d.B, d.C))
    Fa = ((c - w * w * m) + 1j * (w * b)) * X[0].astype(CLD)
    bound = node * (e.G_abs + e.G_lin) + D.C_TERM * U * e.G_abs + 8 * U * (w * w * np.abs(m) + np.abs(c) + w * np.abs(b)) * np.abs(X[0])
    ra = D.worst(Fa, e.F_wave, bound)
    print(f"rh_array_response {name} nn={d.nn} nw={nw}: worst ratio of Z Xi to the bound of F_wave: {ra:.3f}")
    assert ra <= 1.0, (name, nw, ra)
    assert np.all(X[1] == 0), (name, nw, "still water")      # (a quotient: the sign of its zeros is Z's)
