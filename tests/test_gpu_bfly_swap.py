"""GPU: the node-sum butterflies of k_solve_lds (tbfly8, tbfly4, tbfly3: the rows first, by lane swaps;
tests/test_bfly_model.py is their order written out) through what they feed.

(a) Round edges.  Designs of 1, 2, 3, 4, 5, 7, 8 and 9 nodes, each node with its own areas and drag
    coefficients (a sum routed to another node's slot lands outside the bound), on k_solve_lds 2 x 512
    (nw = 513: one lane owns a second bin; nw = 1000: pad lanes in wave 7), 2 x 128 (200), 1 x 512 (257)
    and the two-pass kernel (1025, tbfly3 per node): Bmat, B_drag and F_wave of one linearising pass
    against the long-double reference, with the designs' members, the cases, the bounds and the constants
    of tests/helpers/drag_cases.py as tests/test_gpu_drag.py uses them.
(b) Slot independence.  A 9-node design and three copies of it with 1, 2 and 3 more nodes in a leading
    member of their own, all of whose drag coefficients (and inertial terms) are zero: every node of the
    design then sits in another butterfly slot of its ring round.  The extra nodes add exact zeros, in
    node order, so Bmat of the design's nodes, B_drag, iters and status of a whole fixed point are the
    same bits in all four (nw = 513 on 2 x 512, nw = 200 on 2 x 128).
(c) RMS sums (phase C's tbfly3): std of a converged 513-bin case against NumPy on the returned Xi, within
    the bound of the stats tests (tests/test_gpu_lu.py check_stats: rtol 1e-13).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import drag_cases as D   # noqa: E402

pytestmark = pytest.mark.gpu
HEAD = 1
GUARD = 96
ALL = (0, 1, 2, 3)
KEYS = ("Bmat", "B_drag", "F_wave")
COMPS = {
    "bf1": [("side", 1)],
    "bf2": [("none", 2)],
    "bf3": [("mid", 3)],
    "bf4": [("end", 1), ("mid", 3)],
    "bf5": [("none", 2), ("mid", 3)],
    "bf7": [("side", 1), ("all", 4), ("none", 2)],
    "bf8": [("all", 5), ("mid", 3)],
    "bf9": [("side", 1), ("none", 2), ("all", 5), ("end", 1)],
}
NODE_COUNTS = {"bf1": 1, "bf2": 2, "bf3": 3, "bf4": 4, "bf5": 5, "bf7": 7, "bf8": 8, "bf9": 9}
_DEV = {}


def dev():
    import torch
    return torch.device("cuda", 0)


def tens(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=dev())


def bits(a):
    return np.ascontiguousarray(a).view(np.float64 if a.dtype.kind in "fc" else a.dtype)


def drag_design(name, comp, nw):
    """D.DragDesign of a composition of this file's (the helper's table is left as it is)."""
    assert name not in D.DESIGNS
    D.DESIGNS[name] = comp
    try:
        return D.DragDesign(name, nw)
    finally:
        del D.DESIGNS[name]


def on_device(key, d):
    """(DragDesign, DeviceDesign with both headings tabulated, uhat and finer of heading HEAD on the host)."""
    if key not in _DEV:
        import torch
        from raft.hydro_math import DEG2RAD
        from raft.prep import DeviceDesign
        dd = DeviceDesign(d, device=0)
        assert dd.ensure_headings([h * DEG2RAD for h in D.HEADINGS_DEG]) == [0, 1]
        torch.cuda.synchronize()
        _DEV[key] = (d, dd, dd.uhat[HEAD].cpu().numpy(), dd.finer[HEAD].cpu().numpy())
    return _DEV[key]


def solve(dd, nn, nw, case_ids, nIter, Xi0=None, want=("zeta", "B_drag", "Bmat")):
    """rh_solve_cases (the default solver) on the cases case_ids of D.drag_cases(), heading index HEAD; Bmat
    in a NaN-filled buffer with a tail."""
    import torch
    from raft.solver import CaseSet, solve_batch
    cases = [D.drag_cases()[i] for i in case_ids]
    nc = len(cases)
    cs = CaseSet(np.zeros(nc, dtype=np.int32), [D.HEADINGS_DEG[HEAD]] * nc, [c[0] for c in cases],
                 [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
    raw = torch.full([nc * nn * 9 + GUARD], float("nan"), dtype=torch.float64, device=dev())
    Fw = torch.full([nc, 6, nw], complex(float("nan"), float("nan")), dtype=torch.complex128, device=dev())
    r = solve_batch([dd], cs, nIter, D.XI_START, 0.01, want=want, Xi_init=None if Xi0 is None else tens(Xi0),
                    first_iter=0, F_wave=Fw, out=dict(Bmat=raw[:nc * nn * 9].view(nc, nn, 3, 3)))
    torch.cuda.synchronize()
    assert list(r._keep[1]["head_host"]) == [HEAD] * nc
    out = r.host()
    out["F_wave"], out["raw"] = Fw.cpu().numpy(), raw.cpu().numpy()
    return out


# ------------------------------------------------------------------------------ (a) round edges
@pytest.mark.parametrize("nw, kernel", [(513, "2x512"), (1000, "2x512"), (200, "2x128"), (257, "1x512"), (1025, "two-pass")])
def test_round_edges(nw, kernel):
    from raft import _native as N
    Xi0 = D.motions(nw)
    for name, comp in COMPS.items():
        d, dd, uhat, finer = on_device((name, nw), drag_design(name, comp, nw))
        assert d.nn == NODE_COUNTS[name] and D.solve_kernel(nw, d.nn, d.nm) == kernel
        out = solve(dd, d.nn, nw, ALL, 0, Xi0)
        assert np.all(np.isnan(out["raw"][4 * d.nn * 9:])), (name, nw, "the tail behind Bmat was written")
        worst = {}
        for row, ic in enumerate(ALL):
            assert out["iters"][row] == 1 and out["status"][row] in (N.RH_CASE_CONVERGED, N.RH_CASE_NOT_CONVERGED)
            assert np.all(np.isfinite(out["Xi"][row].real)) and np.all(np.isfinite(out["Xi"][row].imag))
            got = dict(Bmat=out["Bmat"][row], B_drag=out["B_drag"][row], F_wave=out["F_wave"][row])
            if ic == D.STILL:
                assert np.all(out["zeta"][row] == 0)
                for k, a in got.items():
                    assert D.plus_zero(a), (name, nw, "still water", k)
                continue
            ref = D.drag_reference(d, Xi0[ic], out["zeta"][row], uhat, finer)
            bd = D.bounds(ref)
            for k in KEYS:
                worst[k] = max(worst.get(k, 0.0), D.worst(got[k], getattr(ref, k), getattr(bd, k)))
        print(f"{name} nn={d.nn} nw={nw} ({kernel}): worst ratio to the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        for k, v in worst.items():
            assert v <= 1.0, (name, nw, k, v)


# ------------------------------------------------------------------------------ (b) slot independence
PER_MEMBER = ("rA", "mq", "mp1", "mp2")
PER_NODE = ("t", "r_rel", "q", "p1", "p2", "circ", "ds", "drs", "dls", "Cd_q", "Cd_End", "Cd_p1", "Cd_p2", "r", "area",
            "Imat", "a_i")


def padded(base, k, nw):
    """`base` behind k more nodes in a leading member of their own that carry no drag and no inertial
    excitation: the nodes and members of `base` as they are, node for node."""
    d = drag_design(f"{base.name}+{k}", [("side", k)] + base.comp, nw)
    for a in PER_MEMBER:
        getattr(d, a)[1:] = getattr(base, a)
    for a in PER_NODE:
        getattr(d, a)[k:] = getattr(base, a)
    for a in ("Cd_q", "Cd_End", "Cd_p1", "Cd_p2", "a_i", "Imat"):
        getattr(d, a)[:k] = 0.0
    assert not d.axial[:k].any() and np.array_equal(d.axial[k:], base.axial)
    return d


@pytest.mark.parametrize("nw, kernel", [(513, "2x512"), (200, "2x128")])
def test_slot_independence(nw, kernel):
    base = drag_design("bf9", COMPS["bf9"], nw)
    outs = []
    for k in range(4):
        d = base if k == 0 else padded(base, k, nw)
        assert d.nn == 9 + k and D.solve_kernel(nw, d.nn, d.nm) == kernel
        _, dd, _, _ = on_device(("bf9", nw) if k == 0 else (d.name, nw), d)
        out = solve(dd, d.nn, nw, ALL, 12)
        out["Bmat"] = out["Bmat"][:, k:]
        assert np.all(out["raw"][:4 * d.nn * 9].reshape(4, d.nn, 9)[:, :k] == 0), (nw, k, "the leading nodes' Bmat")
        outs.append(out)
    assert outs[0]["iters"].max() > 1, "the fixed point has to iterate for the test to say anything"
    print(f"nw={nw} ({kernel}): iters {list(outs[0]['iters'])} status {list(outs[0]['status'])}")
    for k in range(1, 4):
        for key in ("Bmat", "B_drag", "iters", "status"):
            assert np.array_equal(bits(outs[k][key]), bits(outs[0][key])), (nw, k, key)


# ------------------------------------------------------------------------------ (c) RMS sums
def test_std_of_a_converged_case():
    from raft import _native as N
    nw = 513
    d, dd, _, _ = on_device(("bf9", nw), drag_design("bf9", COMPS["bf9"], nw))
    out = solve(dd, d.nn, nw, (0, 1, 3), 40, want=("zeta", "std"))
    assert np.all(out["status"] == N.RH_CASE_CONVERGED), out["status"]
    x = out["Xi"].copy()
    x[:, 3:] *= 180.0 / np.pi
    ref = np.sqrt(0.5 * (np.abs(x) ** 2).sum(axis=2))
    print("std: worst relative difference", float(np.max(np.abs(out["std"] - ref) / ref)))
    np.testing.assert_allclose(out["std"], ref, rtol=1e-13)
