"""GPU: the wave-table kernels (k_wave_tables, k_wave_tables_nodes + k_wave_force_sum,
k_wave_tables_batch) element by element against a long-double reference, on a synthetic design that
aims at every branch of wave_node in one grid.

The design, the reference and the criteria are tests/helpers/wave_cases.py (checked on the CPU by
tests/test_wave_cases.py): depth 200 with k h below 1, on and next to the deep-water switch 89.4 and
above 710 (where sinh and cosh overflow and only the deep branch stays finite), nodes at z = -0.01 and
z = -150, positions up to 1000 m from the origin, PRP-relative positions with an offset, random frames,
a non-symmetric Imat, a_i of both signs, MacCamy-Fuchs nodes with a random complex imat_mcf, three
headings with 0 and pi/2 among them.  Shapes (nn, nw, nhead): nn = 1, 8 run the single-launch kernel,
9 and 21 the node-grid kernel and the force sum (21 leaves a partial node group), nw = 63, 65, 130
leave pad lanes.

Criteria (u = 2^-53, A = |th| + 2 k h + 8): uhat and kproj within 4 A u s per element, finer within
4 (A_max + nn + 16) u S; every table finite; a sentinel tail behind each table untouched; the batched
launch equal to the per-design one bit for bit, with and without a velocity table.  The worst ratio to
each bound is printed (pytest -s); DESIGN.md "Accuracy of the wave tables, sea state and second-order
force" holds the table of one run.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wave_cases as W   # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 96                      # sentinel elements behind every table
SENT = complex(-7.25e11, 3.5e-9)
_CACHE = {}


def dev():
    import torch
    return torch.device("cuda", 0)


def tabulate(wd, betas):
    """rh_wave_tables of the design wd for the headings betas into tables with a sentinel tail:
    (uhat, kproj, finer, tails) on the host."""
    import torch
    from raft import _native as N
    from raft.prep import DeviceDesign
    dd = DeviceDesign(wd, device=0)
    dd.headings = tuple(float(b) for b in betas)
    nh, nn, nw = len(betas), wd.nn, wd.nw
    sizes = dict(uhat=nh * nn * 3 * nw, kproj=nh * nn * 3 * nw, finer=nh * 6 * nw)
    bufs = {k: torch.full([n + GUARD], SENT, dtype=torch.complex128, device=dev()) for k, n in sizes.items()}
    beta_t = torch.tensor(dd.headings, dtype=torch.float64, device=dev())
    d = dd._make_struct()
    N.check(N.lib().rh_wave_tables(N.context(0), ctypes.byref(d), N.ptr(beta_t), N.ptr(bufs["uhat"]), N.ptr(bufs["finer"]),
                                   N.ptr(bufs["kproj"]), N.stream_handle(torch, dev())), "rh_wave_tables")
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    tails = {k: host[k][sizes[k]:] for k in sizes}
    return (host["uhat"][:sizes["uhat"]].reshape(nh, nn, 3, nw), host["kproj"][:sizes["kproj"]].reshape(nh, nn, 3, nw),
            host["finer"][:sizes["finer"]].reshape(nh, 6, nw), tails)


def check_tables(label, wd, betas, uhat, kproj, finer):
    ref = W.wave_reference(wd, betas)
    for name, a in (("uhat", uhat), ("kproj", kproj), ("finer", finer)):
        assert np.all(np.isfinite(a.real)) and np.all(np.isfinite(a.imag)), f"{label}: {name} not finite"
    ru, rk, rf = W.table_ratios(ref, uhat, kproj, finer, wd.nn)
    print(f"{label}: worst ratio to the bound: uhat {ru:.3f}, kproj {rk:.3f}, finer {rf:.3f}")
    assert ru <= 1.0, (label, "uhat", ru)
    assert rk <= 1.0, (label, "kproj", rk)
    assert rf <= 1.0, (label, "finer", rf)


@pytest.mark.parametrize("shape", W.SHAPES, ids=str)
def test_wave_tables_against_long_double(shape):
    nn, nw, nh = shape
    wd = W.WaveDesign(nn, nw)
    betas = W.HEADINGS[:nh]
    uhat, kproj, finer, tails = tabulate(wd, betas)
    for name, t in tails.items():                           # pad lanes (nw % 64 != 0) store nothing
        assert np.all(t == SENT), f"{shape}: the tail of {name} was written"
    deep = wd.k * wd.depth > 710
    if nw >= 9:
        assert deep.any()
    check_tables(f"rh_wave_tables {shape} ({'k_wave_tables' if nn <= 8 else 'k_wave_tables_nodes + k_wave_force_sum'})",
                 wd, betas, uhat, kproj, finer)


def batch_designs():
    """The (8, 65) and (21, 65) designs with 3 and 2 headings: hstride = 3 exceeds the second's nhead."""
    wds = [W.WaveDesign(8, 65), W.WaveDesign(21, 65)]
    design_idx = np.array([0, 0, 0, 1, 1], dtype=np.int32)
    betas = np.array([W.HEADINGS[0], W.HEADINGS[1], W.HEADINGS[2], W.HEADINGS[0], W.HEADINGS[1]])
    return wds, design_idx, betas


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def test_wave_tables_batch_bit_equal_to_per_design():
    """rh_wave_tables_batch through prep.tabulate_batch, then the same launch with the descriptors' uhat
    NULL (as raft/sweep_block.py writes them): kproj and finer the same bits, uhat untouched."""
    import torch
    from raft import _native as N
    from raft import prep as P
    wds, design_idx, betas = batch_designs()
    dds = [P.DeviceDesign(wd, device=0) for wd in wds]
    head = P.tabulate_batch(dds, design_idx, betas)
    torch.cuda.synchronize()
    assert [len(dd.headings) for dd in dds] == [3, 2]
    got = []
    for wd, dd, sel in zip(wds, dds, (design_idx == 0, design_idx == 1)):
        assert np.array_equal(np.asarray(dd.headings)[head[sel]], betas[sel])
        u, k, f = dd.uhat.cpu().numpy(), dd.kproj.cpu().numpy(), dd.finer.cpu().numpy()
        u1, k1, f1, _ = tabulate(wd, dd.headings)
        for name, a, b in (("uhat", u, u1), ("kproj", k, k1), ("finer", f, f1)):
            assert np.array_equal(bits(a), bits(b)), f"batch vs per-design ({wd.nn}, {wd.nw}): {name}"
        check_tables(f"rh_wave_tables_batch ({wd.nn}, {wd.nw}, {len(dd.headings)})", wd, dd.headings, u, k, f)
        got.append((k, f))
    # once more without a velocity table
    U, K, Fi = (dds[0]._tab[name][0] for name in ("uhat", "kproj", "finer"))
    for t in (U, K, Fi):
        t.fill_(SENT)
    arr = P.descriptor_block(dds, strip_finer=True)
    arr._rec["uhat"][:] = 0
    assert arr[0].uhat is None and arr[1].uhat is None and arr[1].kproj
    bm = np.zeros([2, 3])
    for j, dd in enumerate(dds):
        bm[j, :len(dd.headings)] = dd.headings
    beta_t = torch.tensor(bm, dtype=torch.float64, device=dev())
    N.check(N.lib().rh_wave_tables_batch(N.context(0), arr, 2, N.ptr(beta_t), 3, N.stream_handle(torch, dev())),
            "rh_wave_tables_batch")
    torch.cuda.synchronize()
    assert bool((U == SENT).all()), "uhat NULL: the velocity table was written"
    for dd, (k, f) in zip(dds, got):
        assert np.array_equal(bits(dd._tab_view("kproj").cpu().numpy()), bits(k)), "uhat NULL: kproj differs"
        assert np.array_equal(bits(dd._tab_view("finer").cpu().numpy()), bits(f)), "uhat NULL: finer differs"
