"""Designs, poses, current cases, references and criteria of the pose-design and current-load checks
(raft-teststuff_amd/csrc/rh_pose.h): shared by tests/test_pose_host.py (the host build of the header
against the Python) and tests/test_gpu_pose.py (the device against the host build).

Bounds (fixed here, from the number format, not from what the code gives):
  * counts, mstart and every pose-independent column: equal exactly (they are copied);
  * unit-vector entries (q, p1, p2 and their squared norms): 16 eps;
  * positions and member moment arms: 64 eps x the largest position magnitude of the pose.
    These outputs are three-term products of rotation entries that differ from numpy's by an ulp or two
    of sin / cos; the bounds are about 30 x that and ten orders below any logic error;
  * current loads: 64 eps x the sum of the magnitudes of the terms of each component, from the long
    double restatement below (the moments of symmetric columns cancel, so the scale is the sum of
    magnitudes, not the result).
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT, load_design

EPS = np.finfo(float).eps
DESIGNS = ["VolturnUS-S_test", "OC3spar_test", "VolturnUS-S_rectcols"]
NNODE = {"VolturnUS-S_test": 143, "OC3spar_test": 51, "VolturnUS-S_rectcols": 149}
_p, _d, _i = ctypes.c_void_p, ctypes.c_double, ctypes.c_int


def poses():
    """68 poses: 65 seeded ones (the generator of tests/test_gpu_moor.py), a 12 m heave that wets more
    nodes, a lifted and tilted pose and the zero pose."""
    from test_gpu_moor import poses as seeded
    return np.concatenate([seeded(65, seed=11), [[0, 0, -12, 0, 0, 0], [3, -2, 7.3, 0.05, -0.08, 0.3], np.zeros(6)]])


def current_cases():
    """12 seeded (speed, heading) pairs and a zero-speed case."""
    rng = np.random.default_rng(12)
    cases = [dict(current_speed=float(u), current_heading=float(h))
             for u, h in zip(rng.uniform(0, 1.5, 12), rng.uniform(0, 360, 12))]
    return cases + [dict(current_speed=0.0, current_heading=40.0)]


_FOWTS = {}


def fowt_at_reference(name):
    """The design's FOWT (min_freq 0.01, max_freq 0.4) at its reference pose with the hydro constants of
    that pose (one per design and process; a test that moves it moves it back)."""
    if name not in _FOWTS:
        import raft
        d = load_design(name)
        d["settings"].update(min_freq=0.01, max_freq=0.4)
        f = raft.Model(d).fowtList[0]
        f.setPosition([f.x_ref, f.y_ref, 0, 0, 0, 0])
        f.calcStatics()
        f.calcHydroConstants()
        _FOWTS[name] = f
    return _FOWTS[name]


def host_lib():
    out = os.path.join(tempfile.mkdtemp(), "pose_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tools", "pose_host.cpp")], check=True)
    L = ctypes.CDLL(out)
    L.rh_pose_designs_host.argtypes = [_i, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p]
    L.rh_pose_designs_host.restype = None
    L.rh_current_loads_host.argtypes = [_i, _i, _p, _p, _p, _p, _i, _p, _p, _d, _d, _d, _d, _p]
    L.rh_current_loads_host.restype = None
    return L


def split_slabs(node, memb, mstart, nn, nm, nnode, nmemb):
    """Per-pose (node [NF, nn_i], memb [MF, nm_i], mstart [nm_i + 1]) from the slabs of rh_pose_designs."""
    from raft import _native as N
    out = []
    for i in range(len(nn)):
        out.append((node[i, :N.NF_COUNT * nn[i]].reshape(N.NF_COUNT, nn[i]).copy(),
                    memb[i, :N.MF_COUNT * nm[i]].reshape(N.MF_COUNT, nm[i]).copy(), mstart[i, :nm[i] + 1].copy()))
    return out


def host_designs(L, host, X):
    """The host build's tables of poses X [n, 6] for host = pose_device.host_record(fowt)."""
    from raft import _native as N
    memb, node, mstart = (np.ascontiguousarray(a) for a in host)
    nmemb, nnode, n = memb.shape[1], node.shape[1], len(X)
    X = np.ascontiguousarray(X, dtype=float)
    no, mo = np.full([n, N.NF_COUNT * nnode], np.nan), np.full([n, N.MF_COUNT * nmemb], np.nan)
    ms, nn, nm = np.zeros([n, nmemb + 1], dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    L.rh_pose_designs_host(nmemb, nnode, memb.ctypes.data, node.ctypes.data, mstart.ctypes.data, n, X.ctypes.data,
                           no.ctypes.data, mo.ctypes.data, ms.ctypes.data, nn.ctypes.data, nm.ctypes.data)
    return split_slabs(no, mo, ms, nn, nm, nnode, nmemb)


def python_designs(fowt, X):
    """prep.node_table after fowt.setPosition(X_i), per pose; the FOWT is moved back."""
    from raft.prep import node_table
    r0 = fowt.r6.copy()
    out = []
    for x in X:
        fowt.setPosition(x)
        table, _, members, mstart = node_table(fowt)
        out.append((table, members, mstart))
    fowt.setPosition(r0)
    return out


def compare_designs(got, ref, what):
    """The criteria of the module docstring on per-pose tables `got` against `ref`.  Returns the largest
    residuals in units of their bounds."""
    from raft import _native as N
    NF = N.NF
    worst = dict(unit=0.0, pos=0.0)
    for ip, ((gt, gm, gs), (rt, rm, rs)) in enumerate(zip(got, ref)):
        tag = f"{what}, pose {ip}"
        assert gt.shape == rt.shape and gm.shape == rm.shape, tag      # nn, nm
        np.testing.assert_array_equal(gs, rs, err_msg=tag)              # mstart
        # every pose-independent column but MCF, which the pose record holds at 0 (VolturnUS-S_rectcols has
        # two MacCamy-Fuchs members: node_table flags them, their Imat rows are zeros on both sides)
        keep = np.r_[NF["AQ"]:NF["MCF"], NF["I00"]:N.NF_COUNT]
        np.testing.assert_array_equal(gt[keep], rt[keep], err_msg=tag)
        assert not gt[NF["MCF"]].any()
        scale = np.abs(rt[NF["RX"]:NF["XZ"] + 1]).max()
        unit_m = np.r_[0:3, 6:9, 12:15, 18:21]
        arm_m = np.r_[3:6, 9:12, 15:18]
        e_unit = max(np.abs(gt[NF["QX"]:NF["P2Z"] + 1] - rt[NF["QX"]:NF["P2Z"] + 1]).max(),
                     np.abs(gm[unit_m] - rm[unit_m]).max()) / (16 * EPS)
        e_pos = max(np.abs(gt[:NF["XZ"] + 1] - rt[:NF["XZ"] + 1]).max(), np.abs(gm[arm_m] - rm[arm_m]).max()) \
            / (64 * EPS * scale)
        assert e_unit <= 1.0, (tag, e_unit)
        assert e_pos <= 1.0, (tag, e_pos)
        worst["unit"], worst["pos"] = max(worst["unit"], e_unit), max(worst["pos"], e_pos)
    return worst


def host_current_loads(L, host, fowt, cases):
    memb, node, mstart = (np.ascontiguousarray(a) for a in host)
    U = np.array([c["current_speed"] for c in cases], dtype=float)
    H = np.array([c["current_heading"] for c in cases], dtype=float)
    X_ref = np.ascontiguousarray(fowt.r6, dtype=float)
    D = np.full([len(cases), 6], np.nan)
    L.rh_current_loads_host(memb.shape[1], node.shape[1], memb.ctypes.data, node.ctypes.data, mstart.ctypes.data,
                            X_ref.ctypes.data, len(cases), U.ctypes.data, H.ctypes.data, float(fowt.depth),
                            float(fowt._current_zref()), float(fowt.shearExp_water), float(fowt.rho_water), D.ctypes.data)
    return D


def current_longdouble(fowt, case):
    """FOWT.calcCurrentLoads restated in long double from the FOWT's (double) geometry at its current
    pose: (D [6], S [6]) with S the sum of the magnitudes of every term added into each component."""
    ld = np.longdouble
    rho, depth, expo = ld(fowt.rho_water), ld(fowt.depth), ld(fowt.shearExp_water)
    Zref = ld(fowt._current_zref())
    U = ld(case["current_speed"])
    pi = ld(4) * np.arctan(ld(1))
    hr = ld(case["current_heading"]) * pi / ld(180)
    ch, sh = np.cos(hr), np.sin(hr)
    D, S = np.zeros(6, dtype=ld), np.zeros(6, dtype=ld)
    r0 = fowt.r6[:3].astype(ld)
    for mem in fowt.memberList:
        circ = mem.shape == "circular"
        q, p1, p2 = mem.q.astype(ld), mem.p1.astype(ld), mem.p2.astype(ld)
        for il in range(mem.ns):
            if not (mem.r[il, 2] < 0):
                continue
            r = mem.r[il].astype(ld)
            v = U * ((depth - abs(r[2])) / (depth + Zref)) ** expo
            vrel = np.array([v * ch, v * sh, ld(0)], dtype=ld)
            vq = np.sum(vrel * q) * q
            vp = vrel - vq
            vp1 = np.sum(vrel * p1) * p1
            vp2 = np.sum(vrel * p2) * p2
            norm = lambda a: np.sqrt(np.sum(a * a))   # noqa: E731
            ds, drs, dls = np.atleast_1d(mem.ds[il]).astype(ld), np.atleast_1d(mem.drs[il]).astype(ld), ld(mem.dls[il])
            if circ:
                aq, ap1, ap2 = pi * ds[0] * dls, ds[0] * dls, ds[0] * dls
                aend = abs(pi * ds[0] * drs[0])
                n1 = n2 = norm(vp)
            else:
                aq = 2 * (ds[0] + ds[0]) * dls
                ap1, ap2 = ds[0] * dls, ds[1] * dls
                aend = abs((ds[0] + drs[0]) * (ds[1] + drs[1]) - (ds[0] - drs[0]) * (ds[1] - drs[1]))
                n1, n2 = norm(vp1), norm(vp2)
            nq = norm(vq)
            half = ld(0.5)
            terms = [half * rho * aq * ld(mem.coef("Cd_q", il)) * nq * vq,
                     half * rho * ap1 * ld(mem.coef("Cd_p1", il)) * n1 * vp1,
                     half * rho * ap2 * ld(mem.coef("Cd_p2", il)) * n2 * vp2,
                     half * rho * aend * ld(mem.coef("Cd_End", il)) * nq * vq]
            f = sum(terms)
            fa = sum(np.abs(t) for t in terms)
            x = r - r0
            D[:3] += f
            S[:3] += fa
            D[3:] += np.cross(x, f)
            xa = np.abs(x)
            S[3:] += [xa[1] * fa[2] + xa[2] * fa[1], xa[2] * fa[0] + xa[0] * fa[2], xa[0] * fa[1] + xa[1] * fa[0]]
    return D, S


def check_current(D, ref, what):
    """|D - D_ld| <= 64 eps S per component and case.  Returns the largest residual in units of the bound."""
    worst = 0.0
    for ic, (d, (dl, s)) in enumerate(zip(D, ref)):
        err = np.abs(d.astype(np.longdouble) - dl)
        bound = 64 * EPS * s
        assert np.all(err <= bound), (what, ic, err, bound)
        worst = max(worst, float(np.max(err[s > 0] / bound[s > 0])) if np.any(s > 0) else 0.0)
    return worst
