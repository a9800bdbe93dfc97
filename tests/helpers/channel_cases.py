"""Shared by tests/test_channels_host.py and tests/test_gpu_channels.py: the host build of
csrc/rh_channels.h (tools/channels_host.cpp), the tables of one rh_turbine_channels call as host
arrays, the Python reference values of the turbine channels (FOWT.rotor_channels and
FOWT._aero_outputs after calcTurbineConstants(case, bem=pair)), and the error measures."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import aero_cases as AC

ROOT = AC.ROOT
TURBULENCES = [0.1, "IB_NTM"]
PITCH0 = 0.043                              # a mean platform pitch [rad]
CHANNELS = ["AxRNA", "Mbase", "omega", "torque", "bPitch"]
MEANS = CHANNELS + ["power"]

_p, _i, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


def host_lib():
    """tools/channels_host.cpp compiled with g++ (no fused multiply-add, as the device build)."""
    out = os.path.join(tempfile.mkdtemp(), "channels_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tools", "channels_host.cpp")], check=True)
    L = ctypes.CDLL(out)
    L.rh_chan_control_tf_host.argtypes = [_p, _p, _d, _i, _p, _p, _p]
    L.rh_chan_control_tf_host.restype = None
    L.rh_turbine_channels_host.argtypes = [_i, _i, _i, _d, _p, _p, _p, _i, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i,
                                           _p, _p, _p, _p]
    L.rh_turbine_channels_host.restype = _i
    return L


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Tables:
    """The arguments of one rh_turbine_channels call as host arrays.  Xi [ncase, nrow, 6, nw] complex;
    pairs: None, or the dict of pair_case, pair_rotor, modes, pair_vw, loads, dloads, param, op,
    pair_row and V_w."""

    def __init__(self, w, dw, Xi, geom, pitch0=None, pairs=None):
        self.w, self.dw = _f64(w), float(dw)
        self.Xi = np.ascontiguousarray(Xi, dtype=np.complex128)
        self.geom = _f64(geom)
        self.pitch0 = None if pitch0 is None else _f64(pitch0)
        self.pairs = pairs
        self.ncase, self.nrow, _, self.nw = self.Xi.shape
        self.nrot = self.geom.shape[0]


def host_channels(L, t, psd=True, expect=0):
    """rh_turbine_channels_host on Tables t: psd [ncase, nrot, 5, nw] (None without), std
    [ncase, nrot, 5], avg [ncase, nrot, 6] of the host-compiled header; expect: its return code."""
    P = np.zeros([t.ncase, t.nrot, 5, t.nw]) if psd else None
    S, A = np.zeros([t.ncase, t.nrot, 5]), np.zeros([t.ncase, t.nrot, 6])
    ptr = lambda a: None if a is None else a.ctypes.data                           # noqa: E731
    if t.pairs is None:
        npair, nvw, cols, tabs, V = 0, 0, [None] * 4, [None] * 5, None
    else:
        q = t.pairs
        cols = [_i32(q[k]) for k in ("pair_case", "pair_rotor", "modes", "pair_vw")]
        tabs = [_f64(q[k]) for k in ("loads", "dloads", "param", "op", "pair_row")]
        V = _f64(q["V_w"])
        npair, nvw = len(cols[0]), V.shape[0]
    rc = L.rh_turbine_channels_host(t.ncase, t.nrow, t.nw, t.dw, ptr(t.w), ptr(t.Xi), ptr(t.pitch0), t.nrot, ptr(t.geom),
                                    npair, ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), *(ptr(a) for a in tabs),
                                    ptr(cols[3]), nvw, ptr(V), ptr(P), ptr(S), ptr(A))
    assert rc == expect, rc
    return P, S, A


def seeded_xi(seed, ncase, nrow, nw, wind_row=True):
    """Motions of physical size: metres in the translations, hundredths of a radian in the rotations;
    with wind_row one further row of zeros, the reference's wind row.  A case's rows depend on the seed
    and its own index alone, not on ncase."""
    X = np.zeros([ncase, nrow, 6, nw], dtype=complex)
    for c in range(ncase):
        rng = np.random.default_rng([seed, c])
        X[c] = rng.normal(size=[nrow, 6, nw]) + 1j * rng.normal(size=[nrow, 6, nw])
    X[:, :, 3:] *= 0.01
    if wind_row:
        X = np.concatenate([X, np.zeros([ncase, 1, 6, nw])], axis=1)
    return X


def pair_tables(fowt, case, pin, ir=0):
    """The pair tables of one (case, rotor) of a posed FOWT: pin from aero_cases.pair_inputs."""
    from raft.rotor_device import chan_pair_row
    rot = fowt.rnaList[ir]
    speed = float(case["wind_speed"])
    op = np.array([*rot.operating_point(speed), *rot.inflow_angles(case)])
    V_w = np.sqrt(rot.IECKaimal(case)[3])
    return dict(pair_case=[0], pair_rotor=[ir], modes=[pin["mode"]], pair_vw=[0], loads=pin["loads"][None],
                dloads=pin["dloads"][None], param=pin["param"][None], op=op[None], pair_row=chan_pair_row(rot)[None],
                V_w=V_w[None])


def empty_results(nr, nw):
    """The arrays saveTurbineOutputs hands _aero_outputs, as it allocates them."""
    res = {f"{k}_{s}": np.zeros(nr) for k in ("AxRNA", "Mbase", "omega") for s in ("avg", "std", "max", "min")}
    res.update({f"{k}_{s}": np.zeros(nr) for k in ("torque", "bPitch") for s in ("avg", "std")})
    res.update({f"{k}_PSD": np.zeros([nw, nr]) for k in CHANNELS})
    res["power_avg"] = np.zeros(nr)
    return res


def numpy_motion_channels(fowt, Xi, pitch0):
    """AxRNA and the aero-free Mbase of every rotor from rotor_channels' coefficient rows in numpy, as
    rh_channel_stats applies them: (psd [2 nrot, nw], std [2 nrot], means [2 nrot])."""
    fowt.Xi0 = np.array([0.0, 0.0, 0.0, 0.0, pitch0, 0.0])
    coef, means = fowt.rotor_channels()
    w2 = np.asarray(fowt.w) ** 2
    x = np.einsum("kd,rdb->krb", coef[:, 0], Xi) + w2 * np.einsum("kd,rdb->krb", coef[:, 1], Xi)
    return np.sum(0.5 * np.abs(x) ** 2 / fowt.dw, axis=1), np.sqrt(0.5 * np.sum(np.abs(x) ** 2, axis=(1, 2))), means


def python_channels(fowt, case, bem, Xi, pitch0):
    """The Python's channels of one case: calcTurbineConstants(case, bem=bem), then rotor_channels in
    numpy for AxRNA and the aero-free Mbase and _aero_outputs on Xi [nrow + 1, 6, nw] (last row zero).
    Returns the results dict of saveTurbineOutputs' rotor channels."""
    fowt.calcTurbineConstants(dict(case), ptfm_pitch=0, bem=bem)
    nr, nw = fowt.nrotors, fowt.nw
    psd, std, means = numpy_motion_channels(fowt, Xi, pitch0)
    res = empty_results(nr, nw)
    for j, name in enumerate(["AxRNA", "Mbase"]):
        sl = slice(j * nr, (j + 1) * nr)
        res[f"{name}_std"], res[f"{name}_PSD"], res[f"{name}_avg"] = std[sl].copy(), psd[sl].T.copy(), means[sl].copy()
        res[f"{name}_max"], res[f"{name}_min"] = means[sl] + 3 * std[sl], means[sl] - 3 * std[sl]
    fowt.Xi = Xi
    fowt._aero_outputs(res, dict(case))
    return res


def mbase_cancellation(fowt, Xi, ir=0):
    """From the Python alone: over rows and bins, the largest sum of the magnitudes of the terms of Mbase
    (the two of M_I, M_w, M_X) divided by the magnitude of their sum, with the FOWT's current A_aero and
    B_aero (after calcTurbineConstants)."""
    from raft.rotor_device import chan_geom_table
    from raft import _native as N
    g = chan_geom_table(fowt)[ir]
    mt, zCG, hArm, ICG, zBase, zrel = (g[N.CG[k]] for k in ("MT", "ZCG", "HARM", "ICG", "ZBASE", "ZREL"))
    w = np.asarray(fowt.w)
    Xs, Xp = Xi[:-1, 0, :], Xi[:-1, 4, :]
    terms = [-mt * (-w ** 2 * (Xs + zCG * Xp)) * hArm, -ICG * (-w ** 2 * Xp), mt * fowt.g * hArm * Xp,
             -(-w ** 2 * fowt.A_aero[0, 0, :, ir] + 1j * w * fowt.B_aero[0, 0, :, ir]) * (zrel - zBase) ** 2 * Xp]
    return float(np.max(sum(np.abs(t) for t in terms) / np.abs(sum(terms))))


def rel(got, ref):
    """Normwise difference relative to the reference's largest entry (zero reference: exact zeros)."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    scale = np.abs(ref).max() if ref.size else 0.0
    if scale == 0.0:
        assert not np.any(got)
        return 0.0
    return float(np.linalg.norm((got - ref).ravel()) / scale)


def channel_errors(P, S, A, res, ir=0):
    """The differences of one case's rotor ir between the header's (psd [nrot, 5, nw], std [nrot, 5],
    avg [nrot, 6]) and the Python's results dict: name -> relative difference."""
    out = {}
    for k, name in enumerate(CHANNELS):
        out[f"{name}_PSD"] = rel(P[ir, k], res[f"{name}_PSD"][:, ir])
        out[f"{name}_std"] = rel(S[ir, k], res[f"{name}_std"][ir])
    for k, name in enumerate(MEANS):
        out[f"{name}_avg"] = rel(A[ir, k], res[f"{name}_avg"][ir])
    return out


def synthetic_tables(ncase_layout, nw, nrow, seed=3, w=None):
    """Two synthetic rotors (different z_rel, geometry, mode and V_w row; the pairs of
    aero_cases.synthetic_pairs) laid over cases: ncase_layout a list with, per case, the rotors that
    have a pair there ([] none, [0], [1] or [0, 1]).  Xi has nrow rows (no added zero row)."""
    from raft import _native as N
    loads, dloads, param, modes = AC.synthetic_pairs()
    w = np.linspace(0.05, 2.0, nw) if w is None else np.asarray(w, dtype=float)
    geom = np.zeros([2, N.CG_COUNT])
    geom[0] = [150.0, 2.2e6, 62.0, 47.0, 3.1e9, 9.81, 15.0, 1.0]
    geom[1] = [138.0, 1.7e6, 55.0, 43.0, 2.4e9, 9.81, 12.0, 1.0]
    prow = np.zeros([2, N.CP_COUNT])
    prow[0] = [150.0, -3.8e7, -4.6e6, 0.0]
    prow[1] = [140.0, -2.9e7, -3.1e6, 0.0]
    V = np.stack([2.0 / (1.0 + np.arange(nw)), 0.5 + 0.01 * np.arange(nw), 1.0 + 0.0 * w])
    op = np.array([[10.0, 7.1, 2.0, 0.1, 0.02], [12.0, 7.5, 5.0, 0.1, -0.03]])
    pc = [c for c, rs in enumerate(ncase_layout) for _ in rs]
    pr = [r for rs in ncase_layout for r in rs]
    pairs = None
    if pc:
        pairs = dict(pair_case=pc, pair_rotor=pr, modes=[modes[r] for r in pr], pair_vw=[(c + r) % 3 for c, r in zip(pc, pr)],
                     loads=loads[pr] * (1.0 + 0.01 * np.array(pc))[:, None], dloads=dloads[pr], param=param[pr], op=op[pr],
                     pair_row=prow[pr], V_w=V)
    ncase = len(ncase_layout)
    return Tables(w, 0.05, seeded_xi(seed, ncase, nrow, nw, wind_row=False), geom, 0.01 * (1 + np.arange(ncase)), pairs)
