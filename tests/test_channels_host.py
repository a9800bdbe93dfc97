"""CPU check of the device turbine channels (raft-teststuff_amd/csrc/rh_channels.h) against the Python
they restate (FOWT.rotor_channels, FOWT._aero_outputs, the control transfer function of
Rotor.calcAero): the header is compiled for the host with g++ (tools/channels_host.cpp), so the same
channel arithmetic the GPU runs is compared here without a GPU.  Also the ABI entry's validation and
the Python surface's refusals."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_design

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import aero_cases as AC  # noqa: E402
import channel_cases as CC  # noqa: E402

# The worst difference between the host-compiled header and the Python over the 80 cases of
# test_channels_against_python (aeroServoMod 1 and 2, five speeds, two headings, turbulence 0.1 and
# "IB_NTM", one and three response rows; the design's 40 bins), measured on the CPU: every PSD normwise
# over the bins relative to the channel's largest PSD entry, every standard deviation and mean
# relative to its magnitude, C(w) relative to |C| per bin:
#   PSD 7.45e-16 (Mbase; omega 5.82e-16, torque 5.24e-16, bPitch 3.76e-16, AxRNA 5.11e-16),
#   std 6.59e-16 (bPitch), means 1.44e-16 (Mbase), C(w) bit-equal.
# A few roundings per term: the header squares re and im where numpy squares hypot(re, im), and sums the
# bins in order where numpy sums pairwise.
# The tests assert at ten times the worst of them, and never above 1e-10.  The largest ratio of the sum
# of the magnitudes of Mbase's terms to the magnitude of their sum over the tested rows and bins: 13.
CHANNEL_MEASURED = 7.45e-16
CHANNEL_BAR = min(10 * CHANNEL_MEASURED, 1e-10)
CANCELLATION_MAX = 1e3


@pytest.fixture(scope="module")
def lib():
    return CC.host_lib()


@pytest.fixture(scope="module")
def cases():
    """mod -> (fowt, [(case, pair inputs)]) for the five speeds and two headings; the blade-element
    solves are computed once."""
    out = {}
    for mod in (1, 2):
        fowt = AC.posed_model(mod).fowtList[0]
        fowt.calcStatics()                      # the tower masses and inertias the Mbase channel reads
        rows = []
        for h in AC.HEADINGS:
            for U in AC.SPEEDS:
                case = AC.wind_case(U, h)
                rows.append((case, AC.pair_inputs(fowt, case)))
        out[mod] = (fowt, rows)
    return out


def _variants(rows):
    """Every (case, pair) with both turbulences and one and three response rows."""
    n = 0
    for case, pin in rows:
        for turb in CC.TURBULENCES:
            for nrow in (1, 3):
                n += 1
                yield dict(case, turbulence=turb), pin, nrow, n


# ------------------------------------------------------------------------------ against the Python
def test_kaimal_amplitude_is_finite(cases):
    """A condition on the inputs: IECKaimal is finite and positive at every bin for both turbulences at
    all five speeds, so that no comparison below is between NaNs."""
    fowt, rows = cases[2]
    worst = 0.0
    for case, pin, nrow, n in _variants(rows):
        V = np.sqrt(fowt.rnaList[0].IECKaimal(case)[3])
        assert V.shape == (fowt.nw,) and np.all(np.isfinite(V)) and np.all(V > 0)
        worst = max(worst, V.max())
    print(f"largest V_w {worst:.3g}")


def test_control_transfer_function_matches_python(lib, cases):
    """C(w) of the header against rot.C, relative to |C| per bin."""
    from raft.rotor_device import chan_pair_row
    fowt, rows = cases[2]
    rot, w = fowt.rnaList[0], np.ascontiguousarray(fowt.w, dtype=float)
    worst = 0.0
    for case, pin in rows:
        fowt.calcTurbineConstants(dict(case), ptfm_pitch=0, bem=[pin["bem"]])
        par, D = np.ascontiguousarray(pin["param"]), np.ascontiguousarray(pin["dloads"])
        re, im = np.zeros(len(w)), np.zeros(len(w))
        lib.rh_chan_control_tf_host(par.ctypes.data, D.ctypes.data, chan_pair_row(rot)[0], len(w), w.ctypes.data,
                                    re.ctypes.data, im.ctypes.data)
        assert np.all(np.abs(rot.C) > 0)
        err = float(np.max(np.abs((re + 1j * im) - rot.C) / np.abs(rot.C)))
        worst = max(worst, err)
        assert err <= CHANNEL_BAR, (case["wind_speed"], case["wind_heading"], err)
    print(f"C(w): worst difference {worst:.3e}")


def test_torque_gains_are_the_rotor_s_own(cases):
    """The torque channel reads rot.kp_tau and rot.ki_tau as _aero_outputs does: above rated the
    parameter row's gated gains are zero and the channel row's are not."""
    from raft import _native as N
    from raft.rotor_device import chan_pair_row
    fowt, rows = cases[2]
    rot = fowt.rnaList[0]
    row = chan_pair_row(rot)
    assert row[N.CP["KP_TAU"]] == rot.kp_tau != 0 and row[N.CP["KI_TAU"]] == rot.ki_tau != 0
    assert row[N.CP["ZHUB"]] == rot.r3[2]
    assert any(pin["param"][N.AP["KP_TAU"]] == 0 for _, pin in rows)


@pytest.mark.parametrize("mod", [1, 2])
def test_channels_against_python(lib, cases, mod):
    """PSD, standard deviation and mean of every channel of the host-compiled header against
    rotor_channels and _aero_outputs, per case; the cancellation in Mbase as a condition on the inputs."""
    from raft.rotor_device import chan_geom_table
    fowt, rows = cases[mod]
    worst, cancel, pitching = {}, 0.0, mod == 1
    for case, pin, nrow, n in _variants(rows):
        Xi = CC.seeded_xi(n, 1, nrow, fowt.nw)
        res = CC.python_channels(fowt, case, [pin["bem"]], Xi[0], CC.PITCH0)
        q = CC.pair_tables(fowt, case, pin)
        assert np.array_equal(q["V_w"][0], fowt.rnaList[0].V_w.real) and np.all(np.isfinite(q["V_w"]))
        c = CC.mbase_cancellation(fowt, Xi[0])
        cancel = max(cancel, c)
        assert c < CANCELLATION_MAX, (case, c)
        t = CC.Tables(fowt.w, fowt.dw, Xi, chan_geom_table(fowt), [CC.PITCH0], q)
        P, S, A = CC.host_channels(lib, t)
        errs = CC.channel_errors(P[0], S[0], A[0], res)
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(errs.values()) <= CHANNEL_BAR, (case, nrow, {k: v for k, v in errs.items() if v > CHANNEL_BAR})
        assert np.all(res["Mbase_std"] > 0) and np.all(res["AxRNA_std"] > 0) and res["Mbase_avg"][0] != 0
        if mod == 2:
            assert all(res[f"{k}_std"][0] > 0 and res[f"{k}_avg"][0] != 0 for k in ("omega", "torque"))
            assert res["power_avg"][0] > 0
            pitching = pitching or res["bPitch_std"][0] > 0          # (below rated the pitch gains are zero)
            assert np.array_equal(res["wind_PSD"], 0.5 * q["V_w"][0] ** 2 / fowt.dw)
        else:       # mode 1: the control channels and their means are the reference's exact zeros
            assert not np.any(P[0, 0, 2:]) and not np.any(S[0, 0, 2:]) and not np.any(A[0, 0, 2:])
            assert not any(np.any(res[f"{k}_{s}"]) for k in ("omega", "torque", "bPitch") for s in ("avg", "std", "PSD"))
    assert pitching
    print(f"aeroServoMod {mod}: Mbase cancellation {cancel:.3g}; worst differences " +
          ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))


def test_mode_1_reaction_term_is_the_thrust_derivative(lib, cases):
    """Mode 1: M_X uses b = dT/dU and a = 0: Mbase equals numpy's M_I + M_w + M_X with those."""
    from raft import _native as N
    from raft.rotor_device import chan_geom_table
    fowt, rows = cases[1]
    case, pin = rows[3]
    Xi = CC.seeded_xi(77, 1, 3, fowt.nw)
    t = CC.Tables(fowt.w, fowt.dw, Xi, chan_geom_table(fowt), [CC.PITCH0], CC.pair_tables(fowt, case, pin))
    P, S, A = CC.host_channels(lib, t)
    g = t.geom[0]
    mt, zCG, hArm, ICG, zBase, zrel = (g[N.CG[k]] for k in ("MT", "ZCG", "HARM", "ICG", "ZBASE", "ZREL"))
    w, Xs, Xp = t.w, Xi[0, :, 0, :], Xi[0, :, 4, :]
    B00 = pin["dloads"][0] * pin["param"][N.AP["RQ"]] ** 2
    dyn = -mt * (-w ** 2 * (Xs + zCG * Xp)) * hArm - ICG * (-w ** 2 * Xp) + mt * fowt.g * hArm * Xp \
        - (1j * w * B00) * (zrel - zBase) ** 2 * Xp
    assert CC.rel(P[0, 0, 1], np.sum(0.5 * np.abs(dyn) ** 2 / fowt.dw, axis=0)) <= CHANNEL_BAR
    assert B00 > 0


# ------------------------------------------------------------------------------ layouts at the ABI level
def test_two_rotors_on_one_case(lib):
    """Two synthetic rotors on one case equal the two single-rotor results bit for bit; so do the same
    rotors alone on the neighbouring cases."""
    for nw, nrow in ((1, 1), (37, 3)):
        both = CC.synthetic_tables([[0], [], [0, 1], [1]], nw, nrow)
        P, S, A = CC.host_channels(lib, both)
        assert np.all(np.isfinite(P)) and np.all(S[:, :, :2] > 0)
        for ir in (0, 1):
            layout = [[0] if ir in rs else [] for rs in ([0], [], [0, 1], [1])]
            one = CC.synthetic_tables(layout, nw, nrow)
            q, full = one.pairs, both.pairs
            keep = [i for i, r in enumerate(full["pair_rotor"]) if r == ir]
            for k in ("loads", "dloads", "param", "op", "pair_row"):       # the pair's own rows of the two-rotor table
                q[k] = np.asarray(full[k])[keep]
            q["pair_vw"], q["modes"] = [full["pair_vw"][i] for i in keep], [full["modes"][i] for i in keep]
            one.geom = np.ascontiguousarray(both.geom[ir:ir + 1])
            one.nrot = 1
            P1, S1, A1 = CC.host_channels(lib, one)
            assert np.array_equal(P1[:, 0], P[:, ir]) and np.array_equal(S1[:, 0], S[:, ir])
            assert np.array_equal(A1[:, 0], A[:, ir])
        assert np.all(S[2, 0, 2:] > 0) and not np.any(S[2, 1, 2:])      # rotor 0 is mode 2, rotor 1 mode 1
        assert not np.any(S[1, :, 2:]) and not np.any(P[1, :, 2:]) and not np.any(A[1, :, 2:])
        Pn, Sn, An = CC.host_channels(lib, both, psd=False)
        assert Pn is None and np.array_equal(Sn, S) and np.array_equal(An, A)


def test_a_case_without_a_pair_between_two_wind_cases(lib, cases):
    """[pair, none, pair] on the real design: the middle case has zero control channels, and its Mbase
    and AxRNA equal rotor_channels' numpy; the outer cases equal their single-case results bit for bit."""
    from raft.rotor_device import chan_geom_table
    fowt, rows = cases[2]
    (c0, p0), (c2, p2) = rows[1], rows[8]
    q0, q2 = CC.pair_tables(fowt, c0, p0), CC.pair_tables(fowt, c2, p2)
    pairs = {k: np.concatenate([np.asarray(q0[k]), np.asarray(q2[k])]) for k in q0}
    pairs["pair_case"], pairs["pair_vw"] = [0, 2], [0, 1]
    Xi = CC.seeded_xi(5, 3, 3, fowt.nw)
    geom = chan_geom_table(fowt)
    P, S, A = CC.host_channels(lib, CC.Tables(fowt.w, fowt.dw, Xi, geom, [CC.PITCH0] * 3, pairs))
    assert not np.any(P[1, 0, 2:]) and not np.any(S[1, 0, 2:]) and not np.any(A[1, 0, 2:])
    psd, std, means = CC.numpy_motion_channels(fowt, Xi[1], CC.PITCH0)
    nr = fowt.nrotors
    for j in (0, 1):
        assert CC.rel(P[1, 0, j], psd[j * nr]) <= CHANNEL_BAR and CC.rel(S[1, 0, j], std[j * nr]) <= CHANNEL_BAR
        assert CC.rel(A[1, 0, j], means[j * nr]) <= CHANNEL_BAR
    for c, q in ((0, q0), (2, q2)):
        P1, S1, A1 = CC.host_channels(lib, CC.Tables(fowt.w, fowt.dw, Xi[c:c + 1], geom, [CC.PITCH0], q))
        assert np.array_equal(P1[0], P[c]) and np.array_equal(S1[0], S[c]) and np.array_equal(A1[0], A[c])
    none = CC.host_channels(lib, CC.Tables(fowt.w, fowt.dw, Xi[1:2], geom, [CC.PITCH0], None))
    assert all(np.array_equal(a[0], b[1]) for a, b in zip(none, (P, S, A)))


def test_host_entry_refuses_bad_tables(lib):
    """The pair-column checks the ABI entry runs (rh::chan::check_pairs), one by one, through the host
    entry: the return code is -(1 + the reason)."""
    def with_(**kw):
        t = CC.synthetic_tables([[0], [], [0, 1], [1]], 5, 1)
        t.pairs.update(kw)
        return t
    CC.host_channels(lib, with_(pair_case=[0, 2, 4, 4]), expect=-2)          # a case row out of range
    CC.host_channels(lib, with_(pair_case=[0, 2, 1, 3]), expect=-3)          # decreasing
    CC.host_channels(lib, with_(modes=[2, 2, 3, 1]), expect=-5)              # a mode other than 1 or 2
    CC.host_channels(lib, with_(pair_rotor=[0, 0, 2, 1]), expect=-6)         # a rotor out of range
    CC.host_channels(lib, with_(pair_rotor=[0, 1, 1, 1]), expect=-7)         # a rotor twice on one case
    CC.host_channels(lib, with_(pair_vw=[0, 1, 3, 1]), expect=-8)            # a V_w row out of range
    nine = CC.synthetic_tables([[0] * 9], 5, 1)
    CC.host_channels(lib, nine, expect=-4)                                   # more than 8 pairs on a case
    t = with_()
    t.nrow = 0
    CC.host_channels(lib, t, expect=-1)


def test_stand_alone_program_runs():
    """tools/channels_host.cpp's own main (both modes, a case without a pair, two rotors on a case,
    nw 1 and 67, nrow 1 and 3, a batch without pairs, refused tables) under the address and
    undefined-behaviour sanitizers."""
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(), "channels_host")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-DCHANNELS_HOST_MAIN", "-o", exe, os.path.join(AC.ROOT, "tools", "channels_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from raft import _native as N
    return N, N.lib()


def _abi_args(ncase=3, nrow=1, nw=3, nrot=2, npair=2, pair_case=(0, 2), pair_rotor=(0, 1), modes=(1, 2), pair_vw=(0, 1),
              nvw=2, ctx=True):
    """Host buffers standing in for every pointer: the entry validates before it touches any of them
    (and before it reads the context), so no device is needed to see a refusal."""
    keep = dict(ctx=ctypes.create_string_buffer(4096), buf=np.zeros(4096),
                cols=[np.array(a, dtype=np.int32) for a in (pair_case, pair_rotor, modes, pair_vw)])
    b = keep["buf"].ctypes.data
    pc, pr, md, pv = (a.ctypes.data for a in keep["cols"])
    args = [ctypes.addressof(keep["ctx"]) if ctx else None, ncase, nrow, nw, 0.05, b, b, b, nrot, b, npair, b, pc, b, pr, md,
            b, b, b, b, b, b, pv, nvw, b, b, b, b, None]
    return args, keep


def test_symbol_version_and_layouts(native):
    N, L = native
    assert hasattr(L, "rh_turbine_channels") and L.rh_version() == 8
    src = open(os.path.join(AC.ROOT, "include", "rafthip.h")).read()
    assert f"RH_CP_COUNT = {N.CP_COUNT}" in src and f"RH_CG_COUNT = {N.CG_COUNT}" in src
    assert f"RH_TC_COUNT = {N.TC_COUNT}" in src and f"RH_TC_SPECTRA = {N.TC_SPECTRA}" in src
    assert f"#define RH_CHAN_MAX_ROTORS {N.CHAN_MAX_ROTORS}" in src
    for names, table, prefix in ((["AXRNA", "MBASE", "OMEGA", "TORQUE", "BPITCH"], N.TC, "RH_TC_"),
                                 (["ZHUB", "KP_TAU", "KI_TAU"], N.CP, "RH_CP_"),
                                 (["ZREL", "MT", "ZCG", "HARM", "ICG", "G", "ZBASE", "HAS_TOWER"], N.CG, "RH_CG_")):
        assert [table[k] for k in names] == list(range(len(names)))          # the enum counts from zero ...
        at = [src.index(prefix + k) for k in names]
        assert at == sorted(at)                                                # ... in this order
    assert N.TC["POWER"] == 5 and "RH_TC_POWER = 5" in src
    assert N.AP_COUNT == 24 and "RH_AP_COUNT = 24" in src                      # the parameter row stays as it is


def test_entry_refuses_bad_arguments(native):
    N, L = native
    call = lambda args: L.rh_turbine_channels(*args)                           # noqa: E731
    args, keep = _abi_args(ctx=False)
    assert call(args) == N.RH_EINVAL and b"null context" in L.rh_last_error()
    for k, what in ((1, "ncase"), (2, "nrow"), (3, "nw"), (8, "nrot")):
        args, keep = _abi_args()
        args[k] = 0
        assert call(args) == N.RH_EINVAL and what.encode() in L.rh_last_error()
    args, keep = _abi_args()
    args[10] = -1
    assert call(args) == N.RH_EINVAL and b"npair" in L.rh_last_error()
    args, keep = _abi_args(nvw=0)
    assert call(args) == N.RH_EINVAL and b"nvw" in L.rh_last_error()
    args, keep = _abi_args(nrot=17)
    assert call(args) == N.RH_EINVAL and b"at most 16" in L.rh_last_error()
    args, keep = _abi_args()
    args[4] = 0.0
    assert call(args) == N.RH_EINVAL and b"dw" in L.rh_last_error()
    for k in (5, 6, 9, 26, 27, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 24):     # required pointers, one by one
        args, keep = _abi_args()
        args[k] = None
        assert call(args) == N.RH_EINVAL and b"null" in L.rh_last_error(), k
    for kw, msg in ((dict(pair_case=(2, 0)), b"decreases"), (dict(pair_case=(0, 3)), b"outside [0, 3)"),
                    (dict(pair_case=(-1, 0)), b"outside [0, 3)"), (dict(modes=(1, 3)), b"aeroServoMod 3"),
                    (dict(pair_rotor=(0, 2)), b"rotor 2 outside [0, 2)"), (dict(pair_rotor=(-1, 1)), b"rotor -1 outside"),
                    (dict(pair_case=(1, 1), pair_rotor=(1, 1)), b"names rotor 1 twice"),
                    (dict(pair_vw=(0, 2)), b"V_w row 2 outside [0, 2)"), (dict(pair_vw=(-1, 0)), b"V_w row -1 outside"),
                    (dict(nrot=16, npair=9, pair_case=(0,) * 9, pair_rotor=tuple(range(9)), modes=(1,) * 9,
                          pair_vw=(0,) * 9), b"more than 8 pairs")):
        args, keep = _abi_args(**kw)
        assert call(args) == N.RH_EINVAL and msg in L.rh_last_error(), (kw, L.rh_last_error())


# ------------------------------------------------------------------------------ Python surface
WIND = AC.wind_case(10.0, 0.0)


def test_analyze_cases_batch_refusals():
    import raft
    m = raft.Model(load_design("VolturnUS-S_aero"))
    assert inspect.signature(m.analyzeCasesBatch).parameters["channels"].default is False
    with pytest.raises(NotImplementedError, match="channels=True with statics=True"):
        m.analyzeCasesBatch([dict(WIND)], channels=True, statics=True)
    with pytest.raises(NotImplementedError, match="channels=True with statics=True"):
        m.analyzeCasesBatch([dict(WIND)], channels=True, statics=True, aero_device=True)
    with pytest.raises(NotImplementedError, match="needs aero_device=True"):
        m.analyzeCasesBatch([dict(WIND)], channels=True)
    with pytest.raises(NotImplementedError, match="needs aero_device=True"):
        m.analyzeCasesBatch([dict(WIND, turbine_status="parked"), dict(WIND)], channels=True, rotor_device=True)
    with pytest.raises(NotImplementedError, match="aero_device=True with statics=True"):       # channels=False is accepted:
        m.analyzeCasesBatch([dict(WIND)], channels=False, statics=True, aero_device=True)     # the next refusal speaks
    farm = raft.Model(load_design("VolturnUS-S_farm_aero"))
    assert farm.nFOWT > 1
    with pytest.raises(NotImplementedError, match="channels=True on an array"):
        farm.analyzeCasesBatch([dict(WIND)], channels=True)


def test_channel_tables_of_the_design():
    """The geometry table holds rotor_channels' values: its coefficient rows follow from it."""
    import raft
    from raft import _native as N
    from raft.rotor_device import chan_geom_table
    fowt = raft.Model(load_design("VolturnUS-S_aero")).fowtList[0]
    fowt.calcStatics()
    fowt.Xi0 = np.zeros(6)
    g = chan_geom_table(fowt)
    coef, _ = fowt.rotor_channels()
    nr = fowt.nrotors
    assert g.shape == (nr, N.CG_COUNT) and np.all(g[:, N.CG["HAS_TOWER"]] == 1.0)
    for ir in range(nr):
        mt, zCG, hArm, ICG = (g[ir, N.CG[k]] for k in ("MT", "ZCG", "HARM", "ICG"))
        assert coef[ir, 1, 4] == g[ir, N.CG["ZREL"]]
        assert coef[nr + ir, 0, 4] == mt * g[ir, N.CG["G"]] * hArm
        assert coef[nr + ir, 1, 0] == mt * hArm and coef[nr + ir, 1, 4] == mt * hArm * zCG + ICG
        assert g[ir, N.CG["ZBASE"]] == zCG - hArm or abs(g[ir, N.CG["ZBASE"]] - (zCG - hArm)) < 1e-12
