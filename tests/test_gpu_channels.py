"""GPU: turbine output channels of batched cases on the device (csrc/rh_channels.hip through
raft/rotor_device.py, FOWT.turbineChannelsBatch and the channels= keyword of analyzeCasesBatch)
against the host build of the same header (tools/channels_host.cpp, which tests/test_channels_host.py
ties to the Python) and against the host path it replaces (calcTurbineConstants, solveDynamics and
saveTurbineOutputs per case).

Shapes of the entry check: nw = 1, 63, 64, 65 and 257 (one bin, both sides of a wave, two strides of
the 256 lanes with one bin in the second) times 1, 3 and 67 cases times 1 and 3 response rows; two
synthetic rotors of different geometry, aeroServoMod 2 and 1, laid over the cases so that one launch
holds cases with one pair, with none and with both, and three V_w rows."""
import os
import sys

import numpy as np
import pytest

from conftest import golden_cases, load_design, load_golden, statics_of

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import aero_cases as AC  # noqa: E402
import channel_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

from test_channels_host import CHANNEL_BAR  # noqa: E402  (measured on the CPU there)
from test_gpu_aero_mb import FIVE, XI_BAR, fresh  # noqa: E402  (the five cases and the two paths' Xi difference)

# analyzeCasesBatch(aero_device=True, channels=True) against the host path: the channels are linear in
# Xi and their PSDs and variances quadratic, so the two paths' Xi difference (XI_BAR, ten times what was
# measured between them) enters a PSD at most twice; the channel arithmetic adds the CPU bar.
# Measured on the device (MI355X), worst over the five cases and all keys, each key normwise relative to
# the host entry's largest value: 1.77e-15 with aeroServoMod 1 (Mbase_PSD; Xi itself differed by 2.10e-16),
# 4.88e-14 with aeroServoMod 2 (AxRNA_PSD, whose w^4 weights the high bins, where the response is small
# and its relative difference largest; Xi normwise 1.01e-15; every control channel below 9e-16); the case
# with two sea states 2.19e-14 (AxRNA_PSD).  Asserted at ten times the measured figure, and never above
# the derived sum.
BATCH_MEASURED = {1: 1.77e-15, 2: 4.88e-14}
BATCH_BAR = {mod: min(10 * BATCH_MEASURED[mod], CHANNEL_BAR + 2 * XI_BAR[mod]) for mod in (1, 2)}
RTOL = 1e-9          # against the reference's golden, as tests/test_gpu_aero.py has it

NWS = [1, 63, 64, 65, 257]
NCASES = [1, 3, 67]
NROWS = [1, 3]
PATTERN = [[0], [], [0, 1], [1], [0, 1], [0], []]


def grid(nw):
    return np.array([0.5]) if nw == 1 else np.linspace(0.03, 1.3, nw)


def tables(nw, ncase, nrow):
    return CC.synthetic_tables([PATTERN[c % len(PATTERN)] for c in range(ncase)], nw, nrow, seed=nw + nrow, w=grid(nw))


def device_channels(t, psd=True):
    """rh_turbine_channels on device copies of host Tables: psd, std, avg as NumPy arrays."""
    import torch
    from raft.rotor_device import turbine_channels
    dev = torch.device("cuda:0")
    Xi = torch.tensor(t.Xi, dtype=torch.complex128, device=dev)
    w = torch.tensor(t.w, dtype=torch.float64, device=dev)
    out = turbine_channels(torch, dev, 0, Xi, w, t.dw, t.geom, t.pitch0, t.pairs, psd=psd)
    torch.cuda.synchronize()
    return (None if out["psd"] is None else out["psd"].cpu().numpy()), out["std"].cpu().numpy(), out["avg"].cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    return CC.host_lib()


@pytest.fixture(scope="module")
def launches():
    """(nw, ncase, nrow) -> the device's (psd, std, avg), launched once and shared."""
    out = {}

    def get(nw, ncase, nrow):
        key = (nw, ncase, nrow)
        if key not in out:
            out[key] = device_channels(tables(nw, ncase, nrow))
        return out[key]
    return get


def worst_difference(got, want):
    """Per (case, rotor, channel): PSD rows normwise relative to their largest entry, scalars relative
    to their magnitude; the largest of them."""
    got, want = np.asarray(got), np.asarray(want)
    if got.ndim == 4:
        scale = np.abs(want).max(axis=3)
        err = np.linalg.norm(got - want, axis=3)
    else:
        scale, err = np.abs(want), np.abs(got - want)
    assert not np.any(got[scale == 0])          # where the reference is zero, exact zeros
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0)))


# ------------------------------------------------------------------------------ the entry against the header
@pytest.mark.parametrize("nrow", NROWS)
@pytest.mark.parametrize("ncase", NCASES)
@pytest.mark.parametrize("nw", NWS)
def test_entry_against_the_host_header(lib, launches, nw, ncase, nrow):
    """Every case's PSDs, standard deviations and means against the host-compiled header at the CPU
    bar; every output written; the control channels of a rotor without a mode-2 pair exact zeros."""
    t = tables(nw, ncase, nrow)
    hP, hS, hA = CC.host_channels(lib, t)
    dP, dS, dA = launches(nw, ncase, nrow)
    assert all(np.all(np.isfinite(a)) for a in (dP, dS, dA))
    worst = max(worst_difference(dP, hP), worst_difference(dS, hS), worst_difference(dA, hA))
    same = all(np.array_equal(a, b) for a, b in ((dP, hP), (dS, hS), (dA, hA)))
    print(f"nw={nw}, ncase={ncase}, nrow={nrow}: worst difference {worst:.2e}, bit-equal: {same}")
    assert worst <= CHANNEL_BAR, worst
    if ncase >= 3:
        assert np.all(dS[0, 0, 2:] > 0) and not np.any(dS[1, :, 2:]) and not np.any(dS[2, 1, 2:])
        assert np.all(dS[:3, :, :2] > 0)
    if (nw, ncase) == (65, 3):      # once without the PSD: the other outputs keep their bits
        nP, nS, nA = device_channels(t, psd=False)
        assert nP is None and np.array_equal(nS, dS) and np.array_equal(nA, dA)


@pytest.mark.parametrize("nrow", NROWS)
@pytest.mark.parametrize("nw", NWS)
def test_rows_are_independent(launches, nw, nrow):
    """Row 0 of the 67-case launch equals the 1-case launch bit for bit, rows 0..2 the 3-case launch."""
    one, three, many = (launches(nw, n, nrow) for n in NCASES)
    for k in range(3):
        assert np.array_equal(many[k][:1], one[k])
        assert np.array_equal(many[k][:3], three[k])


def test_a_batch_without_pairs_and_refusals_with_a_context(lib):
    """npair = 0 with null pair tables against the header; a bad table is refused before any launch."""
    t = tables(65, 3, 3)
    t.pairs = None
    for got, want in zip(device_channels(t), CC.host_channels(lib, t)):
        assert worst_difference(got, want) <= CHANNEL_BAR
    t = tables(5, 3, 1)
    t.pairs["pair_rotor"] = [0, 1, 1]
    with pytest.raises(ValueError, match="names rotor 1 twice"):
        device_channels(t)
    t = tables(5, 3, 1)
    t.pairs["pair_vw"] = [0, 3, 1]
    with pytest.raises(ValueError, match=r"V_w row 3 outside \[0, 3\)"):
        device_channels(t)


# ------------------------------------------------------------------------------ analyzeCasesBatch
CHANNEL_KEYS = [f"{k}_{s}" for k in ("AxRNA", "Mbase", "omega") for s in ("avg", "std", "max", "min", "PSD")] + \
    [f"{k}_{s}" for k in ("torque", "bPitch") for s in ("avg", "std", "PSD")] + ["power_avg", "wind_PSD"]


def ready(mod):
    """A newly built model with its statics (the tower masses and inertias Mbase reads)."""
    m = fresh(mod)
    f = m.fowtList[0]
    f.calcStatics()
    f.calcHydroConstants()
    return m, f


def host_metrics(m, f, case, bem):
    """calcTurbineConstants + solveDynamics + saveTurbineOutputs of one case: (Xi, results)."""
    f.calcTurbineConstants(dict(case), ptfm_pitch=0, bem=bem)
    Xi = m.solveDynamics(dict(case))
    res = {}
    f.saveTurbineOutputs(res, dict(case))
    return Xi, res


def key_difference(got, want):
    """One key of one case: normwise relative to the reference's largest entry (zeros: exact)."""
    return CC.rel(np.asarray(got), np.asarray(want))


@pytest.fixture(scope="module")
def batch():
    """mod -> (the batch result with channels=True, the host path's results per case); solved once."""
    out = {}
    for mod in (1, 2):
        cases = [dict(c) for c in FIVE]
        m, f = ready(mod)
        got = m.analyzeCasesBatch(cases, aero_device=True, channels=True)
        hm, hf = ready(mod)
        bems = hf.rotorLoadsBatch(cases, hm.device)
        order = [4, 0, 1, 2, 3]         # the parked case first: a rotor keeps the C of its last operating case
        host = {i: host_metrics(hm, hf, cases[i], bems[i]) for i in order}
        out[mod] = (got, host)
    return out


@pytest.mark.parametrize("mod", [1, 2])
def test_analyze_cases_batch_channels_against_the_host_path(batch, mod):
    """Every new key of the five cases against the host's case_metrics entry."""
    got, host = batch[mod]
    worst, xi = {}, 0.0
    for i in range(5):
        Xi, res = host[i]
        xi = max(xi, float(np.linalg.norm(got["Xi"][i] - Xi[0]) / np.linalg.norm(Xi[0])))
        for k in CHANNEL_KEYS:
            want = res.get(k, np.zeros_like(got[k][i]))      # (wind_PSD: the host sets it only with a closed loop)
            assert np.shape(got[k][i]) == np.shape(want), k
            d = key_difference(got[k][i], want)
            worst[k] = max(worst.get(k, 0.0), d)
        if i == 4:      # parked: the motion channels as saveTurbineOutputs has them, the control rows zeros
            for k in CHANNEL_KEYS:
                if k.split("_")[0] in ("AxRNA", "Mbase"):
                    assert key_difference(got[k][i], res[k]) <= CHANNEL_BAR, k
                else:
                    assert not np.any(got[k][i]) and not np.any(res.get(k, 0.0)), k
    print(f"aeroServoMod {mod}: Xi difference {xi:.2e}; worst key differences " +
          ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items()) if v > 0))
    assert max(worst.values()) <= BATCH_BAR[mod], {k: v for k, v in worst.items() if v > BATCH_BAR[mod]}
    assert np.all(got["Mbase_std"][:, 0] > 0) and np.all(got["AxRNA_std"][:, 0] > 0)
    live = got["omega_std"][:4, 0] > 0
    assert np.all(live) if mod == 2 else not np.any(live)
    assert (np.all(got["power_avg"][:4, 0] > 1e5) and np.any(got["wind_PSD"][:4])) if mod == 2 else not np.any(got["wind_PSD"])


def test_two_sea_states_against_the_host_path():
    """One case with two sea states: the channels from Xi_waves against the host's multi-row sums."""
    case = dict(AC.wind_case(10.59, 20.0), wave_heading=[0, 30], wave_period=[10, 8], wave_height=[4, 2],
                wave_spectrum=["JONSWAP", "JONSWAP"])
    m, f = ready(2)
    got = m.analyzeCasesBatch([dict(case)], aero_device=True, channels=True)
    assert got["Xi_waves"].shape[1] == 3
    hm, hf = ready(2)
    bems = hf.rotorLoadsBatch([dict(case)], hm.device)
    Xi, res = host_metrics(hm, hf, case, bems[0])
    assert Xi.shape[0] == 3 and np.any(Xi[1])
    worst = {k: key_difference(got[k][0], res[k]) for k in CHANNEL_KEYS}
    print("two sea states: worst key differences " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items()) if v > 0))
    assert max(worst.values()) <= BATCH_BAR[2], worst
    one = m.analyzeCasesBatch([dict(case, wave_heading=0, wave_period=10, wave_height=4, wave_spectrum="JONSWAP")],
                              aero_device=True, channels=True)
    assert np.all(got["Mbase_std"] > one["Mbase_std"])         # the second sea state adds to every sum


def test_a_batch_without_wind_against_the_golden():
    """The wind-0 cases of c2_nw200 with channels=True and no aero_device: AxRNA_* and Mbase_* against the
    reference's own saveTurbineOutputs values, the control channels zeros."""
    import raft
    T = load_golden("c2_nw200")
    m = raft.Model(load_design("VolturnUS-S_example"), statics=[statics_of(T)])
    f = m.fowtList[0]
    f.setPosition(T["r6"])
    f.calcStatics()
    f.calcHydroConstants()
    cases = golden_cases(T)
    got = m.analyzeCasesBatch([dict(c) for c in cases], channels=True)
    assert f.nrotors >= 1 and got["AxRNA_PSD"].shape == (len(cases), f.nw, f.nrotors)
    for ic in range(len(cases)):
        for ch in ["AxRNA", "Mbase"]:
            scale = np.abs(T[f"out_{ch}_std"][ic]).max()
            pscale = np.abs(T[f"out_{ch}_PSD"][ic]).max()
            for st in ["avg", "std", "max", "min"]:
                np.testing.assert_allclose(got[f"{ch}_{st}"][ic], T[f"out_{ch}_{st}"][ic], rtol=RTOL, atol=RTOL * scale,
                                           err_msg=f"{ch}_{st}")
            np.testing.assert_allclose(got[f"{ch}_PSD"][ic], T[f"out_{ch}_PSD"][ic], rtol=RTOL, atol=RTOL * pscale)
    for k in CHANNEL_KEYS:
        if k.split("_")[0] not in ("AxRNA", "Mbase"):
            assert not np.any(got[k]), k


def test_channels_false_is_the_default(batch):
    """Omitting channels, or passing False, returns the same keys and bits, none of them a channel key,
    and channels=True leaves the bits of every other key as they are."""
    cases = [dict(c) for c in FIVE]
    a = ready(2)[0].analyzeCasesBatch([dict(c) for c in cases], aero_device=True)
    b = ready(2)[0].analyzeCasesBatch([dict(c) for c in cases], aero_device=True, channels=False)
    assert sorted(a) == sorted(b) == sorted(["B_drag", "Xi", "f_aero0", "iters", "psd", "status", "std", "zeta"])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    with_channels = batch[2][0]
    assert sorted(with_channels) == sorted(list(a) + CHANNEL_KEYS)
    for k in a:
        assert np.array_equal(a[k], with_channels[k]), k
