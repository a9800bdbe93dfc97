"""Rotor blade-element momentum loads on the device (csrc/rh_rotor.h, rh_rotor.hip).

flatten_rotor() turns a raft.ccblade.CCBlade into the tables of rh_rotor; DeviceRotor wraps
rh_rotor_loads on torch tensors and returns what CCBlade.evaluate returns.  The device covers the
restatement class with iterRe = 1 and airfoils of one Reynolds number, within the ABI's limits;
flatten_rotor() refuses everything else with a NotImplementedError that names the reason, before
any device call.
"""
import ctypes

import numpy as np

from . import _native as N
from .ccblade import CCBlade, define_curvature
from .device_records import DeviceRecords


class FlatRotor:
    """The host tables of one rh_rotor record and the ctypes record over them (host pointers only;
    DeviceRotor adds the device ones)."""

    def __init__(self, scalars, section, nknot, knots, coef):
        self.scalars = scalars
        self.section = np.ascontiguousarray(section, dtype=np.float64)
        self.nknot = np.ascontiguousarray(nknot, dtype=np.int32)
        self.knots = np.ascontiguousarray(knots, dtype=np.float64)
        self.coef = np.ascontiguousarray(coef, dtype=np.float64)
        self.nr, self.nsector = scalars["nr"], scalars["nsector"]

    def fill(self, rec, device_tables=None):
        for k, v in self.scalars.items():
            setattr(rec, k, v)
        rec.pad_ = 0
        rec.section_host, rec.nknot_host = self.section.ctypes.data, self.nknot.ctypes.data
        rec.knots_host, rec.coef_host = self.knots.ctypes.data, self.coef.ctypes.data
        if device_tables is not None:
            rec.section, rec.nknot, rec.knots, rec.coef = (t.data_ptr() for t in device_tables)
        return rec

    def record(self):
        return self.fill(N.RhRotor())


def flatten_rotor(ccblade):
    """The rh_rotor tables of a raft.ccblade.CCBlade.  Host only: no device is touched."""
    if not isinstance(ccblade, CCBlade):
        raise NotImplementedError(f"device rotor: rotor.ccblade is a {type(ccblade).__module__}.{type(ccblade).__name__}, "
                                  "not the restatement class raft.ccblade.CCBlade (another CCBlade evaluates on the host)")
    if ccblade.iterRe != 1:
        raise NotImplementedError(f"device rotor: iterRe = {ccblade.iterRe} (only one pass of the Reynolds-number "
                                  "iteration, iterRe = 1)")
    nr, nsec = len(ccblade.r), int(ccblade.nSector)
    if nr < 1 or nr > N.ROTOR_MAX_SECTIONS:
        raise NotImplementedError(f"device rotor: {nr} blade sections (1 to {N.ROTOR_MAX_SECTIONS})")
    if nsec < 1 or nsec > N.ROTOR_MAX_SECTORS:
        raise NotImplementedError(f"device rotor: {nsec} azimuthal sectors (1 to {N.ROTOR_MAX_SECTORS})")
    splines = []
    for i, af in enumerate(ccblade.af):
        if not getattr(af, "one_Re", False):
            raise NotImplementedError(f"device rotor: airfoil {i} has more than one Reynolds number")
        for sp in (af.cl_spline, af.cd_spline):
            tx, ty, c = sp.tck
            kx, ky = sp.degrees
            if ky != 1 or len(ty) != 4:
                raise NotImplementedError(f"device rotor: airfoil {i} has more than one Reynolds number (spline of "
                                          f"degree {ky} with {len(ty)} knots in Re)")
            if len(tx) > N.ROTOR_MAX_KNOTS:
                raise NotImplementedError(f"device rotor: airfoil {i}: {len(tx)} spline knots in alpha (at most "
                                          f"{N.ROTOR_MAX_KNOTS})")
            splines.append((i, np.asarray(tx, dtype=float), np.asarray(ty, dtype=float), np.asarray(c, dtype=float), kx))
    degrees = {s[4] for s in splines}
    if len(degrees) != 1 or not 1 <= min(degrees) <= 3:
        raise NotImplementedError(f"device rotor: polar splines of degrees {sorted(degrees)} in alpha (one degree "
                                  "from 1 to 3 for all airfoils)")
    kx = degrees.pop()
    stride = max(len(s[1]) for s in splines)
    nknot = np.zeros([2, nr], dtype=np.int32)
    knots = np.zeros([2, nr, stride + 4])
    coef = np.zeros([2, nr, stride, 2])
    for n, (i, tx, ty, c, _) in enumerate(splines):
        p = n % 2                                    # 0 = cl, 1 = cd
        nknot[p, i] = len(tx)
        knots[p, i, :len(tx)] = tx
        knots[p, i, len(tx):stride] = tx[-1]
        knots[p, i, stride:] = ty
        coef[p, i, :len(tx) - kx - 1] = c.reshape(len(tx) - kx - 1, 2)
    # the stations' geometry: the inflow's (define_curvature of the stations) and thrust_torque's
    # (the path hub, stations, tip, where the loads are zero)
    x_az, y_az, z_az, cone, _ = define_curvature(ccblade.r, ccblade.precurve, ccblade.presweep, ccblade.precone)
    rfull = np.r_[ccblade.Rhub, ccblade.r, ccblade.Rtip]
    curvefull = np.r_[0.0, ccblade.precurve, ccblade.precurveTip]
    sweepfull = np.r_[0.0, ccblade.presweep, ccblade.presweepTip]
    _, _, z_full, cone_full, s = define_curvature(rfull, curvefull, sweepfull, ccblade.precone)
    ds = s[1:] - s[:-1]
    section = np.zeros([N.RS_COUNT, nr])
    section[N.RS["R"]], section[N.RS["CHORD"]], section[N.RS["THETA"]] = ccblade.r, ccblade.chord, ccblade.theta
    section[N.RS["XAZ"]], section[N.RS["YAZ"]], section[N.RS["ZAZ"]] = x_az, y_az, z_full[1:-1]
    section[N.RS["CONE"]] = cone
    section[N.RS["WEIGHT"]] = 0.5 * (ds[:-1] + ds[1:])
    section[N.RS["CONE_PATH"]] = cone_full[1:-1]
    opt = ccblade.bemoptions
    scalars = dict(nr=nr, nsector=nsec, B=int(ccblade.B), usecd=int(bool(opt["usecd"])),
                   tiploss=int(bool(opt["tiploss"])), hubloss=int(bool(opt["hubloss"])),
                   wakerotation=int(bool(opt["wakerotation"])), kx=int(kx), knot_stride=int(stride),
                   Rhub=float(ccblade.Rhub), Rtip=float(ccblade.Rtip), rho=float(ccblade.rho), mu=float(ccblade.mu),
                   precone=float(ccblade.precone), hubHt=float(ccblade.hubHt), shearExp=float(ccblade.shearExp))
    return FlatRotor(scalars, section, nknot, knots, coef)


def bem_pair(nr, loads8, dloads6, Omega_rpm):
    """One operating point's (loads, derivs) in the form of CCBlade.evaluate (npts = 1): what
    Rotor.runCCBlade takes as `bem`."""
    T, Y, Z, Q, My, Mz, Mb, P = (np.array([v], dtype=float) for v in loads8)
    loads = dict(T=T, Y=Y, Z=Z, Q=Q, My=My, Mz=Mz, Mb=Mb, P=P)
    derivs = {}
    if dloads6 is not None:
        d = np.asarray(dloads6, dtype=float).reshape(2, 3)
        w = Omega_rpm * np.pi / 30.0

        def block(v):
            return {"dUinf": np.diag(v[0:1]), "dOmega": np.diag(v[1:2]), "dpitch": np.diag(v[2:3]),
                    "dr": np.zeros((1, nr))}
        derivs["dT"] = block(d[0])
        derivs["dQ"] = block(d[1])
        derivs["dP"] = block(d[1] * w + np.array([0.0, Q[0] * np.pi / 30.0, 0.0]))
    return loads, derivs


def aero_mode(rot, ir):
    """aeroServoMod of an operating rotor as rh_rotor_aero_mb takes it, 1 or 2; anything else is
    refused by name (host only: no device is touched)."""
    mod = rot.aeroServoMod
    if mod not in (1, 2):
        raise NotImplementedError(f"device aero-servo matrices: rotor {ir} has aeroServoMod = {mod} (1 or 2)")
    return int(mod)


def aero_param_row(rot, speed, mode):
    """The rh_rotor_aero_mb parameter row of one (case, rotor) pair at the rotor's current pose and
    yaw (after Rotor.inflow_angles of the case): everything Rotor.calcAero and
    FOWT.calcTurbineConstants use that does not depend on the bin.  The gains are interpolated at
    the case's wind speed and the torque gains gated as calcAero does; the gyroscopic vector takes
    the rotor speed at `speed`, not at Uhub, as calcTurbineConstants has it."""
    row = np.zeros(N.AP_COUNT)
    row[N.AP["MODE"]] = mode
    row[N.AP["RQ"]:N.AP["RQ"] + 9] = np.asarray(rot.R_q, dtype=float).reshape(9)
    row[N.AP["RHUB"]:N.AP["RHUB"] + 3] = rot.r_hub_rel
    kp_beta = -np.interp(speed, rot.Uhub, rot.kp_0)
    ki_beta = -np.interp(speed, rot.Uhub, rot.ki_0)
    row[N.AP["I_DRIVETRAIN"]], row[N.AP["NG"]], row[N.AP["K_FLOAT"]] = rot.I_drivetrain, rot.Ng, rot.k_float
    row[N.AP["KP_BETA"]], row[N.AP["KI_BETA"]] = kp_beta, ki_beta
    row[N.AP["KP_TAU"]], row[N.AP["KI_TAU"]] = rot.kp_tau * (kp_beta == 0), rot.ki_tau * (ki_beta == 0)
    Omega_rpm = np.interp(speed, rot.Uhub, rot.Omega_rpm)
    row[N.AP["GYRO"]:N.AP["GYRO"] + 3] = rot.I_drivetrain * (rot.q * Omega_rpm * 2 * np.pi / 60)
    return row


def chan_pair_row(rot):
    """The rh_turbine_channels row of one (case, rotor) pair next to its aero_param_row: the hub height
    the floating feedback of Rotor.calcAero divides by, and the torque gains as FOWT._aero_outputs reads
    them from the rotor (not gated by the pitch gains, unlike the parameter row's)."""
    row = np.zeros(N.CP_COUNT)
    row[N.CP["ZHUB"]], row[N.CP["KP_TAU"]], row[N.CP["KI_TAU"]] = rot.r3[2], rot.kp_tau, rot.ki_tau
    return row


def chan_geom_table(fowt):
    """The per-rotor geometry table [nrotors, CG_COUNT] of rh_turbine_channels, each value formed as
    FOWT.rotor_channels and FOWT._aero_outputs form it.  A rotor index at or beyond the number of
    towers has no tower-base moment (HAS_TOWER 0)."""
    from .fowt import translate_matrix_6to6
    geom = np.zeros([fowt.nrotors, N.CG_COUNT])
    for ir, rot in enumerate(fowt.rnaList):
        geom[ir, N.CG["ZREL"]], geom[ir, N.CG["G"]] = rot.r_rel[2], fowt.g
    for ir, rot in enumerate(fowt.rnaList[:len(fowt.mtower)]):
        mt = fowt.mtower[ir] + rot.mRNA
        zCG = (fowt.rCG_tow[ir][2] * fowt.mtower[ir] + rot.r_rel[2] * rot.mRNA) / mt
        tower = fowt.memberList[fowt.nplatmems + ir]
        zBase = tower.rA[2]
        ICG = (translate_matrix_6to6(tower.M_struc, [0, 0, -zCG])[4, 4] + rot.mRNA * (rot.r_rel[2] - zCG) ** 2
               + rot.IrRNA)
        for k, v in (("MT", mt), ("ZCG", zCG), ("HARM", zCG - zBase), ("ICG", ICG), ("ZBASE", zBase), ("HAS_TOWER", 1.0)):
            geom[ir, N.CG[k]] = v
    return geom


def turbine_channels(torch, device, dev_index, Xi, w, dw, geom, pitch0=None, pairs=None, psd=True):
    """rh_turbine_channels on the current stream of `device`.  Xi: device complex128 [ncase, nrow, 6, nw]
    (or [ncase, 6, nw]); w: device [nw]; geom [nrot, CG_COUNT] (chan_geom_table); pitch0 [ncase] or None.
    pairs: None for a batch without wind, or a dict of the pair tables: pair_case, pair_rotor, modes,
    pair_vw (host integers [npair]), loads, dloads, param, op (device tensors, as rh_rotor_loads and
    DeviceRotor.aero_mb hold them), pair_row [npair, CP_COUNT] and V_w [nvw, nw] (host or device).
    Returns device tensors psd [ncase, nrot, TC_SPECTRA, nw] (None with psd=False),
    std [ncase, nrot, TC_SPECTRA] and avg [ncase, nrot, TC_COUNT]."""
    f64 = dict(dtype=torch.float64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    if Xi.dim() == 3:
        Xi = Xi[:, None]
    Xi = Xi.contiguous()
    ncase, nrow, ndof, nw = Xi.shape
    if ndof != 6 or Xi.dtype != torch.complex128 or int(w.shape[0]) != nw:
        raise ValueError(f"turbine_channels: Xi complex128 [ncase, nrow, 6, {int(w.shape[0])}] expected, got "
                         f"{Xi.dtype} {list(Xi.shape)}")
    geom = np.ascontiguousarray(geom, dtype=np.float64)
    nrot = geom.shape[0]
    if geom.shape != (nrot, N.CG_COUNT):
        raise ValueError(f"turbine_channels: geom of shape [nrot, {N.CG_COUNT}] expected")
    as_dev = lambda a: a.to(**f64).contiguous() if torch.is_tensor(a) else \
        torch.tensor(np.ascontiguousarray(a, dtype=np.float64), **f64)                              # noqa: E731
    geom_dev = as_dev(geom)
    p0 = None if pitch0 is None else as_dev(pitch0)
    if p0 is not None and tuple(p0.shape) != (ncase,):
        raise ValueError("turbine_channels: one mean pitch per case expected")
    npair, nvw, host, dev = 0, 0, [None] * 4, [None] * 9
    if pairs is not None and len(pairs["pair_case"]):
        host = [np.ascontiguousarray(pairs[k], dtype=np.int32) for k in ("pair_case", "pair_rotor", "modes", "pair_vw")]
        npair = len(host[0])
        V_w = as_dev(pairs["V_w"])
        nvw = int(V_w.shape[0])
        tabs = [as_dev(pairs[k]) for k in ("loads", "dloads", "param", "op", "pair_row")]
        if tuple(tabs[1].shape) == (npair, 6):        # dloads as a flat row per pair
            tabs[1] = tabs[1].reshape(npair, 2, 3)
        want = [(npair, 8), (npair, 2, 3), (npair, N.AP_COUNT), (npair, 5), (npair, N.CP_COUNT)]
        if any(h.shape != (npair,) for h in host) or any(tuple(t.shape) != s for t, s in zip(tabs, want)) \
                or tuple(V_w.shape) != (nvw, nw):
            raise ValueError("turbine_channels: one entry of every pair table per pair and V_w [nvw, nw] expected")
        dev = [torch.tensor(host[0], **i32), torch.tensor(host[1], **i32), torch.tensor(host[3], **i32), *tabs, V_w]
    out_psd = torch.empty([ncase, nrot, N.TC_SPECTRA, nw], **f64) if psd else None
    out_std = torch.empty([ncase, nrot, N.TC_SPECTRA], **f64)
    out_avg = torch.empty([ncase, nrot, N.TC_COUNT], **f64)
    hp = lambda a: None if a is None else a.ctypes.data                                             # noqa: E731
    pc_dev, pr_dev, pv_dev, loads, dloads, param, op, prow, V_w = dev
    N.check(N.lib().rh_turbine_channels(N.context(dev_index), ncase, nrow, nw, float(dw), N.ptr(w), N.ptr(Xi), N.ptr(p0),
                                        nrot, N.ptr(geom_dev), npair, N.ptr(pc_dev), hp(host[0]), N.ptr(pr_dev),
                                        hp(host[1]), hp(host[2]), N.ptr(loads), N.ptr(dloads), N.ptr(param), N.ptr(op),
                                        N.ptr(prow), N.ptr(pv_dev), hp(host[3]), nvw, N.ptr(V_w), N.ptr(out_psd),
                                        N.ptr(out_std), N.ptr(out_avg), N.stream_handle(torch, device)),
            "rh_turbine_channels")
    return dict(psd=out_psd, std=out_std, avg=out_avg, _keep=(Xi, geom_dev, p0, dev))


class DeviceRotor(DeviceRecords):
    """One or more rotors resident on the device; operating points pick a rotor through rot_idx."""

    def __init__(self, rotors, device=0):
        self.flat = [r if isinstance(r, FlatRotor) else flatten_rotor(r) for r in rotors]   # refusals first
        super().__init__(device)
        torch = self.torch
        self.nrot = len(self.flat)
        self.nr_max = max(f.nr for f in self.flat)
        self.ns_max = max(f.nsector for f in self.flat)
        self._tables = []
        self._arr = (N.RhRotor * self.nrot)()
        for i, f in enumerate(self.flat):
            tabs = (torch.tensor(f.section, dtype=torch.float64, device=self.device).contiguous(),
                    torch.tensor(f.nknot, dtype=torch.int32, device=self.device).contiguous(),
                    torch.tensor(f.knots, dtype=torch.float64, device=self.device).contiguous(),
                    torch.tensor(f.coef, dtype=torch.float64, device=self.device).contiguous())
            self._tables.append(tabs)
            f.fill(self._arr[i], tabs)
        self._arr_dev = self.upload(self._arr)

    def launch(self, rot_idx, op, derivatives=True, sections=False):
        """rh_rotor_loads at op [n, 5] = Uinf, Omega_rpm, pitch_deg, tilt, yaw.  rot_idx [n] (any
        integers: an index outside [0, nrot) gives that row status 3) or None.  Returns device
        tensors loads [n,8], dloads [n,2,3] or None, sec [n,ns_max,nr_max,3] or None, status [n]."""
        torch = self.torch
        op = torch.as_tensor(np.asarray(op, dtype=float) if not torch.is_tensor(op) else op, dtype=torch.float64,
                             device=self.device).contiguous()
        n = op.shape[0]
        if list(op.shape) != [n, 5]:
            raise ValueError(f"expected op of shape [n, 5], got {list(op.shape)}")
        idx = self.index(rot_idx, n, name="rot_idx")
        f64 = dict(dtype=torch.float64, device=self.device)
        loads = torch.empty([n, 8], **f64)
        dloads = torch.empty([n, 2, 3], **f64) if derivatives else None
        sec = torch.empty([n, self.ns_max, self.nr_max, 3], **f64) if sections else None
        status = torch.empty([n], dtype=torch.int32, device=self.device)
        N.check(N.lib().rh_rotor_loads(N.context(self.dev_index), self._arr, N.ptr(self._arr_dev), self.nrot, n,
                                       N.ptr(idx), N.ptr(op), N.ptr(loads), N.ptr(dloads), N.ptr(sec), N.ptr(status),
                                       N.stream_handle(torch, self.device)), "rh_rotor_loads")
        return dict(loads=loads, dloads=dloads, sec=sec, status=status, _keep=(op, idx))

    def aero_mb(self, res, ncase, pair_case, modes, param, w, M0, B0):
        """rh_rotor_aero_mb on the stream of launch(): res its result for the pairs (with
        derivatives), consumed on the device; pair_case [npair] the case row of each pair
        (non-decreasing, the pairs of a case in rotor order), modes [npair] their aeroServoMod,
        param [npair, AP_COUNT] their rows (aero_param_row); w [nw], M0, B0 ([6, 6] or [nw, 6, 6])
        device tensors of the base design.  Returns device tensors M [ncase, nw, 6, 6],
        B [ncase, nw, 6, 6] and f_aero0 [ncase, 6], and with them the pair tables it holds on the
        device (loads, dloads, param, op) and the host columns pair_case and modes, for
        turbine_channels()."""
        torch = self.torch
        pc = np.ascontiguousarray(pair_case, dtype=np.int32)
        md = np.ascontiguousarray(modes, dtype=np.int32)
        par = np.ascontiguousarray(param, dtype=np.float64)
        npair, nw = len(pc), int(w.shape[0])
        if md.shape != (npair,) or par.shape != (npair, N.AP_COUNT) or res["loads"].shape[0] != npair \
                or res["dloads"] is None:
            raise ValueError("aero_mb: one mode, parameter row and rh_rotor_loads row (with derivatives) per pair expected")
        if not np.array_equal(par[:, N.AP["MODE"]], md):     # the kernel reads the table's, the entry validates md
            raise ValueError("aero_mb: the parameter rows' mode column differs from modes")
        per_bin = M0.dim() == 3
        if tuple(M0.shape) != ((nw, 6, 6) if per_bin else (6, 6)) or B0.shape != M0.shape:
            raise ValueError(f"aero_mb: M0 and B0 of shape [6, 6] or [{nw}, 6, 6] expected")
        f64 = dict(dtype=torch.float64, device=self.device)
        pc_dev = torch.tensor(pc, dtype=torch.int32, device=self.device)
        par_dev = torch.tensor(par, **f64)
        M = torch.empty([ncase, nw, 6, 6], **f64)
        B = torch.empty([ncase, nw, 6, 6], **f64)
        f0 = torch.empty([ncase, 6], **f64)
        N.check(N.lib().rh_rotor_aero_mb(N.context(self.dev_index), ncase, npair, nw, N.ptr(w), N.ptr(pc_dev),
                                         pc.ctypes.data, md.ctypes.data, N.ptr(res["loads"]), N.ptr(res["dloads"]),
                                         N.ptr(par_dev), N.ptr(M0), N.ptr(B0), int(per_bin), N.ptr(M), N.ptr(B),
                                         N.ptr(f0), N.stream_handle(torch, self.device)), "rh_rotor_aero_mb")
        return dict(M=M, B=B, f_aero0=f0, loads=res["loads"], dloads=res["dloads"], param=par_dev, op=res["_keep"][0],
                    pair_case=pc, modes=md, _keep=(pc_dev, par_dev, res))

    def turbine_channels(self, Xi, w, dw, geom, pitch0=None, pairs=None, psd=True):
        """rh_turbine_channels on the stream of launch() and aero_mb(): see turbine_channels()."""
        return turbine_channels(self.torch, self.device, self.dev_index, Xi, w, dw, geom, pitch0, pairs, psd)

    def evaluate(self, rot_idx, Uinf, Omega_rpm, pitch_deg, tilt, yaw, derivatives=True, sections=False):
        """CCBlade.evaluate of every operating point (tilt and yaw [rad] as Rotor.runCCBlade sets
        them on the CCBlade object).  Returns (loads, derivs, status) and, with sections, sec: loads
        a dict of arrays [n] (T, Y, Z, Q, My, Mz, Mb, P), derivs the dict of dT / dQ / dP blocks with
        their diagonal matrices (empty without derivatives), status [n], sec [n,ns_max,nr_max,3]."""
        cols = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, dtype=float)) for v in
                                     (Uinf, Omega_rpm, pitch_deg, tilt, yaw)))
        op = np.stack(cols, axis=1)
        out = self.launch(rot_idx, op, derivatives, sections)
        L = out["loads"].cpu().numpy()
        status = out["status"].cpu().numpy()
        loads = {k: L[:, i].copy() for i, k in enumerate(("T", "Y", "Z", "Q", "My", "Mz", "Mb", "P"))}
        derivs = {}
        if derivatives:
            d = out["dloads"].cpu().numpy()
            w = op[:, 1] * np.pi / 30.0
            n = len(op)

            def block(v):
                return {"dUinf": np.diag(v[:, 0]), "dOmega": np.diag(v[:, 1]), "dpitch": np.diag(v[:, 2]),
                        "dr": np.zeros((n, self.nr_max))}
            derivs["dT"] = block(d[:, 0])
            derivs["dQ"] = block(d[:, 1])
            derivs["dP"] = block(d[:, 1] * w[:, None] + np.c_[0 * w, loads["Q"] * np.pi / 30.0, 0 * w])
        if sections:
            return loads, derivs, status, out["sec"].cpu().numpy()
        return loads, derivs, status
