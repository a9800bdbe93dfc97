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
        B [ncase, nw, 6, 6] and f_aero0 [ncase, 6]."""
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
        return dict(M=M, B=B, f_aero0=f0, _keep=(pc_dev, par_dev, res))

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
