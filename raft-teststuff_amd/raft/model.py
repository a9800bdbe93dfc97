"""Model: the frequency-domain response solve of a (multi-)FOWT system on MI355X.

Drop-in for the reference entry points on the hot path (raft/raft_model.py):
  Model(design)                   frequency grid + FOWTs                 :30-170
  Model.solveDynamics(case, ...)  drag fixed point + system response     :852-1146
  Model.analyzeCases(...)         per-case loop + motion outputs          :244-388
plus the batched form the reference does not have:
  Model.analyzeCasesBatch(cases)  every case in ONE device call (one workgroup per case).

By default the batch does not solve mean offsets (solveStatics: MoorPy equilibrium): the platform
stays at its reference position, exactly the state the goldens are generated in.
  Model.solveStaticsBatch(cases)  the mean offsets of every case on the device (csrc/rh_moor.hip);
  analyzeCasesBatch(cases, statics=True) solves each case at its own offset pose, as analyzeCases does.
  Model.solveStaticsArrayBatch(cases)  the same for moored arrays: N FOWTs on the array-level system
  and / or their own systems, free points included (csrc/rh_moor_array.hip);
  analyzeArrayBatch(cases, statics=True) solves each case of the farm at its own offset poses.
"""
import ctypes

import numpy as np

from . import _native as N
from .fowt import FOWT, mooring_outputs
from .hydro_math import DEG2RAD, get_from_dict, wave_numbers
from .second_order import file_qtf_forces, qtf_index_error, sea_spectra, solve_batch_2nd
from .solver import BatchResult, CaseSet, solve_batch


class CaseMB:
    """A per-case view of a DeviceDesign: the same node and wave tables, its own per-bin M and
    B [nw, 6, 6] device tensors (an operating rotor's aero-servo terms for one case)."""

    def __init__(self, base, M, B):
        self.base, self._M, self._B = base, M, B

    @classmethod
    def of_case(cls, fowt, base, case, bem=None):
        """The view of `base` with the M and B that calcTurbineConstants(case, bem=bem) gives `fowt`,
        which is left with that case's turbine constants."""
        import torch
        from .prep import linear_matrices
        fowt.calcTurbineConstants(dict(case), ptfm_pitch=0, bem=bem)
        M, B, _, _ = linear_matrices(fowt)
        f64 = dict(dtype=torch.float64, device=base.device)
        return cls(base, torch.tensor(M, **f64).contiguous(), torch.tensor(B, **f64).contiguous())

    def __getattr__(self, name):
        return getattr(self.__dict__["base"], name)

    def ensure_headings(self, betas):
        return self.base.ensure_headings(betas)

    def struct(self):
        d = N.RhDesign.from_buffer_copy(self.base.struct())
        d.M, d.B, d.mb_per_bin = N.ptr(self._M), N.ptr(self._B), 1
        return d


class FurtherSeaStates:
    """The sea states after the first of every case of a batch (raft/raft_model.py:1049-1065), case
    after case.  seas: _case_sea_states of every case, nws their sea-state counts.  Host only:
    pairs [(case, sea state)], case / sea their index arrays, the picked columns heading [deg],
    spectrum, Hs, Tp, gamma, betas [rad] and nwm, the batch's largest sea-state count."""

    def __init__(self, seas, nws):
        self.pairs = [(i, h) for i in range(len(seas)) for h in range(1, int(nws[i]))]
        self.case = np.array([i for i, _ in self.pairs], dtype=np.int64)
        self.sea = np.array([h for _, h in self.pairs], dtype=np.int64)
        self.heading, self.spectrum, self.Hs, self.Tp, self.gamma = ([seas[i][k][h] for i, h in self.pairs]
                                                                     for k in range(5))
        self.betas = np.array(self.heading, dtype=float) * DEG2RAD
        self.nwm = int(max(nws)) if len(nws) else 0

    def spectra(self, dd):
        """S and zeta [m, nw] of the pairs on design dd's grid (rh_sea_state, one launch)."""
        return sea_spectra(dd, [N.SPECTRUM_CODES[x] for x in self.spectrum], self.Hs, self.Tp, self.gamma)

    def scatter(self, first, further, rows):
        """[n, rows, ...] in the reference's layout: row 0 of case i is first[i], row h the entry of
        further [m, ...] for the pair (i, h); rows of absent sea states are zero."""
        import torch
        out = torch.zeros([first.shape[0], rows, *first.shape[1:]], dtype=first.dtype, device=first.device)
        out[:, 0] = first
        out[torch.tensor(self.case, dtype=torch.long, device=first.device),
            torch.tensor(self.sea, dtype=torch.long, device=first.device)] = further
        return out


class Model:
    def __init__(self, design, nTurbines=1, statics=None, device=0):
        """statics: optional per-FOWT dicts of calcStatics outputs (M_struc, C_struc, C_hydro,
        B_struc, W_struc, W_hydro) and C_moor; see FOWT.setStatics."""
        self.fowtList = []
        self.coords = []
        self.nDOF = 0
        if "settings" not in design:
            design["settings"] = {}
        st = design["settings"]
        min_freq = get_from_dict(st, "min_freq", default=0.01, dtype=float)
        max_freq = get_from_dict(st, "max_freq", default=1.00, dtype=float)
        self.XiStart = get_from_dict(st, "XiStart", default=0.1, dtype=float)
        self.nIter = get_from_dict(st, "nIter", default=15, dtype=int)
        self.w = self.frequency_grid(design)   # :55
        self.nw = len(self.w)
        self.depth = get_from_dict(design["site"], "water_depth", dtype=float)
        self.k = wave_numbers(self.w, self.depth)
        self.device = device
        self.K_array = None          # array-level mooring stiffness override [6N,6N] (else from self.ms)
        self.ms = None               # array-level mooring system (raft/raft_model.py:83-102)
        if "array" in design:
            self.nFOWT = len(design["array"]["data"])
            if "turbine" in design and "turbines" not in design:
                design["turbines"] = [design["turbine"]]
            if "platform" in design and "platforms" not in design:
                design["platforms"] = [design["platform"]]
            if "mooring" in design and "moorings" not in design:
                design["moorings"] = [design["mooring"]]
            info = [dict(zip(design["array"]["keys"], row)) for row in design["array"]["data"]]
            if "array_mooring" in design:
                from .mooring import MooringSystem
                am = design["array_mooring"]
                if "file" not in am:
                    raise Exception("When using 'array_mooring', a MoorDyn-style input file must be provided as 'file'.")
                self.ms = MooringSystem(depth=self.depth)
                for i in range(self.nFOWT):
                    self.ms.add_body([info[i]["x_location"], info[i]["y_location"], 0, 0, 0, 0])
                self.ms.load_moordyn(am["file"])
            for i in range(self.nFOWT):
                d_i = {"site": design["site"]}
                if info[i]["turbineID"] != 0:
                    d_i["turbine"] = design["turbines"][info[i]["turbineID"] - 1]
                d_i["platform"] = design["platforms"][info[i]["platformID"] - 1]
                d_i["mooring"] = None if info[i]["mooringID"] == 0 else design["moorings"][info[i]["mooringID"] - 1]
                self.fowtList.append(FOWT(d_i, self.w, self.ms.bodies[i] if self.ms else None, depth=self.depth,
                                          x_ref=info[i]["x_location"],
                                          y_ref=info[i]["y_location"], heading_adjust=info[i]["heading_adjust"],
                                          device=device))
                self.coords.append([info[i]["x_location"], info[i]["y_location"]])
                self.nDOF += 6
        else:
            self.nFOWT = 1
            self.fowtList.append(FOWT(design, self.w, None, depth=self.depth, device=device))
            self.coords.append([0.0, 0.0])
            self.nDOF += 6
        if statics is not None:
            for f, s in zip(self.fowtList, statics):
                f.setStatics(s)
        self.design = design
        self.mooring_currentMod = get_from_dict(design.get("mooring") or {}, "currentMod", default=0, dtype=int)
        if self.ms is not None:
            self.ms.initialize()
        self.results = {}

    @staticmethod
    def frequency_grid(design):
        """The first-order frequency grid [rad/s] of a design's settings (raft/raft_model.py:55)."""
        st = design.get("settings", {})
        min_freq = get_from_dict(st, "min_freq", default=0.01, dtype=float)
        max_freq = get_from_dict(st, "max_freq", default=1.00, dtype=float)
        return np.arange(min_freq, max_freq + 0.5 * min_freq, min_freq) * 2 * np.pi

    # --------------------------------------------------------------------- dynamics
    def solveDynamics(self, case, tol=0.01, conv_plot=0, RAO_plot=0, display=0):
        """raft/raft_model.py:852-1146 on the device.  Returns Xi [nWaves+1, 6N, nw] and sets
        fowt.Xi, fowt.Z, fowt.B_hydro_drag, fowt.F_hydro_drag, member Bmat like the reference.
        potSecOrder=1 FOWTs follow :966-989: first convergence -> RAO -> slender-body QTF ->
        second-order force -> a second drag pass from iteration 1 with the un-relaxed XiLast."""
        import torch
        iCase = case.get("iCase") if isinstance(case, dict) else None
        Zs, Fws = [], []
        for i, fowt in enumerate(self.fowtList):
            fowt.calcHydroExcitation(case, memberList=fowt.memberList)
            dd = fowt.device_design()
            dev = dd.device
            nW = fowt.nWaves
            fowt.Fhydro_2nd = np.zeros([nW, 6, self.nw], dtype=complex)
            fowt.Fhydro_2nd_mean = np.zeros([nW, 6])
            fowt._f2nd_w = [None] * nW
            cs = CaseSet([0], [case["wave_heading"][0]], [N.SPECTRUM_CODES[case["wave_spectrum"][0]]],
                         [case["wave_height"][0]], [case["wave_period"][0]], [case["wave_gamma"][0]])
            if display > 0:
                print("Solving for system response to wave excitation in primary wave direction")
            second = fowt.potSecOrder == 1
            want = ("zeta", "B_drag", "Bmat", "Z") + (("rao", "Xi_prev") if second else ())
            fext = None
            if fowt.potSecOrder == 2:   # external QTF: second-order load inside the drag loop (:903-904)
                fm, f = fowt.calcHydroForce_2ndOrd(fowt.beta[0], fowt._S_dev[0], iCase=iCase, iWT=i)
                fowt.Fhydro_2nd_mean[0], fowt.Fhydro_2nd[0] = fm, f
                fext = fowt._f2nd_dev.to(torch.complex128)[None].contiguous()
                fowt._f2nd_w[0] = fext[0]
            res = solve_batch([dd], cs, self.nIter, self.XiStart, tol, want=want, fext=fext)
            status, iters = self._check_pass(res, tol, display)
            fowt.iterations_pair = [iters]
            if second and status == N.RH_CASE_CONVERGED:
                if display > 1:
                    print("Resolving for system response in primary wave direction, now with second-order wave loads.")
                fowt.calcQTF_slenderBody(waveHeadInd=0, Xi0=res["rao"][0], verbose=True, iCase=iCase, iWT=i)
                fm, f = fowt.calcHydroForce_2ndOrd(fowt.beta[0], fowt._S_dev[0], iCase=iCase, iWT=i)
                fowt.Fhydro_2nd_mean[0], fowt.Fhydro_2nd[0] = fm, f
                fext = fowt._f2nd_dev.to(torch.complex128)[None].contiguous()
                fowt._f2nd_w[0] = fext[0]
                res = solve_batch([dd], cs, self.nIter, self.XiStart, tol, want=("zeta", "B_drag", "Bmat", "Z"),
                                  fext=fext, Xi_init=res["Xi_prev"].contiguous(), first_iter=1)
                status, iters = self._check_pass(res, tol, display)
                fowt.iterations_pair.append(iters)
            if status != N.RH_CASE_CONVERGED and display > 0:
                print("WARNING - solveDynamics iteration did not converge to the tolerance.")
            fowt.iterations, fowt.converged = iters, status == N.RH_CASE_CONVERGED
            Z = res["Z"][0]                                   # [nw,6,6]
            fowt.Z = np.moveaxis(Z.cpu().numpy(), 0, 2)
            fowt.B_hydro_drag = res["B_drag"][0].cpu().numpy()
            fowt._Bmat_dev = res["Bmat"][0].reshape(-1, 9).contiguous()
            fowt._scatter_bmat(fowt._Bmat_dev.cpu().numpy())
            Zs.append(Z)
            # excitation of every sea state with the final linearisation (:1049-1061)
            Fw = []
            for ih in range(nW):
                Fd = torch.tensor(fowt.calcDragExcitation(ih), dtype=torch.complex128, device=dev)
                if fowt.potSecOrder == 2 and ih > 0:                   # :1059-1060
                    fm, f = fowt.calcHydroForce_2ndOrd(fowt.beta[ih], fowt._S_dev[ih])
                    fowt.Fhydro_2nd_mean[ih], fowt.Fhydro_2nd[ih] = fm, f
                    fowt._f2nd_w[ih] = fowt._f2nd_dev.to(torch.complex128)
                F = dd.excitation_table()[fowt._heads[ih]] * fowt._zeta_dev[ih][None, :] + Fd
                if fowt._f2nd_w[ih] is not None:
                    F = F + fowt._f2nd_w[ih]
                Fw.append(F)
            Fws.append(Fw)
            fowt._res = res
        nW = self.fowtList[-1].nWaves           # the last FOWT's nWaves
        dev = self.fowtList[0].device_design().device
        Xi = torch.zeros([nW + 1, self.nDOF, self.nw], dtype=torch.complex128, device=dev)
        single = self.nFOWT == 1 and self.K_array is None and self.ms is None
        for ih in range(nW):
            if single and ih == 0:
                Xi[0] = self.fowtList[0]._res["Xi"][0]                 # Zinv F_wave(0) == last solve
            else:
                Xi[ih] = self._system_solve(Zs, [Fw[ih] for Fw in Fws])
            # second-order loads of the other sea states (:1067-1083)
            if ih > 0 and any(f.potSecOrder == 1 for f in self.fowtList):
                for i, fowt in enumerate(self.fowtList):
                    if fowt.potSecOrder != 1:
                        continue
                    z = fowt._zeta_dev[ih]
                    x = Xi[ih, 6 * i:6 * i + 6]
                    rao = torch.where(z.abs() > 1e-6, x / torch.where(z == 0, torch.ones_like(z), z), torch.zeros_like(x))
                    fowt.calcQTF_slenderBody(waveHeadInd=ih, Xi0=rao, verbose=True, iCase=iCase, iWT=i)
                    fm, f = fowt.calcHydroForce_2ndOrd(fowt.beta[ih], fowt._S_dev[ih])
                    fowt.Fhydro_2nd_mean[ih], fowt.Fhydro_2nd[ih] = fm, f
                    Fws[i][ih] = Fws[i][ih] + fowt._f2nd_dev.to(torch.complex128)
                Xi[ih] = self._system_solve(Zs, [Fw[ih] for Fw in Fws])
        self.Xi = Xi.cpu().numpy()
        if np.isnan(self.Xi).any():
            # the array solve stores NaN in the rows of a bin whose elimination met an exactly zero
            # pivot (every fixed point above passed _check_pass, so nothing else leaves NaN here);
            # the reference's solve raises there (raft/raft_model.py:1065)
            raise np.linalg.LinAlgError("Singular matrix")
        self._xi_dev_all = Xi
        for i, fowt in enumerate(self.fowtList):
            xi_i = Xi[:, 6 * i:6 * i + 6, :].contiguous()
            psd = torch.empty([6, self.nw], dtype=torch.float64, device=dev)
            std = torch.empty([6], dtype=torch.float64, device=dev)
            N.check(N.lib().rh_motion_stats(N.context(self.device), 1, nW + 1, self.nw, float(fowt.dw), N.ptr(xi_i),
                                            N.ptr(psd), N.ptr(std), N.stream_handle(torch, dev)), "rh_motion_stats")
            fowt._stats = {"psd": psd.cpu().numpy(), "std": std.cpu().numpy()}
            fowt._xi_dev = xi_i                        # device copy for the derived channels
            fowt.Xi = self.Xi[:, 6 * i:6 * i + 6, :]
        self.results["response"] = {}
        return self.Xi

    @staticmethod
    def _check_pass(res, tol, display):
        """Status handling of one drag fixed point (raft/raft_model.py:954-966)."""
        iters = int(res["iters"].item())
        status = int(res["status"].item())
        if status == N.RH_CASE_NAN:
            raise Exception("Nan detected in response vector Xi.")
        if status == N.RH_CASE_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")
        if display > 1 and status == N.RH_CASE_CONVERGED:
            print(f" Iteration {iters - 1}, converged (< {tol})")
        return status, iters

    def array_stiffness(self):
        """Array-level mooring stiffness added to Z_sys (raft/raft_model.py:1030-1031): the
        K_array override, else the array mooring system's analytic coupled stiffness."""
        if self.K_array is not None:
            return np.asarray(self.K_array, dtype=float)
        if self.ms is not None:
            return self.ms.coupled_stiffness_analytic()
        return None

    def _system_solve(self, Zs, Fs):
        """Z_sys = blockdiag(Z_i) (+ K_array); Xi = Z_sys^-1 F (raft/raft_model.py:1021-1065)."""
        import torch
        dev = Zs[0].device
        nf = len(Zs)
        Z = torch.stack(Zs).contiguous()                  # [nf, nw, 6, 6]
        F = torch.cat(Fs, dim=0).contiguous()             # [6nf, nw]
        K = None
        Ka = self.array_stiffness()
        if Ka is not None:
            K = torch.tensor(Ka, dtype=torch.float64, device=dev).contiguous()
        X = torch.empty([6 * nf, self.nw], dtype=torch.complex128, device=dev)
        N.check(N.lib().rh_system_solve(N.context(self.device), nf, self.nw, N.ptr(Z), N.ptr(K), N.ptr(F), N.ptr(X),
                                        N.stream_handle(torch, dev)), "rh_system_solve")
        return X

    # --------------------------------------------------------------------- statics
    def solveStatics(self, case, display=0):
        """Mean offsets of every FOWT for a load case (raft/raft_model.py:479-790): linear
        hydrostatics about the reference position (statics_mod 0), constant environmental
        loads (forcing_mod 0: mean aero = 0 here, current drag, mean wave drift), nonlinear
        mooring forces, Newton steps on the total stiffness through dsolve2.  Leaves every
        FOWT at its offset pose (setPosition), as the reference does."""
        from .dsolve import dsolve2
        nD = self.nDOF
        K_hs, F_und = [], np.zeros(nD)
        F_env = np.zeros(nD)
        X_init = np.zeros(nD)
        if case and isinstance(case.get("wind_speed"), list) and len(case["wind_speed"]) != len(self.fowtList):
            raise IndexError("List of wind speeds must be the same length as the list of wind turbines")
        for i, fowt in enumerate(self.fowtList):
            X_init[6 * i:6 * i + 6] = [fowt.x_ref, fowt.y_ref, 0, 0, 0, 0]
            fowt.setPosition(X_init[6 * i:6 * i + 6])
            fowt.calcStatics()
            K_hs.append(fowt.C_struc + fowt.C_hydro)
            F_und[6 * i:6 * i + 6] += fowt.W_struc + fowt.W_hydro
            if case:
                ci = self._fowt_case(case, i)
                fowt.calcTurbineConstants(ci, ptfm_pitch=0)
                fowt.calcHydroConstants()
                F_env[6 * i:6 * i + 6] = np.sum(fowt.f_aero0, axis=1) + fowt.calcCurrentLoads(ci)
                if getattr(fowt, "Fhydro_2nd_mean", None) is not None:
                    F_env[6 * i:6 * i + 6] += np.sum(fowt.Fhydro_2nd_mean, axis=0)
        # uniform current on the mooring lines (raft/raft_model.py:561-577): set for this case,
        # cleared otherwise, on the array system and every FOWT's own system
        cur = np.zeros(3)
        if case and self.mooring_currentMod > 0:
            speed = get_from_dict(case, "current_speed", shape=0, default=0.0)
            head = get_from_dict(case, "current_heading", shape=0, default=0)
            if speed > 0:
                cur = np.array([speed * np.cos(np.radians(head)), speed * np.sin(np.radians(head)), 0.0])
        for sysm in [self.ms] + [fowt.ms for fowt in self.fowtList]:
            if sysm is not None:
                sysm.current = cur.copy()
        tols = np.array([0.05, 0.05, 0.05, 0.005, 0.005, 0.005] * len(self.fowtList))

        def eval_func(X, args):
            for i, fowt in enumerate(self.fowtList):
                fowt.setPosition(X[6 * i:6 * i + 6])
            if self.ms is not None:
                self.ms.set_body_positions([X[6 * i:6 * i + 6] for i in range(self.nFOWT)])
            Fnet = np.zeros(nD)
            for i, fowt in enumerate(self.fowtList):
                Xi0 = X[6 * i:6 * i + 6] - np.array([fowt.x_ref, fowt.y_ref, 0, 0, 0, 0])
                Fnet[6 * i:6 * i + 6] += F_und[6 * i:6 * i + 6]
                Fnet[6 * i:6 * i + 6] += -np.matmul(K_hs[i], Xi0)
                if case:
                    Fnet[6 * i:6 * i + 6] += F_env[6 * i:6 * i + 6]
                Fnet[6 * i:6 * i + 6] += fowt.F_moor0
                if self.ms is not None:
                    Fnet[6 * i:6 * i + 6] += self.ms.body_forces(self.ms.bodies[i], lines_only=True)
            return Fnet, dict(status=1), False

        def step_func(X, args, Y, oths, Ytarget, err, tol_, it, maxIter):
            K = np.zeros([nD, nD])
            if self.ms is not None:
                K += self.ms.coupled_stiffness_analytic()
            for i, fowt in enumerate(self.fowtList):
                K6 = K_hs[i].copy()
                if fowt.ms is not None:
                    K6 += fowt.ms.coupled_stiffness_analytic()
                K[6 * i:6 * i + 6, 6 * i:6 * i + 6] += K6
            kmean = np.mean(K.diagonal())
            for i in range(nD):
                if K[i, i] == 0:
                    K[i, i] = kmean
            dX = np.linalg.solve(K, Y)
            for _ in range(10):                       # strengthen the diagonal on a backward step (:738-748)
                if sum(dX * Y) < 0:
                    for i in range(nD):
                        K[i, i] += 0.1 * abs(K[i, i])
                    dX = np.linalg.solve(K, Y)
                else:
                    break
            return dX

        X, Y, info = dsolve2(eval_func, X_init, step_func=step_func, tol=tols, a_max=1.6, maxIter=20,
                             args={"display": display})
        self.Xs2, self.Es2 = info["Xs"], info["Es"]
        if case and "iCase" in case:
            self.results.setdefault("mean_offsets", []).append(self.Xs2[-1])
        if display > 0:
            for i, fowt in enumerate(self.fowtList):
                print(f"Found mean offets of FOWT {i + 1} with surge = {fowt.Xi0[0]: .2f} m,  sway  = "
                      f"{fowt.Xi0[1]: .2f},  and heave = {fowt.Xi0[2]: .2f} m")
        return X

    @staticmethod
    def _fowt_case(case, i):
        """A copy of a case as FOWT i sees it: a per-FOWT wind_speed list reduced to its entry i."""
        ci = dict(case)
        if isinstance(case.get("wind_speed"), list):
            ci["wind_speed"] = case["wind_speed"][i]
        return ci

    def _reference_poses(self):
        """X_ref [nFOWT, 6] of the FOWTs."""
        return np.array([[f.x_ref, f.y_ref, 0, 0, 0, 0] for f in self.fowtList], dtype=float)

    def _array_rotor_loads(self, cases):
        """[FOWT][case] bem arguments: FOWT.rotorLoadsBatch of every FOWT at its current pose, one launch each."""
        return [fowt.rotorLoadsBatch([self._fowt_case(c, i) for c in cases], self.device)
                for i, fowt in enumerate(self.fowtList)]

    def _mean_loads(self, cases, F_und, bems=None, D_cur=None):
        """F_const [n, nFOWT, 6] = F_und [nFOWT, 6] + F_env of every (case, FOWT) at the FOWTs' current
        poses, F_env built as solveStatics builds it: the mean aero loads (bems[FOWT][case]: the rotors'
        loads from the device, else the host evaluates), current drag (D_cur[FOWT][case]: from the device,
        FOWT.currentLoadsBatch, else calcCurrentLoads per case) and the mean wave drift."""
        F_const = np.zeros([len(cases), self.nFOWT, 6])
        for ic, case in enumerate(cases):
            for i, fowt in enumerate(self.fowtList):
                ci = self._fowt_case(case, i)
                fowt.calcTurbineConstants(ci, ptfm_pitch=0, bem=bems[i][ic] if bems else None)
                if D_cur is not None:
                    fowt.D_hydro = D_cur[i][ic].copy()       # (where calcCurrentLoads leaves it)
                else:
                    fowt.calcCurrentLoads(ci)
                F_env = np.sum(fowt.f_aero0, axis=1) + fowt.D_hydro
                if getattr(fowt, "Fhydro_2nd_mean", None) is not None:
                    F_env = F_env + np.sum(fowt.Fhydro_2nd_mean, axis=0)
                F_const[ic, i] = F_und[i] + F_env
        return F_const

    def _line_currents(self, cases):
        """The uniform current on the mooring lines of every case, [n, 3], by solveStatics' rule:
        speed (cos heading, sin heading, 0) with mooring currentMod > 0 and a positive speed, else zero."""
        cur = np.zeros([len(cases), 3])
        if self.mooring_currentMod > 0:
            for i, case in enumerate(cases):
                speed = get_from_dict(case, "current_speed", shape=0, default=0.0)
                head = get_from_dict(case, "current_heading", shape=0, default=0)
                if speed > 0:
                    cur[i] = [speed * np.cos(np.radians(head)), speed * np.sin(np.radians(head)), 0.0]
        return cur

    def _refuse_array_line_current(self, who):
        if self.nFOWT != 1 or self.ms is not None:
            raise NotImplementedError(f"{who}: line_current=True on an array (current on array-level, shared and "
                                      "free-point lines is not on the device: the host model it would restate does "
                                      "not solve the moored-array design in current; DESIGN.md §7)")

    def _statics_batch_inputs(self, cases, F_extra=None, bems=None, current_device=False, line_current=False):
        """The host side of solveStaticsBatch: the device mooring system, X_ref [6], K_hs [6,6],
        F_const [n,6] = W_struc + W_hydro + F_env (+ F_extra) and the line warm state at X_ref.
        line_current: the cases' currents go to the device per case, so a currentMod 1 design is not refused.
        bems: None (the host evaluates the rotors), or a list, filled here after every refusal with the
        rotors' device loads at X_ref (_array_rotor_loads) for the caller that needs them again.
        current_device: the current loads of all cases from one launch (FOWT.currentLoadsBatch at X_ref)."""
        from .mooring_device import DeviceMooring, warm_state
        if line_current:
            self._refuse_array_line_current("solveStaticsBatch")
        if self.nFOWT != 1 or self.ms is not None:
            raise NotImplementedError("solveStaticsBatch: a single FOWT with its own mooring system (arrays and "
                                      "array-level mooring are solved by solveStatics)")
        fowt = self.fowtList[0]
        if fowt.ms is None:
            raise NotImplementedError("solveStaticsBatch: the FOWT has no mooring system")
        if not line_current and self.mooring_currentMod > 0 and any(
                get_from_dict(c, "current_speed", shape=0, default=0.0) > 0 for c in cases):
            raise NotImplementedError("solveStaticsBatch: current on the mooring lines (mooring currentMod 1); pass "
                                      "line_current=True to solve it on the device")
        # the host object carries no current: the device takes it per case (with line_current), and
        # solveStatics clears it for a case without one
        fowt.ms.current = np.zeros(3)
        if getattr(self, "_moor_dev", None) is None or self._moor_dev[0] is not fowt.ms:
            self._moor_dev = (fowt.ms, DeviceMooring([fowt.ms], self.device))
        dm = self._moor_dev[1]
        X_ref = self._reference_poses()[0]
        fowt.setPosition(X_ref)
        fowt.calcStatics()
        K_hs = fowt.C_struc + fowt.C_hydro
        warm0 = warm_state(fowt.ms)                      # the line solutions at the reference pose
        if bems is not None:
            bems[:] = self._array_rotor_loads(cases)
        D_cur = [fowt.currentLoadsBatch([self._fowt_case(c, 0) for c in cases], self.device)] if current_device else None
        F_const = self._mean_loads(cases, [fowt.W_struc + fowt.W_hydro], bems, D_cur)[:, 0]
        if F_extra is not None:
            F_const += np.asarray(F_extra, dtype=float).reshape(len(cases), 6)
        return dm, X_ref, K_hs, F_const, warm0

    def solveStaticsBatch(self, cases, F_extra=None, host=True, rotor_device=False, current_device=False,
                          line_current=False):
        """The mean offsets of many load cases in two device launches (rh_statics_solve, then
        rh_moor_eval at the solved poses): solveStatics' Newton per case, every case's lines in
        adjacent lanes (csrc/rh_moor.hip).  A single FOWT with its own mooring system; F_extra
        [n, 6]: further constant loads per case.  The environmental loads are built on the host
        as solveStatics builds them.  Returns X [n,6], Xi0 [n,6], F_moor [n,6], C_moor [n,6,6],
        Tmoor_avg [n,2L], J_moor [n,2L,6], iters [n] (evaluations: len(Model.Xs2) of the host
        path) and status [n] (0 = converged, else _native.MOOR_STATUS); numpy arrays, or device
        tensors with host=False.  The model is left at its reference pose.  rotor_device=True takes the
        rotors' blade-element loads of all cases from one device launch (FOWT.rotorLoadsBatch) instead of
        one host CCBlade evaluation per case; a case whose rotor solve fails raises RuntimeError.
        current_device=True takes the current loads of all cases from one rh_current_loads launch
        (FOWT.currentLoadsBatch) instead of one calcCurrentLoads per case; the rest of the environmental
        loads is unchanged.
        line_current=True solves a mooring currentMod 1 design: each case's uniform current on the lines
        (solveStatics' rule: speed (cos heading, sin heading, 0) with a positive current_speed, else
        zero) goes into the Newton (rh_statics_solve_current) and into the evaluation at the solved poses
        (rh_moor_eval_current), so F_moor, C_moor, Tmoor_avg and J_moor are those of the host system
        with that case's current still set, as analyzeCases reads them after solveStatics.  Without it
        such a design with a current case raises NotImplementedError; on an array it raises too.
        The defaults change nothing."""
        return self._solve_statics_batch(cases, F_extra, host, [] if rotor_device else None, current_device,
                                         line_current)

    def _solve_statics_batch(self, cases, F_extra, host, bems, current_device=False, line_current=False):
        """solveStaticsBatch with the rotor loads as _statics_batch_inputs takes them."""
        dm, X_ref, K_hs, F_const, warm0 = self._statics_batch_inputs(cases, F_extra, bems, current_device, line_current)
        cur = self._line_currents(cases) if line_current else None
        n = len(cases)
        sol = dm.solve_statics(np.tile(X_ref, (n, 1)), np.tile(K_hs, (n, 1, 1)), F_const, np.tile(warm0, (n, 1, 1)),
                               current=cur)
        ev = dm.eval(sol["X"], warm=sol["warm"], jacobian=True, current=cur)
        torch = dm.torch
        status = torch.maximum(sol["status"], ev["status"])
        out = dict(X=sol["X"], Xi0=sol["X"] - torch.tensor(X_ref, dtype=torch.float64, device=dm.device),
                   F_moor=ev["F"], C_moor=ev["K"], Tmoor_avg=ev["T"], J_moor=ev["J"], iters=sol["iters"], status=status)
        return {k: v.cpu().numpy() for k, v in out.items()} if host else out

    def _statics_array_inputs(self, cases, F_extra=None, bems=None):
        """The host side of solveStaticsArrayBatch: the merged record and one record per system,
        X_ref [N,6], K_hs [N,6,6], F_const [n,N,6] and the state (line warm starts, free
        points) of every system with the FOWTs at their reference poses.  Every refusal is raised
        before the device is touched.  bems: as _statics_batch_inputs takes it."""
        from .mooring_array_device import array_state, flatten_array
        own = [f.ms for f in self.fowtList]
        if self.ms is None and all(s is None for s in own):
            raise NotImplementedError("solveStaticsArrayBatch: the model has no mooring system")
        if self.mooring_currentMod > 0 and any(get_from_dict(c, "current_speed", shape=0, default=0.0) > 0
                                               for c in cases):
            raise NotImplementedError("solveStaticsArrayBatch: current on the mooring lines (mooring currentMod 1)")
        for c in cases:
            if isinstance(c.get("wind_speed"), list) and len(c["wind_speed"]) != len(self.fowtList):
                raise IndexError("List of wind speeds must be the same length as the list of wind turbines")
        for sysm in [self.ms] + own:
            if sysm is not None:
                sysm.current = np.zeros(3)               # as solveStatics clears it for a case without one
        rec = flatten_array(self)                        # (refusals: before any device call)
        if rec.nbody != self.nFOWT:
            raise NotImplementedError("solveStaticsArrayBatch: the last FOWT has no mooring line")
        subs = [rec] if len(rec.systems) == 1 else [rec] + [flatten_array([(ms, range(len(ms.bodies)))])
                                                            for ms, _ in rec.systems]
        nf, n = self.nFOWT, len(cases)
        X_ref = self._reference_poses()
        K_hs, F_und = np.zeros([nf, 6, 6]), np.zeros([nf, 6])
        for i, fowt in enumerate(self.fowtList):
            fowt.setPosition(X_ref[i])
            fowt.calcStatics()
            K_hs[i] = fowt.C_struc + fowt.C_hydro
            F_und[i] = fowt.W_struc + fowt.W_hydro
        if self.ms is not None:
            self.ms.set_body_positions(list(X_ref))
        warm0, free0 = array_state(rec)                  # the state at the reference poses, read once
        if bems is not None:
            bems[:] = self._array_rotor_loads(cases)
        F_const = self._mean_loads(cases, F_und, bems)
        if n:
            # the members' added mass at the reference pose, as solveStatics leaves it (once per FOWT: it
            # reads the pose alone, and neither the turbine constants nor the current loads read its results)
            for fowt in self.fowtList:
                fowt.calcHydroConstants()
        if F_extra is not None:
            F_const += np.asarray(F_extra, dtype=float).reshape(n, nf, 6)
        return rec, subs, X_ref, K_hs, F_const, warm0, free0

    def solveStaticsArrayBatch(self, cases, F_extra=None, host=True, rotor_device=False):
        """The mean offsets of many load cases of N >= 1 FOWTs moored by the array-level system and / or
        their own systems, in two device launches (rh_array_statics_solve on the merged record, then
        rh_moor_array_eval of every system at the solved poses): Model.solveStatics' Newton per case
        with the free points' equilibrium inside every evaluation (csrc/rh_moor_array.hip).  Every case
        starts from the state of the model at its reference poses (line warm starts and free points
        read once, after moving the FOWTs there and re-solving), so a case's result is solveStatics'
        on a freshly built model.  F_extra [n, 6N]: further constant loads.  Returns X [n,6N], Xi0,
        F_moor [n,6N], K_array [n,6N,6N] (the array system's share), C_moor / F_moor0 (per FOWT: its
        own system's [n,6,6] / [n,6], or None), Tmoor_avg [n,2L] and J_moor [n,2L,6N] of the array
        system (None without one), Tmoor_avg_own / J_moor_own (per FOWT, [n,2Li] / [n,2Li,6] or None),
        iters [n] (evaluations: len(Model.Xs2) of the host path), status [n] (0 = converged, else
        _native.MOOR_STATUS); numpy arrays, or device tensors with host=False.  The model is left at
        its reference pose.  rotor_device: as solveStaticsBatch, one launch per FOWT."""
        return self._solve_statics_array_batch(cases, F_extra, host, [] if rotor_device else None)

    def _solve_statics_array_batch(self, cases, F_extra, host, bems):
        """solveStaticsArrayBatch with the rotor loads as _statics_batch_inputs takes them."""
        from .mooring_array_device import DeviceArrayMooring
        rec, subs, X_ref, K_hs, F_const, warm0, free0 = self._statics_array_inputs(cases, F_extra, bems)
        # the device records are kept between calls while the freshly flattened tables equal theirs
        dm = getattr(self, "_moor_arr_dev", None)
        if dm is None or dm.dev_index != self.device or not dm.same_tables(subs):
            dm = self._moor_arr_dev = DeviceArrayMooring(subs, self.device)
        torch = dm.torch
        n, nf = len(cases), self.nFOWT
        nb, nl, nfp = dm.nb, dm.nl, dm.nf
        f64 = dict(dtype=torch.float64, device=dm.device)

        def padded(a, rows, width):
            out = np.zeros([rows, width])
            out[:a.shape[0]] = a
            return out
        rep = lambda a: np.tile(a, (n,) + (1,) * a.ndim)   # noqa: E731
        sol = dm.solve_statics(rep(padded(X_ref, nb, 6)), rep(np.concatenate([K_hs, np.zeros([nb - nf, 6, 6])])),
                               np.concatenate([F_const, np.zeros([n, nb - nf, 6])], axis=1), rep(padded(warm0, nl, 2)),
                               rep(padded(free0, nfp, 3)), sys_idx=np.zeros(n, dtype=np.int32))
        X = sol["X"][:, :6 * nf]
        # every system at the solved poses: its share of force and stiffness, its tensions and their Jacobian
        ns = len(rec.systems)
        first = 0 if ns == 1 else 1
        r6 = torch.zeros([ns, n, nb, 6], **f64)
        wm = torch.zeros([ns, n, nl, 2], **f64)
        fr = torch.zeros([ns, n, nfp, 3], **f64)
        for k, (ms, bodies) in enumerate(rec.systems):
            for j, b in enumerate(bodies):
                r6[k, :, j] = X[:, 6 * b:6 * b + 6]
            rows = torch.tensor(rec.lines_of(k), dtype=torch.long, device=dm.device)
            wm[k, :, :len(rows)] = sol["warm"][:, rows]
            if k == rec.free_sys:
                fr[k, :, :rec.nfree] = sol["free"][:, :rec.nfree]
        ev = dm.eval(r6.view(ns * n, nb, 6), wm.view(ns * n, nl, 2), fr.view(ns * n, nfp, 3),
                     sys_idx=np.repeat(np.arange(first, first + ns, dtype=np.int32), n), jacobian=True)
        Fk, Kk = ev["F"].view(ns, n, 6 * nb), ev["K"].view(ns, n, 6 * nb, 6 * nb)
        Tk, Jk = ev["T"].view(ns, n, 2 * nl), ev["J"].view(ns, n, 2 * nl, 6 * nb)
        status = torch.maximum(sol["status"], ev["status"].view(ns, n).max(dim=0).values)
        F_moor = torch.zeros([n, 6 * nf], **f64)
        out = dict(X=X.contiguous(), K_array=torch.zeros([n, 6 * nf, 6 * nf], **f64), C_moor=[None] * nf,
                   F_moor0=[None] * nf, Tmoor_avg=None, J_moor=None, Tmoor_avg_own=[None] * nf, J_moor_own=[None] * nf)
        for k, (ms, bodies) in enumerate(rec.systems):
            L = len(ms.lines)
            cols = list(range(L)) + list(range(nl, nl + L))
            dof = [6 * j + d for j in range(len(bodies)) for d in range(6)]
            T, J = Tk[k][:, cols].contiguous(), Jk[k][:, cols][:, :, dof].contiguous()
            for j, b in enumerate(bodies):
                F_moor[:, 6 * b:6 * b + 6] += Fk[k][:, 6 * j:6 * j + 6]
            if ms is self.ms:
                out["K_array"] = Kk[k][:, :6 * nf, :6 * nf].contiguous()
                out["Tmoor_avg"], out["J_moor"] = T, J
            else:
                i = bodies[0]
                out["C_moor"][i], out["F_moor0"][i] = Kk[k][:, :6, :6].contiguous(), Fk[k][:, :6].contiguous()
                out["Tmoor_avg_own"][i], out["J_moor_own"][i] = T, J
        out.update(Xi0=out["X"] - torch.tensor(X_ref.reshape(-1), **f64), F_moor=F_moor, iters=sol["iters"], status=status,
                   free=sol["free"])
        if not host:
            return out
        cpu = lambda v: None if v is None else v.cpu().numpy()   # noqa: E731
        return {k: [cpu(x) for x in v] if isinstance(v, list) else cpu(v) for k, v in out.items()}

    # the steps analyzeCasesBatch(statics=True) and analyzeArrayBatch(statics=True) share
    def _refuse_pose_analysis(self, who, cases, pose_chunk):
        """What `who`(statics=True) refuses, before the device is touched.  Returns the cases' sea states."""
        array = who == "analyzeArrayBatch"
        if any(f.potSecOrder > 0 for f in self.fowtList):
            raise NotImplementedError(f"{who}(statics=True): potSecOrder > 0 (the reference solves the "
                                      "statics twice around the dynamics, raft/raft_model.py:301-318)")
        if (array and self.K_array is not None) or any("C_moor" in (f._statics or {}) for f in self.fowtList):
            raise NotImplementedError(f"{who}(statics=True): the mooring stiffness was given as a fixture "
                                      f"({'K_array, or ' if array else ''}setStatics with a C_moor): there is no system "
                                      "to solve")
        if int(pose_chunk) < 1:
            raise ValueError("pose_chunk must be >= 1")
        seas = [self._case_sea_states(c) for c in cases]
        if any(len(s[0]) > 1 for s in seas):
            raise NotImplementedError(f"{who}(statics=True): several sea states per case")
        return seas

    @staticmethod
    def _design_at_pose(fowt, case, X_ref, X, bem, moor, headings):
        """The DeviceDesign of one (case, FOWT) at its solved pose X, with `headings` [deg] tabulated:
        the FOWT is moved there exactly as solveStatics leaves it, turbine and hydro constants at the
        reference pose, members and rotors at the offset pose, and C_moor and F_moor0 of its own
        mooring system from the device (moor; None without one)."""
        fowt.setPosition(X_ref)
        fowt.calcTurbineConstants(case, ptfm_pitch=0, bem=bem)
        fowt.calcHydroConstants()
        fowt.setPosition(X)
        if moor is not None:
            fowt.C_moor, fowt.F_moor0 = moor[0].copy(), moor[1].copy()
        fowt._dd = fowt._host = None
        dd = fowt.device_design()
        dd.ensure_headings(np.asarray(headings, dtype=float) * DEG2RAD)
        return dd

    def _restore_reference_poses(self, X_ref):
        """Every FOWT back at its reference pose, the design of its last solved pose dropped."""
        for fowt, x in zip(self.fowtList, X_ref):
            fowt.setPosition(x)
            fowt._dd = fowt._host = None

    def _tension_channels(self, J, Xi):
        """Tmoor_PSD [n, 2L, nw] and Tmoor_std [n, 2L] of mooring_outputs: the tension amplitudes J Xi,
        the PSD over w[0] as the reference has it."""
        import torch
        a2 = torch.matmul(J, Xi.real.contiguous()) ** 2 + torch.matmul(J, Xi.imag.contiguous()) ** 2   # [n, 2L, nw]
        return 0.5 * a2 / float(self.w[0]), torch.sqrt(0.5 * a2.sum(dim=2))

    def _pose_device_chunks(self, fowt, cases, seas, sb, bems, tol, want, pose_chunk):
        """The drag fixed points of analyzeCasesBatch(statics=True, pose_device=True): every chunk of
        pose_chunk cases through PoseRecord.designs (the poses' node and member tables and wave tables
        from two launches) and one solve_batch.  The FOWT stays at its reference pose, where the turbine
        and hydro constants are taken; cases without an operating rotor share one M and B, a case with
        one gets its own per-bin pair (CaseMB.of_case's) from the host."""
        import torch
        from .pose_device import pose_record
        from .prep import linear_matrices
        n = len(cases)
        dev = sb["X"].device
        f64 = dict(dtype=torch.float64, device=dev)
        X_ref = self._reference_poses()[0]
        if n:      # the aero-free design
            fowt.calcTurbineConstants(dict(self._fowt_case(cases[0], 0), wind_speed=0.0), ptfm_pitch=0)
        fowt.calcHydroConstants()
        rec = pose_record(fowt, self.device)

        def mb_of():
            M, B, _, per_bin = linear_matrices(fowt)
            return torch.tensor(M, **f64).contiguous(), torch.tensor(B, **f64).contiguous(), per_bin
        shared = mb_of()
        # C_lin of every case: prep.linear_matrices' (C_struc + C_moor) + C_hydro with the case's own C_moor
        C = ((torch.tensor(fowt.C_struc, **f64) + sb["C_moor"]) + torch.tensor(fowt.C_hydro, **f64)).contiguous()
        parts = []
        for c0 in range(0, n, int(pose_chunk)):
            ids = list(range(c0, min(n, c0 + int(pose_chunk))))
            rows = []
            for i in ids:
                ci = self._fowt_case(cases[i], 0)
                if any(fowt._rotor_operates(ir, ci) for ir in range(fowt.nrotors)):
                    # the rotors' part of setPosition(X_ref), as the per-case path runs it ahead of the turbine
                    # constants: the hub offsets follow the yaw the previous evaluation left (Rotor.setYaw)
                    for rot in fowt.rnaList:
                        rot.setPosition(X_ref)
                    fowt.calcTurbineConstants(dict(ci), ptfm_pitch=0, bem=bems[0][i] if bems else None)
                    rows.append(mb_of())
                else:
                    rows.append(shared)
            hd, sp, Hs, Tp, gm = ([seas[i][k][0] for i in ids] for k in range(5))
            blk = rec.designs(sb["X"][ids[0]:ids[-1] + 1], C[ids[0]:ids[-1] + 1], rows,
                              np.asarray(hd, dtype=float) * DEG2RAD, self.nIter, self.XiStart)
            cs = CaseSet(np.arange(len(ids), dtype=np.int32), hd, sp, Hs, Tp, gm)
            res = solve_batch(blk, cs, self.nIter, self.XiStart, tol, want=tuple(want), prepared=rec.case_columns(cs))
            parts.append({k: v.clone() for k, v in res.items()})
            torch.cuda.synchronize(dev)                  # the chunk's tables are released below
            del res, blk
        if n:      # the turbine constants of the last case and the rotors at X_ref, as the per-case path leaves them
            if rows[-1] is shared:
                fowt.calcTurbineConstants(dict(self._fowt_case(cases[-1], 0)), ptfm_pitch=0)
            for rot in fowt.rnaList:
                rot.setPosition(X_ref)
        fowt._dd = fowt._host = None
        return parts

    def _analyze_cases_statics(self, cases, tol, want, host, pose_chunk, rotor_device=False, pose_device=False,
                               line_current=False):
        """analyzeCasesBatch(statics=True): every case at its own mean-offset pose, as
        analyzeCases solves it when the mooring is a system.  Offsets, C_moor and the tension
        Jacobian of every case come from solveStaticsBatch; each case then gets its own
        DeviceDesign (the FOWT moved to its pose exactly as solveStatics leaves it: turbine and
        hydro constants at the reference pose, members and rotors at the offset pose, C_moor from
        the device), and the drag fixed points run in chunks of pose_chunk views.  pose_device: the
        current loads of the statics and every chunk's designs from the device (_pose_device_chunks).
        line_current: the statics with each case's current on the mooring lines (solveStaticsBatch's)."""
        import torch
        if line_current:
            self._refuse_array_line_current("analyzeCasesBatch(statics=True)")
        if self.nFOWT != 1 or self.ms is not None:
            raise NotImplementedError("analyzeCasesBatch(statics=True): arrays (their statics couple the FOWTs; "
                                      "use analyzeCases)")
        fowt = self.fowtList[0]
        if pose_device:
            from .pose_device import MCF_REFUSAL, host_record
            if any(mem.MCF for mem in fowt.memberList):
                raise NotImplementedError("analyzeCasesBatch(pose_device=True): " + MCF_REFUSAL)
            if fowt.bem_excitation():
                raise NotImplementedError("analyzeCasesBatch(pose_device=True): a design with BEM excitation (its "
                                          "potential-flow tables are tabulated per design; use pose_device=False)")
            host_record(fowt)                            # (the kernels' member and node limits)
        seas = self._refuse_pose_analysis("analyzeCasesBatch", cases, pose_chunk)
        self._calc_bem_once()
        # (the rotor loads are those of the reference pose, where _design_at_pose takes the turbine constants)
        bems = [] if rotor_device else None
        sb = self._solve_statics_batch(cases, None, False, bems, current_device=pose_device,
                                       line_current=line_current)
        if pose_device:
            parts = self._pose_device_chunks(fowt, cases, seas, sb, bems, tol, want, pose_chunk)
            return self._pose_results(cases, sb, parts, host)
        X = sb["X"].cpu().numpy()
        C = sb["C_moor"].cpu().numpy()
        Fm = sb["F_moor"].cpu().numpy()
        X_ref = self._reference_poses()
        n = len(cases)
        parts = []
        for c0 in range(0, n, int(pose_chunk)):
            ids = range(c0, min(n, c0 + int(pose_chunk)))
            views = [self._design_at_pose(fowt, self._fowt_case(cases[i], 0), X_ref[0], X[i], bems[0][i] if bems else None,
                                          (C[i], Fm[i]), seas[i][0]) for i in ids]
            hd, sp, Hs, Tp, gm = ([seas[i][k][0] for i in ids] for k in range(5))
            cs = CaseSet(np.arange(len(views), dtype=np.int32), hd, sp, Hs, Tp, gm)
            res = solve_batch(views, cs, self.nIter, self.XiStart, tol, want=tuple(want))
            parts.append({k: v.clone() for k, v in res.items()})
            torch.cuda.synchronize(views[0].device)      # the chunk's tables are released below
            del res, views
        self._restore_reference_poses(X_ref)
        return self._pose_results(cases, sb, parts, host)

    def _pose_results(self, cases, sb, parts, host):
        """The result of analyzeCasesBatch(statics=True) from the chunks' solves and the statics."""
        import torch
        n = len(cases)
        res = BatchResult({k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]} if parts else {})
        if n:
            res["Tmoor_PSD"], res["Tmoor_std"] = self._tension_channels(sb["J_moor"], res["Xi"])
            res["Tmoor_avg"] = sb["Tmoor_avg"]
            res["mean_offsets"] = sb["X"]
            res["statics_iters"] = sb["iters"]
            res["statics_status"] = sb["status"]
        return res.host() if host else res

    def solveEigen(self, display=0):
        """Natural frequencies [Hz] and mode shapes of the moored system
        (raft/raft_model.py:391-476): M = M_struc + A_hydro_morison, C = C_struc + C_hydro +
        C_moor (+ yaw stiffness, + array mooring).  Host LAPACK on a 6N x 6N pencil."""
        nD = self.nDOF
        M_tot = np.zeros([nD, nD])
        C_tot = np.zeros([nD, nD])
        for i, fowt in enumerate(self.fowtList):
            i1, i2 = 6 * i, 6 * i + 6
            M_tot[i1:i2, i1:i2] += fowt.M_struc + fowt.A_hydro_morison
            C_tot[i1:i2, i1:i2] += fowt.C_struc + fowt.C_hydro + fowt.C_moor
            C_tot[i1 + 5, i1 + 5] += fowt.yawstiff
        if self.ms is not None:
            C_tot += self.ms.coupled_stiffness_analytic()
        message = ""
        for i in range(nD):
            if M_tot[i, i] < 1.0:
                message += f"Diagonal entry {i} of system mass matrix is less than 1 ({M_tot[i, i]}). "
            if C_tot[i, i] < 1.0:
                message += f"Diagonal entry {i} of system stiffness matrix is less than 1 ({C_tot[i, i]}). "
        if message:
            raise RuntimeError("System matrices computed by RAFT have one or more small or negative diagonals: "
                               + message)
        eigenvals, eigenvectors = np.linalg.eig(np.linalg.solve(M_tot, C_tot))
        if any(eigenvals <= 0.0):
            raise RuntimeError("Error: zero or negative system eigenvalues detected.")
        ind_list = []
        for i in range(nD - 1, -1, -1):              # DOF order by the largest mode component (:442-456)
            vec = np.abs(eigenvectors[i, :])
            for _ in range(nD):
                ind = np.argmax(vec)
                if ind in ind_list:
                    vec[ind] = 0.0
                else:
                    ind_list.append(ind)
                    break
        ind_list.reverse()
        fns = np.sqrt(eigenvals[ind_list]) / 2.0 / np.pi
        modes = eigenvectors[:, ind_list]
        if display > 0:
            print("Fn (Hz)" + "".join([f"{fn:10.4f}" for fn in fns]))
        self.results["eigen"] = {"frequencies": fns, "modes": modes}
        return fns, modes

    def analyzeUnloaded(self, ballast=0, heave_tol=1):
        """Unloaded equilibrium and mooring properties (raft/raft_model.py:184-241)."""
        if len(self.fowtList) > 1:
            raise Exception("analyzeUnloaded is an old method that only works for a single FOWT.")
        if ballast:
            raise NotImplementedError("ballast adjustment (raft/raft_model.py:1434-1625) is outside the accelerated path")
        f0 = self.fowtList[0]
        f0.setPosition(np.zeros(6))
        f0.D_hydr0 = np.zeros(6)
        f0.f_aero0 = np.zeros([6, f0.nrotors])
        self.C_moor0 = np.zeros([6, 6])
        self.F_moor0 = np.zeros(6)
        for ms in (self.ms, f0.ms):
            if ms is not None:
                self.C_moor0 += ms.coupled_stiffness_fd()
                self.F_moor0 += ms.coupled_forces(lines_only=True)
        for fowt in self.fowtList:
            fowt.calcStatics()
            fowt.calcHydroConstants()
        self.results["properties"] = {}
        self.solveStatics(None)
        self.results["properties"]["offset_unloaded"] = self.fowtList[0].Xi0

    def calcOutputs(self):
        """System property outputs of the first FOWT (raft/raft_model.py:1150-1189)."""
        fowt = self.fowtList[0]
        if "properties" in self.results:
            C0 = getattr(self, "C_moor0", np.zeros([6, 6]))
            P = self.results["properties"]
            P["tower mass"] = fowt.mtower
            P["tower CG"] = fowt.rCG_tow
            P["substructure mass"] = fowt.m_sub
            P["substructure CG"] = fowt.rCG_sub
            P["shell mass"] = fowt.m_shell
            P["ballast mass"] = fowt.m_ballast
            P["ballast densities"] = fowt.pb
            P["total mass"] = fowt.M_struc[0, 0]
            P["total CG"] = fowt.rCG
            P["roll inertia at subCG"] = fowt.props["Ixx_sub"]
            P["pitch inertia at subCG"] = fowt.props["Iyy_sub"]
            P["yaw inertia at subCG"] = fowt.props["Izz_sub"]
            P["buoyancy (pgV)"] = fowt.rho_water * fowt.g * fowt.V
            P["center of buoyancy"] = fowt.rCB
            P["C hydrostatic"] = fowt.C_hydro
            P["C system"] = fowt.C_struc + fowt.C_hydro + C0
            P["F_lines0"] = getattr(self, "F_moor0", np.zeros(6))
            P["C_lines0"] = C0
            P["M support structure"] = fowt.M_struc_sub
            P["A support structure"] = fowt.A_hydro_morison + fowt.A_BEM[:, :, -1]
            P["C support structure"] = fowt.C_struc_sub + fowt.C_hydro + C0
        return self.results

    # --------------------------------------------------------------------- cases
    def analyzeCases(self, display=0, meshDir=None, RAO_plot=False):
        """raft/raft_model.py:244-388: per case, mean offsets (solveStatics), the response
        solve on the device, and the output channels of every FOWT (plus array-level mooring
        tensions).  When every FOWT's mooring stiffness was given as a fixture (setStatics with a
        C_moor, e.g. the reference-run goldens), the platforms stay at their reference position."""
        nCases = len(self.design["cases"]["data"])
        self.results["properties"] = {}
        self.results["case_metrics"] = {}
        self.results["mean_offsets"] = []
        for fowt in self.fowtList:
            fowt.setPosition([fowt.x_ref, fowt.y_ref, 0, 0, 0, 0])
            fowt.calcStatics()
            fowt.calcBEM(meshDir=meshDir)          # :258-263 (coefficient files only: no BEM solver run)
        for iCase in range(nCases):
            if display > 0:
                print(f"\n--------------------- Running Case {iCase + 1} ----------------------")
                print(self.design["cases"]["data"][iCase])
            case = dict(zip(self.design["cases"]["keys"], self.design["cases"]["data"][iCase]))
            case["iCase"] = iCase
            nWaves = 1 if np.isscalar(case["wave_heading"]) else len(case["wave_heading"])
            self.results["case_metrics"][iCase] = {}
            fixture = all("C_moor" in (f._statics or {}) for f in self.fowtList)
            if fixture:       # mooring given as a stiffness fixture (setStatics): positions held at the reference
                for fowt in self.fowtList:
                    fowt.calcTurbineConstants(case, ptfm_pitch=0)
                    fowt.calcHydroConstants()
            else:
                self.solveStatics(case, display=display)
            self.solveDynamics(case, RAO_plot=RAO_plot, display=display)
            if any(f.potSecOrder > 0 for f in self.fowtList):
                if not fixture:
                    self.solveStatics(case)
                for fowt in self.fowtList:
                    fowt.Fhydro_2nd_mean *= 0
            for i, fowt in enumerate(self.fowtList):
                self.results["case_metrics"][iCase][i] = {}
                fowt.saveTurbineOutputs(self.results["case_metrics"][iCase][i], case)
            if self.ms is not None:
                self.results["case_metrics"][iCase]["array_mooring"] = mooring_outputs(
                    self.ms, self._xi_dev_all, self.w, self.device, nWaves + 1)
        return self.results

    def analyzeCasesBatch(self, cases, tol=0.01, want=("psd", "std", "zeta", "B_drag"), host=True, statics=False,
                          pose_chunk=32, rotor_device=False, aero_device=False, channels=False, pose_device=False,
                          line_current=False):
        """Solve many cases in one device call (one workgroup per case's drag fixed point).
        cases: list of case dicts (wave_heading/spectrum/period/height/gamma, each a scalar or
        one entry per sea state; with wind_speed > 0 on an operating rotor, that case's
        aero-servo M and B from calcTurbineConstants).  Returns a dict of arrays: Xi [n,6,nw]
        (the first sea state), iters, status, psd [n,6,nw], std [n,6], ...
        A case with several sea states is solved as Model.solveDynamics solves it
        (raft/raft_model.py:918-1065): the drag linearisation from its first sea state, then the
        response to each sea state with that linearisation frozen (one rh_heading_response launch
        for every extra sea state of the batch); Xi_waves [n, nW+1, 6, nw] holds them in the
        reference's layout (nW = the batch's largest sea-state count, rows of absent sea states
        and the last row zero) and psd / std sum over the sea states (getPSD / getRMS).
        Second-order loads (raft/raft_model.py:899-1083) as solveDynamics applies them
        (raft/second_order.py): potSecOrder=2 adds the .12d QTF's force of every sea state
        (f2nd_mean [n,6] of sea state 0, f2nd_mean_waves [n,nW,6] with several sea states);
        potSecOrder=1 solves twice, the QTF of each converged case's RAO between the passes
        (iters_pair [n,2]); several sea states per case raise the reference's IndexError (Q8).
        Arrays (nFOWT > 1) go through analyzeArrayBatch: Xi [n,6N,nw], iters [n,N], ...
        statics=True solves every case at its own mean-offset pose with that pose's mooring stiffness,
        as analyzeCases does when the mooring is a system: the offsets of all cases from
        solveStaticsBatch (two device launches), then the drag fixed points in chunks of pose_chunk
        per-case designs.  Added keys: mean_offsets [n,6], Tmoor_avg [n,2L], Tmoor_std [n,2L],
        Tmoor_PSD [n,2L,nw] (mooring_outputs' channels), statics_iters, statics_status.  One sea state
        per case; arrays, potSecOrder > 0 and a C_moor fixture raise NotImplementedError.
        statics=False (the default) holds the platform at its reference position.
        rotor_device=True takes the blade-element loads of every case with an operating rotor from one
        device launch (FOWT.rotorLoadsBatch) ahead of the per-case loop instead of one host CCBlade
        evaluation per case; a case whose rotor solve fails raises RuntimeError.  The default changes
        nothing.
        aero_device=True (single FOWT, statics=False) also forms every wind case's per-bin M and B on
        the device (FOWT.aeroMBBatch: the rotor launch and one rh_rotor_aero_mb launch on the same
        stream; it implies the device rotor solve): no per-case host arithmetic over bins and no
        per-case upload, each such case's design a view of one row of two [n_wind, nw, 6, 6] tensors.
        The result gains f_aero0 [n, 6], the mean aero load about the platform reference point (zeros
        for a case without aero).  The wind excitation and the Kaimal spectrum are not computed (the
        solve reads neither), and the FOWT's host attributes A_aero, B_aero, f_aero and B_gyro stay as
        the aero-free design sets them: all zeros.  With statics=True and on an array it raises
        NotImplementedError.  The default changes nothing.
        channels=True (single FOWT, statics=False) adds the turbine output channels saveTurbineOutputs
        leaves in case_metrics, from one rh_turbine_channels launch after the solve on its stream
        (FOWT.turbineChannelsBatch): AxRNA_ and Mbase_ avg / std / max / min [n, nrot] and PSD
        [n, nw, nrot], omega_ avg / std / max / min / PSD, torque_ and bPitch_ avg / std / PSD,
        power_avg and wind_PSD [n, nw], over every sea state of a case.  A batch with an operating
        rotor needs aero_device=True (the pair tensors live on the device only there); with
        statics=True and on an array it raises NotImplementedError.  The default changes nothing.
        pose_device=True (single FOWT, with statics=True) keeps the per-case design work of statics=True on
        the device: the statics take the current loads of all cases from one rh_current_loads launch
        (solveStaticsBatch's current_device), and every chunk of pose_chunk cases gets its node and member
        tables at the cases' poses from one rh_pose_designs launch and its wave tables from one
        rh_wave_tables_batch launch (raft/pose_device.py), so no FOWT is moved, no design uploaded and no
        table launched per case.  Same result keys; the model stays at its reference pose.  Without
        statics=True it raises ValueError; arrays, MacCamy-Fuchs members and designs with BEM excitation
        raise NotImplementedError.  The default changes nothing.
        line_current=True (single FOWT, with statics=True) solves a mooring currentMod 1 design with each
        case's uniform current on the mooring lines (solveStaticsBatch's line_current): offsets, C_moor,
        F_moor0, Tmoor_avg and the tension Jacobian are those of the host system with the case's current
        set, as analyzeCases has them.  It composes with rotor_device and pose_device.  Without it a
        currentMod > 0 design with a current case raises NotImplementedError; without statics=True it
        raises ValueError, on an array NotImplementedError.  The default changes nothing."""
        if line_current and not statics:
            raise ValueError("analyzeCasesBatch: line_current=True needs statics=True (without it no mooring system "
                             "is solved: the platform is held at its reference position)")
        if pose_device and not statics:
            raise ValueError("analyzeCasesBatch: pose_device=True needs statics=True (without it every case is solved "
                             "at the reference pose and there is no per-case design)")
        if channels and statics:
            raise NotImplementedError("analyzeCasesBatch: channels=True with statics=True (the per-pose path keeps no "
                                      "pair tensors on the device; use saveTurbineOutputs per case there)")
        if channels and self.nFOWT != 1:
            raise NotImplementedError("analyzeCasesBatch: channels=True on an array (analyzeArrayBatch forms no "
                                      "turbine channels)")
        if aero_device and statics:
            raise NotImplementedError("analyzeCasesBatch: aero_device=True with statics=True (the per-pose path "
                                      "rebuilds a design per case; use rotor_device=True there)")
        if aero_device and self.nFOWT != 1:
            raise NotImplementedError("analyzeCasesBatch: aero_device=True on an array (analyzeArrayBatch without "
                                      "statics does not evaluate rotors)")
        if statics:
            return self._analyze_cases_statics(cases, tol, want, host, pose_chunk, rotor_device, pose_device,
                                               line_current)
        if self.nFOWT != 1:
            return self.analyzeArrayBatch(cases, tol=tol, host=host, rotor_device=rotor_device)
        fowt = self.fowtList[0]
        self._calc_bem_once()
        seas = [self._case_sea_states(c) for c in cases]
        nws = np.array([len(s[0]) for s in seas], dtype=np.int64)
        if fowt.potSecOrder == 1 and len(cases) and nws.max() > 1:
            raise qtf_index_error(1)      # the slender-body QTF of sea state 1
        hd, sp, Hs, Tp, gm = ([s[k][0] for s in seas] for k in range(5))
        multi = len(cases) > 0 and nws.max() > 1
        want_fp = tuple(want) + (("Bmat", "B_drag") if multi else ())
        sel = [i for i, c in enumerate(cases) if self._operating_rotor(fowt, c)]
        if channels and sel and not aero_device:
            raise NotImplementedError("analyzeCasesBatch: channels=True on a batch with an operating rotor needs "
                                      "aero_device=True (the rotor loads and parameter rows the channels read are kept "
                                      "on the device only there)")
        if multi:  # every heading tabulated before the fixed point (its tables stay put)
            fowt.device_design().ensure_headings(np.concatenate([np.asarray(s[0], dtype=float) for s in seas]) * DEG2RAD)
        if sel:     # (a batch without an operating rotor leaves the turbine constants as they are)
            fowt.calcTurbineConstants(dict(cases[0], wind_speed=0.0), ptfm_pitch=0)     # the aero-free design
        base = fowt.device_design()
        views, idx = [base], np.zeros(len(cases), dtype=np.int32)
        mb = None
        if sel:
            # operating rotors: each such case gets its own per-bin M and B (its rotors' aero-servo
            # added mass and damping, FOWT.calcTurbineConstants) on the shared node and wave tables
            base.ensure_headings(np.unique(np.asarray(hd, dtype=float)) * DEG2RAD)
            if aero_device:      # every wind case's M and B from two launches; its CaseMB views a row of them
                mb = fowt.aeroMBBatch([dict(cases[i]) for i in sel], base, self.device)
                if mb is not None:
                    for row, i in enumerate(sel):
                        views.append(CaseMB(base, mb["M"][row], mb["B"][row]))
                        idx[i] = len(views) - 1
            else:
                bems = dict(zip(sel, fowt.rotorLoadsBatch([dict(cases[i]) for i in sel], self.device))) \
                    if rotor_device else {}
                for i in sel:
                    views.append(CaseMB.of_case(fowt, base, cases[i], bems.get(i)))
                    idx[i] = len(views) - 1
        cs = CaseSet(idx, hd, sp, Hs, Tp, gm)
        res = solve_batch_2nd(views, [fowt] * len(views), cs, self.nIter, self.XiStart, tol, want=want_fp)
        if multi:
            self._extra_sea_states(res, views, idx, seas, nws, want)
        if aero_device:
            import torch
            f0 = torch.zeros([len(cases), 6], dtype=torch.float64, device=base.device)
            if mb is not None:
                f0[torch.tensor(sel, dtype=torch.long, device=base.device)] = mb["f_aero0"]
            res["f_aero0"] = f0
        if channels:
            res.update(fowt.turbineChannelsBatch(cases, res["Xi_waves"] if multi else res["Xi"], mb, self.device,
                                                 case_rows=sel))
        return res.host() if host else res

    def _calc_bem_once(self):
        """FOWT.calcBEM as analyzeCases calls it (raft/raft_model.py:258-263), for the batched entry
        points: potModMaster 3 reads the coefficient files with sorted headings (once per FOWT and
        pose of the tables: the files do not change), configurations that need a BEM solver run raise."""
        for fowt in self.fowtList:
            if fowt._bem_solver_needed() or (fowt.potModMaster == 3 and not getattr(fowt, "_bem_sorted", False)):
                fowt.calcBEM()
                fowt._bem_sorted = True

    @staticmethod
    def _case_sea_states(case):
        """The sea states of one case dict, read as FOWT.calcHydroExcitation reads them
        (raft/raft_fowt.py:982-1014): (heading [deg], spectrum, Hs, Tp, gamma), one entry each
        per sea state."""
        c = dict(case)
        hd = c.get("wave_heading", 0)
        nW = 1 if np.isscalar(hd) else len(hd)
        col = lambda k, **kw: list(np.atleast_1d(get_from_dict(c, k, shape=nW, **kw)))   # noqa: E731
        sp = [str(x) for x in col("wave_spectrum", dtype=str, default="JONSWAP")]
        for x in sp:
            if x not in N.SPECTRUM_CODES:
                raise ValueError(f"Wave spectrum input '{x}' not recognized.")
        return ([float(x) for x in col("wave_heading", dtype=float, default=0)], sp,
                [float(x) for x in col("wave_height", dtype=float)], [float(x) for x in col("wave_period", dtype=float)],
                [float(x) for x in col("wave_gamma", dtype=float, default=0)])

    def _extra_sea_states(self, res, views, idx, seas, nws, want):
        """The response of every case's further sea states with its drag linearisation frozen
        (raft/raft_model.py:1049-1065): their spectra (rh_sea_state), one rh_heading_response
        launch for all of them, Xi_waves [n, nW+1, 6, nw] and psd / std over all sea states
        (rh_motion_stats, getPSD / getRMS of raft/raft_fowt.py:1831-1875)."""
        import torch
        n, nw = len(seas), self.nw
        ext = FurtherSeaStates(seas, nws)
        dd = views[0]
        dev = dd.device
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        heads = dd.ensure_headings(ext.betas)
        ctx, s = N.context(self.device), N.stream_handle(torch, dev)
        m = len(ext.pairs)
        S, zeta = ext.spectra(dd)
        sel = torch.tensor(ext.case, dtype=torch.long, device=dev)
        bdrag = res["B_drag"].index_select(0, sel).contiguous()
        bmat = res["Bmat"].index_select(0, sel).contiguous()
        XiE = torch.empty([m, 6, nw], dtype=torch.complex128, device=dev)
        fext = None
        fowt = self.fowtList[0]
        if fowt.potSecOrder == 2:      # the .12d QTF's force of each further sea state (:1059-1061)
            fext, fm = file_qtf_forces(dd, fowt, ext.betas, S)
            res["f2nd_mean_waves"] = ext.scatter(res["f2nd_mean"], fm, ext.nwm)
        arr = (N.RhDesign * len(views))(*[v.struct() for v in views])
        # (the index tensors are held in names: a temporary freed before the call returns would
        # hand its block to the next allocation, and the kernel would read the other array)
        didx = torch.tensor(np.asarray(idx)[ext.case], **i32)
        hidx = torch.tensor(heads, **i32)
        N.check(N.lib().rh_heading_response_ext(ctx, arr, len(views), m, N.ptr(didx), N.ptr(hidx), N.ptr(zeta),
                                                N.ptr(bdrag), N.ptr(bmat), int(bmat.shape[1]), N.ptr(fext), N.ptr(XiE),
                                                s), "rh_heading_response_ext")
        res["Xi_waves"] = Xw = ext.scatter(res["Xi"], XiE, ext.nwm + 1)
        if "psd" in want or "std" in want:
            psd = torch.empty([n, 6, nw], **f64)
            std = torch.empty([n, 6], **f64)
            N.check(N.lib().rh_motion_stats(ctx, n, ext.nwm + 1, nw, float(dd.dw), N.ptr(Xw), N.ptr(psd), N.ptr(std), s),
                    "rh_motion_stats")
            res["psd"], res["std"] = psd, std
        res["nWaves"] = torch.tensor(nws, dtype=torch.int64, device=dev)

    @staticmethod
    def _operating_rotor(fowt, case):
        """Whether calcTurbineConstants gives this case aero terms (raft/raft_fowt.py:795-812).
        A batch case without a wind_speed entry is a sea state alone (wind 0), as batch cases
        have always been read here."""
        if fowt.nrotors == 0:
            return False
        status = get_from_dict(case, "turbine_status", shape=0, dtype=str, default="operating")
        speed = get_from_dict(case, "wind_speed", shape=0, default=0.0)
        return status == "operating" and speed > 0.0 and bool(np.any(np.atleast_1d(fowt._aero_mod) > 0))

    def prepareArrayBatch(self, cases):
        """The per-batch inputs of analyzeArrayBatch resident on the device: the (case, FOWT)
        case table with its wave tables (solver.prepare_batch), the FOWT descriptors and the
        array stiffness.  Reusable for repeated solves of the same sea states.  Every heading of
        every sea state is tabulated here, before any descriptor is made."""
        import torch
        nf, n = self.nFOWT, len(cases)
        self._calc_bem_once()
        dds = [f.device_design() for f in self.fowtList]   # (node counts may differ: Bmat rows padded to the largest)
        seas = [self._case_sea_states(c) for c in cases]
        nws = np.array([len(x[0]) for x in seas], dtype=np.int64)
        if any(f.potSecOrder == 1 for f in self.fowtList):
            raise NotImplementedError("analyzeArrayBatch: potSecOrder=1 in a coupled array; the reference adds the "
                                      "force to F_lin[i1:i2] of the whole system (raft/raft_model.py:988, SURVEY.md Q5)")
        allh = np.unique(np.concatenate([np.asarray(x[0], dtype=float) for x in seas])) * DEG2RAD if n else []
        for d in dds:
            d.ensure_headings(allh)
        hd, sp, Hs, Tp, gm = ([x[k][0] for x in seas] for k in range(5))
        rep = lambda v: [x for x in v for _ in range(nf)]          # case-major, FOWT-minor
        cs = CaseSet(np.tile(np.arange(nf, dtype=np.int32), n), rep(hd), rep(sp), rep(Hs), rep(Tp), rep(gm))
        dev = dds[0].device
        from .solver import prepare_batch
        Ka = self.array_stiffness()
        return dict(n=n, dds=dds, cs=cs, prep=prepare_batch(dds, cs), dev=dev, nws=nws, ext=FurtherSeaStates(seas, nws),
                    arr=(N.RhDesign * nf)(*[d.struct() for d in dds]),
                    K=None if Ka is None else torch.tensor(Ka, dtype=torch.float64, device=dev).contiguous())

    def analyzeArrayBatch(self, cases=None, tol=0.01, host=True, marks=None, prepared=None, statics=False,
                          pose_chunk=32, rotor_device=False):
        """The coupled-array response of many cases (raft/raft_model.py:852-1065 for nFOWT > 1)
        in a few device calls instead of per-case, per-FOWT host round trips:
          1. every (case, FOWT) drag fixed point in one rh_solve_cases launch (outputs: zeta,
             the node drag matrices, B_drag, and each entry's wave excitation of sea state 0
             with its final linearisation, F_wave);
          2. rh_array_solve_stats: per (case, bin) each FOWT's impedance rebuilt from the
             design's matrices and B_drag, Z_sys = blockdiag(Z_i) + array mooring stiffness and
             Xi = Z_sys^-1 F_wave, and the per-FOWT motion PSD / RMS from the solution in
             registers (rh_motion_stats' values, bit for bit);
          3. cases with several sea states (:1049-1065): the excitation of every further
             (sea state, FOWT) with the linearisation frozen (rh_wave_excitation) and the same
             coupled solve for all of them in one more launch; psd / std then sum over the sea
             states (rh_motion_stats over Xi_waves, getPSD / getRMS) and Xi_waves
             [n, nW+1, 6N, nw] holds every response in the reference's layout.
        FOWTs with potSecOrder=2 add their .12d QTF's force to each sea state's excitation
        (:903-904, :1059-1061; f2nd_mean [n, N, 6]).
        Returns Xi [n, 6N, nw], iters / status [n, N], psd [n, N, 6, nw], std [n, N, 6], zeta.
        A (case, bin) whose coupled solve meets an exactly zero pivot (a singular Z_sys, or for two
        FOWTs a singular first block Z_1 + K_11) comes back with NaN in all its 6N rows of Xi, and that
        case's psd bin and std are NaN: the batch is not interrupted and nothing is raised here (the
        reference, and Model.solveDynamics, raise LinAlgError for such a case).
        prepared: prepareArrayBatch(cases) of an earlier call (then `cases` is not needed).
        marks: optional two timing events recorded around the fixed-point launch (bench).
        statics=True solves every case at its own mean-offset pose, as analyzeCases does: the offsets
        of all cases from solveStaticsArrayBatch, every (case, FOWT) design at its own pose in chunks
        of pose_chunk cases, and the coupled solve with the case's own array stiffness
        (rh_array_solve_stats_ext).  Added keys: mean_offsets [n,6N], statics_iters, statics_status,
        and the reference's array_mooring channels (raft/raft_model.py:351-373) Tmoor_avg [n,2L],
        Tmoor_std, Tmoor_PSD [n,2L,nw] (over w[0]), Tmoor_max / Tmoor_min (+- 3 std).  One sea state
        per case; potSecOrder > 0 and a K_array / C_moor fixture raise NotImplementedError.
        rotor_device=True (with statics=True, the form that evaluates the rotors) takes every FOWT's
        blade-element loads from one device launch per FOWT, as analyzeCasesBatch does."""
        import torch
        if statics:
            return self._analyze_array_statics(cases, tol, host, pose_chunk, rotor_device)
        P = prepared if prepared is not None else self.prepareArrayBatch(cases)
        nf, n, nw = self.nFOWT, P["n"], self.nw
        dds, cs, prep, dev = P["dds"], P["cs"], P["prep"], P["dev"]
        multi = n > 0 and int(P["nws"].max()) > 1
        # X first holds each (case, FOWT)'s F_wave, written by its fixed point with the final
        # linearisation ([n, 6 nf, nw] is the [n nf, 6, nw] layout of the fixed point's entries),
        # then the coupled response (rh_array_solve_stats)
        X = torch.empty([n, 6 * nf, nw], dtype=torch.complex128, device=dev)
        if marks:
            marks[0].record(torch.cuda.current_stream(dev))
        res = solve_batch_2nd(dds, self.fowtList, cs, self.nIter, self.XiStart, tol,
                              want=("zeta", "Bmat", "B_drag", "noXi"), prepared=prep, F_wave=X.view(n * nf, 6, nw))
        if marks:
            marks[1].record(torch.cuda.current_stream(dev))
        arr = P["arr"]
        s = N.stream_handle(torch, dev)
        ctx = N.context(self.device)
        K = P["K"]
        psd = std = None
        if not multi:
            psd = torch.empty([n * nf, 6, nw], dtype=torch.float64, device=dev)
            std = torch.empty([n * nf, 6], dtype=torch.float64, device=dev)
        N.check(N.lib().rh_array_solve_stats(ctx, arr, nf, nf, n, N.ptr(prep["design"]), N.ptr(res["B_drag"]), N.ptr(K),
                                             N.ptr(X), float(self.fowtList[0].dw), N.ptr(psd), N.ptr(std), s),
                "rh_array_solve_stats")
        out = {"Xi": X, "iters": res["iters"].view(n, nf), "status": res["status"].view(n, nf),
               "zeta": res["zeta"].view(n, nf, nw)[:, 0]}
        if "f2nd_mean" in res:
            out["f2nd_mean"] = res["f2nd_mean"].view(n, nf, 6)
        keep = [res, arr, K]
        if multi:
            psd, std = self._array_extra_sea_states(P, res, X, out, keep)
        out["psd"], out["std"] = psd.view(n, nf, 6, nw), std.view(n, nf, 6)
        out["_keep"] = tuple(keep)
        if host:
            return {k: v.cpu().numpy() for k, v in out.items() if k != "_keep"}
        return out

    def _analyze_array_statics(self, cases, tol, host, pose_chunk, rotor_device=False):
        """analyzeArrayBatch(statics=True): see there.  Every FOWT is moved to its pose as solveStatics
        leaves it (turbine and hydro constants at the reference pose, members and rotors at the
        offset pose, its own system's C_moor from the device)."""
        import torch
        from .solver import prepare_batch
        seas = self._refuse_pose_analysis("analyzeArrayBatch", cases, pose_chunk)
        self._calc_bem_once()
        # (the rotor loads are those of the reference poses, where _design_at_pose takes the turbine constants)
        bems = [] if rotor_device else None
        sb = self._solve_statics_array_batch(cases, None, False, bems)
        nf, n, nw = self.nFOWT, len(cases), self.nw
        Xs = sb["X"].cpu().numpy()
        Cm = [None if c is None else c.cpu().numpy() for c in sb["C_moor"]]
        Fm = [None if c is None else c.cpu().numpy() for c in sb["F_moor0"]]
        X_ref = self._reference_poses()
        dev = sb["X"].device
        ctx, s = N.context(self.device), N.stream_handle(torch, dev)
        parts = []
        for c0 in range(0, n, int(pose_chunk)):
            ids = list(range(c0, min(n, c0 + int(pose_chunk))))
            dds = [self._design_at_pose(fowt, self._fowt_case(cases[i], f), X_ref[f], Xs[i, 6 * f:6 * f + 6],
                                        bems[f][i] if bems else None, None if Cm[f] is None else (Cm[f][i], Fm[f][i]),
                                        seas[i][0])
                   for i in ids for f, fowt in enumerate(self.fowtList)]
            m = len(ids)
            rep = lambda k: [seas[i][k][0] for i in ids for _ in range(nf)]   # noqa: E731
            cs = CaseSet(np.arange(m * nf, dtype=np.int32), rep(0), rep(1), rep(2), rep(3), rep(4))
            prep = prepare_batch(dds, cs)
            X = torch.empty([m, 6 * nf, nw], dtype=torch.complex128, device=dev)
            res = solve_batch_2nd(dds, [self.fowtList[k % nf] for k in range(m * nf)], cs, self.nIter, self.XiStart, tol,
                                  want=("zeta", "Bmat", "B_drag", "noXi"), prepared=prep, F_wave=X.view(m * nf, 6, nw))
            arr = (N.RhDesign * (m * nf))(*[d.struct() for d in dds])
            K = sb["K_array"][ids[0]:ids[-1] + 1].contiguous()
            psd = torch.empty([m * nf, 6, nw], dtype=torch.float64, device=dev)
            std = torch.empty([m * nf, 6], dtype=torch.float64, device=dev)
            N.check(N.lib().rh_array_solve_stats_ext(ctx, arr, m * nf, nf, m, N.ptr(prep["design"]), N.ptr(res["B_drag"]),
                                                     N.ptr(K), 36 * nf * nf, N.ptr(X), float(self.fowtList[0].dw),
                                                     N.ptr(psd), N.ptr(std), s), "rh_array_solve_stats_ext")
            parts.append({"Xi": X, "iters": res["iters"].view(m, nf).clone(), "status": res["status"].view(m, nf).clone(),
                          "zeta": res["zeta"].view(m, nf, nw)[:, 0].clone(), "psd": psd.view(m, nf, 6, nw),
                          "std": std.view(m, nf, 6)})
            torch.cuda.synchronize(dev)                   # the chunk's tables are released below
            del res, dds, prep, arr, K
        self._restore_reference_poses(X_ref)
        out = {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]} if parts else {}
        if n:
            out["mean_offsets"], out["statics_iters"], out["statics_status"] = sb["X"], sb["iters"], sb["status"]
            if sb["J_moor"] is not None:      # the reference's array_mooring channels
                out["Tmoor_PSD"], out["Tmoor_std"] = self._tension_channels(sb["J_moor"], out["Xi"])
                out["Tmoor_avg"] = sb["Tmoor_avg"]
                out["Tmoor_max"] = out["Tmoor_avg"] + 3 * out["Tmoor_std"]
                out["Tmoor_min"] = out["Tmoor_avg"] - 3 * out["Tmoor_std"]
        return {k: v.cpu().numpy() for k, v in out.items()} if host else out

    def _array_extra_sea_states(self, P, res, X, out, keep):
        """Step 3 of analyzeArrayBatch: the further sea states of every case (one excitation and
        one coupled-solve launch for all of them), Xi_waves and the statistics over all rows.  As in
        step 2, a singular (sea state, bin) returns NaN rows, which its case's psd / std inherit."""
        import torch
        nf, n, nw = self.nFOWT, P["n"], self.nw
        dds, dev, nws, ext = P["dds"], P["dev"], P["nws"], P["ext"]
        nwm = ext.nwm
        ctx, s = N.context(self.device), N.stream_handle(torch, dev)
        i32 = dict(dtype=torch.int32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        m = len(ext.pairs)
        S, zeta = ext.spectra(dds[0])
        # entries (extra sea state, FOWT), sea-state-major: the [m, 6 nf, nw] layout of the solve
        src = np.array([i * nf + f for i, _ in ext.pairs for f in range(nf)], dtype=np.int64)
        heads = np.array([dds[f].ensure_headings([b])[0] for b in ext.betas for f in range(nf)], dtype=np.int32)
        didx = torch.tensor(np.tile(np.arange(nf, dtype=np.int32), m), **i32)
        hidx = torch.tensor(heads, **i32)
        srct = torch.tensor(src, dtype=torch.long, device=dev)
        ze = zeta.repeat_interleave(nf, dim=0).contiguous()
        bmat = res["Bmat"].index_select(0, srct).contiguous()
        bdrag = res["B_drag"].index_select(0, srct).contiguous()
        XE = torch.empty([m, 6 * nf, nw], dtype=torch.complex128, device=dev)
        N.check(N.lib().rh_wave_excitation(ctx, P["arr"], nf, m * nf, N.ptr(didx), N.ptr(hidx), N.ptr(ze), N.ptr(bmat),
                                           N.ptr(XE), s), "rh_wave_excitation")
        FE = XE.view(m, nf, 6, nw)
        if any(f.potSecOrder == 2 for f in self.fowtList):
            fme = torch.zeros([m, nf, 6], **f64)
            for f, fowt in enumerate(self.fowtList):
                if fowt.potSecOrder != 2:
                    continue
                fx, fme[:, f] = file_qtf_forces(dds[f], fowt, ext.betas, S)          # (:1059-1061)
                FE[:, f] += fx
            out["f2nd_mean_waves"] = ext.scatter(out["f2nd_mean"], fme, nwm)
        N.check(N.lib().rh_array_solve_stats(ctx, P["arr"], nf, nf, m, N.ptr(didx), N.ptr(bdrag), N.ptr(P["K"]),
                                             N.ptr(XE), float(self.fowtList[0].dw), None, None, s),
                "rh_array_solve_stats")
        out["Xi_waves"] = Xw = ext.scatter(X, XE, nwm + 1)
        out["nWaves"] = torch.tensor(nws, dtype=torch.int64, device=dev)
        rows = Xw.view(n, nwm + 1, nf, 6, nw).permute(0, 2, 1, 3, 4).contiguous()      # [n, nf, nW+1, 6, nw]
        psd = torch.empty([n * nf, 6, nw], **f64)
        std = torch.empty([n * nf, 6], **f64)
        N.check(N.lib().rh_motion_stats(ctx, n * nf, nwm + 1, nw, float(self.fowtList[0].dw), N.ptr(rows), N.ptr(psd),
                                        N.ptr(std), s), "rh_motion_stats")
        keep += [S, zeta, didx, hidx, ze, bmat, bdrag, XE, rows]
        return psd, std


def _load_design(input_file):
    """A design dict from a dict or a YAML file (raft/raft_model.py:2029-2039).  Pickled
    designs are refused: unpickling can execute code from the file."""
    if isinstance(input_file, dict):
        return input_file
    if str(input_file).endswith((".pkl", ".pickle")):
        raise ValueError("pickled design files are not loaded (unpickling can execute code); pass a YAML file or a dict")
    import yaml
    print("\n\nLoading RAFT input file: " + str(input_file))
    with open(input_file) as fh:
        return yaml.safe_load(fh)


def runRAFT(input_file, turbine_file="", plot=0, ballast=False, station_plot=[]):
    """Set up and run RAFT for a design (raft/raft_model.py:2024-2061): Model, unloaded
    equilibrium, every load case of design['cases'] (mean offsets, device response solve,
    output channels) and the system property outputs.  Returns the Model."""
    design = _load_design(input_file)
    print(" --- making model ---")
    model = Model(design)
    print(" --- analyzing unloaded ---")
    model.analyzeUnloaded(ballast=ballast)
    print(" --- analyzing cases ---")
    model.analyzeCases(display=1)
    model.calcOutputs()
    if plot:
        raise NotImplementedError("plotting is outside the accelerated path")
    return model


def runRAFTFarm(input_file, plot=0):
    """Set up and run a RAFT farm (raft/raft_model.py:2065-2095): no unloaded analysis and no
    calcOutputs (as in the reference); analyzeCases over the coupled array."""
    design = _load_design(input_file)
    print(" --- making model ---")
    model = Model(design)
    print("**Note: RAFTFarm cannot run model.analyzeUnloaded()")
    print(" --- analyzing cases ---")
    model.analyzeCases(display=1)
    print("**Note: model.calcOutputs is not supported yet for multi-turbine Farm configurations")
    if plot:
        raise NotImplementedError("plotting is outside the accelerated path")
    return model
