"""Quasi-static mooring and mean offsets on the device (csrc/rh_moor.h, rh_moor.hip).

flatten() turns a MooringSystem (raft/mooring.py) into the line table of rh_moor_system and
flatten_drag() into the drag table of its line types; DeviceMooring wraps rh_moor_eval and
rh_statics_solve on torch tensors, and rh_moor_eval_current / rh_statics_solve_current when a
current per pose or case is given.  The device covers ONE coupled body whose lines each join one
fixed point and one body-attached point; flatten() refuses everything else with a
NotImplementedError that names the reason, before any device call.  A uniform current on the lines
(mooring currentMod 1) is an argument of eval() and solve_statics(), one vector per pose or case:
MooringSystem.current is one case's state on the host object, so a system that still carries one
is refused.
"""
import ctypes

import numpy as np

from . import _native as N
from .device_records import DeviceRecords
from .mooring import Point


def flatten(ms):
    """The line table [ML_COUNT, nline] (float64, the order of enum rh_moor_line_field) of a
    MooringSystem, with its depth and catenary tolerance.  Host only: no device is touched."""
    if any(p.type == Point.FREE for p in ms.points):
        raise NotImplementedError("device mooring: free points (their equilibrium is solved on the host only)")
    if len(ms.bodies) != 1:
        raise NotImplementedError(f"device mooring: {len(ms.bodies)} coupled bodies (one body per system; the "
                                  "array-level system of a farm stays on the host)")
    if np.any(np.asarray(ms.current, dtype=float)):
        raise NotImplementedError("device mooring: the system's own current is set (one case's state on the host "
                                  "object; clear it and pass the current per case: eval / solve_statics(current=...))")
    if not ms.lines:
        raise NotImplementedError("device mooring: a system without lines")
    if len(ms.lines) > N.MOOR_MAX_LINES:
        raise NotImplementedError(f"device mooring: {len(ms.lines)} lines (at most {N.MOOR_MAX_LINES})")
    rel = {id(p): rr for p, rr in ms.bodies[0].points}
    tab = np.zeros([N.ML_COUNT, len(ms.lines)])
    for i, ln in enumerate(ms.lines):
        a, b = id(ln.pA) in rel, id(ln.pB) in rel
        if a and b:
            raise NotImplementedError(f"device mooring: line {ln.number} joins two points of the body")
        if not a and not b:
            raise NotImplementedError(f"device mooring: line {ln.number} joins two fixed points")
        if ln.type["w"] < 0:
            raise NotImplementedError(f"device mooring: line {ln.number} is buoyant (W < 0)")
        fixed, att = (ln.pB, ln.pA) if a else (ln.pA, ln.pB)
        tab[0:3, i] = fixed.r
        tab[3:6, i] = rel[id(att)]
        tab[6, i], tab[7, i], tab[8, i] = ln.L, ln.type["EA"], ln.type["w"]
        tab[9, i] = 0.0 if a else 1.0
    return tab, float(ms.depth), float(ms.cat_tol)


def flatten_drag(ms):
    """The drag table [MD_COUNT, nline] (float64, the order of enum rh_moor_drag_field) that
    Line.current_load reads: d, Cd and CdAx of each line's type, and the system's rho."""
    tab = np.zeros([N.MD_COUNT, len(ms.lines)])
    for i, ln in enumerate(ms.lines):
        tab[:, i] = ln.type["d"], ln.type.get("Cd", 0.0), ln.type.get("CdAx", 0.0), ms.rho
    return tab


def finite_current(current, n):
    """The currents [n, 3] of a call as a float64 array; a wrong shape or a non-finite entry raises
    ValueError (on the host, before any launch)."""
    cur = np.array(current.cpu() if hasattr(current, "cpu") else current, dtype=float)
    if cur.shape != (n, 3):
        raise ValueError(f"device mooring: current of shape {list(cur.shape)}, expected [{n}, 3]")
    if not np.all(np.isfinite(cur)):
        raise ValueError("device mooring: non-finite current")
    return cur


def warm_state(ms):
    """The catenary warm start (HF, VF) of every line, [nline, 2]."""
    return np.array([[ln.HF, ln.VF] for ln in ms.lines], dtype=float)


class DeviceMooring(DeviceRecords):
    """One or more mooring systems resident on the device.  Poses and cases pick a system through
    sys_idx; the T and J outputs have 2 nl_max rows per pose: TA of line l in row l, TB in row
    nl_max + l (for a single system this is MooringSystem.tensions()' order)."""

    def __init__(self, systems, device=0):
        flat = [flatten(ms) for ms in systems]          # every refusal before the first device call
        super().__init__(device)
        torch = self.torch
        self.nline = [t.shape[1] for t, _, _ in flat]
        self.nl_max = max(self.nline)
        self.nsys = len(flat)
        self._tables = [torch.tensor(t, dtype=torch.float64, device=self.device).contiguous() for t, _, _ in flat]
        self._arr = (N.RhMoorSystem * self.nsys)()
        for i, (_, depth, tol) in enumerate(flat):
            self._arr[i].nline, self._arr[i].pad_ = self.nline[i], 0
            self._arr[i].depth, self._arr[i].tol = depth, tol
            self._arr[i].line = self._tables[i].data_ptr()
        self._arr_dev = self.upload(self._arr)
        drag = np.zeros([self.nsys, N.MD_COUNT, self.nl_max])       # columns of lines a system lacks: zeros
        for i, ms in enumerate(systems):
            drag[i, :, :self.nline[i]] = flatten_drag(ms)
        self._drag = torch.tensor(drag, dtype=torch.float64, device=self.device).contiguous()

    def eval(self, r6, sys_idx=None, warm=None, jacobian=False, current=None):
        """rh_moor_eval at poses r6 [n, 6].  warm [n, nl_max, 2] or None (cold).  current [n, 3] or
        None: a uniform current on the lines of each pose (rh_moor_eval_current; a pose with zero
        current gets the bits of the call without).  Returns device tensors F [n,6], K [n,6,6],
        T [n,2 nl_max], J [n,2 nl_max,6] (or None), status [n], warm."""
        n = len(r6)
        cur = None if current is None else finite_current(current, n)      # (checked before anything is uploaded)
        torch = self.torch
        cur = None if cur is None else self.f64(cur, [n, 3])
        r6 = self.f64(r6, [n, 6])
        idx = self.index(sys_idx, n, limit=self.nsys)
        f64 = dict(dtype=torch.float64, device=self.device)
        w = torch.zeros([n, self.nl_max, 2], **f64) if warm is None else self.f64(warm, [n, self.nl_max, 2]).clone()
        F = torch.empty([n, 6], **f64)
        K = torch.empty([n, 6, 6], **f64)
        T = torch.empty([n, 2 * self.nl_max], **f64)
        J = torch.empty([n, 2 * self.nl_max, 6], **f64) if jacobian else None
        status = torch.empty([n], dtype=torch.int32, device=self.device)
        head = (N.context(self.dev_index), self._arr, N.ptr(self._arr_dev), self.nsys, n, N.ptr(idx), N.ptr(r6))
        tail = (N.ptr(w), N.ptr(F), N.ptr(K), N.ptr(T), N.ptr(J), N.ptr(status), N.stream_handle(torch, self.device))
        if cur is None:
            N.check(N.lib().rh_moor_eval(*head, *tail), "rh_moor_eval")
        else:
            N.check(N.lib().rh_moor_eval_current(*head, N.ptr(self._drag), N.ptr(cur), *tail), "rh_moor_eval_current")
        return dict(F=F, K=K, T=T, J=J, status=status, warm=w, _keep=(r6, idx, cur))

    def solve_statics(self, X_ref, K_hs, F_const, warm0=None, sys_idx=None, current=None):
        """rh_statics_solve: X_ref [n,6], K_hs [n,6,6], F_const [n,6], warm0 [n,nl_max,2] or None.
        current [n, 3] or None: a uniform current on the lines of each case (rh_statics_solve_current).
        Returns device tensors X [n,6], warm [n,nl_max,2], iters [n], status [n]."""
        n = len(X_ref)
        cur = None if current is None else finite_current(current, n)      # (checked before anything is uploaded)
        torch = self.torch
        cur = None if cur is None else self.f64(cur, [n, 3])
        X_ref = self.f64(X_ref, [n, 6])
        K_hs = self.f64(K_hs, [n, 6, 6])
        F_const = self.f64(F_const, [n, 6])
        w0 = None if warm0 is None else self.f64(warm0, [n, self.nl_max, 2])
        idx = self.index(sys_idx, n, limit=self.nsys)
        f64 = dict(dtype=torch.float64, device=self.device)
        X = torch.empty([n, 6], **f64)
        w = torch.empty([n, self.nl_max, 2], **f64)
        iters = torch.empty([n], dtype=torch.int32, device=self.device)
        status = torch.empty([n], dtype=torch.int32, device=self.device)
        head = (N.context(self.dev_index), self._arr, N.ptr(self._arr_dev), self.nsys, n, N.ptr(idx), N.ptr(X_ref),
                N.ptr(K_hs), N.ptr(F_const))
        tail = (N.ptr(w0), N.ptr(X), N.ptr(w), N.ptr(iters), N.ptr(status), N.stream_handle(torch, self.device))
        if cur is None:
            N.check(N.lib().rh_statics_solve(*head, *tail), "rh_statics_solve")
        else:
            N.check(N.lib().rh_statics_solve_current(*head, N.ptr(self._drag), N.ptr(cur), *tail),
                    "rh_statics_solve_current")
        return dict(X=X, warm=w, iters=iters, status=status, _keep=(X_ref, K_hs, F_const, w0, idx, cur))
