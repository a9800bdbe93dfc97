"""General mooring systems and the mean offsets of moored arrays on the device
(csrc/rh_moor_array.h, rh_moor_array.hip).

flatten_array() merges the mooring systems a model's statics see (each FOWT's own system, if it
has one, and the array-level system) into one record: a point table, a line table with each line's
own depth and catenary tolerance, and the system every line came from.  DeviceArrayMooring wraps
rh_moor_array_eval and rh_array_statics_solve on torch tensors.  Covered: several bodies, free
points (in one of the merged systems), lines between two bodies, between two points of one body,
free-free and free-fixed lines.  Refused by name with NotImplementedError before any device call:
current on the lines, buoyant lines (W < 0), a line joining two fixed points, free points in more
than one system, more than ARR_MAX_BODIES bodies, ARR_MAX_FREE free points or MOOR_MAX_LINES lines.
"""
import numpy as np

from . import _native as N
from .device_records import DeviceRecords
from .mooring import MooringSystem, Point

FIXED, ON_BODY, FREE = 0, 1, 2          # point kinds of the point table


class ArrayRecord:
    """One flattened record: point [MP_COUNT, npoint] and line [MAL_COUNT, nline] tables (float64, the
    row order of enum rh_moor_point_field / rh_moor_aline_field), membership [nline] (the index into
    `systems` each line came from), and the scalars of the system that holds the free points."""

    def __init__(self, point, line, nbody, nfree, free_sys, g, rho, free_tol, free_depth, systems, free_points):
        self.point, self.line = point, line
        self.nbody, self.nfree, self.free_sys = nbody, nfree, free_sys
        self.g, self.rho, self.free_tol, self.free_depth = g, rho, free_tol, free_depth
        self.systems = systems              # [(MooringSystem, [global body index of each of its bodies])]
        self.free_points = free_points      # the Point objects of the free points, in table order
        self.npoint, self.nline = point.shape[1], line.shape[1]
        self.membership = line[N.MAL["SYS"]].astype(int)

    def lines_of(self, k):
        """Rows of the record's lines that belong to systems[k] (in that system's line order)."""
        return np.nonzero(self.membership == k)[0]


def _systems_of(obj):
    if isinstance(obj, MooringSystem):
        return [(obj, list(range(len(obj.bodies))))]
    if hasattr(obj, "fowtList"):
        out = [(f.ms, [i]) for i, f in enumerate(obj.fowtList) if f.ms is not None and f.ms.lines]
        if obj.ms is not None:
            out.append((obj.ms, list(range(len(obj.ms.bodies)))))
        return out
    return [(ms, list(bodies)) for ms, bodies in obj]


def flatten_array(model_or_systems):
    """The merged record of a Model (every FOWT's own system and the array-level system), of one
    MooringSystem, or of a list of (MooringSystem, [global body index per body]) pairs.
    Host only: no device is touched."""
    systems = _systems_of(model_or_systems)
    if not systems or not any(ms.lines for ms, _ in systems):
        raise NotImplementedError("device array mooring: no mooring lines")
    nbody = 1 + max(max(b) for _, b in systems if len(b))
    if nbody > N.ARR_MAX_BODIES:
        raise NotImplementedError(f"device array mooring: {nbody} bodies (at most {N.ARR_MAX_BODIES})")
    with_free = [k for k, (ms, _) in enumerate(systems) if any(p.type == Point.FREE for p in ms.points)]
    if len(with_free) > 1:
        raise NotImplementedError("device array mooring: free points in more than one system (separate systems "
                                  "are separate equilibrium problems on the host)")
    points, lines, free_points = [], [], []
    for k, (ms, bodies) in enumerate(systems):
        if np.any(np.asarray(ms.current, dtype=float)):
            raise NotImplementedError("device array mooring: current on the lines (mooring currentMod 1 with a current)")
        owner = {id(p): (bodies[ib], rr) for ib, b in enumerate(ms.bodies) for p, rr in b.points}
        row = {}
        for p in ms.points:
            if p.type == Point.FREE:
                kind, idx, xyz = FREE, len(free_points), p.r
                free_points.append(p)
            elif id(p) in owner:
                kind, idx, xyz = ON_BODY, owner[id(p)][0], owner[id(p)][1]
            else:
                kind, idx, xyz = FIXED, 0, p.r
            row[id(p)] = len(points)
            points.append([kind, idx, xyz[0], xyz[1], xyz[2], p.m, p.v])
        for ln in ms.lines:
            a, b = row[id(ln.pA)], row[id(ln.pB)]
            if points[a][0] == FIXED and points[b][0] == FIXED:
                raise NotImplementedError(f"device array mooring: line {ln.number} joins two fixed points")
            if ln.type["w"] < 0:
                raise NotImplementedError(f"device array mooring: line {ln.number} is buoyant (W < 0)")
            lines.append([a, b, ln.L, ln.type["EA"], ln.type["w"], ms.depth, ms.cat_tol, k])
    if len(free_points) > N.ARR_MAX_FREE:
        raise NotImplementedError(f"device array mooring: {len(free_points)} free points (at most {N.ARR_MAX_FREE})")
    if len(lines) > N.MOOR_MAX_LINES:
        raise NotImplementedError(f"device array mooring: {len(lines)} lines (at most {N.MOOR_MAX_LINES})")
    fs = with_free[0] if with_free else -1
    src = systems[fs][0] if with_free else systems[0][0]
    return ArrayRecord(np.ascontiguousarray(np.array(points, dtype=float).T), np.ascontiguousarray(np.array(lines, dtype=float).T),
                       nbody, len(free_points), fs, float(src.g), float(src.rho), float(src.free_tol), float(src.depth),
                       systems, free_points)


def array_state(rec):
    """The state a solve starts from: the catenary warm start (HF, VF) of every line of the record
    [nline, 2] and the free-point positions [nfree, 3], read from the record's systems as they are."""
    warm = np.array([[ln.HF, ln.VF] for ms, _ in rec.systems for ln in ms.lines], dtype=float).reshape(-1, 2)
    free = np.array([p.r for p in rec.free_points], dtype=float).reshape(-1, 3)
    return warm, free


class DeviceArrayMooring(DeviceRecords):
    """One or more records resident on the device; poses and cases pick a record through sys_idx.
    Outputs are laid out for the largest record: nb = largest nbody, nl = largest nline, nf = largest
    nfree; T and J have 2 nl rows per pose (TA of line l in row l, TB in row nl + l); rows and columns
    a record lacks are zero."""

    def __init__(self, records, device=0):
        self.records = [r if isinstance(r, ArrayRecord) else flatten_array(r) for r in records]   # refusals first
        super().__init__(device)
        torch = self.torch
        self.nsys = len(self.records)
        self.nb = max(r.nbody for r in self.records)
        self.nl = max(r.nline for r in self.records)
        self.nf = max(r.nfree for r in self.records)
        f64 = dict(dtype=torch.float64, device=self.device)
        self._pt = [torch.tensor(r.point, **f64).contiguous() for r in self.records]
        self._ln = [torch.tensor(r.line, **f64).contiguous() for r in self.records]
        self._arr = (N.RhMoorArraySystem * self.nsys)()
        for i, r in enumerate(self.records):
            a = self._arr[i]
            a.nbody, a.npoint, a.nline, a.nfree, a.free_sys, a.pad_ = r.nbody, r.npoint, r.nline, r.nfree, r.free_sys, 0
            a.g, a.rho, a.free_tol, a.free_depth = r.g, r.rho, r.free_tol, r.free_depth
            a.point, a.line = self._pt[i].data_ptr(), self._ln[i].data_ptr()
            a.point_host, a.line_host = r.point.ctypes.data, r.line.ctypes.data
        self._arr_dev = self.upload(self._arr)

    def same_tables(self, records):
        """Whether `records` (ArrayRecord) hold exactly the tables and scalars resident on the device."""
        key = lambda r: (r.nbody, r.nfree, r.free_sys, r.g, r.rho, r.free_tol, r.free_depth)   # noqa: E731
        return len(records) == len(self.records) and all(
            key(a) == key(b) and a.point.shape == b.point.shape and a.line.shape == b.line.shape
            and np.array_equal(a.point, b.point) and np.array_equal(a.line, b.line)
            for a, b in zip(records, self.records))

    def eval(self, r6, warm, free, sys_idx=None, jacobian=False):
        """rh_moor_array_eval at poses r6 [n, nb, 6] from the state warm [n, nl, 2] (or None: cold) and
        free [n, nf, 3].  Returns device tensors F [n, 6nb], K [n, 6nb, 6nb], T [n, 2nl], J [n, 2nl, 6nb]
        (or None), nev [n] (line passes of each pose's equilibrium), status [n], and the solved
        state warm, free."""
        torch = self.torch
        n = len(r6)
        nD = 6 * self.nb
        r6 = self.f64(r6, [n, self.nb, 6])
        f64 = dict(dtype=torch.float64, device=self.device)
        w = torch.zeros([n, self.nl, 2], **f64) if warm is None else self.f64(warm, [n, self.nl, 2]).clone()
        fr = self.f64(free, [n, self.nf, 3]).clone()
        idx = self.index(sys_idx, n)
        F = torch.zeros([n, nD], **f64)
        K = torch.zeros([n, nD, nD], **f64)
        T = torch.zeros([n, 2 * self.nl], **f64)
        J = torch.zeros([n, 2 * self.nl, nD], **f64) if jacobian else None
        nev = torch.zeros([n], dtype=torch.int32, device=self.device)
        status = torch.zeros([n], dtype=torch.int32, device=self.device)
        N.check(N.lib().rh_moor_array_eval(N.context(self.dev_index), self._arr, N.ptr(self._arr_dev), self.nsys, n,
                                           N.ptr(idx), N.ptr(r6), N.ptr(w), N.ptr(fr), N.ptr(F), N.ptr(K), N.ptr(T),
                                           N.ptr(J), N.ptr(nev), N.ptr(status), N.stream_handle(torch, self.device)),
                "rh_moor_array_eval")
        return dict(F=F, K=K, T=T, J=J, nev=nev, status=status, warm=w, free=fr, _keep=(r6, idx))

    def solve_statics(self, X_ref, K_hs, F_const, warm0, free0, sys_idx=None):
        """rh_array_statics_solve: X_ref [n, nb, 6], K_hs [n, nb, 6, 6], F_const [n, nb, 6], warm0
        [n, nl, 2] or None, free0 [n, nf, 3].  Returns device tensors X [n, 6nb], warm, free, iters [n],
        status [n]."""
        torch = self.torch
        n = len(X_ref)
        X_ref = self.f64(X_ref, [n, self.nb, 6])
        K_hs = self.f64(K_hs, [n, self.nb, 6, 6])
        F_const = self.f64(F_const, [n, self.nb, 6])
        w0 = None if warm0 is None else self.f64(warm0, [n, self.nl, 2])
        f0 = self.f64(free0, [n, self.nf, 3])
        idx = self.index(sys_idx, n)
        f64 = dict(dtype=torch.float64, device=self.device)
        X = torch.zeros([n, 6 * self.nb], **f64)
        w = torch.zeros([n, self.nl, 2], **f64)
        fr = torch.zeros([n, self.nf, 3], **f64)
        iters = torch.zeros([n], dtype=torch.int32, device=self.device)
        status = torch.zeros([n], dtype=torch.int32, device=self.device)
        N.check(N.lib().rh_array_statics_solve(N.context(self.dev_index), self._arr, N.ptr(self._arr_dev), self.nsys, n,
                                               N.ptr(idx), N.ptr(X_ref), N.ptr(K_hs), N.ptr(F_const), N.ptr(w0),
                                               N.ptr(f0), N.ptr(X), N.ptr(w), N.ptr(fr), N.ptr(iters), N.ptr(status),
                                               N.stream_handle(torch, self.device)), "rh_array_statics_solve")
        return dict(X=X, warm=w, free=fr, iters=iters, status=status, _keep=(X_ref, K_hs, F_const, w0, f0, idx))
