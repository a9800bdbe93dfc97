"""Per-case offset-pose designs and current loads on the device (csrc/rh_pose.h, rh_pose.hip).

host_record() turns a FOWT at its reference pose into the tables of rh_pose_record: the members at
the zero pose and, for ALL strip nodes, the node-table columns a pose does not change.  PoseRecord
holds them on the device and wraps the two calls: designs() gives every pose of a chunk its own node
and member tables (rh_pose_designs), its wave tables (one rh_wave_tables_batch launch) and its
rh_design descriptor, as one BlockDesigns for solver.solve_batch; current_loads() is
FOWT.calcCurrentLoads for every case of a batch (rh_current_loads).  What the device does not cover
(MacCamy-Fuchs members, more members or nodes than the kernels' limits) is refused by name.
"""
import ctypes

import numpy as np

from . import _native as N
from .device_records import DeviceRecords
from .sweep_block import BlockDesigns


MCF_REFUSAL = ("device pose designs: MacCamy-Fuchs members (their inertial excitation depends on the frequency; use "
               "pose_device=False)")


def host_record(fowt):
    """(memb [PM_COUNT, nmemb], node [NF_COUNT, nnode], mstart [nmemb + 1]) of a FOWT: the member rows
    of enum rh_pose_member_field and every strip node's pose-independent columns as prep.node_table
    computes them (rows AQ .. T; the position and unit-vector rows stay zero: the device writes them).
    Imat and a_i are the members' current ones: those of calcHydroConstants at the reference pose when
    the caller ran it there.  Host only: no device is touched."""
    mems = fowt.memberList
    nnode = sum(mem.ns for mem in mems)
    if not 1 <= len(mems) <= N.POSE_MAX_MEMBERS or not 1 <= nnode <= N.POSE_MAX_NODES:
        raise NotImplementedError(f"device pose designs: {len(mems)} members with {nnode} strip nodes (at most "
                                  f"{N.POSE_MAX_MEMBERS} and {N.POSE_MAX_NODES})")
    memb = np.zeros([N.PM_COUNT, len(mems)])
    node = np.zeros([N.NF_COUNT, nnode])
    mstart = np.zeros(len(mems) + 1, dtype=np.int32)
    NF = N.NF
    j = 0
    for m, mem in enumerate(mems):
        _, q, p1, p2 = mem.zero_pose_frame()
        memb[:, m] = [*mem.rA0, *mem.rB0, mem.l, *q, *p1, *p2]
        circ = mem.shape == "circular"
        for il in range(mem.ns):
            ds, drs, dls = np.atleast_1d(mem.ds[il]), np.atleast_1d(mem.drs[il]), mem.dls[il]
            if circ:
                areas = [np.pi * ds[0] * dls, ds[0] * dls, ds[0] * dls, np.abs(np.pi * ds[0] * drs[0])]
            else:
                areas = [2 * (ds[0] + ds[0]) * dls, ds[0] * dls, ds[1] * dls,
                         np.abs((ds[0] + drs[0]) * (ds[1] + drs[1]) - (ds[0] - drs[0]) * (ds[1] - drs[1]))]
            node[NF["AQ"]:NF["AEND"] + 1, j] = areas
            node[NF["CDQ"]:NF["CDEND"] + 1, j] = [mem.coef("Cd_q", il), mem.coef("Cd_p1", il), mem.coef("Cd_p2", il),
                                                  mem.coef("Cd_End", il)]
            node[NF["CIRC"], j] = 1.0 if circ else 0.0
            node[NF["AI"], j] = mem.a_i[il]
            node[NF["I00"]:NF["I22"] + 1, j] = mem.Imat[il].ravel()
            node[NF["T"], j] = mem.ls[il]
            j += 1
        mstart[m + 1] = j
    return memb, node, mstart


class PoseRecord(DeviceRecords):
    """A FOWT's rh_pose_record on the device, with its frequency grid and site scalars."""

    def __init__(self, fowt, device=0, host=None):
        self.host = host if host is not None else host_record(fowt)      # every refusal before the first device call
        self.mcf = any(mem.MCF for mem in fowt.memberList)
        super().__init__(device)
        torch = self.torch
        memb, node, mstart = self.host
        self.nmemb, self.nnode = memb.shape[1], node.shape[1]
        f64 = dict(dtype=torch.float64, device=self.device)
        self._memb = torch.tensor(memb, **f64).contiguous()
        self._node = torch.tensor(node, **f64).contiguous()
        self._mstart = torch.tensor(mstart, dtype=torch.int32, device=self.device)
        self._mstart_host = np.ascontiguousarray(mstart, dtype=np.int32)
        self.w = torch.tensor(np.asarray(fowt.w, dtype=float), **f64)
        self.k = torch.tensor(np.asarray(fowt.k, dtype=float), **f64)
        self.nw = int(fowt.nw)
        self.dw, self.depth, self.rho, self.g = float(fowt.dw), float(fowt.depth), float(fowt.rho_water), float(fowt.g)
        r = self.rec = N.RhPoseRecord()
        r.nmemb, r.nnode = self.nmemb, self.nnode
        r.memb, r.node, r.mstart = self._memb.data_ptr(), self._node.data_ptr(), self._mstart.data_ptr()
        r.mstart_host = self._mstart_host.ctypes.data

    def same_tables(self, host):
        return all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(self.host, host))

    def pose_tables(self, X):
        """rh_pose_designs at poses X [n, 6]: device tensors node [n, NF_COUNT nnode], memb [n, MF_COUNT
        nmemb], mstart [n, nmemb + 1] (slabs; pose i's tables at the head of row i) and the host arrays
        nn [n], nm [n], read back in one copy."""
        torch = self.torch
        n = len(X)
        X = self.f64(X, [n, 6])
        f64 = dict(dtype=torch.float64, device=self.device)
        node = torch.empty([n, N.NF_COUNT * self.nnode], **f64)
        memb = torch.empty([n, N.MF_COUNT * self.nmemb], **f64)
        mstart = torch.empty([n, self.nmemb + 1], dtype=torch.int32, device=self.device)
        cnt = torch.empty([2, n], dtype=torch.int32, device=self.device)
        N.check(N.lib().rh_pose_designs(N.context(self.dev_index), ctypes.byref(self.rec), n, N.ptr(X), N.ptr(node),
                                        N.ptr(memb), N.ptr(mstart), ctypes.c_void_p(cnt.data_ptr()),
                                        ctypes.c_void_p(cnt.data_ptr() + 4 * n), N.stream_handle(torch, self.device)),
                "rh_pose_designs")
        c = cnt.cpu().numpy()
        return dict(node=node, memb=memb, mstart=mstart, nn=c[0].astype(np.int64), nm=c[1].astype(np.int64), _keep=(X,))

    def designs(self, X, C, M_B_rows, headings, nIter=15, XiStart=0.1):
        """The designs of poses X [n, 6] as one BlockDesigns for solver.solve_batch.  C: a contiguous
        [n, 36] (or [n, 6, 6]) device tensor, row i the stiffness C_lin of pose i.  M_B_rows: one (M, B,
        per_bin) of device tensors for all poses, or a list with one per pose (M, B [36], or [nw, 36]
        with per_bin).  headings [n] (rad): the one wave heading tabulated for each pose.  The
        descriptors are written column-wise (as sweep_block.prepare_block writes a block's), kproj /
        finer are slices of two allocations filled by one rh_wave_tables_batch launch; uhat is NULL."""
        torch = self.torch
        n, nw = len(X), self.nw
        if self.mcf:
            raise NotImplementedError(MCF_REFUSAL)
        if not torch.is_tensor(C) or C.numel() != 36 * n or C.dtype != torch.float64 or not C.is_contiguous():
            raise ValueError("PoseRecord.designs: C must be a contiguous float64 device tensor of n x 36 entries")
        rows = [M_B_rows] * n if isinstance(M_B_rows, tuple) else list(M_B_rows)
        if len(rows) != n or len(headings) != n:
            raise ValueError("PoseRecord.designs: one (M, B, per_bin) and one heading per pose")
        T = self.pose_tables(X)
        nn, nm = T["nn"], T["nm"]
        if n and nn.min() < 1:
            raise NotImplementedError(f"device pose designs: pose {int(np.argmin(nn))} leaves no strip node submerged")
        rec = np.zeros(n, dtype=np.dtype(N.RhDesign))
        i = np.arange(n, dtype=np.int64)
        rec["w"], rec["k"] = self.w.data_ptr(), self.k.data_ptr()
        rec["node"] = T["node"].data_ptr() + 8 * N.NF_COUNT * self.nnode * i
        rec["memb"] = T["memb"].data_ptr() + 8 * N.MF_COUNT * self.nmemb * i
        rec["mstart"] = T["mstart"].data_ptr() + 4 * (self.nmemb + 1) * i
        rec["nw"], rec["nn"], rec["nm"], rec["nhead"] = nw, nn, nm, 1
        rec["dw"], rec["depth"], rec["rho"], rec["g"] = self.dw, self.depth, self.rho, self.g
        rec["pdyn_rho_g"] = 1025.0 * 9.81                      # getWaveKin defaults (prep.DeviceDesign._make_struct)
        rec["M"] = [r[0].data_ptr() for r in rows]
        rec["B"] = [r[1].data_ptr() for r in rows]
        rec["mb_per_bin"] = [1 if r[2] else 0 for r in rows]
        rec["C"] = C.data_ptr() + 8 * 36 * i
        size = nn * 3 * nw
        c128 = dict(dtype=torch.complex128, device=self.device)
        K = torch.empty([int(size.sum())], **c128)
        Fi = torch.empty([n * 6 * nw], **c128)
        rec["uhat"] = 0
        rec["kproj"] = K.data_ptr() + 16 * np.concatenate([[0], np.cumsum(size)[:-1]])
        rec["finer"] = Fi.data_ptr() + 16 * 6 * nw * i
        arr = (N.RhDesign * n).from_buffer(rec)
        arr._rec = rec
        beta_t = self.f64(np.asarray(headings, dtype=float).reshape(n, 1), [n, 1])
        N.check(N.lib().rh_wave_tables_batch(N.context(self.dev_index), arr, n, N.ptr(beta_t), 1,
                                             N.stream_handle(torch, self.device)), "rh_wave_tables_batch")
        return BlockDesigns(torch, self.device, self.dev_index, arr, n, nw, int(nn.max()) if n else 0, nIter, XiStart,
                            (T, K, Fi, beta_t, rec, C, rows, self))

    def case_columns(self, cases):
        """The prepared case columns of solver.prepare_batch for a CaseSet over designs() (each pose has
        its one heading at table index 0)."""
        from .solver import balanced_order
        torch = self.torch
        n = cases.n
        head = np.zeros(n, dtype=np.int32)
        order = balanced_order(cases, head)
        ints = torch.from_numpy(np.concatenate([cases.design_idx, head, cases.spectrum, order]).astype(np.int32, copy=False)
                                ).to(self.device)
        flts = torch.from_numpy(np.concatenate([cases.Hs, cases.Tp, cases.gamma]).astype(np.float64, copy=False)
                                ).to(self.device)
        return dict(design=ints[:n], head=ints[n:2 * n], spectrum=ints[2 * n:3 * n], order=ints[3 * n:4 * n],
                    Hs=flts[:n], Tp=flts[n:2 * n], gamma=flts[2 * n:], head_host=head)

    def current_loads(self, X_ref, speed, heading_deg, depth, Zref, shearExp, rho):
        """rh_current_loads: the device tensor D [n, 6] of the cases' current loads at X_ref (a pure
        translation), about X_ref[:3]."""
        torch = self.torch
        n = len(speed)
        X_ref = np.ascontiguousarray(X_ref, dtype=float)
        if X_ref.shape != (6,):
            raise ValueError("current_loads: X_ref [6]")
        U = self.f64(speed, [n])
        H = self.f64(heading_deg, [n])
        D = torch.empty([n, 6], dtype=torch.float64, device=self.device)
        N.check(N.lib().rh_current_loads(N.context(self.dev_index), ctypes.byref(self.rec), X_ref.ctypes.data, n, N.ptr(U),
                                         N.ptr(H), float(depth), float(Zref), float(shearExp), float(rho), N.ptr(D),
                                         N.stream_handle(torch, self.device)), "rh_current_loads")
        D._keep = (U, H)
        return D


def pose_record(fowt, device=0):
    """The FOWT's PoseRecord on `device`, kept on the FOWT until its tables change (a new
    calcHydroConstants result, other members) or the device does."""
    host = host_record(fowt)
    cached = getattr(fowt, "_pose_dev", None)
    if cached is None or cached.dev_index != device or not cached.same_tables(host):
        cached = fowt._pose_dev = PoseRecord(fowt, device, host=host)
    return cached
