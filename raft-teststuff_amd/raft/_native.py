"""ctypes binding of librafthip.so (include/rafthip.h).

This is the drop-in boundary: the reference has no FFI, so the binding
a maintainer adds on the reference side is exactly this module.
There is no CPU fallback: importing the product on a machine without the built library
or without a visible GPU raises at the first call that needs the device.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAFTHIP_LIB", os.path.join(os.path.dirname(_HERE), "librafthip.so"))

RH_OK, RH_EINVAL, RH_ENAN, RH_ESINGULAR, RH_EHIP = 0, -1, -2, -3, -4
RH_QTF_INCIDENT_CACHED = 1
RH_CASE_CONVERGED, RH_CASE_NOT_CONVERGED, RH_CASE_NAN, RH_CASE_SINGULAR = 1, 0, -2, -3
SPECTRUM_CODES = {"JONSWAP": 0, "unit": 1, "constant": 2, "none": 3, "still": 3}

# node-table field order (enum rh_node_field)
NODE_FIELDS = ["RX", "RY", "RZ", "XX", "XY", "XZ", "QX", "QY", "QZ", "P1X", "P1Y", "P1Z", "P2X", "P2Y", "P2Z",
               "AQ", "AP1", "AP2", "AEND", "CDQ", "CDP1", "CDP2", "CDEND", "CIRC", "AI", "MCF",
               "I00", "I01", "I02", "I10", "I11", "I12", "I20", "I21", "I22", "T"]
NF = {name: i for i, name in enumerate(NODE_FIELDS)}
NF_COUNT = len(NODE_FIELDS)
MF_COUNT = 21   # enum rh_member_field: cq[6], c1[6], c2[6], |q|^2, |p1|^2, |p2|^2

_p = ctypes.c_void_p


class RhDesign(ctypes.Structure):
    _fields_ = [("nw", ctypes.c_int), ("nn", ctypes.c_int), ("nhead", ctypes.c_int), ("mb_per_bin", ctypes.c_int),
                ("dw", ctypes.c_double), ("depth", ctypes.c_double), ("rho", ctypes.c_double), ("g", ctypes.c_double),
                ("pdyn_rho_g", ctypes.c_double),
                ("w", _p), ("k", _p), ("node", _p), ("nm", ctypes.c_int), ("memb", _p), ("mstart", _p),
                ("imat_mcf", _p), ("uhat", _p), ("finer", _p), ("kproj", _p),
                ("M", _p), ("B", _p), ("C", _p)]


class RhCases(ctypes.Structure):
    _fields_ = [("ncase", ctypes.c_int), ("design", _p), ("head", _p), ("spectrum", _p),
                ("Hs", _p), ("Tp", _p), ("gamma", _p), ("nIter", ctypes.c_int),
                ("XiStart", ctypes.c_double), ("tol", ctypes.c_double), ("fext", _p), ("order", _p),
                ("Xi_init", _p), ("first_iter", ctypes.c_int)]


class RhSolveOut(ctypes.Structure):
    _fields_ = [("Xi", _p), ("Xi_last", _p), ("iters", _p), ("status", _p), ("zeta", _p), ("B_drag", _p),
                ("Bmat", _p), ("psd", _p), ("std", _p), ("rao", _p), ("Z", _p), ("Xi_prev", _p), ("margin", _p),
                ("F_wave", _p)]


class RhQtfDesign(ctypes.Structure):
    _fields_ = [("n2", ctypes.c_int), ("nq", ctypes.c_int), ("nmq", ctypes.c_int), ("nkr", ctypes.c_int),
                ("beta", ctypes.c_double), ("depth", ctypes.c_double), ("rho", ctypes.c_double), ("g", ctypes.c_double),
                ("w2", _p), ("k2", _p), ("qnode", _p), ("qmemb", _p), ("qmstart", _p), ("kstart", _p),
                ("kray", _p), ("hank", _p), ("order", ctypes.c_int)]


class RhBemDesign(ctypes.Structure):
    _fields_ = [("nw", ctypes.c_int), ("nhb", ctypes.c_int), ("nh", ctypes.c_int), ("pad_", ctypes.c_int),
                ("heading_adjust_deg", ctypes.c_double), ("x_ref", ctypes.c_double), ("y_ref", ctypes.c_double),
                ("k", _p), ("headings_deg", _p), ("X", _p), ("beta", _p), ("finer", _p), ("fbem", _p), ("fexc", _p)]


class RhMoorSystem(ctypes.Structure):
    _fields_ = [("nline", ctypes.c_int), ("pad_", ctypes.c_int), ("depth", ctypes.c_double), ("tol", ctypes.c_double),
                ("line", _p)]


# line-table field order (enum rh_moor_line_field)
MOOR_LINE_FIELDS = ["FX", "FY", "FZ", "AX", "AY", "AZ", "L", "EA", "W", "END"]
ML_COUNT = len(MOOR_LINE_FIELDS)
# drag-table row order of the calls with current on the lines (enum rh_moor_drag_field)
MOOR_DRAG_FIELDS = ["D", "CD", "CDAX", "RHO"]
MD_COUNT = len(MOOR_DRAG_FIELDS)
MOOR_MAX_LINES = 64
MOOR_STATUS = {0: "ok", 1: "catenary: XF < 0", 2: "catenary: L <= 0", 3: "catenary: EA <= 0",
               4: "catenary did not converge", 5: "statics Newton did not converge", 6: "singular step matrix",
               7: "system index out of range",
               8: "free-point equilibrium not converged within 500 evaluations",
               9: "singular free-point / condensation matrix"}


class RhMoorArraySystem(ctypes.Structure):
    _fields_ = [("nbody", ctypes.c_int), ("npoint", ctypes.c_int), ("nline", ctypes.c_int), ("nfree", ctypes.c_int),
                ("free_sys", ctypes.c_int), ("pad_", ctypes.c_int), ("g", ctypes.c_double), ("rho", ctypes.c_double),
                ("free_tol", ctypes.c_double), ("free_depth", ctypes.c_double), ("point", _p), ("line", _p),
                ("point_host", _p), ("line_host", _p)]


class RhPoseRecord(ctypes.Structure):
    _fields_ = [("nmemb", ctypes.c_int), ("nnode", ctypes.c_int), ("memb", _p), ("node", _p), ("mstart", _p),
                ("mstart_host", _p)]


# member-table row order of rh_pose_record (enum rh_pose_member_field) and the limits of its two calls
POSE_MEMBER_FIELDS = ["RA0X", "RA0Y", "RA0Z", "RB0X", "RB0Y", "RB0Z", "L", "Q0X", "Q0Y", "Q0Z", "P10X", "P10Y", "P10Z",
                      "P20X", "P20Y", "P20Z"]
PM_COUNT = len(POSE_MEMBER_FIELDS)
POSE_MAX_MEMBERS, POSE_MAX_NODES = 256, 1024


# point-table and line-table row order of a general system (enum rh_moor_point_field, rh_moor_aline_field)
MOOR_POINT_FIELDS = ["KIND", "INDEX", "X", "Y", "Z", "M", "V"]
MP = {name: i for i, name in enumerate(MOOR_POINT_FIELDS)}
MP_COUNT = len(MOOR_POINT_FIELDS)
MOOR_ALINE_FIELDS = ["A", "B", "L", "EA", "W", "DEPTH", "TOL", "SYS"]
MAL = {name: i for i, name in enumerate(MOOR_ALINE_FIELDS)}
MAL_COUNT = len(MOOR_ALINE_FIELDS)
ARR_MAX_BODIES, ARR_MAX_FREE = 4, 8


class RhRotor(ctypes.Structure):
    _fields_ = [("nr", ctypes.c_int), ("nsector", ctypes.c_int), ("B", ctypes.c_int), ("usecd", ctypes.c_int),
                ("tiploss", ctypes.c_int), ("hubloss", ctypes.c_int), ("wakerotation", ctypes.c_int),
                ("kx", ctypes.c_int), ("knot_stride", ctypes.c_int), ("pad_", ctypes.c_int),
                ("Rhub", ctypes.c_double), ("Rtip", ctypes.c_double), ("rho", ctypes.c_double), ("mu", ctypes.c_double),
                ("precone", ctypes.c_double), ("hubHt", ctypes.c_double), ("shearExp", ctypes.c_double),
                ("section", _p), ("nknot", _p), ("knots", _p), ("coef", _p),
                ("section_host", _p), ("nknot_host", _p), ("knots_host", _p), ("coef_host", _p)]


# section-table row order (enum rh_rotor_section_field) and the limits of rh_rotor_loads
ROTOR_SECTION_FIELDS = ["R", "CHORD", "THETA", "XAZ", "YAZ", "ZAZ", "CONE", "WEIGHT", "CONE_PATH"]
RS = {name: i for i, name in enumerate(ROTOR_SECTION_FIELDS)}
RS_COUNT = len(ROTOR_SECTION_FIELDS)
ROTOR_MAX_SECTIONS, ROTOR_MAX_SECTORS, ROTOR_MAX_KNOTS = 64, 16, 128
ROTOR_STATUS = {0: "ok", 1: "a blade section without a sign change of the BEM residual in any bracket",
                2: "non-finite rotor load", 3: "rotor index out of range"}
# parameter-row layout of rh_rotor_aero_mb (enum rh_aero_param_field) and its limit of pairs per case
AP = {"MODE": 0, "RQ": 1, "RHUB": 10, "I_DRIVETRAIN": 13, "NG": 14, "K_FLOAT": 15, "KP_BETA": 16, "KI_BETA": 17,
      "KP_TAU": 18, "KI_TAU": 19, "GYRO": 20}
AP_COUNT = 24
AERO_MAX_PAIRS = 8
# rh_turbine_channels: the channel order (enum rh_turbine_channel), the per-pair row (enum
# rh_chan_pair_field), the per-rotor geometry row (enum rh_chan_geom_field) and the limit of rotors
TC = {"AXRNA": 0, "MBASE": 1, "OMEGA": 2, "TORQUE": 3, "BPITCH": 4, "POWER": 5}
TC_SPECTRA, TC_COUNT = 5, 6
CP = {"ZHUB": 0, "KP_TAU": 1, "KI_TAU": 2}
CP_COUNT = 4
CG = {"ZREL": 0, "MT": 1, "ZCG": 2, "HARM": 3, "ICG": 4, "G": 5, "ZBASE": 6, "HAS_TOWER": 7}
CG_COUNT = 8
CHAN_MAX_ROTORS = 16


class NativeError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


def lib():
    """Load librafthip.so once; raise loudly if it is missing (no fallback path)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NativeError(f"librafthip.so not found at {LIB_PATH}: build it with "
                                  "`python -c 'import __graft_entry__ as g; g.build()'`")
            # torch first: its bundled HIP runtime has the same SONAME (libamdhip64.so.7) as the
            # one librafthip links, so loading torch first makes both share ONE runtime.  Loaded
            # the other way round, torch brings a second HIP/HSA runtime into the process and
            # the library's hipGetDeviceCount finds no device.
            import torch  # noqa: F401
            L = ctypes.CDLL(LIB_PATH)
            L.rh_last_error.restype = ctypes.c_char_p
            for name, args in {
                "rh_ctx_create": [ctypes.c_int, ctypes.POINTER(_p)],
                "rh_ctx_destroy": [_p],
                "rh_wave_tables": [_p, ctypes.POINTER(RhDesign), _p, _p, _p, _p, _p],
                "rh_wave_tables_batch": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, _p, ctypes.c_int, _p],
                "rh_bem_excitation": [_p, ctypes.c_int, _p, ctypes.c_int, _p, _p, ctypes.c_int, _p, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double, _p, _p, _p, _p],
                "rh_bem_excitation_batch": [_p, ctypes.c_int, ctypes.POINTER(RhBemDesign), _p, _p],
                "rh_moor_eval": [_p, ctypes.POINTER(RhMoorSystem), _p, ctypes.c_int, ctypes.c_int, _p, _p, _p, _p, _p, _p,
                                 _p, _p, _p],
                "rh_statics_solve": [_p, ctypes.POINTER(RhMoorSystem), _p, ctypes.c_int, ctypes.c_int, _p, _p, _p, _p,
                                     _p, _p, _p, _p, _p, _p],
                "rh_moor_eval_current": [_p, ctypes.POINTER(RhMoorSystem), _p, ctypes.c_int, ctypes.c_int, _p, _p, _p, _p,
                                         _p, _p, _p, _p, _p, _p, _p],
                "rh_statics_solve_current": [_p, ctypes.POINTER(RhMoorSystem), _p, ctypes.c_int, ctypes.c_int, _p, _p, _p,
                                             _p, _p, _p, _p, _p, _p, _p, _p, _p],
                "rh_moor_array_eval": [_p, ctypes.POINTER(RhMoorArraySystem), _p, ctypes.c_int, ctypes.c_int, _p, _p, _p,
                                       _p, _p, _p, _p, _p, _p, _p, _p],
                "rh_array_statics_solve": [_p, ctypes.POINTER(RhMoorArraySystem), _p, ctypes.c_int, ctypes.c_int, _p,
                                           _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p],
                "rh_pose_designs": [_p, ctypes.POINTER(RhPoseRecord), ctypes.c_int, _p, _p, _p, _p, _p, _p, _p],
                "rh_current_loads": [_p, ctypes.POINTER(RhPoseRecord), _p, ctypes.c_int, _p, _p, ctypes.c_double,
                                     ctypes.c_double, ctypes.c_double, ctypes.c_double, _p, _p],
                "rh_rotor_loads": [_p, ctypes.POINTER(RhRotor), _p, ctypes.c_int, ctypes.c_int, _p, _p, _p, _p, _p, _p,
                                   _p],
                "rh_rotor_aero_mb": [_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                     ctypes.c_int, _p, _p, _p, _p],
                "rh_turbine_channels": [_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, _p, _p, _p,
                                        ctypes.c_int, _p, ctypes.c_int, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                        ctypes.c_int, _p, _p, _p, _p, _p],
                "rh_solve_cases": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, ctypes.POINTER(RhCases),
                                   ctypes.POINTER(RhSolveOut), _p],
                "rh_heading_response": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, ctypes.c_int, _p, _p, _p, _p,
                                        _p, _p, _p],
                "rh_heading_response_ext": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, ctypes.c_int, _p, _p, _p,
                                            _p, _p, ctypes.c_int, _p, _p, _p],
                "rh_linearize": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, _p, _p, _p, _p, _p, _p],
                "rh_drag_excitation": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, _p, _p, _p, _p],
                "rh_lin_partial_sums": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, _p, _p, ctypes.c_int, ctypes.c_int,
                                        _p, _p],
                "rh_bin_step": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, _p, _p, _p, ctypes.c_double, ctypes.c_int,
                                ctypes.c_int, _p, _p, _p, _p, _p, _p],
                "rh_sea_state": [_p, ctypes.c_int, ctypes.c_int, _p, ctypes.c_double, _p, _p, _p, _p, _p, _p, _p],
                "rh_motion_stats": [_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, _p, _p, _p, _p],
                "rh_system_solve": [_p, ctypes.c_int, ctypes.c_int, _p, _p, _p, _p, _p],
                "rh_system_solve_batch": [_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _p, _p, _p, _p, _p],
                "rh_array_response": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, ctypes.c_int, ctypes.c_int, _p, _p,
                                      _p, _p, _p, _p, _p, _p],
                "rh_array_response_stats": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            _p, _p, _p, _p, _p, _p, _p, ctypes.c_double, _p, _p, _p, _p],
                "rh_array_solve_stats": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, ctypes.c_int, ctypes.c_int, _p, _p,
                                         _p, _p, ctypes.c_double, _p, _p, _p],
                "rh_array_solve_stats_ext": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, ctypes.c_int, ctypes.c_int, _p,
                                             _p, _p, ctypes.c_longlong, _p, ctypes.c_double, _p, _p, _p],
                "rh_wave_excitation": [_p, ctypes.POINTER(RhDesign), ctypes.c_int, ctypes.c_int, _p, _p, _p, _p, _p,
                                       _p],
                "rh_channel_stats": [_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, _p,
                                     _p, ctypes.c_int, _p, _p, _p, _p],
                "rh_qtf_slender": [_p, ctypes.POINTER(RhQtfDesign), ctypes.c_int, _p, _p, _p, _p, _p,
                                   ctypes.c_longlong, _p],
                "rh_qtf_slender_ext": [_p, ctypes.POINTER(RhQtfDesign), ctypes.c_int, _p, _p, _p, _p, _p,
                                       ctypes.c_longlong, ctypes.c_int, _p],
                "rh_qtf_slender_rows": [_p, ctypes.POINTER(RhQtfDesign), ctypes.c_int, _p, _p, _p, ctypes.c_int,
                                        ctypes.c_int, _p, _p, ctypes.c_longlong, _p],
                "rh_qtf_keeps_incident": [_p, ctypes.POINTER(RhQtfDesign)],
                "rh_qtf_hermitian_fill": [_p, ctypes.c_int, _p, _p],
                "rh_set_solver": [_p, ctypes.c_int],
                "rh_set_qtf_waves": [_p, ctypes.c_int],
                "rh_set_qtf_path": [_p, ctypes.c_int],
                "rh_qtf_hankel": [_p, ctypes.c_int, _p, ctypes.c_int, _p, _p, _p],
                "rh_force_2nd": [_p, ctypes.c_int, _p, _p, ctypes.c_int, _p, ctypes.c_double, _p, _p, _p, _p],
                "rh_force_2nd_batch": [_p, ctypes.c_int, ctypes.c_int, _p, _p, ctypes.c_int, _p, ctypes.c_int, _p,
                                       ctypes.c_double, _p, _p, _p, _p],
                "rh_force_2nd_spectrum": [_p, ctypes.c_int, _p, _p, ctypes.c_int, _p, ctypes.c_double, _p, _p, _p, _p,
                                          _p],
                "rh_prep_designs": [ctypes.c_int, _p, _p, ctypes.c_int, _p, _p, ctypes.c_int, ctypes.POINTER(_p)],
                "rh_prep_layout": [_p, _p],
                "rh_prep_copy": [_p, _p, _p, _p],
                "rh_qtf_tables": [ctypes.c_int, _p, ctypes.c_longlong, ctypes.c_double, _p, ctypes.c_longlong, _p,
                                  ctypes.c_longlong, _p],
            }.items():
                fn = getattr(L, name)
                fn.argtypes = args
                fn.restype = ctypes.c_int
            L.rh_prep_free.argtypes = [_p]
            L.rh_prep_free.restype = None
            L.rh_prep_imat.argtypes = [_p, ctypes.c_int, _p]
            L.rh_prep_imat.restype = ctypes.c_longlong
            L.rh_version.restype = ctypes.c_int
            L.rh_solve_noxi_max_bins.argtypes = []
            L.rh_solve_noxi_max_bins.restype = ctypes.c_int
            L.rh_qtf_workspace_bytes.argtypes = [ctypes.POINTER(RhQtfDesign)]
            L.rh_qtf_workspace_bytes.restype = ctypes.c_longlong
            _lib = L
    return _lib


def check(rc, what=""):
    """Map a C-ABI return code onto the reference's exception types."""
    if rc == RH_OK:
        return
    msg = lib().rh_last_error().decode(errors="replace")
    if rc == RH_EINVAL:
        raise ValueError(f"{what}: {msg}")
    if rc == RH_ENAN:
        raise Exception("Nan detected in response vector Xi.")   # raft/raft_model.py:957
    if rc == RH_ESINGULAR:
        raise np.linalg.LinAlgError("Singular matrix")
    raise NativeError(f"{what}: {msg}")


_ctx = {}


def context(device=0):
    """Per-(thread, device) library context (the ABI is thread-compatible, not thread-safe)."""
    key = (threading.get_ident(), device)
    c = _ctx.get(key)
    if c is None:
        h = _p()
        check(lib().rh_ctx_create(device, ctypes.byref(h)), "rh_ctx_create")
        c = _ctx[key] = h
    return c


def ptr(t):
    """Device pointer of a torch tensor (or None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("device tensor expected")
    if not t.is_contiguous():
        raise ValueError("contiguous tensor expected")
    return ctypes.c_void_p(t.data_ptr())


def stream_handle(torch, device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
