"""WAMIT-format first-order potential-flow coefficient files (.1 and .3) and their
interpolation onto a model's frequency grid.

The reference reads these files through pyHAMS (raft/raft_fowt.py:663-664, :727-728).  The
reader here is the project's own, written to the contract those call sites rely on:

* periods and headings are kept in order of first appearance in the file (no sorting);
* the file's columns are returned as they are (no scaling, no transposition);
* .1 rows with four columns (the zero- and infinite-frequency rows carry no damping) are
  accepted, with B = 0;
* with TFlag the first column holds periods: a negative period maps to w = 0, a zero period
  to w = inf, any other period T to 2 pi / T (WAMIT v7 manual, PER < 0 / PER = 0); without
  TFlag the first column is returned as frequencies;
* entries absent from the file are zero.

Host-side parsing of data the device consumes (rh_bem_excitation) or that enters the
per-bin M and B of a design (prep.linear_matrices).
"""
import numpy as np


def _rows(path, ncol_min):
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if len(p) < ncol_min:
                raise ValueError(f"{path}:{ln}: expected at least {ncol_min} columns, found {len(p)}")
            out.append([float(x) for x in p])
    if not out:
        raise ValueError(f"{path}: no data rows")
    return out


def _first_appearance(values):
    order = {}
    for v in values:
        if v not in order:
            order[v] = len(order)
    return order


def _omega(per, TFlag):
    per = np.asarray(per, dtype=float)
    if not TFlag:
        return per.copy()
    w = np.empty(len(per))
    for i, T in enumerate(per):
        w[i] = 0.0 if T < 0 else (np.inf if T == 0 else 2 * np.pi / T)
    return w


def read_wamit1(path, TFlag=False):
    """A WAMIT .1 file (rows PER I J A [B]).  Returns (A [6,6,nper], B [6,6,nper], w [nper])."""
    rows = _rows(path, 4)
    per = _first_appearance(r[0] for r in rows)
    A = np.zeros([6, 6, len(per)])
    B = np.zeros([6, 6, len(per)])
    for r in rows:
        i, j, ip = int(r[1]) - 1, int(r[2]) - 1, per[r[0]]
        if not (0 <= i < 6 and 0 <= j < 6):
            raise ValueError(f"{path}: mode indices ({i + 1}, {j + 1}) outside 1..6")
        A[i, j, ip] = r[3]
        if len(r) > 4:
            B[i, j, ip] = r[4]
    return A, B, _omega(list(per), TFlag)


def read_wamit3(path, TFlag=False):
    """A WAMIT .3 file (rows PER BETA I Mod Pha Re Im).  Returns (Mod, Pha, Re, Im
    [nhead,6,nper], w [nper], heads [nhead] in the file's degrees)."""
    rows = _rows(path, 7)
    per = _first_appearance(r[0] for r in rows)
    heads = _first_appearance(r[1] for r in rows)
    out = np.zeros([4, len(heads), 6, len(per)])
    for r in rows:
        i = int(r[2]) - 1
        if not 0 <= i < 6:
            raise ValueError(f"{path}: mode index {i + 1} outside 1..6")
        out[:, heads[r[1]], i, per[r[0]]] = r[3:7]
    return out[0], out[1], out[2], out[3], _omega(list(per), TFlag), np.array(list(heads), dtype=float)


def bem_tables(hydroPath, w, rho, g, sort_headings):
    """A_BEM, B_BEM [6,6,nw], X_BEM [nhead,6,nw] and BEM_headings [deg, 0..360) of the files
    hydroPath + '.1' / '.3' on the grid w, as FOWT.readHydro (sort_headings False,
    raft/raft_fowt.py:719-767) and FOWT.calcBEM (True, :661-714) build them: the first two
    frequency entries of the .1 data dropped, entry 0 of the added mass, zero damping and zero
    excitation appended at w = 0, linear interpolation that raises outside the files' range,
    and each heading's excitation rotated into its own wave frame."""
    from scipy.interpolate import interp1d
    addedMass, damping, w1 = read_wamit1(hydroPath + ".1", TFlag=True)
    M, P, R, I, w3, heads = read_wamit3(hydroPath + ".3", TFlag=True)
    headings = np.array(heads) % 360
    if sort_headings:
        idx = np.argsort(headings)
        headings = headings[idx]
        R, I = R[idx, :, :], I[idx, :, :]
        frame = headings                 # calcBEM rotates by the sorted 0..360 headings (:697-699)
    else:
        frame = np.array(heads)          # readHydro by the file's own values (:750-752)
    w = np.asarray(w, dtype=float)
    w1x, w3x = np.hstack([w1[2:], 0.0]), np.hstack([w3, 0.0])
    for name, wx in ((".1", w1x), (".3", w3x)):
        if w.min() < wx.min() or w.max() > wx.max():
            raise ValueError(f"{hydroPath}{name}: the model frequencies [{w.min():.4g}, {w.max():.4g}] rad/s reach "
                             f"outside the file's range [{wx.min():.4g}, {wx.max():.4g}] rad/s")
    nh = len(heads)
    a = interp1d(w1x, np.dstack([addedMass[:, :, 2:], addedMass[:, :, 0]]), assume_sorted=False, axis=2)(w)
    b = interp1d(w1x, np.dstack([damping[:, :, 2:], np.zeros([6, 6])]), assume_sorted=False, axis=2)(w)
    re = interp1d(w3x, np.dstack([R, np.zeros([nh, 6])]), assume_sorted=False, axis=2)(w)
    im = interp1d(w3x, np.dstack([I, np.zeros([nh, 6])]), assume_sorted=False, axis=2)(w)
    A_BEM = rho * a
    B_BEM = rho * b
    Xt = rho * g * (re + 1j * im)
    X = np.zeros_like(Xt)
    for ih in range(nh):
        s, c = np.sin(np.radians(frame[ih])), np.cos(np.radians(frame[ih]))
        X[ih, 0, :] = c * Xt[ih, 0, :] + s * Xt[ih, 1, :]
        X[ih, 1, :] = -s * Xt[ih, 0, :] + c * Xt[ih, 1, :]
        X[ih, 2, :] = Xt[ih, 2, :]
        X[ih, 3, :] = c * Xt[ih, 3, :] + s * Xt[ih, 4, :]
        X[ih, 4, :] = -s * Xt[ih, 3, :] + c * Xt[ih, 4, :]
        X[ih, 5, :] = Xt[ih, 5, :]
    if np.isnan(A_BEM).any():
        raise Exception("NaN values detected in HAMS calculations for added mass. Check the geometry.")
    if np.isnan(B_BEM).any():
        raise Exception("NaN values detected in HAMS calculations for damping. Check the geometry.")
    if np.isnan(X).any():
        raise Exception("NaN values detected in HAMS calculations for excitation. Check the geometry.")
    return A_BEM, B_BEM, X, headings
