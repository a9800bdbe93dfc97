"""Synthetic designs, grids, a long-double reference and the criterion for the direct tests of the
slender-body QTF kernels (tests/test_gpu_qtf_cases.py; checked on the CPU by tests/test_qtf_cases.py).

Designs are small member dictionaries put through raft.member.Member (the strip tables the product
makes) on a stand-in for the FOWT with the four attributes raft.qtf reads (memberList, rho_water, g,
depth); oracle_tables() states the same members as the table dictionary of oracle.qtf_oracle.

The reference, qtf_reference(), restates oracle/qtf_oracle.py qtf_slender branch for branch (grad_u1,
grad_pres1st, pot2nd, correction_kay, _member_terms, the Pinkster term, the RAO interpolation, the
Hermitian fill, the k h >= 10 and k h > 89.4 switches decided on the doubles as the oracle decides
them) in NumPy longdouble / clongdouble of the double inputs (w2, k2 = wave_numbers(w2, depth), the
node tables, the RAO, M_struc); the Hankel derivatives come from mpmath at 40 digits.  Beside
ref[n2, n2, 6] it returns the scale S[n2, n2, 6]: the sum of the absolute values of every addend of an
entry at the finest granularity the restatement has -- each force addend of each node (strip, end
volume and end pressure apart) and of each waterline, each product of the Pinkster cross products, each
Hankel order of each Kim & Yue row; in a moment each of the two products of r x f.  u S bounds the
rounding a reassociated double sum of those addends carries.

Criterion: worst(x, ref, S) = max |x - ref| / (u S), u = 2^-53, over all pairs and DOFs; where S is 0
the entry has no addend and x must be exactly 0.
"""
import types

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).eps < 2.0 ** -60, "np.longdouble is not an extended type here"
U = 2.0 ** -53
DEG2RAD = 0.017453292519943295
RHO, G = 1025.0, 9.81
# The float64 oracle's own worst() against this reference over every synthetic case on which it is finite,
# and the cap of max S / |ref|: measured and asserted by tests/test_qtf_cases.py (its header has the date).
# The oracle's distance is the (2 k h) u relative error of cosh(k (z + h)) / sinh(k h) formed in double
# below the k h = 89.4 switch of the Airy kinematics: a rounded argument of size k h moves an exponential by
# k h u.  A_FIX, for the reference-pinned fixtures, is that bound for a product of two such ratios: the three
# arguments of each ratio carry up to 3 k h u together, 6 x 89.4 u for the pair, plus 64 u for the sums.
A_ORC = 201.0
AMP_CAP = 2.0e4
A_FIX = 6 * 89.4 + 64
BAR = 8 * max(A_ORC, 4.0)          # the device bar of tests/test_gpu_qtf_cases.py, in units of u S

# ------------------------------------------------------------------------------------------------
# designs
# ------------------------------------------------------------------------------------------------
_MEMBERS = {
    # vertical, tapered, MacCamy-Fuchs, through the surface; a repeated station gives an inner dls == 0 node
    "col": dict(rA=[6, -4, -18], rB=[6, -4, 8], shape="circ", stations=[0, 14, 14, 26], d=[9, 9, 7.5, 6], MCF=True,
                dlsMax=6, Ca=0.93, CaEnd=0.7),
    # inclined, rectangular, submerged, Ca_p1 != Ca_p2 and varying along the member (Rainey term)
    "pont": dict(rA=[-10, 3, -16], rB=[2, 9, -11], shape="rect", stations=[0, 1], d=[[4, 2.5], [3, 2]], gamma=20.0,
                 dlsMax=5, Ca=[[0.9, 0.6], [0.8, 0.55]], CaEnd=0.5),
    # inclined, circular, through the surface; its top wet strip is partly submerged (Q12)
    "brace": dict(rA=[-8, -6, -12], rB=[-2, -1, 5], shape="circ", stations=[0, 1], d=[2, 1.6], dlsMax=4, Ca=0.97,
                  CaEnd=0.6),
    # horizontal; its two end nodes (dls == 0) carry end volumes
    "hor": dict(rA=[-5, 8, -9], rB=[7, 4, -9], shape="circ", stations=[0, 1], d=[3, 2], dlsMax=7, Ca=1.0, CaEnd=0.8),
    "hor2": dict(rA=[-5, 8, -9], rB=[7, 4, -9], shape="circ", stations=[0, 1], d=[3, 2], dlsMax=5, Ca=1.0, CaEnd=0.8),
    # entirely above the water: skipped
    "dry": dict(rA=[0, 0, 3], rB=[4, 2, 9], shape="circ", stations=[0, 1], d=[1, 1], dlsMax=3),
    "dry2": dict(rA=[-3, 1, 2], rB=[-3, 1, 7], shape="rect", stations=[0, 1], d=[[1, 2], [1, 2]], dlsMax=3),
    # a second vertical column, not MacCamy-Fuchs
    "col2": dict(rA=[-12, 10, -7], rB=[-12, 10, 4], shape="circ", stations=[0, 1], d=[5, 5], dlsMax=3, Ca=0.9,
                 CaEnd=0.6),
    # "one": vertical circular non-MCF columns through the surface with 1, 8 and 9 wet nodes
    "one1": dict(rA=[4, 3, -1], rB=[4, 3, 9], shape="circ", stations=[0, 1], d=[6, 6], dlsMax=20, Ca=0.95, CaEnd=0.6),
    "one8": dict(rA=[4, 3, -14], rB=[4, 3, 4], shape="circ", stations=[0, 1], d=[6, 6], dlsMax=2, Ca=0.95, CaEnd=0.6),
    "one9": dict(rA=[4, 3, -16], rB=[4, 3, 4], shape="circ", stations=[0, 1], d=[6, 6], dlsMax=2, Ca=0.95, CaEnd=0.6),
    # a MacCamy-Fuchs spar whose lowest nodes sit at z = -150 m and -136.5 m
    "spar": dict(rA=[2, -3, -150], rB=[2, -3, 12], shape="circ", stations=[0, 1], d=[8, 8], MCF=True, dlsMax=30,
                 Ca=0.95, CaEnd=0.6),
}

DESIGNS = {
    "one": ["one1"], "one8": ["one8"], "one9": ["one9"],
    "mix": ["col", "pont", "brace", "hor", "dry"],              # nmq = 4, nq even: 2 pad rows of K
    "tail0": ["col", "hor2"],                                   # nmq = 2, nq odd: no pad row
    "tail15": ["col", "pont", "brace", "hor", "dry", "col2"],   # nmq = 5, nq even: 15 pad rows
    "spar": ["spar", "brace", "hor"],
    "dry": ["dry", "dry2"],                                     # nq = 0: the Pinkster term alone
}
# what each design is there for: (nq, nmq, nkr), asserted by tests/test_qtf_cases.py
EXPECT = {"one": (1, 1, 0), "one8": (8, 1, 0), "one9": (9, 1, 0), "mix": (20, 4, 7), "tail0": (11, 2, 7),
          "tail15": (24, 5, 7), "spar": (16, 3, 8), "dry": (0, 0, 0)}


def make_fowt(design, depth):
    """The stand-in for a FOWT: what raft.qtf.QtfDevice / native_tables / build_tables read."""
    from raft.member import Member
    mems = []
    for name in DESIGNS[design]:
        m = Member(dict(_MEMBERS[name], name=name, type=2), 1)
        m.calcHydroConstants(rho=RHO, g=G)                      # a_i of the wet nodes
        mems.append(m)
    return types.SimpleNamespace(memberList=mems, rho_water=RHO, g=G, depth=float(depth), design=design)


def mass_matrix():
    """A symmetric M_struc with every inertia coupling (the QTF reads M[0, 0] and M[3:, 3:])."""
    M = np.zeros([6, 6])
    M[0, 0] = M[1, 1] = M[2, 2] = 2.3e6
    M[3:, 3:] = np.array([[9.1e8, 1.2e7, -3.4e7], [1.2e7, 8.7e8, 2.2e7], [-3.4e7, 2.2e7, 1.1e9]])
    M[0, 4] = M[4, 0] = -2.3e6 * 7.0
    M[1, 3] = M[3, 1] = 2.3e6 * 7.0
    return M


def oracle_tables(fowt, w):
    """The table dictionary oracle.qtf_oracle.qtf_slender takes, of the stand-in's members."""
    rows = []
    for im, mem in enumerate(fowt.memberList):
        for il in range(mem.ns):
            rows.append(dict(member=im, r=mem.r[il].copy(), q=mem.q, p1=mem.p1, p2=mem.p2,
                             ds=np.resize(np.atleast_1d(mem.ds[il]).astype(float), 2),
                             drs=np.resize(np.atleast_1d(mem.drs[il]).astype(float), 2), dls=float(mem.dls[il]),
                             Ca_p1=mem.coef("Ca_p1", il), Ca_p2=mem.coef("Ca_p2", il), Ca_End=mem.coef("Ca_End", il),
                             a_i=float(mem.a_i[il])))
    T = {"node_member": np.array([r["member"] for r in rows], dtype=np.int64)}
    for k in ("r", "q", "p1", "p2", "ds", "drs", "dls", "Ca_p1", "Ca_p2", "Ca_End", "a_i"):
        T["node_" + k] = np.array([r[k] for r in rows], dtype=float)
    ml = fowt.memberList
    T.update(member_circ=np.array([int(m.shape == "circular") for m in ml]),
             member_mcf=np.array([int(bool(m.MCF)) for m in ml]), member_rA=np.array([m.rA for m in ml]),
             member_rB=np.array([m.rB for m in ml]), w=np.asarray(w, dtype=float), M_struc=mass_matrix(),
             depth=np.float64(fowt.depth), rho=np.float64(fowt.rho_water), g=np.float64(fowt.g))
    return T


# ------------------------------------------------------------------------------------------------
# grids, environments, RAOs
# ------------------------------------------------------------------------------------------------
def _threshold_grid(h):
    """17 frequencies in depth h; two neighbouring pairs bracket k h = 10 and k h = 89.4 by +-1e-3."""
    wt = [np.sqrt(G * (x / h) * np.tanh(x)) for x in (10.0, 89.4)]          # 0.7004 and 2.0941 rad/s at 200 m
    base = np.linspace(0.35, 2.35, 13)
    return np.sort(np.concatenate([base, [wt[0] * (1 - 1e-3), wt[0] * (1 + 1e-3), wt[1] * (1 - 1e-3), wt[1] * (1 + 1e-3)]]))


def _grid(n2):
    if n2 == 1:
        return np.array([0.83])
    return np.linspace(0.31, 2.17, n2) + 1e-3 / np.pi


W1 = np.linspace(0.2, 3.1, 30)               # first-order grid that covers every second-order grid
W1_COARSE = np.linspace(0.4, 1.4, 8)         # coarser, and begins and ends inside the second-order grid

# name -> (design, depth, w2, heading [deg], RAO kind: "moving" | "fixed" | "coarse")
CASES = {}
for _n2, _hd in zip((1, 2, 15, 16, 17, 33), (30.0, 200.0, 90.0, 30.0, 200.0, 30.0)):
    CASES[f"one_n{_n2}"] = ("one", 200.0, _grid(_n2), _hd, "moving")
for _n2, _hd in zip((1, 2, 15, 16, 17, 33), (200.0, 90.0, 0.0, 200.0, 30.0, 90.0)):
    CASES[f"mix_n{_n2}"] = ("mix", 200.0, _grid(_n2), _hd, "moving")
CASES.update({
    "one8": ("one8", 200.0, _grid(17), 30.0, "moving"),
    "one9": ("one9", 200.0, _grid(17), 200.0, "moving"),
    "tail0": ("tail0", 200.0, _grid(17), 30.0, "moving"),
    "tail15": ("tail15", 200.0, _grid(17), 200.0, "moving"),
    "thresholds": ("mix", 200.0, _threshold_grid(200.0), 30.0, "moving"),
    "deep_node": ("spar", 200.0, np.linspace(0.4, 3.0, 16), 30.0, "moving"),
    "shallow": ("mix", 30.0, np.linspace(0.28, 1.9, 16), 200.0, "moving"),
    "deep": ("mix", 1000.0, np.linspace(0.4, 2.6, 16), 30.0, "moving"),
    "fixed": ("mix", 200.0, _grid(17), 30.0, "fixed"),
    "coarse": ("mix", 200.0, _grid(17), 90.0, "coarse"),
    "head0": ("tail15", 200.0, _grid(16), 0.0, "moving"),
    "dry": ("dry", 200.0, _grid(17), 30.0, "moving"),
})
_u = _grid(17).copy()
_u[[5, 6]] = _u[[6, 5]]
CASES["unsorted"] = ("mix", 200.0, _u, 30.0, "moving")
SORTED = [c for c in CASES if c != "unsorted"]
CACHED = ["mix_n17", "tail0", "tail15", "mix_n16"]       # kept incident parts: "mix" and the K-tail designs


def rao(kind, seed=0):
    """(w [nw], Xi0 [6, nw] or None): a smooth complex RAO that moves in all six DOFs."""
    if kind == "fixed":
        return W1.copy(), None
    w = (W1_COARSE if kind == "coarse" else W1).copy()
    rng = np.random.default_rng(1234 + seed)
    amp = np.array([0.8, 0.6, 0.5, 0.03, 0.04, 0.02])[:, None] * (1 + 0.5 * np.cos(1.7 * w + np.arange(6)[:, None]))
    ph = rng.uniform(-np.pi, np.pi, [6, 1]) + 0.9 * np.arange(1, 7)[:, None] * w
    return w, amp * np.exp(1j * ph)


def case(name, seed=0):
    """Everything of one case: the stand-in, the grids, the RAO, the oracle's tables."""
    from raft.hydro_math import wave_numbers
    design, depth, w2, hd, kind = CASES[name]
    fowt = make_fowt(design, depth)
    w, X = rao(kind, seed)
    k2 = wave_numbers(w2, depth)
    T = oracle_tables(fowt, w)
    Xz = np.zeros([6, len(w)], dtype=complex) if X is None else X
    return types.SimpleNamespace(name=name, design=design, fowt=fowt, depth=depth, w2=w2.copy(), k2=k2,
                                 beta=float(np.deg2rad(hd)), kind=kind, w=w, Xi0=X, Xz=Xz, T=T, M=T["M_struc"],
                                 n2=len(w2))


# ------------------------------------------------------------------------------------------------
# the long-double reference
# ------------------------------------------------------------------------------------------------
def _interp0(x, xp, fp):
    """np.interp(x, xp, fp, left=0, right=0) in long double (xp increasing; x in any order)."""
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, len(xp) - 2)
    v = fp[j] + (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j])
    v = np.where(x == xp[-1], fp[-1], v)
    return np.where((x < xp[0]) | (x > xp[-1]), CLD(0), v)


_HANK = {}


def _mp_of(x):
    import mpmath
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def _ld_of(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def hank_d(x):
    """D_n(x) = 0.5 (H1_{n-1}(x) - H1_{n+1}(x)), n = 0..11, of a long-double x: mpmath at 40 digits."""
    import mpmath
    key = (float(x), float(x - LD(float(x))))
    hit = _HANK.get(key)
    if hit is None:
        with mpmath.workdps(40):
            xm = _mp_of(x)
            H = [mpmath.hankel1(n, xm) for n in range(-1, 13)]
            D = [(H[n] - H[n + 2]) / 2 for n in range(12)]
            hit = np.array([CLD(_ld_of(d.real)) + CLD(1j) * CLD(_ld_of(d.imag)) for d in D], dtype=CLD)
        _HANK[key] = hit
    return hit


def _hank_table(kR):
    return np.array([hank_d(x) for x in kR], dtype=CLD)          # [n2, 12]


class _Acc:
    """Q [npair, 6] and its scale S: put(f, r) adds [f; r x f] of a force addend f [npair, 3]."""

    def __init__(self, npair):
        self.Q = np.zeros([npair, 6], dtype=CLD)
        self.S = np.zeros([npair, 6], dtype=LD)

    def put(self, f, r):
        a = np.abs(f)
        self.Q[:, :3] += f
        self.S[:, :3] += a
        for d, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
            self.Q[:, 3 + d] += r[i] * f[:, j] - r[j] * f[:, i]
            self.S[:, 3 + d] += np.abs(r[i]) * a[:, j] + np.abs(r[j]) * a[:, i]


def _mv(A, x):
    if A.ndim == 2:
        return x @ A.T
    return (A * x[:, None, :]).sum(axis=-1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _cross_abs(a, b):
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], axis=-1)


def _small_rotate(r, th):
    return np.array([-th[2] * r[1] + th[1] * r[2], th[2] * r[0] - th[0] * r[2], -th[1] * r[0] + th[0] * r[1]])


def _kinematics(r, Xi, w):
    dr = Xi[:3] + _small_rotate(r, Xi[3:])
    v = 1j * w * dr
    return dr, v, 1j * w * v


def _kh(k, h):
    return k.astype(float) * float(h)          # the switches are decided on the doubles, as the oracle decides them


def _wave_kin(beta, w, k, h, r, rho, g):
    nw = len(w)
    zeta = np.exp(-1j * (k * (np.cos(beta) * r[0] + np.sin(beta) * r[1])))
    u = np.zeros([3, nw], dtype=CLD)
    ud = np.zeros([3, nw], dtype=CLD)
    z = r[2]
    if z <= 0:
        deep = _kh(k, h) > 89.4
        s_sh = np.where(deep, np.exp(k * z), np.sinh(k * (z + h)) / np.sinh(k * h))
        c_sh = np.where(deep, np.exp(k * z), np.cosh(k * (z + h)) / np.sinh(k * h))
        u[0] = w * zeta * c_sh * np.cos(beta)
        u[1] = w * zeta * c_sh * np.sin(beta)
        u[2] = 1j * w * zeta * s_sh
        ud[:] = 1j * w * u
        return u, ud, zeta * (rho * g) * np.where(deep, np.exp(k * z) + np.exp(-k * (z + 2 * h)),
                                                   np.cosh(k * (z + h)) / np.cosh(k * h))
    return u, ud, np.zeros(nw, dtype=CLD)


def _grad_u1(w, k, beta, h, r):
    n = len(w)
    g = np.zeros([n, 3, 3], dtype=CLD)
    x, y, z = r
    cb, sb = np.cos(beta * LD(DEG2RAD)), np.sin(beta * LD(DEG2RAD))           # Q1
    if z > 0:
        return g
    deep = _kh(k, h) >= 10
    kxy = np.where(deep, np.exp(k * z), np.cosh(k * (z + h)) / np.sinh(k * h))
    kz = np.where(deep, np.exp(k * z), np.sinh(k * (z + h)) / np.sinh(k * h))
    ph = np.exp(-1j * (k * (np.cos(beta) * x + np.sin(beta) * y)))
    aux = w * cb * ph
    g[:, 0, 0] = -1j * aux * kxy * k * cb
    g[:, 0, 1] = -1j * aux * kxy * k * sb
    g[:, 0, 2] = aux * k * kz
    aux = w * sb * ph
    g[:, 1, 0] = g[:, 0, 1]
    g[:, 1, 1] = -1j * aux * kxy * k * sb
    g[:, 1, 2] = aux * k * kz
    aux = 1j * w * ph
    g[:, 2, 0] = g[:, 0, 2]
    g[:, 2, 1] = g[:, 0, 1]                                                    # Q2
    g[:, 2, 2] = aux * k * kxy
    g[~(k > 0)] = 0
    return g


def _grad_pres1st(k, beta, h, r, rho, g):
    out = np.zeros([len(k), 3], dtype=CLD)
    x, y, z = r
    cb, sb = np.cos(beta * LD(DEG2RAD)), np.sin(beta * LD(DEG2RAD))
    if z > 0:
        return out
    deep = _kh(k, h) >= 10
    kxy = np.where(deep, np.exp(k * z), np.cosh(k * (z + h)) / np.cosh(k * h))
    kz = np.where(deep, np.exp(k * z), np.sinh(k * (z + h)) / np.cosh(k * h))
    ph = np.exp(-1j * (k * (cb * x + sb * y)))
    out[:, 0] = rho * g * kxy * ph * (-1j * k * cb)
    out[:, 1] = rho * g * kxy * ph * (-1j * k * sb)
    out[:, 2] = rho * g * kz * ph * k
    out[~(k > 0)] = 0
    return out


def pot2nd_denominator(w1, w2, k1, k2, beta, h, g):
    """The two terms of the second-order potential's denominator, in long double."""
    b = LD(beta) * LD(DEG2RAD)
    kx, ky = (k1 - k2) * np.cos(b), (k1 - k2) * np.sin(b)
    nk = np.sqrt(kx * kx + ky * ky)
    return (w1 - w2) ** 2 / g, nk * np.tanh(nk * h)


def _pot2nd(w1, w2, k1, k2, beta, h, r, g, rho):
    n = len(w1)
    acc = np.zeros([n, 3], dtype=CLD)
    p = np.zeros(n, dtype=CLD)
    z = r[2]
    b = beta * LD(DEG2RAD)                                                     # Q1
    cb, sb = np.cos(b), np.sin(b)
    m = (w1 != w2) & (k1 > 0) & (k2 > 0)
    if z > 0 or not m.any():
        return acc, p
    w1, w2, k1, k2 = w1[m], w2[m], k1[m], k2[m]
    kx = k1 * cb - k2 * cb
    ky = k1 * sb - k2 * sb
    nk = np.sqrt(kx * kx + ky * ky)
    t1, t2 = np.tanh(k1 * h), np.tanh(k2 * h)
    g12 = (-1j * g / (2 * w1)) * ((k1 ** 2) * (1 - t1 ** 2) - 2 * k1 * k2 * (1 + t1 * t2)) / \
        ((w1 - w2) ** 2 / g - nk * np.tanh(nk * h))
    g21 = (-1j * g / (2 * w2)) * ((k2 ** 2) * (1 - t2 ** 2) - 2 * k2 * k1 * (1 + t2 * t1)) / \
        ((w2 - w1) ** 2 / g - nk * np.tanh(nk * h))
    aux = 0.5 * (g21 + np.conj(g12))
    kxy = np.cosh(nk * (z + h)) / np.cosh(nk * h)
    kz = np.sinh(nk * (z + h)) / np.cosh(nk * h)
    ph = np.exp(-1j * (kx * r[0] + ky * r[1]))
    a = np.zeros([len(w1), 3], dtype=CLD)
    a[:, 0] = aux * kxy * ph * ((w1 - w2) * kx)
    a[:, 1] = aux * kxy * ph * ((w1 - w2) * ky)
    a[:, 2] = aux * kz * ph * (1j * (w1 - w2) * nk)
    acc[m] = a
    p[m] = aux * kxy * ph * (-1j * rho * (w1 - w2))
    return acc, p


def _omega_mat(v):
    n = len(v)
    H = np.zeros([n, 3, 3], dtype=CLD)
    H[:, 0, 1], H[:, 0, 2] = v[:, 2], -v[:, 1]
    H[:, 1, 0], H[:, 1, 2] = -v[:, 2], v[:, 0]
    H[:, 2, 0], H[:, 2, 1] = v[:, 1], -v[:, 0]
    return -H


class _Member:
    """oracle.qtf_oracle.MemberView in long double."""

    def __init__(self, T, im):
        sel = np.nonzero(np.asarray(T["node_member"]) == im)[0]
        ld = lambda k: np.asarray(T[k], dtype=float)[sel].astype(LD)      # noqa: E731
        self.r = ld("node_r")
        self.q, self.p1, self.p2 = ld("node_q")[0], ld("node_p1")[0], ld("node_p2")[0]
        self.ds, self.drs, self.dls = ld("node_ds"), ld("node_drs"), ld("node_dls")
        self.Ca_p1, self.Ca_p2, self.Ca_End, self.a_i = ld("node_Ca_p1"), ld("node_Ca_p2"), ld("node_Ca_End"), ld("node_a_i")
        self.circ, self.mcf = bool(T["member_circ"][im]), bool(T["member_mcf"][im])
        self.rA, self.rB = T["member_rA"][im].astype(LD), T["member_rB"][im].astype(LD)
        self.qMat, self.p1Mat, self.p2Mat = np.outer(self.q, self.q), np.outer(self.p1, self.p1), np.outer(self.p2, self.p2)
        self.ns = len(sel)


def _correction_kay(acc, mem, h, w2, k2, i1, i2, beta, rho, g, Nm=10):
    if not mem.mcf:
        return
    W1, W2, K1, K2 = w2[i1], w2[i2], k2[i1], k2[i2]
    npair = len(i1)
    part = _Acc(npair)
    cb, sb = np.cos(beta), np.sin(beta)
    kk = np.stack([K1 * cb - K2 * cb, K1 * sb - K2 * sb, 0 * K1], axis=1)
    bv = np.array([cb, sb, LD(0)])
    pf = np.dot(bv, mem.p1) * mem.p1 + np.dot(bv, mem.p2) * mem.p2
    pf = pf / np.sqrt(np.sum(pf * pf))
    if not (mem.rA[2] * mem.rB[2] < 0):
        return
    rwl = mem.rA + (mem.rB - mem.rA) * (0 - mem.rA[2]) / (mem.rB[2] - mem.rA[2])
    radii = 0.5 * mem.ds[:, 0]
    j = int(np.clip(np.searchsorted(mem.r[:, 2], 0, side="right") - 1, 0, mem.ns - 2))      # np.interp(0, z, radii)
    R = radii[j] + (radii[j + 1] - radii[j]) / (mem.r[j + 1, 2] - mem.r[j, 2]) * (0 - mem.r[j, 2])
    phase = np.exp(-1j * (kk @ rwl))
    pi = np.arctan(LD(1)) * 4

    def omega(D, nn):
        return 1 / (D[i1, nn + 1] * np.conj(D[i2, nn])) - 1 / (D[i1, nn] * np.conj(D[i2, nn + 1]))

    def put(terms, at):
        """terms [Nm + 1][npair] complex: the row's force is Re(sum) * phase along pf, at `at`."""
        val = np.real(sum(terms))
        sc = sum(np.abs(np.real(t)) for t in terms)
        f = (val * phase)[:, None] * pf[None, :]
        part.put(f, at)
        # put() took |f| of the summed orders; the scale of the orders apart replaces it
        fa = sc[:, None] * np.abs(pf)[None, :]
        a = np.abs(f)
        part.S[:, :3] += fa - a
        for d, (i, jj) in enumerate(((1, 2), (2, 0), (0, 1))):
            part.S[:, 3 + d] += np.abs(at[i]) * (fa[:, jj] - a[:, jj]) + np.abs(at[jj]) * (fa[:, i] - a[:, i])

    k1R, k2R = K1 * R, K2 * R
    D = _hank_table(k2 * R)
    put([-rho * g * R * 2j / pi / (k1R * k2R) * omega(D, nn) for nn in range(Nm + 1)], rwl)
    for il in range(mem.ns - 1):
        z1 = mem.r[il, 2]
        if z1 > 0:
            continue
        z2 = mem.r[il + 1, 2]
        z2 = LD(0) if z2 > 0 else z2
        R1 = mem.ds[il, 0] / 2
        if mem.dls[il] == 0:
            R1 = mem.ds[il, 0]
        R2 = mem.ds[il + 1, 0] / 2
        if mem.dls[il + 1] == 0:
            R2 = mem.ds[il, 0]                                                  # Q9
        Rm = 0.5 * (R1 + R2)
        k1R, k2R = K1 * Rm, K2 * Rm
        H = h / Rm
        k1h, k2h = k1R * H, k2R * H
        eq = W1 == W2
        with np.errstate(divide="ignore", invalid="ignore"):
            a2 = np.sinh((K1 + K2) * (z2 + h)) / (k1h + k2h)
            a1 = np.sinh((K1 + K2) * (z1 + h)) / (k1h + k2h)
            d2 = np.sinh((K1 - K2) * (z2 + h)) / (k1h - k2h)
            d1 = np.sinh((K1 - K2) * (z1 + h)) / (k1h - k2h)
        Im = np.where(eq, 0.5 * (a2 - (z2 + h) / h - a1 + (z1 + h) / h), 0.5 * (a2 - d2 - a1 + d1))
        Ip = np.where(eq, 0.5 * (a2 + (z2 + h) / h - a1 - (z1 + h) / h), 0.5 * (a2 + d2 - a1 - d1))
        ch1, ch2 = np.cosh(k1h), np.cosh(k2h)
        D = _hank_table(k2 * Rm)
        terms = [rho * g * Rm * 2j / pi / (k1R * k2R) * omega(D, nn) * (
            k1h * k2h / np.sqrt(k1h * np.tanh(k1h)) / np.sqrt(k2h * np.tanh(k2h))
            * (Im + Ip * nn * (nn + 1) / k1R / k2R) / ch1 / ch2) for nn in range(Nm + 1)]
        put(terms, 0.5 * (mem.r[il] + mem.r[il + 1]))
    acc.Q += np.where((K1 < K2)[:, None], np.conj(part.Q), part.Q)
    acc.S += part.S


def _member_terms(acc, mem, Xi, w2, k2, i1, i2, beta, h, rho, g):
    n2 = len(w2)
    W1, W2, K1, K2 = w2[i1], w2[i2], k2[i1], k2[i2]
    q, p1Mat, p2Mat, qMat = mem.q, mem.p1Mat, mem.p2Mat, mem.qMat
    nodeV = np.zeros([mem.ns, n2, 3], dtype=CLD)
    dr = np.zeros_like(nodeV)
    u = np.zeros_like(nodeV)
    gu = np.zeros([mem.ns, n2, 3, 3], dtype=CLD)
    gp = np.zeros([mem.ns, n2, 3], dtype=CLD)
    var = np.zeros([mem.ns, n2], dtype=CLD)
    for il in range(mem.ns):
        r = mem.r[il]
        d_, v_, _ = _kinematics(r, Xi, w2)
        dr[il], nodeV[il] = d_.T, v_.T
        u[il] = _wave_kin(beta, w2, k2, h, r, rho, g)[0].T
        gu[il] = _grad_u1(w2, k2, beta, h, r)
        var[il] = (u[il] - nodeV[il]) @ q
        gp[il] = _grad_pres1st(k2, beta, h, r, rho, g)
    gdudt = 1j * w2[None, :, None, None] * gu
    cross_wl = mem.r[-1, 2] * mem.r[0, 2] < 0
    eta = np.zeros(n2, dtype=CLD)
    ud_wl = np.zeros([n2, 3], dtype=CLD)
    dr_wl = np.zeros([n2, 3], dtype=CLD)
    a_wl = np.zeros([n2, 3], dtype=CLD)
    r_int = None
    if cross_wl:
        r_int = mem.r[0] + (mem.r[-1] - mem.r[0]) * (0 - mem.r[0, 2]) / (mem.r[-1, 2] - mem.r[0, 2])
        _, udw, et = _wave_kin(beta, w2, k2, h, r_int, LD(1), LD(1))
        ud_wl, eta = udw.T, et
        d_, _, a_ = _kinematics(r_int, Xi, w2)
        dr_wl, a_wl = d_.T, a_.T
    ge1 = np.zeros([n2, 3], dtype=CLD)
    for iw in range(n2):
        ge1[iw] = -g * (_cross(Xi[3:, iw], mem.p1)[2] * mem.p1 + _cross(Xi[3:, iw], mem.p2)[2] * mem.p2)
    eta_r = eta - dr_wl[:, 2]
    O1 = _omega_mat(1j * W1[:, None] * Xi[3:, i1].T)
    O2 = _omega_mat(1j * W2[:, None] * Xi[3:, i2].T)
    Ca_p1 = Ca_p2 = None
    pi = np.arctan(LD(1)) * 4
    for il in range(mem.ns):
        r = mem.r[il]
        if r[2] >= 0:
            continue
        Ca_p1, Ca_p2, Ca_End = mem.Ca_p1[il], mem.Ca_p2[il], mem.Ca_End[il]
        CmM = (1 + Ca_p1) * p1Mat + (1 + Ca_p2) * p2Mat
        CaM = Ca_p1 * p1Mat + Ca_p2 * p2Mat
        ds, drs, dls = mem.ds[il], mem.drs[il], mem.dls[il]
        v_i = 0.25 * pi * ds[0] ** 2 * dls if mem.circ else ds[0] * ds[1] * dls
        if float(r[2]) + 0.5 * float(dls) > 0:                                 # Q12
            v_i = v_i * (0.5 * dls - r[2]) / dls
        if mem.circ:
            ve = pi / 12 * abs((ds[0] + drs[0]) ** 3 - (ds[0] - drs[0]) ** 3)
        else:
            ve = pi / 12 * ((np.mean(ds + drs)) ** 3 - (np.mean(ds - drs)) ** 3)
        ai = mem.a_i[il]
        put = lambda f: acc.put(f, r)                                          # noqa: E731
        acc2, p2 = _pot2nd(W1, W2, K1, K2, beta, h, r, g, rho)
        put(rho * v_i * _mv(CmM, acc2))
        put(ai * p2[:, None] * q[None, :])
        put(rho * ve * Ca_End * _mv(qMat, acc2))
        conv = 0.25 * (_mv(gu[il, i1], np.conj(u[il, i2])) + _mv(np.conj(gu[il, i2]), u[il, i1]))
        put(rho * v_i * _mv(CmM, conv))
        put(rho * ve * Ca_End * _mv(qMat, conv))
        dwdz1 = (gu[il, i1] @ q) @ q
        dwdz2 = (gu[il, i2] @ q) @ q
        vel1 = nodeV[il, i1] - np.outer(nodeV[il, i1] @ q, q)
        vel2 = nodeV[il, i2] - np.outer(nodeV[il, i2] @ q, q)
        u1 = u[il, i1] - np.outer(u[il, i1] @ q, q)
        u2 = u[il, i2] - np.outer(u[il, i2] @ q, q)
        a = 0.25 * (dwdz1[:, None] * np.conj(u2 - vel2) + np.conj(dwdz2)[:, None] * (u1 - vel1))
        a = a - np.outer(a @ q, q)
        put(rho * v_i * _mv(CaM, a))
        acc_n = 0.25 * _mv(gdudt[il, i1], np.conj(dr[il, i2])) + 0.25 * _mv(np.conj(gdudt[il, i2]), dr[il, i1])
        put(rho * v_i * _mv(CmM, acc_n))
        put(rho * ve * Ca_End * _mv(qMat, acc_n))
        pn = 0.25 * np.sum(gp[il, i1] * np.conj(dr[il, i2]), axis=1) + 0.25 * np.sum(np.conj(gp[il, i2]) * dr[il, i1], axis=1)
        put(ai * pn[:, None] * q[None, :])
        va1 = var[il, i1][:, None] * q[None, :]
        va2 = var[il, i2][:, None] * q[None, :]
        put(-0.25 * 2 * _mv(CaM, _mv(O1, np.conj(va2)) + _mv(np.conj(O2), va1)) * (rho * v_i))
        u1a = u[il, i1] - vel1                                                  # Q3
        u2a = u[il, i2] - vel2
        V1 = gu[il, i1] + O1
        V2 = gu[il, i2] + O2
        aux = 0.25 * (_mv(V1, np.conj(_mv(CaM, u2a))) + _mv(np.conj(V2), _mv(CaM, u1a)))
        aux = aux - _mv(qMat, aux)
        put(rho * v_i * aux)
        u1b = u1a - _mv(qMat, u1a)
        u2b = u2a - _mv(qMat, u2a)
        aux = 0.25 * (_mv(CaM, _mv(V1, np.conj(u2b))) + _mv(CaM, _mv(np.conj(V2), u1b)))
        put(-rho * v_i * aux)
        pdrop = -2 * 0.25 * 0.5 * rho * np.sum(_mv(p1Mat + p2Mat, u[il, i1] - vel1) *
                                               np.conj(_mv(CaM, u[il, i2] - vel2)), axis=1)
        put(ai * pdrop[:, None] * q[None, :])
    if cross_wl:
        i_wl = np.where(mem.r[:, 2] < 0)[0][-1]
        if mem.circ:
            d_wl = 0.5 * (mem.ds[i_wl, 0] + mem.ds[i_wl + 1, 0]) if i_wl != mem.ns - 1 else mem.ds[i_wl, 0]
            area = 0.25 * pi * d_wl ** 2
        else:
            if i_wl != mem.ns - 1:
                d1 = 0.5 * (mem.ds[i_wl, 0] + mem.ds[i_wl + 1, 0])
                d2 = 0.5 * (mem.ds[i_wl, 1] + mem.ds[i_wl + 1, 1])
            else:
                d1, d2 = mem.ds[i_wl, 0], mem.ds[i_wl, 1]
            area = d1 * d2
        CmM = (1 + Ca_p1) * p1Mat + (1 + Ca_p2) * p2Mat
        CaM = Ca_p1 * p1Mat + Ca_p2 * p2Mat
        fe = 0.25 * (ud_wl[i1] * np.conj(eta_r[i2])[:, None] + np.conj(ud_wl[i2]) * eta_r[i1][:, None])
        acc.put(rho * area * _mv(CmM, fe), r_int)
        ae = 0.25 * (a_wl[i1] * np.conj(eta_r[i2])[:, None] + np.conj(a_wl[i2]) * eta_r[i1][:, None])
        acc.put(-rho * area * _mv(CaM, ae), r_int)
        acc.put(-0.25 * rho * area * (ge1[i1] * np.conj(eta_r[i2])[:, None] + np.conj(ge1[i2]) * eta_r[i1][:, None]), r_int)


def qtf_reference(T, Xi0, w2, k2, beta):
    """qtf_slender in long double: (ref [n2, n2, 6] clongdouble, S [n2, n2, 6] longdouble)."""
    rho, g, h = LD(float(T["rho"])), LD(float(T["g"])), LD(float(T["depth"]))
    w = np.asarray(T["w"], dtype=float).astype(LD)
    w2d = np.asarray(w2, dtype=float)
    n2 = len(w2d)
    w2, k2 = w2d.astype(LD), np.asarray(k2, dtype=float).astype(LD)
    beta = LD(float(beta))
    X0 = np.zeros([6, len(w)], dtype=CLD) if Xi0 is None else np.asarray(Xi0, dtype=complex).astype(CLD)
    Xi = np.array([_interp0(w2, w, X0[d]) for d in range(6)], dtype=CLD)
    M = np.asarray(T["M_struc"], dtype=float).astype(LD)
    acl = -w2 ** 2 * Xi
    F1 = np.zeros([6, n2], dtype=CLD)
    F1[0:3] = M[0, 0] * acl[0:3]
    F1[3:6] = M[3:, 3:] @ acl[3:]
    F1a = np.zeros([6, n2], dtype=LD)
    F1a[0:3] = np.abs(M[0, 0]) * np.abs(acl[0:3])
    F1a[3:6] = np.abs(M[3:, 3:]) @ np.abs(acl[3:])
    i1, i2 = np.triu_indices(n2)
    keep = w2d[i2] >= w2d[i1]
    i1, i2 = i1[keep], i2[keep]
    acc = _Acc(len(i1))
    th1, th2 = Xi[3:, i1].T, Xi[3:, i2].T
    for s in (slice(0, 3), slice(3, 6)):                            # Pinkster IV rotation term
        acc.Q[:, s] += 0.25 * (_cross(th1, np.conj(F1[s, i2].T)) + _cross(np.conj(th2), F1[s, i1].T))
        acc.S[:, s] += 0.25 * (_cross_abs(np.abs(th1), F1a[s, i2].T) + _cross_abs(np.abs(th2), F1a[s, i1].T))
    for im in range(len(T["member_rA"])):
        mem = _Member(T, im)
        if mem.rA[2] > 0 and mem.rB[2] > 0:
            continue
        _member_terms(acc, mem, Xi, w2, k2, i1, i2, beta, h, rho, g)
        _correction_kay(acc, mem, h, w2, k2, i1, i2, beta, rho, g)
    ref = np.zeros([n2, n2, 6], dtype=CLD)
    S = np.zeros([n2, n2, 6], dtype=LD)
    ref[i1, i2] = acc.Q
    S[i1, i2] = acc.S
    d = np.arange(n2)
    for k in range(6):                                              # Hermitian fill
        q = ref[:, :, k].copy()
        ref[:, :, k] = q + np.conj(q).T
        ref[d, d, k] -= np.conj(q[d, d])
        s = S[:, :, k].copy()
        S[:, :, k] = s + s.T
        S[d, d, k] -= s[d, d]
    return ref, S


_REF = {}


def reference(name, seed=0):
    """(case, ref, S) of a named case, computed once per process."""
    key = (name, seed)
    if key not in _REF:
        c = case(name, seed)
        ref, S = qtf_reference(c.T, c.Xi0, c.w2, c.k2, c.beta)
        _REF[key] = (c, ref, S)
    return _REF[key]


_BAR = {}


def bar(name, seed=0):
    """The device bar of a case in units of u S: 8 max(A_orc of this case, 4), the float64 oracle's own
    worst() on this case's inputs, never more than BAR; BAR itself where the oracle is not finite ("deep")."""
    key = (name, seed)
    if key not in _BAR:
        from oracle import qtf_oracle as Q
        c, ref, S = reference(name, seed)
        with np.errstate(all="ignore"):
            o = Q.qtf_slender(c.T, c.Xz, c.w2, c.k2, c.beta)[:, :, 0, :]
        a = worst(o, ref, S)
        _BAR[key] = min(BAR, 8 * max(a, 4.0)) if np.isfinite(a) else BAR
    return _BAR[key]


# ------------------------------------------------------------------------------------------------
# the criterion
# ------------------------------------------------------------------------------------------------
def worst(x, ref, S):
    """max |x - ref| / (u S) over all pairs and DOFs; inf where x is not finite, or where S == 0 (no
    addend) and x is not exactly 0."""
    x = np.asarray(x)
    if x.shape != ref.shape:
        raise ValueError(f"shape {x.shape} against {ref.shape}")
    if not np.all(np.isfinite(x.view(float))):
        return np.inf
    e = np.abs(x.astype(CLD) - ref)
    zero = S == 0
    if np.any(e[zero] != 0):
        return np.inf
    return float((e[~zero] / (LD(U) * S[~zero])).max()) if (~zero).any() else 0.0


def beyond_range(c):
    """[n2, n2] pairs beyond the stated range of the device ("Accuracy of the slender-body QTF"):
    with Kim & Yue rows, the pairs whose exp(k1 (z2 + h)) exp(k2 (z2 + h)) at the top interval (z2 = 0) is
    no finite double, (k1 + k2) h > ln(DBL_MAX) = 709.78 -- where the reference's own
    sinh((k1 + k2)(z2 + h)) overflows too.  The exponentials are the doubles of the device's table."""
    if EXPECT[c.design][2] == 0:                      # no Kim & Yue row
        return np.zeros([c.n2, c.n2], dtype=bool)
    with np.errstate(over="ignore"):
        e = np.exp(c.k2 * (0.0 + c.depth))
        return ~np.isfinite(e[:, None] * e[None, :])


def worst_per_dof(x, ref, S):
    return [worst(np.ascontiguousarray(x[..., d]), ref[..., d], S[..., d]) for d in range(6)]


def amplification(ref, S):
    """max S / |ref| over the entries above 1e-6 of their DOF's largest |ref|."""
    a = np.abs(ref)
    out = 0.0
    for d in range(6):
        m = a[..., d] > 1e-6 * a[..., d].max()
        if m.any():
            out = max(out, float((S[..., d][m] / a[..., d][m]).max()))
    return out
