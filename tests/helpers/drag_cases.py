"""Inputs, the long-double reference and the criteria for the direct tests of the Borgman drag
linearisation (tests/test_gpu_drag.py; checked on the CPU by tests/test_drag_cases.py): the per-node
sums of |v_rel|^2 over the bins, the node matrices Bmat, the translated B_drag and the drag
excitation, as k_solve_lds (every instantiation), k_solve_cases, k_lin_sums + k_lin_bdrag,
k_lin_partial + k_bin_step, k_drag_exc and k_heading_resp restate them.

The reference is the formulas of oracle/raft_oracle.py (hydro_linearization, drag_excitation, get_rms,
translate_matrix_3to6, translate_force_3to6) in NumPy longdouble / clongdouble of the double inputs
the device gets.  The wave amplitudes zeta, the unit-amplitude wave velocity uhat and the inertial
excitation finer are data: the doubles the device itself produced (or, on the CPU, the double
oracle's), so that the comparison is of the linearisation alone.  u = 2^-53.

Criteria, per element, nothing masked.  With, per node n and bin b,
    a_b = |zeta_b| ||uhat_b||_1 + w_b (||xi_t||_1 + 2 ||theta||_1 ||r_rel||_1),   S_n = sum_b a_b^2,
  sums   |dev - ref| <= C_SUM (nw + 16) u S_n
  Bmat   the bound of the sums through v = sqrt(s / 2), dv = ds / (4 v_ref), times |K_x| |e_i e_j| for
         each of the four coefficients B_x = K_x v_x (K_x = sqrt(8/pi) rho/2 area Cd), plus
         C_TERM u sum_x |B_x e_i e_j|
  B_drag translate_matrix_3to6 of the Bmat bounds with |r_rel| (every entry of H in absolute value),
         summed over the nodes, plus C_NODE (nn + 16) u of the same sum of the |B_x e_i e_j|
  F_drag translate_force_3to6 of (Bmat bound) |zeta uhat| with |r_rel|, summed over the nodes, plus
         C_NODE (nn + 16) u of the same sum of the |B_x e_i e_j| |zeta uhat|
  F_wave the bound of F_drag plus C_NODE (nn + 16) u (|zeta finer| + |fext|).
The constants: tests/test_drag_cases.py measures the same formulas in float64 against the long-double
reference and asserts that they stay within a quarter of every bound; each constant is the smallest
power of two for which that holds on these inputs, fixed in the order C_SUM (the sums), C_TERM (Bmat,
given C_SUM), C_NODE (B_drag, F_drag, F_wave and the excitation of a random Bmat, given both): 2^-4
(S_n, a sum of squared 1-norms, overestimates the sums' own terms; the two-bin grids set it), 16, and
1/2 (set by the excitation of the random Bmat on the 11-node design).  The factor four is left for the
device's other summation orders (wave partials, pass order, member factoring) and for its r_A + t q in
place of the stored r_rel.  DESIGN.md, "Accuracy of the drag linearisation", holds the
measured ratios.
"""
import types

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
DEPTH = 200.0
HEADINGS_DEG = (0.0, 40.0)
OFFSET = np.array([12.5, -7.25, -3.0])        # r = r_rel + OFFSET (the platform reference point is not the origin)
C_SUM, C_TERM, C_NODE = 2.0 ** -4, 16.0, 0.5

# Members of a design: (kind, nodes).  Kinds, by the axial set AQ CDQ != 0 or AEND CDEND != 0:
#   all   circular, Cd_q != 0 on every node, end drag on every third one: every node axial
#   none  rectangular, Cd_q = 0; even nodes Cd_End != 0 with drs = 0, odd nodes a_end != 0 with Cd_End = 0
#   mid   circular, Cd_q = 0, Cd_End != 0, drs != 0 at the middle node only: that node alone is axial
#   end   rectangular, Cd_q = 0, a_end Cd_End != 0 on every node: end drag without axial side drag
#   side  rectangular, Cd_q != 0, a_end Cd_End = 0 on every node (both ways, alternating)
_FULL = lambda long_: [("side", 1), ("none", 2), ("mid", 3), ("all", long_), ("end", 1)]   # noqa: E731
DESIGNS = {
    "default": _FULL(69),                # nn = 76: the most the one-pass 2 x 512 kernel takes with five members
    "nn1": [("side", 1)],
    "nn4": [("end", 1), ("mid", 3)],
    "nn5": [("none", 2), ("mid", 3)],
    "nn11": [("side", 1), ("none", 2), ("mid", 3), ("all", 4), ("end", 1)],
    "nn40": _FULL(33),
    "nn77": _FULL(70),                   # 512 < nw <= 1024 moves to the two-pass kernel
    "nn212": _FULL(205),                 # beyond the two-pass kernel's LDS: the general kernel
}
SMALL = ("nn1", "nn4", "nn5", "nn11")
LARGE = ("nn77", "nn212")


# ------------------------------------------------------------------------------ dispatch by node count
K_LT, K_GHOST, MAX_LDS = 512, 1, 160 * 1024


def solve_lds_smem(nn, nm, NB, LT=K_LT, ser=False, NP=1):
    """Dynamic LDS bytes of k_solve_lds: solve_lds_smem of csrc/rh_solve.hip, term by term."""
    LW = LT // 64
    doubles = ((12 * LT * NB if NP == 1 else 0)
               + (27 if ser and nn * 3 * LW < 27 else nn * 3 * LW)
               + (0 if ser else nn * 36)
               + nn * 9 + (nn + K_GHOST) * 6 + (nn + K_GHOST) + nm * 18 + 2 * LT * NB * NP
               + 36 + 108 + LW * 6 + 36 + LW)
    return 8 * doubles + 4 * (nm + 6)


def general_smem(nn, threads=256):
    """Dynamic LDS bytes of k_solve_cases (rh_solve_cases, csrc/rh_abi.hip)."""
    wv = threads // 64
    return 8 * (wv * nn * 3 + nn * 9 + 36 + wv * 6 + 108 + nn * 5 + wv)


def solve_kernel(nw, nn, nm):
    """The kernel rh_solve_cases(solver 0) launches (the dispatch of csrc/rh_abi.hip)."""
    if nw <= 2 * K_LT:
        if nw <= K_LT // 2:
            nb = 1 if nw <= K_LT // 4 else 2
            if solve_lds_smem(nn, nm, nb, K_LT // 4, True) <= MAX_LDS:
                return f"{nb}x128"
        nb = 1 if nw <= K_LT else 2
        lt = K_LT // 2 if nw <= K_LT // 2 else K_LT
        if solve_lds_smem(nn, nm, nb, lt) <= MAX_LDS:
            return f"{nb}x{lt}"
    if nw <= 4 * K_LT and solve_lds_smem(nn, nm, 2, K_LT, False, 2) <= MAX_LDS:
        return "two-pass"
    assert general_smem(nn) <= MAX_LDS
    return "general"


# ------------------------------------------------------------------------------ the design
class DragDesign:
    """A stand-in FOWT for prep.DeviceDesign (host_tables) with real members: per member an end point
    rA (|rA| <= 60 m) and a right-handed frame (q, p1, p2 = cross(q, p1) as formed), node coordinates
    t ascending from 0, r_rel = rA + t q formed in double, r = r_rel + OFFSET; circular and rectangular
    nodes (AP1 != AP2, CDP1 != CDP2) with the areas of O.drag_coefficients from ds, dls, drs; a random
    non-symmetric Imat and a_i, so that finer is not zero; no MacCamy-Fuchs nodes.  It carries the
    attributes oracle.raft_oracle.hydro_linearization reads of its `nodes` argument.  The geometry
    depends on the name alone, the grid on nw."""

    def __init__(self, name, nw):
        from oracle import raft_oracle as O
        comp = DESIGNS[name]
        self.name, self.comp = name, comp
        rng = np.random.default_rng(sum(map(ord, name)) * 7919 + len(comp))
        self.nm, self.nn = len(comp), sum(c[1] for c in comp)
        self.n = self.nn
        self.nw = nw
        self.dw, self.depth, self.rho_water, self.g = 2.0 / nw, DEPTH, 1025.0, 9.81
        self.w = self.dw * np.arange(1, nw + 1)
        self.k = self.w * self.w / self.g
        nn = self.nn
        self.mstart = np.concatenate([[0], np.cumsum([c[1] for c in comp])]).astype(np.int32)
        self.member = np.repeat(np.arange(self.nm), [c[1] for c in comp])
        self.rA = np.empty([self.nm, 3])
        self.mq, self.mp1, self.mp2 = (np.empty([self.nm, 3]) for _ in range(3))
        self.t = np.zeros(nn)
        self.r_rel = np.empty([nn, 3])
        self.q, self.p1, self.p2 = (np.empty([nn, 3]) for _ in range(3))
        self.circ = np.zeros(nn, dtype=bool)
        self.ds, self.drs = np.zeros([nn, 2]), np.zeros([nn, 2])
        self.dls = np.empty(nn)
        self.Cd_q, self.Cd_End = np.zeros(nn), np.zeros(nn)
        self.Cd_p1, self.Cd_p2 = rng.uniform(0.5, 1.2, nn), rng.uniform(1.3, 2.0, nn)
        for m, (kind, cnt) in enumerate(comp):
            n0 = self.mstart[m]
            sl = slice(n0, n0 + cnt)
            rA = np.array([*rng.uniform(-30.0, 30.0, 2), rng.uniform(-40.0, -15.0)])
            q = rng.standard_normal(3)
            q /= np.linalg.norm(q)
            p1 = np.cross(q, rng.standard_normal(3))
            p1 /= np.linalg.norm(p1)
            p2 = np.cross(q, p1)
            length = rng.uniform(6.0, 12.0) if cnt > 1 else 0.0
            t = np.sort(rng.uniform(0.0, length, cnt))
            t[0] = 0.0
            self.rA[m], self.mq[m], self.mp1[m], self.mp2[m] = rA, q, p1, p2
            self.t[sl] = t
            self.r_rel[sl] = rA + t[:, None] * q
            self.q[sl], self.p1[sl], self.p2[sl] = q, p1, p2
            circ = kind in ("all", "mid")
            self.circ[sl] = circ
            a = rng.uniform(0.5, 6.0, cnt)
            self.ds[sl, 0] = a
            self.ds[sl, 1] = a if circ else a * rng.uniform(0.3, 0.8, cnt)
            self.dls[sl] = rng.uniform(0.3, 2.0, cnt)
            step = rng.uniform(0.1, 0.4, [cnt, 2]) * rng.choice([-1.0, 1.0], [cnt, 1])
            i = np.arange(cnt)
            if kind == "all":
                self.Cd_q[sl] = rng.uniform(0.05, 0.3, cnt)
                self.Cd_End[sl] = 0.6
                self.drs[sl] = np.where((i % 3 == 0)[:, None], step, 0.0)
            elif kind == "none":
                self.Cd_End[sl] = np.where(i % 2 == 0, 0.8, 0.0)
                self.drs[sl] = np.where((i % 2 == 1)[:, None], step, 0.0)
            elif kind == "mid":
                self.Cd_End[sl] = 0.7
                self.drs[sl] = np.where((i == cnt // 2)[:, None], step, 0.0)
            elif kind == "end":
                self.Cd_End[sl] = 1.0
                self.drs[sl] = step
            elif kind == "side":
                self.Cd_q[sl] = rng.uniform(0.05, 0.3, cnt)
                self.Cd_End[sl] = np.where(i % 2 == 0, 0.0, 0.9)
                self.drs[sl] = np.where((i % 2 == 0)[:, None], step, 0.0)
            else:
                raise ValueError(kind)
        self.r = self.r_rel + OFFSET
        assert np.all(self.r[:, 2] < 0)
        self.area = np.array([O.drag_coefficients(None, self, j) for j in range(nn)])     # a_q, a_p1, a_p2, a_end
        self.Imat = rng.standard_normal([nn, 3, 3]) * 1e3
        self.a_i = rng.choice([-1.0, 1.0], nn) * rng.uniform(0.5, 20.0, nn)
        self.mcf = np.zeros(nn, dtype=bool)
        self.Imat_MCF = None
        eye = np.eye(6)
        self.M, self.B, self.C = 1e7 * eye, 1e6 * eye, 1e7 * eye

    @property
    def axial(self):
        """The axial set as the kernels form it, on the stored doubles."""
        return (self.area[:, 0] * self.Cd_q != 0.0) | (self.area[:, 3] * self.Cd_End != 0.0)

    def member_table(self):
        """[MF_COUNT][nm], column by column as prep.node_table forms it."""
        cols = [[*q, *np.cross(rA, q), *p1, *np.cross(rA, p1), *p2, *np.cross(rA, p2), q @ q, p1 @ p1, p2 @ p2]
                for rA, q, p1, p2 in zip(self.rA, self.mq, self.mp1, self.mp2)]
        return np.array(cols, dtype=float).T.copy()

    def host_tables(self):
        from raft import _native as N
        nn = self.nn
        node = np.zeros([N.NF_COUNT, nn])
        for f, v in (("RX", self.r[:, 0]), ("RY", self.r[:, 1]), ("RZ", self.r[:, 2]),
                     ("XX", self.r_rel[:, 0]), ("XY", self.r_rel[:, 1]), ("XZ", self.r_rel[:, 2]),
                     ("QX", self.q[:, 0]), ("QY", self.q[:, 1]), ("QZ", self.q[:, 2]),
                     ("P1X", self.p1[:, 0]), ("P1Y", self.p1[:, 1]), ("P1Z", self.p1[:, 2]),
                     ("P2X", self.p2[:, 0]), ("P2Y", self.p2[:, 1]), ("P2Z", self.p2[:, 2]),
                     ("AQ", self.area[:, 0]), ("AP1", self.area[:, 1]), ("AP2", self.area[:, 2]), ("AEND", self.area[:, 3]),
                     ("CDQ", self.Cd_q), ("CDP1", self.Cd_p1), ("CDP2", self.Cd_p2), ("CDEND", self.Cd_End),
                     ("CIRC", self.circ.astype(float)), ("AI", self.a_i), ("T", self.t)):
            node[N.NF[f]] = v
        node[N.NF["I00"]:N.NF["I00"] + 9] = self.Imat.reshape(nn, 9).T
        parts = [("w", self.w), ("k", self.k), ("node", node), ("memb", self.member_table()),
                 ("M", self.M), ("B", self.B), ("C", self.C)]
        layout, off = {}, 0
        for name, a in parts:
            layout[name] = (off, a.shape)
            off += a.size
        packed = np.concatenate([np.ascontiguousarray(a, dtype=float).ravel() for _, a in parts])
        return dict(packed=packed, layout=layout, imat=None, mstart=self.mstart.copy(), nn=nn, nm=self.nm, per_bin=False)


# ------------------------------------------------------------------------------ motions and sea
def drag_cases():
    """(spectrum, Hs, Tp, gamma, motion): the cases of one call (heading index 1 for all of them).
    motion "random": Xi_init random complex, translations of order 1 m, rotations of order 0.05 rad;
    "zero": Xi_init = 0 (with the spectrum "none": still water)."""
    return [("JONSWAP", 6.0, 10.0, 0.0, "random"), ("unit", 1.0, 9.0, 0.0, "random"),
            ("none", 4.0, 9.0, 0.0, "zero"), ("JONSWAP", 2.5, 7.0, 3.3, "random")]


STILL = 2                                  # the still-water case of drag_cases()
XI_START = 0.1                             # the call with Xi_init = NULL: XiLast = XiStart + 0 i everywhere


def motions(nw, seed=0):
    """Xi_init [ncase][6][nw] of drag_cases()."""
    cases = drag_cases()
    rng = np.random.default_rng(4001 + nw + seed)
    X = rng.standard_normal([len(cases), 6, nw]) + 1j * rng.standard_normal([len(cases), 6, nw])
    X[:, 3:] *= 0.05
    for i, c in enumerate(cases):
        if c[4] == "zero":
            X[i] = 0.0
    return X


def random_bmat(nn, seed=0):
    """Node matrices that no linearisation produced: nine independent entries, not symmetric."""
    rng = np.random.default_rng(77 + nn + seed)
    return rng.standard_normal([nn, 3, 3]) * 10.0 ** rng.uniform(1, 3, [nn, 1, 1])


def sea_zeta(d):
    """zeta [ncase][nw] of drag_cases() from the double oracle (sqrt(2 S dw)): the amplitudes handed to the
    entry points that take them as an argument."""
    from oracle import raft_oracle as O
    zeta = np.zeros([len(drag_cases()), d.nw])
    for i, (sp, Hs, Tp, gam, _) in enumerate(drag_cases()):
        S = {"JONSWAP": lambda: O.jonswap(d.w, Hs, Tp, Gamma=gam), "unit": lambda: np.ones(d.nw),
             "none": lambda: np.zeros(d.nw)}[sp]()
        zeta[i] = np.sqrt(2 * S * d.dw)
    return zeta


def oracle_inputs(d, head=1):
    """sea_zeta, uhat [nn][3][nw] and finer [6][nw] from the double oracle: what the CPU test feeds the
    reference instead of the device's tables."""
    from oracle import raft_oracle as O
    beta = np.array([HEADINGS_DEG[head] * O.DEG2RAD])
    u, _, _, F = O.hydro_excitation(dict(w=d.w, k=d.k, depth=d.depth), d, beta, np.ones([1, d.nw]))
    return sea_zeta(d), u[0], F[0]


# ------------------------------------------------------------------------------ the reference
def _abs2(x):
    return x.real * x.real + x.imag * x.imag


def _h(r):
    return np.array([[0 * r[0], r[2], -r[1]], [-r[2], 0 * r[0], r[0]], [r[1], -r[0], 0 * r[0]]])


def _matrix_3to6(M, r, absolute=False):
    """translate_matrix_3to6; absolute: every entry of H in absolute value (the bound's form)."""
    H = np.abs(_h(r)) if absolute else _h(r)
    out = np.zeros([6, 6], dtype=M.dtype)
    out[:3, :3] = M
    out[:3, 3:] = M @ H
    out[3:, :3] = out[:3, 3:].T
    out[3:, 3:] = H @ M @ H.T
    return out


def _force_3to6(F, r, absolute=False):
    s = 1 if absolute else -1
    m = np.stack([r[1] * F[2] + s * r[2] * F[1], r[2] * F[0] + s * r[0] * F[2], r[0] * F[1] + s * r[1] * F[0]])
    return np.concatenate([F, m], axis=0)


def excitation_reference(d, Bmat, dB_sum, B_abs, zeta, uhat, finer, fext=None, real=LD):
    """F_drag = zeta sum_n T(Bmat_n uhat_n), F_wave = zeta (finer + sum_n T(Bmat_n uhat_n)) + fext, and the
    parts of their bounds: G_sum (of the sums' bound of Bmat, per unit C_SUM), G_abs (of |Bmat|'s
    terms) and G_lin = |zeta finer| + |fext|, each [6][nw]."""
    cplx = CLD if real is LD else complex
    nw = d.nw
    z = zeta.astype(real)
    E = np.zeros([6, nw], dtype=cplx)
    G_sum, G_abs = np.zeros([6, nw], dtype=real), np.zeros([6, nw], dtype=real)
    for n in range(d.nn):
        r = d.r_rel[n].astype(real)
        un = uhat[n].astype(cplx)
        ua = np.abs(z) * np.abs(un)
        E += _force_3to6(Bmat[n].astype(real).astype(cplx) @ un, r)
        G_sum += _force_3to6(dB_sum[n] @ ua, np.abs(r), True)
        G_abs += _force_3to6(B_abs[n] @ ua, np.abs(r), True)
    fin = finer.astype(cplx)
    F_drag = z * E
    F_wave = z * (fin + E)
    G_lin = np.abs(z) * np.abs(fin)
    if fext is not None:
        F_wave = F_wave + fext.astype(cplx)
        G_lin = G_lin + np.abs(fext.astype(cplx))
    return types.SimpleNamespace(F_drag=F_drag, F_wave=F_wave, G_sum=G_sum, G_abs=G_abs, G_lin=G_lin)


def drag_reference(d, Xi, zeta, uhat, finer, fext=None, real=LD):
    """One case: Xi [6][nw], zeta [nw], uhat [nn][3][nw], finer [6][nw] (doubles) -> the per-node sums
    [nn][3] (q; p or p1; p2, 0 for a circular node), their per-bin terms tb [nn][3][nw], Bmat [nn][3][3],
    B_drag [6][6], F_drag and F_wave [6][nw] in `real` precision, with the parts of the bounds: a2
    [nn][nw] (a_b^2; S = its bin sum), dB_sum (the Bmat bound of the sums per unit C_SUM), B_abs
    (sum_x |B_x e_i e_j|), their translated node sums D_sum, D_abs [6][6], and G_sum, G_abs, G_lin
    [6][nw] of the excitation.  vfloor [nn]: the smallest v_x / sqrt(S_n / 2) over the node's sums."""
    from oracle import raft_oracle as O
    cplx = CLD if real is LD else complex
    nn, nw = d.nn, d.nw
    w, z, X = d.w.astype(real), zeta.astype(real), Xi.astype(cplx)
    rho, K8, half = real(d.rho_water), real(O.SQRT_8_PI), real(0.5)
    xt1, th1 = np.abs(X[:3]).sum(axis=0), np.abs(X[3:]).sum(axis=0)
    sums = np.zeros([nn, 3], dtype=real)
    tb = np.zeros([nn, 3, nw], dtype=real)
    a2 = np.zeros([nn, nw], dtype=real)
    Bmat = np.zeros([nn, 3, 3], dtype=real)
    dB_sum, B_abs = np.zeros_like(Bmat), np.zeros_like(Bmat)
    B_drag = np.zeros([6, 6], dtype=real)
    D_sum, D_abs = np.zeros_like(B_drag), np.zeros_like(B_drag)
    vfloor = np.full(nn, np.inf)
    th = X[3:]
    for n in range(nn):
        r = d.r_rel[n].astype(real)
        q, p1, p2 = (v[n].astype(real) for v in (d.q, d.p1, d.p2))
        u0 = z * uhat[n].astype(cplx)
        dr = X[:3] + np.stack([-th[2] * r[1] + th[1] * r[2], th[2] * r[0] - th[0] * r[2], -th[1] * r[0] + th[0] * r[1]])
        vrel = u0 - 1j * w * dr
        vq = (vrel * q[:, None]).sum(axis=0) * q[:, None]
        tb[n, 0] = _abs2(vq).sum(axis=0)
        if d.circ[n]:
            tb[n, 1] = _abs2(vrel - vq).sum(axis=0)
        else:
            tb[n, 1] = _abs2((vrel * p1[:, None]).sum(axis=0) * p1[:, None]).sum(axis=0)
            tb[n, 2] = _abs2((vrel * p2[:, None]).sum(axis=0) * p2[:, None]).sum(axis=0)
        sums[n] = tb[n].sum(axis=1)
        a2[n] = (np.abs(z) * np.abs(uhat[n].astype(cplx)).sum(axis=0) + w * (xt1 + 2 * th1 * np.abs(r).sum())) ** 2
        S = a2[n].sum()
        v = np.sqrt(half * sums[n])
        vx = (v[0], v[1], v[1] if d.circ[n] else v[2], v[0])
        ar = d.area[n].astype(real)
        cd = (real(d.Cd_q[n]), real(d.Cd_p1[n]), real(d.Cd_p2[n]), real(d.Cd_End[n]))
        ex = (q, p1, p2, q)
        Bx = [K8 * vx[i] * half * rho * ar[i] * cd[i] for i in range(4)]
        Ex = [np.outer(e, e) for e in ex]
        Bmat[n] = (Bx[0] * Ex[0] + Bx[1] * Ex[1] + Bx[2] * Ex[2]) + Bx[3] * Ex[3]
        for i in range(4):
            Kx = np.abs(K8 * half * rho * ar[i] * cd[i])
            B_abs[n] += np.abs(Bx[i]) * np.abs(Ex[i])
            if Kx != 0 and S > 0:
                dB_sum[n] += Kx * ((nw + 16) * U * S / (4 * vx[i])) * np.abs(Ex[i])
                vfloor[n] = min(vfloor[n], float(vx[i] / np.sqrt(half * S)))
        B_drag += _matrix_3to6(Bmat[n], r)
        D_sum += _matrix_3to6(dB_sum[n], np.abs(r), True)
        D_abs += _matrix_3to6(B_abs[n], np.abs(r), True)
    exc = excitation_reference(d, Bmat, dB_sum, B_abs, zeta, uhat, finer, fext, real)
    return types.SimpleNamespace(sums=sums, tb=tb, a2=a2, Bmat=Bmat, B_drag=B_drag, dB_sum=dB_sum, B_abs=B_abs,
                                 D_sum=D_sum, D_abs=D_abs, vfloor=vfloor, nn=nn, nw=nw, **vars(exc))


# ------------------------------------------------------------------------------ the criteria
def bounds(ref, lo=0, hi=None):
    """The bound of every output (see the module text); the sums' for the bins [lo, hi)."""
    nn, nw = ref.nn, ref.nw
    hi = nw if hi is None else hi
    S = ref.a2[:, lo:hi].sum(axis=1)
    node = C_NODE * (nn + 16) * U
    b_bmat = C_SUM * ref.dB_sum + C_TERM * U * ref.B_abs
    b_fdrag = C_SUM * ref.G_sum + C_TERM * U * ref.G_abs + node * ref.G_abs
    return types.SimpleNamespace(sums=(C_SUM * ((hi - lo) + 16) * U * S)[:, None] * np.ones(3),
                                 Bmat=b_bmat, B_drag=C_SUM * ref.D_sum + C_TERM * U * ref.D_abs + node * ref.D_abs,
                                 F_drag=b_fdrag, F_wave=b_fdrag + node * ref.G_lin)


def worst(x, ref, bound):
    """max |x - ref| / bound over every element; an element whose bound is zero has to be equal to its
    reference (else inf)."""
    err = np.abs(np.asarray(x).astype(ref.dtype) - ref)
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0


def plus_zero(a):
    """Every element exactly +0 (no -0, no NaN); complex: both parts."""
    a = np.asarray(a)
    parts = (a.real, a.imag) if np.iscomplexobj(a) else (a,)
    return all(bool(np.all(p == 0) and not np.signbit(p).any()) for p in parts)
