"""Inputs, long-double references and criteria for the direct tests of the wave-table, sea-state and
statistics kernels (tests/test_gpu_wave_tables.py, tests/test_gpu_sea_state.py; checked on the CPU by
tests/test_wave_cases.py).

Every reference is NumPy longdouble / clongdouble (80-bit on x86) of the double inputs the device
gets, in the formulas of oracle/raft_oracle.py (wave_kin, hydro_excitation, jonswap, get_psd,
get_rms).  Literal constants of the kernels (0.287, 1.15, M_PI, 57.29577951308232, ...) enter as
the doubles they are.  u = 2^-53.

Wave tables: a synthetic design aims at every branch of wave_node in one grid (WaveDesign).  Per
element of uhat and kproj, with th = k (cb x + sb y) and A = |th| + 2 k h + 8 (the device rounds the
phase and the hyperbolic arguments k (z + h) and k h),
    |dev - ref| <= 4 A u s,
s = |ref| for the vertical velocity, the horizontal amplitude |w c_sh| for the two horizontal ones
(cos(beta) near a zero must not set the scale), and max_c |uhat_c| times the frame entry sum for
kproj.  finer is a node sum that can cancel:
    |dev - ref| <= 4 (A_max + nn + 16) u S,   S = sum over nodes of |f6_n| per (heading, DOF, bin).
"""
import types

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
DEPTH = 200.0
HEADINGS = (0.0, np.pi / 2, 0.7)
# (nn, nw, nhead): nn <= 8 is the single-launch kernel, 9 and 21 the node-grid kernel plus the force sum
# (21: a partial last node group); 63, 65, 130 leave pad lanes
SHAPES = [(1, 1, 1), (8, 65, 3), (9, 63, 1), (21, 130, 3), (21, 64, 2)]
RAD2DEG = 57.29577951308232


# ------------------------------------------------------------------------------ wave tables
def edge_wavenumbers(nw, rng):
    """k per bin (an input of the kernel; it need not satisfy the dispersion relation), depth 200:
    a moderate one, k h < 1, k h on and next to the deep-water switch 89.4, k h > 710 (sinh and cosh
    of it overflow a double) up to k = 4 (k |z| <= 600 at z = -150), then log-uniform fill."""
    ks = 89.4 / DEPTH
    edges = [0.0625, 0.004, np.nextafter(ks, 0.0), ks, np.nextafter(ks, 1.0), 0.4469, 0.4471, 3.56, 4.0, 3.9]
    k = np.exp(rng.uniform(np.log(0.003), np.log(4.0), nw))
    n = min(nw, len(edges))
    k[:n] = edges[:n]
    return k


class WaveDesign:
    """A stand-in FOWT for prep.DeviceDesign (host_tables): nn submerged nodes, node positions r and
    PRP-relative positions r_rel that differ by an offset, a random orthonormal frame per node, a
    random non-symmetric Imat, a_i of both signs, every third node MacCamy-Fuchs with a random
    complex imat_mcf [nn][9][nw], no drag."""

    def __init__(self, nn, nw, seed=0):
        rng = np.random.default_rng(1000 * nn + nw + seed)
        self.nn, self.nw = nn, nw
        self.dw, self.depth, self.rho_water, self.g = 0.125, DEPTH, 1025.0, 9.81
        self.w = np.sort(rng.uniform(0.1, 3.0, nw))
        self.k = edge_wavenumbers(nw, rng)
        r = np.empty([nn, 3])
        r[:, :2] = rng.uniform(-50.0, 50.0, [nn, 2])
        far = np.arange(nn) % 3 == 2                           # farm spacing on some nodes
        # (x and y of one sign there: the headings lie in the first quadrant, so cb x and sb y do not
        # cancel and |th| measures the rounding of the phase, as the criterion's A assumes)
        r[far, :2] = rng.choice([-1.0, 1.0], [far.sum(), 1]) * rng.uniform(500.0, 1000.0, [far.sum(), 2])
        r[:, 2] = rng.uniform(-140.0, -0.5, nn)
        r[0, 2] = -0.01
        if nn > 1:
            r[1, 2] = -150.0
        self.r = r
        self.r_rel = r - np.array([12.5, -7.25, 3.0])
        frames = np.linalg.qr(rng.standard_normal([nn, 3, 3]))[0]
        self.q, self.p1, self.p2 = frames[:, :, 0].copy(), frames[:, :, 1].copy(), frames[:, :, 2].copy()
        self.Imat = rng.standard_normal([nn, 3, 3]) * 1e5
        self.a_i = rng.choice([-1.0, 1.0], nn) * rng.uniform(0.5, 20.0, nn)
        self.mcf = np.arange(nn) % 3 == 1 if nn > 1 else np.array([True])
        self.imat_mcf = (rng.standard_normal([nn, 9, nw]) + 1j * rng.standard_normal([nn, 9, nw])) * 1e5

    def host_tables(self):
        from raft import _native as N
        nn = self.nn
        node = np.zeros([N.NF_COUNT, nn])
        for f, v in (("RX", self.r[:, 0]), ("RY", self.r[:, 1]), ("RZ", self.r[:, 2]),
                     ("XX", self.r_rel[:, 0]), ("XY", self.r_rel[:, 1]), ("XZ", self.r_rel[:, 2]),
                     ("QX", self.q[:, 0]), ("QY", self.q[:, 1]), ("QZ", self.q[:, 2]),
                     ("P1X", self.p1[:, 0]), ("P1Y", self.p1[:, 1]), ("P1Z", self.p1[:, 2]),
                     ("P2X", self.p2[:, 0]), ("P2Y", self.p2[:, 1]), ("P2Z", self.p2[:, 2]),
                     ("CIRC", 1.0), ("AI", self.a_i), ("MCF", self.mcf.astype(float))):
            node[N.NF[f]] = v
        node[N.NF["I00"]:N.NF["I00"] + 9] = self.Imat.reshape(nn, 9).T
        memb = np.zeros([N.MF_COUNT, 1])                       # one member holds every node (unused by the tables)
        memb[2, 0] = memb[6, 0] = memb[13, 0] = 1.0
        memb[18:21, 0] = 1.0
        z = np.zeros([6, 6])
        parts = [("w", self.w), ("k", self.k), ("node", node), ("memb", memb), ("M", z), ("B", z), ("C", z)]
        layout, off = {}, 0
        for name, a in parts:
            layout[name] = (off, a.shape)
            off += a.size
        packed = np.concatenate([np.ascontiguousarray(a, dtype=float).ravel() for _, a in parts])
        return dict(packed=packed, layout=layout, imat=self.imat_mcf.copy(), mstart=np.array([0, nn], dtype=np.int32),
                    nn=nn, nm=1, per_bin=False)


def wave_reference(d, betas, rho_g=1025.0 * 9.81):
    """uhat, kproj [nh][nn][3][nw], f6 [nh][nn][6][nw] (per node) and finer [nh][6][nw] in clongdouble,
    with the scales of the criteria: A [nh][nn][nw], su, sk [nh][nn][3][nw] and S [nh][6][nw]."""
    nh, nn, nw = len(betas), d.nn, d.nw
    w, k, h = d.w.astype(LD), d.k.astype(LD), LD(d.depth)
    deep = d.k * d.depth > 89.4                                # the switch as the device takes it, in double
    uhat = np.zeros([nh, nn, 3, nw], dtype=CLD)
    kproj = np.zeros_like(uhat)
    f6 = np.zeros([nh, nn, 6, nw], dtype=CLD)
    A = np.zeros([nh, nn, nw], dtype=LD)
    su = np.zeros([nh, nn, 3, nw], dtype=LD)
    sk = np.zeros_like(su)
    kz = np.where(deep, LD(0), k)                              # (keeps the unused branch finite)
    for ih, be in enumerate(betas):
        cb, sb = np.cos(LD(be)), np.sin(LD(be))
        for n in range(nn):
            x, y, z = (LD(v) for v in d.r[n])
            th = k * (cb * x + sb * y)
            e = np.cos(th) - 1j * np.sin(th)
            ez = np.exp(k * z)
            skh = np.sinh(kz * h)
            skh = np.where(deep, LD(1), skh)
            s_sh = np.where(deep, ez, np.sinh(kz * (z + h)) / skh)
            c_sh = np.where(deep, ez, np.cosh(kz * (z + h)) / skh)
            c_ch = np.where(deep, ez + np.exp(-k * (z + 2 * h)), np.cosh(kz * (z + h)) / np.cosh(kz * h))
            u = np.stack([w * e * c_sh * cb, w * e * c_sh * sb, 1j * w * e * s_sh])
            uhat[ih, n] = u
            A[ih, n] = np.abs(th) + 2 * k * h + 8
            su[ih, n, 0] = su[ih, n, 1] = np.abs(w * c_sh)
            su[ih, n, 2] = np.abs(u[2])
            umax = np.abs(u).max(axis=0)
            for a, ax in enumerate((d.q[n], d.p1[n], d.p2[n])):
                ax = ax.astype(LD)
                kproj[ih, n, a] = u[0] * ax[0] + u[1] * ax[1] + u[2] * ax[2]
                sk[ih, n, a] = umax * np.abs(ax).sum()
            ud = 1j * w * u
            pd = rho_g * e * c_ch
            if d.mcf[n]:
                Im = d.imat_mcf[n].astype(CLD).reshape(3, 3, nw)
                f = np.einsum("ijb,jb->ib", Im, ud)
            else:
                f = d.Imat[n].astype(LD).astype(CLD) @ ud
            f = f + pd * LD(d.a_i[n]) * d.q[n].astype(LD)[:, None]
            rx, ry, rz = (LD(v) for v in d.r_rel[n])
            f6[ih, n, :3] = f
            f6[ih, n, 3] = f[2] * ry - f[1] * rz
            f6[ih, n, 4] = f[0] * rz - f[2] * rx
            f6[ih, n, 5] = f[1] * rx - f[0] * ry
    finer = f6.sum(axis=1)
    S = np.abs(f6).sum(axis=1)
    return types.SimpleNamespace(uhat=uhat, kproj=kproj, f6=f6, finer=finer, A=A, su=su, sk=sk, S=S)


def table_ratios(ref, uhat, kproj, finer, nn):
    """Worst |x - ref| / bound of the three tables (x double or long double); all references must be
    normal numbers, so no element is left out."""
    tiny = np.finfo(float).tiny
    assert np.all(np.abs(ref.uhat[:, :, 2]) > tiny) and np.all(ref.su > tiny) and np.all(ref.sk > tiny)
    A = ref.A[:, :, None, :]
    ru = np.abs(uhat.astype(CLD) - ref.uhat) / (4 * A * U * ref.su)
    rk = np.abs(kproj.astype(CLD) - ref.kproj) / (4 * A * U * ref.sk)
    Amax = ref.A.max(axis=1)[:, None, :]
    rf = np.abs(finer.astype(CLD) - ref.finer) / (4 * (Amax + nn + 16) * U * ref.S)
    return float(ru.max()), float(rk.max()), float(rf.max())


def oracle_tables(d, betas):
    """The same three tables from the double-precision oracle (O.hydro_excitation, unit amplitude)."""
    from oracle import raft_oracle as O
    T = dict(w=d.w, k=d.k, depth=d.depth)
    nodes = types.SimpleNamespace(n=d.nn, r=d.r, r_rel=d.r_rel, q=d.q, mcf=d.mcf, a_i=d.a_i, Imat=d.Imat,
                                  Imat_MCF=d.imat_mcf.reshape(d.nn, 3, 3, d.nw))
    u, _, _, F = O.hydro_excitation(T, nodes, np.asarray(betas, dtype=float), np.ones([len(betas), d.nw]))
    kp = np.stack([np.einsum("hncb,nc->hnb", u, ax) for ax in (d.q, d.p1, d.p2)], axis=2)
    return u, kp, F


# ------------------------------------------------------------------------------ sea state
def sea_cases():
    """(Hs, Tp, gamma, what it aims at): the IEC gamma branches on and next to their boundaries."""
    return [(4.0, 7.2, 0.0, "Tp/sqrt(Hs) = 3.6 exactly: G = 5"),
            (4.0, np.nextafter(7.2, 8.0), 0.0, "the exp branch, G = 5.0028"),
            (4.0, 10.0, 0.0, "Tp/sqrt(Hs) = 5 exactly: G = 1"),
            (4.0, np.nextafter(10.0, 9.0), 0.0, "just below 5"),
            (1.0, 3.6, 0.0, "3.6 exactly, Hs = 1"),
            (9.3, 17.7, 0.0, "interior, G = 1"),
            (1.2, 4.4, 0.0, "interior, exp branch"),
            (6.0, 12.0, 3.3, "given gamma 3.3"),
            (2.5, 8.0, 1.0, "given gamma 1.0")]


def sea_grid(nw):
    return np.linspace(0.02, 3.0, nw)


def jonswap_ld(ws, Hs, Tp, gamma):
    """oracle jonswap in long double (the branch arguments of the cases above are exact in double)."""
    Hs, Tp = LD(Hs), LD(Tp)
    if not gamma:
        t = Tp / np.sqrt(Hs)
        if t <= LD(3.6):
            G = LD(5.0)
        elif t >= LD(5.0):
            G = LD(1.0)
        else:
            G = np.exp(LD(5.75) - LD(1.15) * t)
    else:
        G = LD(gamma)
    pi = LD(np.pi)
    f = LD(0.5) / pi * np.asarray(ws, dtype=float).astype(LD)
    fp4 = (Tp * f) ** LD(-4.0)
    C = 1 - LD(0.287) * np.log(G)
    sig = np.where(f <= 1 / Tp, LD(0.07), LD(0.09))
    alpha = np.exp(-LD(0.5) * ((f * Tp - 1) / sig) ** 2)
    return LD(0.5) / pi * C * LD(0.3125) * Hs * Hs * fp4 / f * np.exp(-LD(1.25) * fp4) * G ** alpha


def sea_reference(nw, dw):
    """Per JONSWAP case of sea_cases(): (S_ref, zeta_ref, compared bins, e_np) on sea_grid(nw); e_np is
    the worst relative error of the double oracle over the bins whose reference exceeds 1e-300."""
    from oracle import raft_oracle as O
    w = sea_grid(nw)
    out = []
    for Hs, Tp, gam, _ in sea_cases():
        S = jonswap_ld(w, Hs, Tp, gam)
        keep = S > LD(1e-300)
        Snp = O.jonswap(w, Hs, Tp, Gamma=gam)
        e_np = float((np.abs(Snp.astype(LD) - S)[keep] / S[keep]).max()) if keep.any() else 0.0
        out.append((S, np.sqrt(2 * S * LD(dw)), keep, e_np))
    return out


def check_sea(label, ref, S, zeta):
    """The JONSWAP criterion of one case: S (or None) and zeta [nw] against ref = (S_ref, zeta_ref,
    keep, e_np).  Returns the device's worst relative errors (S, zeta)."""
    S_ref, z_ref, keep, e_np = ref
    tol = 8 * max(e_np, 4 * U)
    eS = ez = 0.0
    if S is not None:
        assert np.all(S[~keep] <= 1e-290) and np.all(S[~keep] >= 0), label
        if keep.any():
            eS = float((np.abs(S.astype(LD) - S_ref)[keep] / S_ref[keep]).max())
        assert eS <= tol, (label, eS, tol)
    assert np.all(zeta[~keep] <= np.sqrt(2 * 1e-290 * 1.0)) and np.all(zeta[~keep] >= 0), label
    if keep.any():
        ez = float((np.abs(zeta.astype(LD) - z_ref)[keep] / z_ref[keep]).max())
    assert ez <= 0.5 * tol + 2 * U, (label, ez, tol)
    return eS, ez


# ------------------------------------------------------------------------------ statistics
STAT_SHAPES = [(1, 1, 1), (3, 2, 63), (2, 3, 257), (1, 1, 1000)]       # (ncase, nrow, nw)


def stat_inputs(ncase, nrow, ndof, nw, seed=0):
    rng = np.random.default_rng(7919 * ncase + 131 * nrow + 17 * ndof + nw + seed)
    X = rng.standard_normal([ncase, nrow, ndof, nw]) + 1j * rng.standard_normal([ncase, nrow, ndof, nw])
    return X * 10.0 ** rng.uniform(-2, 1, [ncase, nrow, ndof, 1])


def motion_reference(Xi, dw):
    """psd [ncase][6][nw] = sum_row 0.5 |x|^2 / dw, std [ncase][6] = sqrt(0.5 sum |x|^2), rotations
    (DOF 3..5) in degrees (get_psd / get_rms in long double)."""
    x = Xi.astype(CLD)
    x[:, :, 3:] = x[:, :, 3:] * LD(RAD2DEG)
    m2 = x.real ** 2 + x.imag ** 2
    return (LD(0.5) * m2 / LD(dw)).sum(axis=1), np.sqrt(LD(0.5) * m2.sum(axis=(1, 3)))


def channel_coef(nch, ndof, seed=0):
    """coef [nch][2][ndof] = {a, c}: per DOF one of (0, 0) (the skip branch), only the w^2 term, only a,
    both; mixed signs and scales."""
    rng = np.random.default_rng(100 * nch + ndof + seed)
    coef = rng.standard_normal([nch, 2, ndof]) * 10.0 ** rng.uniform(-1, 2, [nch, 2, ndof])
    kind = (np.arange(ndof)[None, :] + np.arange(nch)[:, None]) % 4
    coef[:, 0][kind <= 1] = 0.0          # kind 0: (0, 0); kind 1: only c
    coef[:, 1][(kind == 0) | (kind == 2)] = 0.0
    return coef


def channel_reference(Xi, w, coef, dw):
    """psd [ncase][nch][nw], std [ncase][nch] of x_k = sum_d a_kd Xi_d + w^2 sum_d c_kd Xi_d in long
    double, and the same expressions of |a|, |c| and |Xi| (the scale of the criterion)."""
    x = Xi.astype(CLD)
    a, c = coef[:, 0].astype(LD), coef[:, 1].astype(LD)
    w2 = w.astype(LD) ** 2
    xk = np.einsum("kd,irdb->irkb", a, x) + w2 * np.einsum("kd,irdb->irkb", c, x)
    xa = np.einsum("kd,irdb->irkb", np.abs(a), np.abs(x)) + w2 * np.einsum("kd,irdb->irkb", np.abs(c), np.abs(x))
    out = []
    for v in (xk.real ** 2 + xk.imag ** 2, xa ** 2):
        out += [(LD(0.5) * v / LD(dw)).sum(axis=1), np.sqrt(LD(0.5) * v.sum(axis=(1, 3)))]
    return out            # psd, std, psd_abs, std_abs
