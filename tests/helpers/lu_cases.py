"""Adversarial inputs, lane layout and high-precision references for the dense complex solves of the
device: rh::lu_solve<6>, rh::lu_factor<6> / rh::lu_apply<6> (csrc/rh_device.h) and the two-FOWT
block solve (csrc/rh_kernels.hip).  NumPy and mpmath only; used by tests/test_lu_cases.py (CPU) and
tests/test_gpu_lu.py (device).

device_lu6 / device_block12 restate the device arithmetic (|re|+|im| pivot, first maximum wins, the
reciprocal pivot conj(p)/|p|^2, the block formulas of k_system_solve_reg<2>).  They serve to design
inputs and to check coverage; they are never the expected value of a device test.  The expected value
is always a bound on the backward error eta (backward_error, residual in 50-digit mpmath), measured
against what numpy.linalg.solve reaches on the same family.
"""
import itertools

import mpmath as mp
import numpy as np

mp.mp.dps = 50
U = 2.0 ** -53
NAN = complex(np.nan, np.nan)


# ------------------------------------------------------------------------------ device arithmetic
def _cabs1(z):
    return np.abs(z.real) + np.abs(z.imag)


def device_lu(A, b, raw=False):
    """rh::lu_solve in numpy for any n.  Returns (x, exchanges, zero_step): exchanges is the list of
    (step, row) with row != step, zero_step the first step that met an exactly zero pivot (None if
    there was none); x is all NaN in that case, as the device stores it (raw: the finite numbers the
    elimination goes on to compute with 1 in place of the zero pivot, which the device never stores)."""
    A = np.array(A, dtype=complex)
    x = np.array(b, dtype=complex)
    n = len(x)
    ex, zero = [], None
    for k in range(n):
        v = _cabs1(A[k:, k])
        p = k + int(np.argmax(v))          # argmax: the first maximum
        if p != k:
            ex.append((k, p))
            A[[k, p], k:] = A[[p, k], k:]
            x[[k, p]] = x[[p, k]]
        if v.max() == 0 and zero is None:
            zero = k
        piv = A[k, k] if v.max() != 0 else 1.0 + 0j
        inv = 1.0 / (piv.real * piv.real + piv.imag * piv.imag)
        rinv = complex(piv.real * inv, -piv.imag * inv)
        A[k, k] = rinv
        for i in range(k + 1, n):
            l = A[i, k] * rinv
            A[i, k + 1:] -= l * A[k, k + 1:]
            x[i] -= l * x[k]
    for k in range(n - 1, -1, -1):
        s = x[k]
        for j in range(k + 1, n):
            s -= A[k, j] * x[j]
        x[k] = s * A[k, k]
    if zero is not None and not raw:
        x = np.full(n, NAN)
    return x, ex, zero


def device_lu6(A, b):
    """(x, exchanges) of rh::lu_solve<6>; x is NaN after an exactly zero pivot."""
    assert np.shape(A) == (6, 6)
    x, ex, _ = device_lu(A, b)
    return x, ex


def zero_pivot_step(A):
    return device_lu(A, np.ones(len(A)))[2]


def device_block12(Z1, Z2, K, F, raw=False):
    """k_system_solve_reg<2>: A = Z1 + K11 factored once, X = A^-1 K12, S = (Z2 + K22) - K21 X,
    x2 = S^-1 (f2 - K21 A^-1 f1), x1 = A^-1 f1 - X x2.  Returns (x, exchanges of A, exchanges of S);
    x is NaN after a zero pivot in A or S (raw: what the arithmetic gives without that rule)."""
    K = np.asarray(K, dtype=float)
    A = Z1 + K[:6, :6]
    D = Z2 + K[6:, 6:]
    y, o1, z1 = device_lu(A, F[:6], raw=True)
    X = np.zeros([6, 6], dtype=complex)
    for j in range(6):
        X[:, j] = device_lu(A, K[:6, 6 + j].astype(complex), raw=True)[0]
    S = D - K[6:, :6] @ X
    g = F[6:] - K[6:, :6] @ y
    x2, o2, z2 = device_lu(S, g, raw=True)
    if (z1 is not None or z2 is not None) and not raw:
        return np.full(12, NAN), o1, o2
    return np.concatenate([y - X @ x2, x2]), o1, o2


def assemble12(Z1, Z2, K):
    Zs = np.array(K, dtype=complex)
    Zs[:6, :6] += Z1
    Zs[6:, 6:] += Z2
    return Zs


# ------------------------------------------------------------------------------ references
def _mpc(z):
    return mp.mpc(float(np.real(z)), float(np.imag(z)))


def backward_error(A, b, x):
    """eta = ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf), the residual formed in mpmath."""
    A, b, x = np.asarray(A), np.asarray(b), np.asarray(x)
    n = len(b)
    xs = [_mpc(v) for v in x]
    rn = mp.mpf(0)
    for i in range(n):
        r = _mpc(b[i])
        for j in range(n):
            if A[i, j] != 0:
                r -= _mpc(A[i, j]) * xs[j]
        rn = max(rn, abs(r))
    den = np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
    return float(rn / mp.mpf(float(den)))


def backward_errors(A, b, x):
    """backward_error of every system of a stack A [m][n][n], b / x [m][n]."""
    return np.array([backward_error(A[i], b[i], x[i]) for i in range(len(A))])


def forward_error(A, b, x):
    """||x - x_exact||_inf / ||x_exact||_inf with x_exact from an mpmath LU solve (a subsample only)."""
    n = len(b)
    M = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            M[i, j] = _mpc(A[i, j])
    xe = mp.lu_solve(M, mp.matrix([_mpc(v) for v in b]))
    num = max(abs(_mpc(x[i]) - xe[i]) for i in range(n))
    return float(num / max(abs(xe[i]) for i in range(n)))


# ------------------------------------------------------------------------------ 6 x 6 families
PAIRS = [(k, p) for k in range(6) for p in range(k + 1, 6)]


def _cplx(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _dominant(rng):
    """Strictly column-dominant in |re|+|im| by a wide margin (a property every Schur complement
    inherits): its elimination exchanges no rows."""
    return 4.0 * np.diag(np.exp(2j * np.pi * rng.random(6))) + 0.12 * _cplx(rng, 6, 6)


def _every_step_perms():
    """Row orders of a dominant matrix whose elimination exchanges at every step 0..4."""
    B = _dominant(np.random.default_rng(5))
    out = []
    for perm in itertools.permutations(range(6)):
        ex = device_lu6(B[list(perm)], np.ones(6))[1]
        if [k for k, _ in ex] == [0, 1, 2, 3, 4]:
            out.append(perm)
    return out


_EVERY = None


def every_step_perms():
    global _EVERY
    if _EVERY is None:
        _EVERY = _every_step_perms()
    return _EVERY


def family_P(seed):
    """Pivot patterns: name -> matrix.  'pair k p' exchanges exactly rows k and p at step k, 'all *'
    exchanges at every step (the two 6-cycles among them), 'reversal' at steps 0, 1, 2, 'none *'
    never.  Each is a dominant matrix with permuted rows; the trace is confirmed with device_lu6."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, p in PAIRS:
        perm = list(range(6))
        perm[k], perm[p] = p, k
        out[f"pair {k} {p}"] = _dominant(rng)[perm]
    out["reversal"] = _dominant(rng)[::-1].copy()
    out["all cycle+"] = _dominant(rng)[[1, 2, 3, 4, 5, 0]]      # exchanges (k, 5) at every step
    out["all cycle-"] = _dominant(rng)[[5, 0, 1, 2, 3, 4]]      # exchanges (k, k + 1) at every step
    ev = every_step_perms()
    for i in range(6):
        out[f"all {i}"] = _dominant(rng)[list(ev[int(rng.integers(len(ev)))])]
    for i in range(4):
        out[f"none {i}"] = _dominant(rng)
    for name, A in out.items():
        ex = device_lu6(A, np.ones(6))[1]
        if name.startswith("pair"):
            k, p = int(name[5]), int(name[7])
            assert ex == [(k, p)], (name, ex)
        elif name.startswith("all"):
            assert [k for k, _ in ex] == [0, 1, 2, 3, 4], (name, ex)
        elif name == "reversal":
            assert ex == [(0, 5), (1, 4), (2, 3)], ex
        else:
            assert ex == [], (name, ex)
    return out


def family_T(seed):
    """Ties: at step k the pivot column holds two entries of equal |re|+|im| = 7 and different moduli
    (5+2i, modulus 5.39, and 3+4i, modulus 5; every sign and both orders).  The first one wins, so no
    row is exchanged at that step; a rule by modulus or a '>=' would exchange.  Rows above k are
    upper triangular, so the trailing block reaches step k untouched, bit for bit."""
    rng = np.random.default_rng(seed)
    out = {}
    vals = [(5 + 2j, 3 + 4j), (3 + 4j, 5 + 2j), (-5 + 2j, 4 - 3j), (2 - 5j, -4 - 3j), (7 + 0j, 3.5 + 3.5j)]
    for k in range(5):
        for t, (a, b) in enumerate(vals):
            A = 0.25 * _cplx(rng, 6, 6)
            for j in range(k):
                A[j + 1:, j] = 0.0
                A[j, j] = 4.0 * np.exp(2j * np.pi * rng.random())
            r = k + 1 + int(rng.integers(5 - k))
            A[k, k], A[r, k] = a, b
            for i in range(k + 1, 6):        # the rest of the trailing block dominant, so that the
                A[i, i] += 4.0               # tie is the only close call
            ex = device_lu6(A, np.ones(6))[1]
            assert all(s != k for s, _ in ex), (k, t, ex)
            assert _cabs1(A[k, k]) == _cabs1(A[r, k]) and abs(A[k, k]) != abs(A[r, k])
            out[f"tie {k} {t}"] = A
    return out


def family_S(seed, m=24):
    """Scaling: D1 R D2 with D = 10^U(-3, 6) per row and per column (as test_solve6_matches_lapack
    scales its rows).  Every pivot modulus stays inside [1e-100, 1e100]."""
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(m):
        A = _cplx(rng, 6, 6) * 10 ** rng.uniform(-3, 6, [6, 1]) * 10 ** rng.uniform(-3, 6, [1, 6])
        out[f"scaled {i}"] = A
    return out


def with_cond(rng, kappa, n=6):
    Uq, _ = np.linalg.qr(_cplx(rng, n, n))
    Vq, _ = np.linalg.qr(_cplx(rng, n, n))
    return Uq @ np.diag(np.logspace(0, -np.log10(kappa), n)) @ Vq.conj().T


def family_C(seed, m=8):
    """Conditioning: kappa_2 in {1e2, 1e6, 1e10}, U diag(s) V^H with log-spaced singular values."""
    rng = np.random.default_rng(seed)
    return {f"cond 1e{e} {i}": with_cond(rng, 10.0 ** e) for e in (2, 6, 10) for i in range(m)}


def family_Z(seed):
    """Exactly singular: the zero matrix; a column of zeros; a rank-5 matrix of small Gaussian
    integers (unit lower triangular L with entries in {-1, 0, 1} times an upper triangular U with
    power-of-two pivots and U[3][3] = 0) whose elimination is exact and meets a zero pivot at step 3."""
    rng = np.random.default_rng(seed)
    out = {"zero": np.zeros([6, 6], dtype=complex)}
    A = _cplx(rng, 6, 6)
    A[:, 2] = 0.0
    out["zero column"] = A
    L = np.tril(rng.integers(-1, 2, [6, 6]), -1) + np.eye(6)
    Ut = np.triu(rng.integers(-2, 3, [6, 6]) + 1j * rng.integers(-2, 3, [6, 6]), 1)
    Ut = Ut + np.diag([4, 2, 4, 0, 2, 4])
    Ut[0, :] = [4, 1, -1j, 2, 1 + 1j, -1]
    out["rank 5"] = (L @ Ut).astype(complex)
    assert np.linalg.matrix_rank(out["rank 5"]) == 5
    assert zero_pivot_step(out["zero"]) == 0 and zero_pivot_step(out["zero column"]) == 2
    assert zero_pivot_step(out["rank 5"]) == 3
    return out


REGULAR6 = {"P": family_P, "T": family_T, "S": family_S, "C": family_C}


# ------------------------------------------------------------------------------ lane layout
WAVE = 64


class Systems:
    """nw systems, one per bin: A [nw][n][n], b [nw][n], fam [nw] family letter, name [nw],
    singular [nw] bool."""

    def __init__(self, A, b, fam, name, singular=None):
        self.A, self.b, self.fam, self.name = A, b, np.array(fam), list(name)
        self.singular = np.zeros(len(A), dtype=bool) if singular is None else singular
        self.nw = len(A)


def _pools(seed, only_p=False):
    P = family_P(seed)
    none = [P[k] for k in P if k.startswith("none")]
    every = [P[k] for k in P if k.startswith("all")]
    fams = [[("P", k, P[k]) for k in P if k.startswith("pair") or k == "reversal"]]
    for fam, f in (() if only_p else (("T", family_T), ("S", family_S), ("C", family_C))):
        d = f(seed + 1)
        fams.append([(fam, k, d[k]) for k in d])
    # the families interleaved, so that one wave of 64 already holds every pair and all four of them
    rest = [f[i] for i in range(max(map(len, fams))) for f in fams if i < len(f)]
    return none, every, rest


def layout(nw, variant=0, seed=11, only_p=False):
    """One 6 x 6 system per bin, bins in waves of 64 consecutive bins (every solve kernel maps 64
    consecutive bins to the lanes of a wave).  The full waves hold, in turn:
      'none'   no lane exchanges at any step,
      'all'    every lane exchanges at every step 0..4 (with different rows from lane to lane),
      'mixed'  even lanes exchange at every step, odd lanes at none,
      'pool'   the 15 exact pairs, the reversal and families T, S and C, lane by lane,
    variant 0 in the order none, all, mixed, pool, pool, ...; variant 1 mixed (odd lanes exchange),
    none, all, pool, ...; variant 2 pool waves only.  A grid with fewer than three full waves holds the
    first of them.  The last, partial wave of a ragged nw alternates 'all' systems with exact pairs:
    every one of its lanes exchanges.  only_p: the pool holds family P alone.  Returns a Systems with
    kind [number of waves] naming each wave."""
    rng = np.random.default_rng(seed + 1000 * variant + nw)
    none, every, rest = _pools(seed + 100 * variant, only_p)
    order = [["none", "all", "mixed", "pool"], ["mixed", "none", "all", "pool"], ["pool"] * 4][variant]
    pairs = [r for r in rest if r[1].startswith("pair")]
    A = np.zeros([nw, 6, 6], dtype=complex)
    fam, name, kinds = [], [], []
    ipool = 0
    for w0 in range(0, nw, WAVE):
        wv = w0 // WAVE
        n = min(WAVE, nw - w0)
        kind = "tail" if n < WAVE else (order[wv] if wv < 4 else "pool")
        kinds.append(kind)
        for l in range(n):
            if kind == "none" or (kind == "mixed" and (l + variant) % 2 == 1):
                f, nm, M = "P", "none", none[(l // 2) % len(none)]
            elif kind == "all" or kind == "mixed":
                f, nm, M = "P", "all", every[(l // 2 + l) % len(every)]
            elif kind == "tail":
                f, nm, M = ("P", "all", every[l % len(every)]) if l % 2 == 0 else pairs[(l // 2) % len(pairs)]
            else:
                f, nm, M = rest[ipool % len(rest)]
                ipool += 1
            A[w0 + l] = M
            fam.append(f)
            name.append(nm)
    s = Systems(A, _cplx(rng, nw, 6), fam, name)
    s.kind = kinds
    return s


def with_singular(s, bins, seed=3):
    """A copy of a layout with family Z at the given bins (zero, zero column, rank 5 in turn)."""
    Z = family_Z(seed)
    keys = list(Z)
    t = Systems(s.A.copy(), s.b.copy(), s.fam.copy(), list(s.name), s.singular.copy())
    t.kind = list(getattr(s, "kind", []))
    for i, b in enumerate(bins):
        t.A[b] = Z[keys[i % 3]]
        t.fam[b] = "Z"
        t.name[b] = keys[i % 3]
        t.singular[b] = True
    return t


def traces(s):
    """[nw][5] bool: does bin b exchange rows at step k (device rule)."""
    out = np.zeros([s.nw, 5], dtype=bool)
    for b in range(s.nw):
        for k, _ in device_lu(s.A[b], s.b[b])[1]:
            out[b, k] = True
    return out


def check_layout(s):
    """The wave conditions of layout(): returns the set of wave kinds present; asserts each wave is
    what its kind says, at every step."""
    tr = traces(s)
    for wv, kind in enumerate(s.kind):
        t = tr[wv * WAVE:(wv + 1) * WAVE]
        if kind == "none":
            assert not t.any(), wv
        elif kind == "all":
            assert t.all(), wv
        elif kind == "mixed":
            assert (t[0::2] != t[1::2]).all() and (t[0::2] == t[0]).all(), wv
        elif kind == "tail":
            assert t.any(axis=1).all(), wv
    return set(s.kind)


# ------------------------------------------------------------------------------ 12 x 12 families
def _k12(rng, kind):
    """Real array stiffness with zero diagonal blocks: 'random' coupling blocks of norm comparable
    to the first block's, 'identity' K12 = K21 = I, 'rows' random with rows 0 and 1 of K12 equal."""
    K = np.zeros([12, 12])
    if kind == "identity":
        K[:6, 6:] = np.eye(6)
        K[6:, :6] = np.eye(6)
        return K
    K[:6, 6:] = rng.standard_normal([6, 6])
    K[6:, :6] = rng.standard_normal([6, 6])
    if kind == "rows":
        K[1, 6:] = K[0, 6:]
    return K


def _second_block(A, K, S):
    """D such that the Schur complement D - K21 A^-1 K12 the block path eliminates is S up to rounding."""
    return S + K[6:, :6] @ np.linalg.solve(A, K[:6, 6:].astype(complex))


def systems12(nw, case, seed=21):
    """One two-FOWT system per bin for a case with one shared real K (the ABI: the complex part lives
    in the diagonal blocks Z1, Z2 only).  Returns (Z [2][nw][6][6], K [12][12], F [nw][12], Systems of
    the assembled 12 x 12 matrices, with kappaA [nw] = kappa_2 of the first block).
      case 0  K random: B-P (both the first block and the Schur complement from family P, laid out by
              layout() variants 0 and 1, so the wave conditions hold for both eliminations), and in
              every eighth bin B-W, a weak first block with kappa_2(A) in {1, 1e4, 1e8} in turn and
              kappa_2(Z_sys) <= 1e3 (both asserted here);
      case 1  K12 = K21 = I: B-P, and in every eighth bin B-0 (A = 0, D random): a regular system
              whose first block is singular;
      case 2  K random with rows 0 and 1 of K12 equal: B-P, and in every sixteenth bin B-Z, rows 0 and
              1 of Z_sys equal with the value 4 (or 4i) leading them as the largest of column 0, so
              the elimination cancels row 1 exactly and both device paths meet a zero pivot."""
    rng = np.random.default_rng(seed + case)
    K = _k12(rng, ["random", "identity", "rows"][case])
    la, ls = layout(nw, 0, seed, only_p=True), layout(nw, 1, seed + 7, only_p=True)
    Z = np.zeros([2, nw, 6, 6], dtype=complex)
    fam, name = [], []
    sing = np.zeros(nw, dtype=bool)
    kA = np.ones(nw)
    for b in range(nw):
        A, f, nm = la.A[b], "B-P", la.name[b] + "/" + ls.name[b]
        D = _second_block(A, K, ls.A[b])
        if case == 0 and b % 8 == 3:
            kap = [1.0, 1e4, 1e8][(b // 8) % 3]
            for _ in range(200):
                A = with_cond(rng, kap)
                D = _cplx(rng, 6, 6)
                if np.linalg.cond(assemble12(A, D, K)) <= 1e3:
                    break
            else:
                raise AssertionError("no B-W draw with kappa(Z_sys) <= 1e3")
            sv = np.linalg.svd(A, compute_uv=False)
            assert abs(sv[0] / sv[-1] / kap - 1) < 1e-3 or kap > 1e7
            f, nm = "B-W", f"kappa {kap:.0e}"
        elif case == 1 and b % 8 == 3:
            A, D, f, nm = np.zeros([6, 6], dtype=complex), _cplx(rng, 6, 6), "B-0", "A = 0"
        elif case == 2 and b % 16 == 7:
            A = 0.5 * _cplx(rng, 6, 6)
            A[0, 0] = 4.0 if (b // 16) % 2 == 0 else 4.0j
            A[1] = A[0]
            D = _cplx(rng, 6, 6)
            f, nm = "B-Z", "rows 0 = 1"
            sing[b] = True
        Z[0, b], Z[1, b] = A, D
        fam.append(f)
        name.append(nm)
        sv = np.linalg.svd(A, compute_uv=False)
        kA[b] = sv[0] / sv[-1] if sv[-1] > 0 else np.inf
    F = _cplx(rng, nw, 12)
    Zs = np.array([assemble12(Z[0, b], Z[1, b], K) for b in range(nw)])
    s = Systems(Zs, F, fam, name, sing)
    s.kappaA = kA
    s.kind = la.kind
    return Z, K, F, s


# ------------------------------------------------------------------------------ criteria
def numpy_eta(s):
    """eta of numpy.linalg.solve on every regular system (NaN for singular ones) and the worst per family."""
    eta = np.full(s.nw, np.nan)
    for b in np.nonzero(~s.singular)[0]:
        eta[b] = backward_error(s.A[b], s.b[b], np.linalg.solve(s.A[b], s.b[b]))
    worst = {f: float(np.nanmax(eta[s.fam == f])) for f in sorted(set(s.fam[~s.singular]))}
    return eta, worst


def gepp_bound(worst):
    """Per family: eta <= 8 max(worst eta of numpy on that family, u)."""
    return {f: 8.0 * max(v, U) for f, v in worst.items()}


def table_row(label, s, eta_dev, worst_np):
    """One printed line per family: worst device eta next to numpy's."""
    rows = []
    for f in sorted(worst_np):
        sel = (s.fam == f) & ~s.singular
        rows.append(f"  {label:<34s} {f:<4s} n={int(sel.sum()):<5d} eta_dev {np.nanmax(eta_dev[sel]):.2e}   "
                    f"eta_numpy {worst_np[f]:.2e}")
    return "\n".join(rows)
