"""The transposing wave reductions of k_solve_lds (tbfly8, tbfly4, tbfly3 of csrc/rh_solve.hip) as a NumPy
model on 64 lanes: the written specification of their exchange order.

Every value meets its partners in one order: lane ^ 32, lane ^ 16, then inside the 16-lane row ^2, ^15, ^1,
^7 (quad_perm [2,3,0,1], row_mirror, quad_perm [1,0,3,2], row_half_mirror).  The two cross-row steps are
the gfx950 row swaps called with two different values: v_permlane32_swap x, y exchanges the upper half
of x with the lower half of y, v_permlane16_swap the odd rows of x with the even rows of y, so that
new x + new y is the pair sum of x in the lower half (the even rows) and the pair sum of y in the upper
half (the odd rows).  The one in-row transposing stage of tbfly8 keeps one of two values by the flag
f0 = bit 1 ^ bit 2 of the lane, which ^2 flips and ^15, ^1, ^7 leave alone (on the writer lanes, where
bit 2 is clear, it is bit 1).

Checked: each slot's total arrives in the writer lanes the kernel stores from, every lane of a value's
group holds the same bits, and the bits of a value's total do not depend on the slot or the network it
is fed into (random doubles and magnitudes 1e-30 .. 1e30, where any change of association shows).
"""
import numpy as np
import pytest

LANE = np.arange(64)
F0 = ((LANE >> 1) ^ (LANE >> 2)) & 1
IN_ROW = (2, 15, 1, 7)


def swap32(x, y):
    """v_permlane32_swap x, y: (new x, new y)."""
    nx, ny = x.copy(), y.copy()
    nx[32:], ny[:32] = y[:32], x[32:]
    return nx, ny


def swap16(x, y):
    """v_permlane16_swap x, y: (new x, new y)."""
    nx, ny = x.copy(), y.copy()
    for r in (0, 32):
        nx[r + 16:r + 32], ny[r:r + 16] = y[r:r + 16], x[r + 16:r + 32]
    return nx, ny


def pair32(x, y):
    a, b = swap32(x, y)
    return a + b


def pair16(x, y):
    a, b = swap16(x, y)
    return a + b


def dpp(v, xor):
    """A full-mask DPP move whose lane i reads lane i ^ xor of its row (xor < 16)."""
    return v[LANE ^ xor]


def row_tail(t, stages=IN_ROW[1:]):
    for s in stages:
        t = t + dpp(t, s)
    return t


def tbfly8(u):
    v = [pair32(u[p], u[p + 4]) for p in range(4)]
    w = [pair16(v[p], v[p + 2]) for p in range(2)]
    keep, send = np.where(F0 == 1, w[1], w[0]), np.where(F0 == 1, w[0], w[1])
    return row_tail(keep + dpp(send, IN_ROW[0]))


def tbfly4(a, b, c, d):
    t = pair16(pair32(a, c), pair32(b, d))
    return row_tail(t, IN_ROW)


def tbfly3(a, b, c):
    return tbfly4(a, b, c, np.zeros(64))


IDX8 = 4 * (LANE >> 5) + 2 * ((LANE >> 4) & 1) + F0        # the value every lane ends with
IDX4 = LANE >> 4
WRITERS8 = [int(i) for i in LANE if (i & 13) == 0]          # the kernel stores from these
WRITERS4 = [0, 16, 32, 48]
WRITERS3 = [0, 16, 32]


def test_writer_lanes():
    assert WRITERS8 == [0, 2, 16, 18, 32, 34, 48, 50]
    assert [int(IDX8[i]) for i in WRITERS8] == list(range(8))
    assert all(IDX8[i] == 4 * (i >> 5) + 2 * ((i >> 4) & 1) + ((i >> 1) & 1) for i in WRITERS8)
    assert [int(IDX4[i]) for i in WRITERS4] == [0, 1, 2, 3]


def test_swap_semantics():
    """Lower half (even rows): {x_L, x_partner}; upper half (odd rows): {y_partner, y_L}."""
    x, y = LANE.astype(float), 100.0 + LANE
    a, b = swap32(x, y)
    assert np.array_equal(a[:32], x[:32]) and np.array_equal(b[:32], x[32:])
    assert np.array_equal(a[32:], y[:32]) and np.array_equal(b[32:], y[32:])
    a, b = swap16(x, y)
    for r in (0, 32):
        assert np.array_equal(a[r:r + 16], x[r:r + 16]) and np.array_equal(b[r:r + 16], x[r + 16:r + 32])
        assert np.array_equal(a[r + 16:r + 32], y[r:r + 16]) and np.array_equal(b[r + 16:r + 32], y[r + 16:r + 32])


def _ints(rng, n):
    return rng.integers(-2 ** 20, 2 ** 20, [n, 64]).astype(float)       # exact sums in any order


def test_totals_arrive_in_the_writer_lanes():
    rng = np.random.default_rng(1)
    u = _ints(rng, 8)
    t = tbfly8(u)
    assert np.array_equal(t, u.sum(axis=1)[IDX8])                       # every lane: the total of its value
    assert [t[i] for i in WRITERS8] == list(u.sum(axis=1))
    q = _ints(rng, 4)
    t = tbfly4(*q)
    assert np.array_equal(t, q.sum(axis=1)[IDX4])
    assert [t[i] for i in WRITERS4] == list(q.sum(axis=1))
    t = tbfly3(*q[:3])
    assert [t[i] for i in WRITERS3] == list(q[:3].sum(axis=1)) and np.all(t[48:] == 0)


def _values(kind, rng):
    if kind == "random":
        return rng.standard_normal(64)
    return rng.choice([-1.0, 1.0], 64) * 10.0 ** rng.uniform(-30, 30, 64)


@pytest.mark.parametrize("kind", ["random", "mixed"])
def test_groups_hold_the_same_bits(kind):
    rng = np.random.default_rng(2)
    u = np.stack([_values(kind, rng) for _ in range(8)])
    t = tbfly8(u)
    for k in range(8):
        assert len(set(t[IDX8 == k].view(np.int64))) == 1
    for t, n in ((tbfly4(*u[:4]), 4), (tbfly3(*u[:3]), 3)):
        for k in range(n):
            assert len(set(t[IDX4 == k].view(np.int64))) == 1


@pytest.mark.parametrize("kind", ["random", "mixed"])
def test_bits_do_not_depend_on_the_slot_or_the_network(kind):
    rng = np.random.default_rng(3)
    for _ in range(20):
        x = _values(kind, rng)
        got = []
        for k in range(8):
            u = np.stack([_values(kind, rng) for _ in range(8)])
            u[k] = x
            got.append(tbfly8(u)[WRITERS8[k]])
        for k in range(4):
            q = [_values(kind, rng) for _ in range(4)]
            q[k] = x
            got.append(tbfly4(*q)[WRITERS4[k]])
        for k in range(3):
            q = [_values(kind, rng) for _ in range(3)]
            q[k] = x
            got.append(tbfly3(*q)[WRITERS3[k]])
        assert len(set(np.array(got).view(np.int64))) == 1, (kind, got)
        # the order, said outright: rows first, then the in-row partners
        s = x[:32] + x[32:]
        s = s[:16] + s[16:]
        for st in IN_ROW:
            s = s + s[np.arange(16) ^ st]
        assert got[0] == s[0]
