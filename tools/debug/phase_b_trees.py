"""Do two builds of k_solve_lds round phase B's 36 translate entries of a node the same way?

Under -ffp-contract=fast which product of a*b + c*d becomes the multiply-add is the compiler's choice,
and it has followed from things as remote as how many entries share a product ("Phase B's
LDS chains").  This reads two device assemblies (hipcc --offload-device-only -S of rh_solve_fast.hip or
rh_abi.hip), executes the per-node stage of phase B of one kernel symbolically (the stretch between two
barriers that holds the node's field loads) and compares, entry by entry, the expression trees of the 36
values written last, over the leaves B0..B8 (the node's Bmat, read back from its LDS row or still in
registers; symmetric entries are one value), rx, ry, rz and the literal 0.  Products commute, signs are
pulled out of products, and p + 0*z is the same value whichever of the two products is the fused one.
Equal trees are equal bits.

Usage: python tools/debug/phase_b_trees.py A.s B.s [mangled kernel name, default the C2 kernel]
(exit status 1 if an entry differs)
"""
import re
import sys

C2 = "_ZN2rh11k_solve_ldsILi2ELi512ELb0ELi1EEEvNS_8CaseArgsE"
VREG = re.compile(r"v\[(\d+):(\d+)\]")


def kernel_body(path, name):
    out, on = [], False
    for ln in open(path):
        if ln.startswith(name + ":"):
            on = True
        elif on and ln.startswith(".Lfunc_end"):
            break
        elif on:
            out.append(ln.rstrip("\n"))
    if not out:
        raise SystemExit(f"{path}: no kernel {name}")
    return out


def lds_writes(body):
    """[(address root, byte offset, expression)] of every LDS write of the per-node stage, in order."""
    bars = [i for i, l in enumerate(body) if re.match(r"\s*s_barrier\b", l)]
    span = [(bars[k], bars[k + 1]) for k in range(len(bars) - 1)
            if sum("global_load_dwordx2" in body[i] for i in range(bars[k], bars[k + 1])) >= 16]
    lo, hi = span[0]
    val, base, out, nload = {}, {}, [], 0   # 64-bit values by their low register; derived address registers

    def low(s):
        m = VREG.match(s)
        return int(m.group(1)) if m else None

    def operand(op):
        op = op.strip()
        neg = op.startswith("-")
        op = op.lstrip("-").strip("|")
        e = val.get(low(op), ("?", op)) if low(op) is not None else ("c", op)
        return ("neg", e) if neg else e

    def off(rest, key="offset"):
        m = re.search(key + r":(\d+)", rest)
        return int(m.group(1)) if m else 0

    def addr(reg, o):
        root, ro = base.get(reg, (reg, 0))
        return root, ro + o

    for i in range(lo, hi):
        l = body[i].split(";")[0].strip()
        if not l or l.endswith(":"):
            continue
        op, _, rest = l.partition(" ")
        a = [x.strip() for x in rest.split(",")]
        d = low(a[0])
        if op == "v_mul_f64":
            val[d] = ("mul", operand(a[1]), operand(a[2]))
        elif op == "v_add_f64":
            val[d] = ("add", operand(a[1]), operand(a[2]))
        elif op == "v_fma_f64":
            val[d] = ("fma", operand(a[1]), operand(a[2]), operand(a[3]))
        elif op == "v_fmac_f64_e32":
            val[d] = ("fma", operand(a[1]), operand(a[2]), operand(a[0]))
        elif op == "v_mov_b64_e32":
            val[d] = operand(a[1])
        elif op == "global_load_dwordx2":
            val[d] = ("G", nload)
            nload += 1
        elif op == "ds_read_b64":
            val[d] = ("L",) + addr(a[1].split()[0], off(rest))
        elif op == "ds_read2_b64":
            val[d] = ("L",) + addr(a[1].split()[0], 8 * off(rest, "offset0"))
            val[d + 2] = ("L",) + addr(a[1].split()[0], 8 * off(rest, "offset1"))
        elif op == "ds_read_b128":
            val[d] = ("L",) + addr(a[1].split()[0], off(rest))
            val[d + 2] = ("L",) + addr(a[1].split()[0], off(rest) + 8)
        elif op == "ds_write_b64":
            out.append(addr(a[0], off(rest)) + (operand(a[1].split()[0]),))
        elif op == "ds_write2_b64":
            out.append(addr(a[0], 8 * off(rest, "offset0")) + (operand(a[1]),))
            out.append(addr(a[0], 8 * off(rest, "offset1")) + (operand(a[2].split()[0]),))
        elif op == "ds_write_b128":
            s = low(a[1].split()[0])
            out.append(addr(a[0], off(rest)) + (val.get(s, ("?", s)),))
            out.append(addr(a[0], off(rest) + 8) + (val.get(s + 2, ("?", s + 2)),))
        elif (op == "v_add_u32_e32" and re.match(r"v\d+$", a[0]) and re.match(r"(0x[0-9a-f]+|\d+)$", a[1])
              and re.match(r"v\d+$", a[2])):
            root, ro = base.get(a[2], (a[2], 0))
            base[a[0]] = (root, ro + int(a[1], 0))
        elif op.startswith("v_"):
            if d is not None:
                val[d] = ("op", op, i)
            elif re.match(r"v(\d+)$", a[0]):   # a 32-bit write into half of a pair: the pair is no longer known
                n = int(a[0][1:])
                for b in (n, n - 1):
                    if b in val:
                        val[b] = ("op32", i)
    return out


def sym(k):
    r, c = divmod(k, 3)
    return "B%d" % (3 * min(r, c) + max(r, c))


def entry_trees(path, name):
    w = lds_writes(kernel_body(path, name))
    ent, names, bm0 = [x[2] for x in w[-36:]], {}, {}

    def leaves(t):
        if isinstance(t, tuple):
            if t and t[0] == "L":
                bm0[t[1]] = min(bm0.get(t[1], 1 << 30), t[2])
            else:
                for y in t:
                    leaves(y)
    for e in ent:
        leaves(e)
    if not bm0:   # Bmat in registers: its values are the ones written as Bq (q_i q_j) + ...
        bq = [x[2] for x in w[:-36] if x[2][0] == "fma" and x[2][2][0] == "mul" and x[2][2][1][0] == "G" and x[2][2][2][0] == "G"]
        q0 = min(min(x[2][1][1], x[2][2][1]) for x in bq)
        for x in bq:
            i, j = sorted([x[2][1][1] - q0, x[2][2][1] - q0])
            names[x] = "B%d" % (3 * i + j)

    def canon(e):   # (sign, tree)
        if e in names:
            return 1, names[e]
        t = e[0]
        if t == "neg":
            s, x = canon(e[1])
            return -s, x
        if t == "c":
            return 1, e[1]
        if t == "L":
            return 1, sym((e[2] - bm0[e[1]]) // 8)
        if t == "G":
            return 1, "G%d" % e[1]
        if t == "mul":
            (s1, a), (s2, b) = canon(e[1]), canon(e[2])
            return s1 * s2, ("mul",) + tuple(sorted([a, b], key=repr))
        if t == "fma":
            (s1, a), (s2, b), (s3, c) = canon(e[1]), canon(e[2]), canon(e[3])
            return 1, ("fma", s1 * s2, tuple(sorted([a, b], key=repr)), s3, c)
        if t == "add":
            return 1, ("add",) + tuple(sorted([canon(e[1]), canon(e[2])], key=repr))
        return 1, repr(e)

    trees = [canon(e) for e in ent]
    # entry (0, 3) is B0 0 - B1 rz + B2 ry: that names the three coordinates among the loaded fields
    txt = repr(trees[3])
    ry = re.search(r"\('B2', '(G\d+)'\)", txt).group(1)
    rz = re.search(r"'B1', '(G\d+)'", txt).group(1)
    rx = (set(re.findall(r"G\d+", repr(trees))) - {ry, rz}).pop()
    ren = {rx: "rx", ry: "ry", rz: "rz"}

    def rename(t):
        if not isinstance(t, tuple):
            return ren.get(t, t)
        t = tuple(rename(x) for x in t)
        if t and t[0] == "mul":
            return ("mul",) + tuple(sorted(t[1:], key=repr))
        if t and t[0] == "fma":
            pr, ad = tuple(sorted(t[2], key=repr)), t[4]
            if isinstance(ad, tuple) and ad and ad[0] == "mul" and (("0" in pr) != ("0" in ad[1:])):
                nz, z = ((ad[1:], t[3]), pr) if "0" in pr else ((pr, t[1]), ad[1:])
                return ("p+0z", nz, z)
            return ("fma", t[1], pr, t[3], ad)
        return t
    return [rename(t) for t in trees]


def main():
    name = sys.argv[3] if len(sys.argv) > 3 else C2
    a, b = entry_trees(sys.argv[1], name), entry_trees(sys.argv[2], name)
    bad = [e for e in range(36) if a[e] != b[e]]
    for e in bad:
        print(f"entry ({e // 6}, {e % 6})\n  A {a[e]}\n  B {b[e]}")
    print(f"{name}: {len(bad)} of 36 entries differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
