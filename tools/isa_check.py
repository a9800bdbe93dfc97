"""ISA gate for librafthip's hot kernels (gfx950).

Compiles the translation units of librafthip (raft-teststuff_amd/csrc/rh_abi.hip,
rh_solve_fast.hip and rh_solve_split.hip, each with its own flags from __graft_entry__.UNITS) to device assembly and
checks every kernel:
  * no dynamic register indexing: `s_set_gpr_idx_*` or `v_movrel*` (a lane-dependent index into
    a register array, lowered with a scalar index, faulted k_qtf_hankel on the box in round 2;
    DESIGN.md §4) -> FAIL in any kernel;
  * no scratch traffic inside a streaming loop of any shipped kernel -- an innermost loop that issues
    buffer/global loads (the node loops of the solve kernels, the pair-tile loops of the QTF) --
    while one of its loads is outstanding (in_flight_scratch): a spill reload there shares
    `vmcnt` with the wave-table prefetch ring and drains it every node (k_solve_pair's first
    build lost 4x in phase A to exactly this) -> FAIL;
  * scratch instructions elsewhere (prologue, solve, member boundaries) are counted and reported;
  * the depth the prefetch rings really keep: per streaming loop, the loads issued per trip and
    min_outstanding, the smallest vmcnt(N) waited for with loads of the loop in flight (`rings=`);
    in the two benched fixed points the phase-A and phase-C node loops must keep
    (ring depth - 1) x loads per slot outstanding (`ringA=`, `ringC=`) -> FAIL below that; the joint
    phase-C loop of the C2 kernel (both bins of a thread per node step) has its own line, `ringCJ=`;
  * the compiler's VGPR and spilled-VGPR counts of every kernel (`vgpr=`, `spill=`), reported.
  * for the C2 kernel, the `s_waitcnt lgkmcnt` count of phase B (`phaseB_lgkm_waits=`): the section runs on
    one wave while seven wait, so its dependent LDS round trips are step time; reported (tests/test_isa_phase_b.py
    gates it), and its static FP64 instruction counts (`fp64_mul=`, `fp64_add=`, `fp64_fma=`), reported
    (tests/test_isa_lu_fma.py holds the first two against the counts before the LU's updates were fused).
Loops are found from the branch structure: a branch to a label that precedes it closes a loop
[label, branch]; a loop that contains no other loop is innermost; it streams if it holds a
buffer_load / global_load.

Usage: python tools/isa_check.py [--asm file.s] [--out report.txt]   (exit status 1 on FAIL)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402  (the build's translation units and their flags)
# Every kernel of the library is on some default dispatch path of rh_abi.hip (the opt-in
# kernels measured slower were removed), so every kernel is held to the streaming-loop rule.  The one exception is the
# general case solve k_solve_cases<NB>, the default for nw > 1024 or node tables beyond the LDS:
# a measured path whose current counts are a ratchet, so a change can only lower
# them.  No other kernel can get a ratchet: an entry here must name a k_solve_cases instantiation.
# (round 5: counted only while a load of the loop is in flight, in_flight_scratch; the ratchets
# fell from 6 / 14 / 14 / 21 to the counts below)
# Ratchets (measured counts; a kernel may only go down).  Round 6 re-measured them with the
# vector-memory counter modelled (vmcnt(N) waits, scratch reloads counted as loads):
# the general k_solve_cases<2> / <4> / <8> show 5 / 5 / 13 scratch accesses with loads in flight
# where the round-5 walk (reset only at vmcnt(0)) saw 0 / 0 / 8 -- the kernels did not change.
ALLOW = {"k_solve_cases<1>": 6, "k_solve_cases<2>": 5, "k_solve_cases<4>": 5, "k_solve_cases<8>": 13}
# the older measure beside it: scratch instructions anywhere inside a streaming loop,
# outstanding loads or not (a reload after a full drain still costs an L2 round trip).  The
# single-bin fast kernels (grids of <= 512 bins; C1-size designs, not the benched C2 / C4
# kernels, which have none) reload 14-20 values in their node loops, never with a load in flight.
ALLOW_LOOP = {"k_solve_cases<1>": 12, "k_solve_cases<2>": 14, "k_solve_cases<4>": 14, "k_solve_cases<8>": 22,
              "k_solve_lds<1, 128, true, 1>": 20, "k_solve_lds<1, 256, false, 1>": 14,
              "k_solve_lds<1, 512, false, 1>": 14}
assert all(k.startswith("k_solve_cases<") for k in ALLOW)
assert all(k.startswith(("k_solve_cases<", "k_solve_lds<1,")) for k in ALLOW_LOOP)
DYN_INDEX = re.compile(r"^\s*(s_set_gpr_idx\w*|v_movrel\w*)")
SCRATCH = re.compile(r"^\s*(scratch_|buffer_\w+.*\boff(en)?\b.*s\[0:3\])")
LABEL = re.compile(r"^(\.LBB\w+|\w+):")
BRANCH = re.compile(r"^\s*s_(cbranch_\w+|branch)\s+(\.LBB\w+)")
STREAM = re.compile(r"^\s*(buffer_load|global_load)")


def compile_asm(defines=(), csrc=None):
    """Device assembly of every translation unit (compiled in parallel), concatenated.  csrc: the source
    directory (default: this tree's; tools/asm_same.py passes that of another revision, which may lack a
    unit added since: that unit is left out)."""
    csrc = csrc or G.CSRC
    fd, path = tempfile.mkstemp(suffix=".s")
    os.close(fd)
    procs, parts = [], []
    for unit, flags in G.UNITS:
        if not os.path.exists(os.path.join(csrc, unit)):
            continue
        part = path + "." + unit + ".s"
        parts.append(part)
        procs.append(subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", *flags,
                                       *defines, "--offload-device-only", "-S", "-o", part, os.path.join(csrc, unit)],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    for p in procs:
        _, err = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(err.decode()[-3000:])
    with open(path, "w") as out:
        for part in parts:
            with open(part) as fh:
                out.write(fh.read())
            os.unlink(part)
    return path


def kernels(lines):
    """{mangled name: [instruction lines]} for every kernel body (up to its .Lfunc_end label)."""
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):   # the whole body: a kernel may end early in several places
                out[name] = body
                name = None
                continue
            body.append(ln)
    return out


def resources(lines):
    """{mangled name: (VGPRs, spilled VGPRs)} from the code objects' metadata notes (the compiler's own
    counts: .vgpr_count / .vgpr_spill_count of each kernel entry, which follow its .name)."""
    out, name = {}, None
    for ln in lines:
        m = re.match(r"^\s*(?:- )?\.(name|vgpr_count|vgpr_spill_count):\s+(\S+)", ln)
        if not m:
            continue
        if m.group(1) == "name":
            name = m.group(2)
        elif name is not None:
            v, sp = out.get(name, (None, None))
            out[name] = (int(m.group(2)), sp) if m.group(1) == "vgpr_count" else (v, int(m.group(2)))
    return out


VMCNT = re.compile(r"^\s*s_waitcnt\s+(?:.*\s)?vmcnt\((\d+)\)")
SCRATCH_LOAD = re.compile(r"^\s*(scratch_load|buffer_load\w*.*\boff(en)?\b.*s\[0:3\])")


def in_flight_scratch(body, a, b):
    """Scratch instructions of the loop [a, b] issued while one of its vector-memory loads is
    still outstanding: the hazard (a reload waits behind the ring's loads, since they share
    vmcnt, and drains it).  Walked in program order from the loop head with the vector-memory
    counter modelled: every load (wave-table stream and scratch reload alike) adds one, and
    `s_waitcnt vmcnt(N)` leaves at most N outstanding.  The loads still outstanding at the back
    edge (a prefetch ring carried into the next iteration) count as outstanding at the head.
    A scratch access once the counter is 0 -- e.g. around the LU of a bin, after its loads are
    consumed -- drains nothing.  (Straight-line walk: a branch inside the loop is followed as if
    both sides ran in order, which can only over-count.)"""
    def walk(carried):
        out, hits = carried, []
        for i in range(a, b + 1):
            ln = body[i]
            m = VMCNT.match(ln)
            if m:
                out = min(out, int(m.group(1)))
            elif SCRATCH.match(ln):
                if out > 0:
                    hits.append(i)
                if SCRATCH_LOAD.match(ln):
                    out += 1
            elif STREAM.match(ln):
                out += 1
        return out, hits
    carried, _ = walk(0)
    return walk(carried)[1]


def ring_depth(body, a, b):
    """(loads per trip, min_outstanding) of the streaming loop [a, b]: the vector-memory loads it issues in
    one trip, and the smallest N of any `s_waitcnt vmcnt(N)` reached inside it while loads are in flight
    (the counter modelled as in in_flight_scratch, with the back edge's loads carried to the head).  A
    prefetch ring D slots deep that really stays full never waits below (D - 1) x loads per slot; a loop
    that drains its ring somewhere shows 0.  None: the loop never waits with a load in flight."""
    def walk(carried):
        out, low = carried, None
        for i in range(a, b + 1):
            ln = body[i]
            m = VMCNT.match(ln)
            if m:
                n = int(m.group(1))
                if out > 0:
                    low = n if low is None else min(low, n)
                out = min(out, n)
            elif SCRATCH_LOAD.match(ln) or STREAM.match(ln):
                out += 1
        return out, low
    loads = sum(1 for i in range(a, b + 1) if STREAM.match(body[i]))
    carried, _ = walk(0)
    return loads, walk(carried)[1]


def ring_depths():
    """kRingA1 and kRingC as rh_solve.hip defines them."""
    with open(os.path.join(G.CSRC, "rh_solve.hip")) as fh:
        src = fh.read()
    return tuple(int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("RH_RING_A", "RH_RING_C"))


# The benched fixed points (C2, C4; two bins per thread), whose two main node loops are gated: the
# phase-A transverse ring (kRingA1 slots of 2 rows x 2 bins) and the phase-C node loop (kRingC slots
# of 2 rows, one bin per pass) must keep all slots but the one being consumed in flight at every wait.
RING_GATED = ("k_solve_lds<2, 512, false, 1>", "k_solve_lds<2, 128, true, 1>")


# The kernel whose phase C takes both bins of a thread in one node sweep (rh_solve.hip, kJointC): its
# kRingC slots hold one (node, bin) each, 2 rows, so a trip of kRingC / 2 nodes issues as many loads as
# a trip of the one-bin loop, and a wait for one slot leaves (kRingC - 1) x 2 outstanding (`ringCJ=`).
JOINT_C = ("k_solve_lds<2, 512, false, 1>",)


def joint_gate(rings):
    """(loads per trip, min_outstanding, needed) of the joint phase-C node loop."""
    _, rc = ring_depths()
    per_trip = (rc // 2) * 4
    hit = [m for l, m in rings if l == per_trip]
    return per_trip, None if not hit or None in hit else min(hit), (rc - 1) * 2


def ring_gate(rings):
    """[(name, loads, min_outstanding, needed)] of the two gated loops among a kernel's streaming loops,
    picked by their loads per trip (the short axial loops issue fewer)."""
    ra, rc = ring_depths()
    out = []
    for name, per_trip, per_slot, depth in (("A", ra * 4, 4, ra), ("C", rc * 2, 2, rc)):
        # (the compiler may emit a loop more than once: every copy counts, the worst one is reported)
        hit = [m for l, m in rings if l == per_trip]
        out.append((name, per_trip, None if not hit or None in hit else min(hit), (depth - 1) * per_slot))
    return out


BARRIER = re.compile(r"^\s*s_barrier\b")
LGKM_WAIT = re.compile(r"^\s*s_waitcnt\s.*lgkmcnt\(")
FIELD_LOAD = re.compile(r"^\s*global_load_dwordx2\b")


def phase_b_lgkm_waits(body):
    """`s_waitcnt lgkmcnt` instructions of phase B of a k_solve_lds body: every one is a point at which
    the one working wave may stand still for an LDS round trip (or a scalar load) while the others wait at
    the barrier.  Phase B is found from its shape: its node loop loads the node's 20-odd fields
    (global_load_dwordx2) between the barrier that closes phase A and the barrier before the node sum,
    the only stretch between two barriers with that many; the barrier after the next one closes phase B.
    None: no such stretch."""
    bars = [i for i, ln in enumerate(body) if BARRIER.match(ln)]
    best = None
    for k in range(len(bars) - 2):
        n = sum(1 for i in range(bars[k], bars[k + 1]) if FIELD_LOAD.match(body[i]))
        if n >= 16 and (best is None or n > best[0]):
            best = (n, k)
    if best is None:
        return None
    k = best[1]
    return sum(1 for i in range(bars[k], bars[k + 2]) if LGKM_WAIT.match(body[i]))


FP64_OP = re.compile(r"^\s*v_(mul|add|fma)c?_f64(_e32|_e64|_dpp)?\s")


def fp64_counts(body):
    """Static counts (mul, add, fma) of a body's `v_mul_f64`, `v_add_f64` and `v_fma_f64` / `v_fmac_f64`: an unfused complex
    multiply-subtract shows as 2 mul + 2 fma + 2 add where 4 fma do (tests/test_isa_lu_fma.py)."""
    n = {"mul": 0, "add": 0, "fma": 0}
    for ln in body:
        m = FP64_OP.match(ln)
        if m:
            n[m.group(1)] += 1
    return n["mul"], n["add"], n["fma"]


def analyse(body):
    labels = {}
    for i, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, ln in enumerate(body):
        m = BRANCH.match(ln)
        if m and m.group(2) in labels and labels[m.group(2)] <= i:
            loops.append((labels[m.group(2)], i))
    inner = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
    inner = [(a, b) for a, b in inner if any(STREAM.match(body[i]) for i in range(a, b + 1))]
    # for the ring measure a node loop counts even where it holds load-free loops of its own (the
    # member-boundary `while`s): every loop that issues loads and holds no other loop that does
    stream = sorted({l for l in loops if any(STREAM.match(body[i]) for i in range(l[0], l[1] + 1))})
    ring_loops = [l for l in stream if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in stream)]
    dyn = [ln.strip() for ln in body if DYN_INDEX.match(ln)]
    scr = [i for i, ln in enumerate(body) if SCRATCH.match(ln)]
    scr_inner = [i for a, b in inner for i in in_flight_scratch(body, a, b)]
    scr_loop = [i for a, b in inner for i in range(a, b + 1) if SCRATCH.match(body[i])]
    return {"dyn": dyn, "scratch": len(scr), "scratch_inner": len(scr_inner), "scratch_loop": len(scr_loop),
            "loops": len(loops), "inner": len(inner), "rings": [ring_depth(body, a, b) for a, b in ring_loops]}


def demangle(n):
    try:
        return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
    except OSError:
        return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--out")
    ap.add_argument("--no-ring-gate", action="store_true", help="report the ring depths without gating them")
    ap.add_argument("-D", action="append", default=[], help="extra preprocessor define (A/B variants)")
    args = ap.parse_args()
    path = args.asm or compile_asm(["-D" + d for d in args.D])
    with open(path) as fh:
        lines = fh.read().split("\n")
    ks, res = kernels(lines), resources(lines)
    rows, fails = [], []
    for name, body in sorted(ks.items()):
        r = analyse(body)
        dn = demangle(name)
        hot = True
        verdict = "ok"
        if r["dyn"]:
            verdict = "FAIL dynamic register indexing: " + "; ".join(sorted(set(r["dyn"])))
        elif hot and (r["scratch_inner"] or r["scratch_loop"]):
            allow = max([v for k, v in ALLOW.items() if k in dn] or [0])
            allow_loop = max([v for k, v in ALLOW_LOOP.items() if k in dn] or [0])
            if r["scratch_inner"] > allow:
                verdict = f"FAIL {r['scratch_inner']} scratch instructions inside streaming loops (allowed {allow})"
            elif r["scratch_loop"] > allow_loop:
                verdict = (f"FAIL {r['scratch_loop']} scratch instructions anywhere in streaming loops "
                           f"(allowed {allow_loop})")
            else:
                verdict = (f"ok (ratchet: {r['scratch_inner']} <= {allow} with loads in flight, {r['scratch_loop']} <= "
                           f"{allow_loop} anywhere in streaming loops, general path)")
        # every streaming loop in program order as loads per trip / min_outstanding ("-": never waits
        # with a load in flight)
        rings = " rings=" + ",".join(f"{l}/{'-' if m is None else m}" for l, m in r["rings"])
        if any(k in dn for k in RING_GATED):
            for ph, per_trip, low, need in ring_gate(r["rings"]):
                rings += f" ring{ph}={'?' if low is None else low}>={need}"
                if (low is None or low < need) and not args.no_ring_gate and not verdict.startswith("FAIL"):
                    verdict = (f"FAIL phase-{ph} ring ({per_trip} loads per trip): min_outstanding "
                               f"{'not found' if low is None else low} < {need}")
        if any(k in dn for k in JOINT_C):
            per_trip, low, need = joint_gate(r["rings"])
            rings += f" ringCJ={'?' if low is None else low}>={need}"
            if (low is None or low < need) and not args.no_ring_gate and not verdict.startswith("FAIL"):
                verdict = (f"FAIL joint phase-C ring ({per_trip} loads per trip): min_outstanding "
                           f"{'not found' if low is None else low} < {need}")
        vg, sp = res.get(name, (None, None))
        rings += f" vgpr={'?' if vg is None else vg} spill={'?' if sp is None else sp}"
        if any(k in dn for k in JOINT_C):
            nb = phase_b_lgkm_waits(body)
            rings += f" phaseB_lgkm_waits={'?' if nb is None else nb}"
            rings += " fp64_mul=%d fp64_add=%d fp64_fma=%d" % fp64_counts(body)
        if verdict.startswith("FAIL"):
            fails.append(dn)
        rows.append(f"{dn:70s} hot={int(hot)} loops={r['loops']:3d} inner={r['inner']:3d} "
                    f"scratch={r['scratch']:4d} in_flight={r['scratch_inner']:3d} in_loops={r['scratch_loop']:3d}  "
                    f"{verdict}{rings}")
    text = "# tools/isa_check.py: gfx950 device assembly of " + " + ".join(u for u, _ in G.UNITS) + "\n" + "\n".join(rows) + "\n"
    text += f"# {len(ks)} kernels, {len(fails)} failing\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    if not args.asm:
        os.unlink(path)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
