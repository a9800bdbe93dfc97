"""Time the per-case preparation of Model.analyzeCasesBatch for N wind cases on VolturnUS-S_aero (wind
speed U(4, 24) m/s, heading U(-30, 30) deg, seeded: the workload of rotor_time.py), in one run:
  (a) rotor_device=True, the yardstick: one rotor launch, then per case FOWT.calcTurbineConstants with
      bem=, prep.linear_matrices and two uploads of [nw, 6, 6];
  (b) aero_device=True: FOWT.aeroMBBatch (the operating points on the host, the rotor launch, one
      rh_rotor_aero_mb launch, the status read back) and a CaseMB view per case;
both from the call of analyzeCasesBatch to the moment it would launch the solve, the device idle
(the solve is replaced by a stop, after a synchronize);
  (c) inside (b), the host forming the pairs' operating points and parameter rows alone;
  (d) the rh_rotor_aero_mb launch alone on tables already on the device, HIP events, and its achieved
      store bandwidth against the bytes it writes (2 x 288 bytes per case and bin).
On the design's own grid and on grids of other bin counts (default: 1000, where 512 cases store
295 MB).  Warm-up calls first; medians over the repeats, with the range.
usage: aero_mb_time.py [N] [out.txt] [nw ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "raft-teststuff_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


class _Stop(Exception):
    pass


def main(n, out_path=None, grids=(None, 1000)):
    import torch
    import raft
    import raft.model as RM
    from raft import _native as N
    from conftest import load_design
    rng = np.random.default_rng(512)
    base = {"turbulence": 0.1, "turbine_status": "operating", "yaw_misalign": 0, "wave_spectrum": "JONSWAP",
            "wave_period": 10, "wave_height": 4, "wave_heading": 0, "current_speed": 0, "current_heading": 0}
    cases = [dict(base, wind_speed=float(u), wind_heading=float(h))
             for u, h in zip(rng.uniform(4, 24, n), rng.uniform(-30, 30, n))]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def stats(x, unit, scale):
        x = np.asarray(x) * scale
        return f"median {np.median(x):.3f} {unit} (min {x.min():.3f}, max {x.max():.3f}, {len(x)} samples)"

    stamp = {}

    def stop(*a, **k):
        torch.cuda.synchronize()
        stamp["t"] = time.perf_counter()
        raise _Stop()

    def prep_time(model, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            model.analyzeCasesBatch([dict(c) for c in cases], **kw)
        except _Stop:
            return stamp["t"] - t0
        raise RuntimeError("the solve was not reached")

    real_solve = RM.solve_batch_2nd
    for nw in grids:
        d = load_design("VolturnUS-S_aero")
        if nw is not None:
            d.setdefault("settings", {}).update(min_freq=0.2 / nw, max_freq=0.2)
        m = raft.Model(d)
        fowt = m.fowtList[0]
        say(f"--- VolturnUS-S_aero, {n} wind cases, nw = {m.nw}" + (" (the design's own grid)" if nw is None else ""))
        RM.solve_batch_2nd = stop
        try:
            reps = 5 if m.nw <= 200 else 3
            prep_time(m, rotor_device=True)                                   # warm-up: code objects, allocator
            ta = [prep_time(m, rotor_device=True) for _ in range(reps)]
            prep_time(m, aero_device=True)
            prep_time(m, aero_device=True)
            tb = [prep_time(m, aero_device=True) for _ in range(max(reps, 10))]
        finally:
            RM.solve_batch_2nd = real_solve
        say(f"(a) preparation with rotor_device=True (yardstick): {stats(ta, 'ms', 1e3)}")
        say(f"(b) preparation with aero_device=True:              {stats(tb, 'ms', 1e3)}")
        say(f"    ratio (a) / (b), medians: {np.median(ta) / np.median(tb):.1f}x")

        # (c) the host part of (b) alone: the pairs, their operating points and parameter rows
        from raft.rotor_device import aero_param_row
        pairs, rotors = fowt._rotor_pairs(cases)
        tc = []
        for _ in range(10):
            t0 = time.perf_counter()
            param = np.zeros([len(pairs), N.AP_COUNT])

            def row(k, rot, speed):
                param[k] = aero_param_row(rot, speed, 1)
            fowt._rotor_pairs(cases)
            op, idx = fowt._rotor_operating_points(pairs, rotors, cases, each=row)
            tc.append(time.perf_counter() - t0)
        say(f"(c) of (b), the host forming {len(pairs)} operating points and parameter rows: {stats(tc, 'ms', 1e3)}")

        # (d) the launch alone
        dr = fowt._device_rotor(rotors, m.device)
        dd = fowt.device_design()
        res = dr.launch(idx, op, derivatives=True)
        pc = np.arange(len(pairs), dtype=np.int32)
        f64 = dict(dtype=torch.float64, device=dr.device)
        pcd = torch.tensor(pc, dtype=torch.int32, device=dr.device)
        M, B = torch.empty([n, m.nw, 6, 6], **f64), torch.empty([n, m.nw, 6, 6], **f64)
        f0 = torch.empty([n, 6], **f64)
        ctx, s = N.context(m.device), N.stream_handle(torch, dr.device)
        nbytes = 2 * n * m.nw * 288
        for mode in (1, 2):
            param[:, N.AP["MODE"]] = mode
            md = np.full(len(pairs), mode, dtype=np.int32)
            pard = torch.tensor(param, **f64)
            ev = []
            for r in range(25):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                N.check(N.lib().rh_rotor_aero_mb(ctx, n, len(pairs), m.nw, N.ptr(dd.w), N.ptr(pcd), pc.ctypes.data,
                                                 md.ctypes.data, N.ptr(res["loads"]), N.ptr(res["dloads"]), N.ptr(pard),
                                                 N.ptr(dd.M), N.ptr(dd.B), int(dd.per_bin), N.ptr(M), N.ptr(B), N.ptr(f0),
                                                 s), "rh_rotor_aero_mb")
                b.record()
                b.synchronize()
                if r >= 5:
                    ev.append(a.elapsed_time(b))
            say(f"(d) the rh_rotor_aero_mb launch, HIP events, aeroServoMod {mode}: {stats(ev, 'us', 1e3)}; "
                f"{nbytes / 1e6:.1f} MB stored, {nbytes / (np.median(ev) * 1e-3) / 1e12:.2f} TB/s")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512, sys.argv[2] if len(sys.argv) > 2 else None,
         tuple([None] + [int(x) for x in sys.argv[3:]]) if len(sys.argv) > 3 else (None, 1000))
