"""Time the turbine output channels of N wind cases on VolturnUS-S_aero with aeroServoMod 2 (wind
speed U(4, 24) m/s, heading U(-30, 30) deg, seeded: the workload of rotor_time.py and aero_mb_time.py),
in one run:
  (a) the yardstick, per case: the host forming FOWT.calcTurbineConstants(case, bem=pair) and
      FOWT._aero_outputs on that case's Xi, which is what a caller of analyzeCasesBatch had to do to get
      these channels from a batch result (on the large grids over a seeded sample of the cases);
  (b) FOWT.turbineChannelsBatch whole: the V_w table on the host (Rotor.IECKaimal once per distinct
      speed), the uploads, one rh_turbine_channels launch, the max / min forms; wall clock around a
      synchronize;
  (c) of (b), the host forming the pair tables and the V_w table alone;
  (d) the rh_turbine_channels launch alone on tables already on the device, HIP events, and its achieved
      bandwidth against its Xi reads (surge and pitch: 32 bytes per case, row and bin) plus its PSD stores
      (40 bytes per case, rotor and bin).
Xi is a seeded response of physical size (the timing does not depend on its values).  On the design's
own grid and on grids of other bin counts (default: 1000).  Warm-up calls first; medians over the
repeats, with the range.
usage: channels_time.py [N] [out.txt] [nw ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "raft-teststuff_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(n, out_path=None, grids=(None, 1000)):
    import torch
    import raft
    from raft import _native as N
    from raft.rotor_device import chan_geom_table
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

    for nw in grids:
        d = load_design("VolturnUS-S_aero")
        d["turbine"]["aeroServoMod"] = 2
        if nw is not None:
            d.setdefault("settings", {}).update(min_freq=0.2 / nw, max_freq=0.2)
        m = raft.Model(d)
        fowt = m.fowtList[0]
        fowt.calcStatics()
        fowt.calcHydroConstants()
        say(f"--- VolturnUS-S_aero, aeroServoMod 2, {n} wind cases, nw = {m.nw}" +
            (" (the design's own grid)" if nw is None else ""))
        Xh = rng.normal(size=[n, 1, 6, m.nw]) + 1j * rng.normal(size=[n, 1, 6, m.nw])
        Xh[:, :, 3:] *= 0.01
        fowt.calcTurbineConstants(dict(cases[0], wind_speed=0.0), ptfm_pitch=0)      # the aero-free design
        dd = fowt.device_design()
        Xi = torch.tensor(Xh, dtype=torch.complex128, device=dd.device)
        mb = fowt.aeroMBBatch([dict(c) for c in cases], dd, m.device)

        # (b) turbineChannelsBatch whole
        def whole():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fowt.turbineChannelsBatch(cases, Xi, mb, m.device)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        whole(), whole()
        tb = [whole()[0] for _ in range(10)]
        say(f"(b) turbineChannelsBatch whole:                      {stats(tb, 'ms', 1e3)}")

        # (c) its host part alone
        tc = []
        for _ in range(10):
            t0 = time.perf_counter()
            pairs, vw, wind_row = fowt._channel_pair_tables(cases, mb)
            geom = chan_geom_table(fowt)
            tc.append(time.perf_counter() - t0)
        say(f"(c) of (b), the host forming the pair tables and {vw.shape[0] - 1} V_w rows: {stats(tc, 'ms', 1e3)}")

        # (d) the launch alone
        f64 = dict(dtype=torch.float64, device=dd.device)
        i32 = dict(dtype=torch.int32, device=dd.device)
        host = [np.ascontiguousarray(pairs[k], dtype=np.int32) for k in ("pair_case", "pair_rotor", "modes", "pair_vw")]
        pcd, prd, pvd = (torch.tensor(host[k], **i32) for k in (0, 1, 3))
        prow, Vd, gd = (torch.tensor(np.ascontiguousarray(a, dtype=float), **f64) for a in (pairs["pair_row"], vw, geom))
        p0 = torch.zeros([n], **f64)
        nrot = geom.shape[0]
        psd = torch.empty([n, nrot, N.TC_SPECTRA, m.nw], **f64)
        std, avg = torch.empty([n, nrot, N.TC_SPECTRA], **f64), torch.empty([n, nrot, N.TC_COUNT], **f64)
        ctx, s = N.context(m.device), N.stream_handle(torch, dd.device)
        nbytes = n * m.nw * (32 + 40 * nrot)
        ev = []
        for r in range(25):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            N.check(N.lib().rh_turbine_channels(ctx, n, 1, m.nw, float(fowt.dw), N.ptr(dd.w), N.ptr(Xi), N.ptr(p0), nrot,
                                                N.ptr(gd), len(host[0]), N.ptr(pcd), host[0].ctypes.data, N.ptr(prd),
                                                host[1].ctypes.data, host[2].ctypes.data, N.ptr(mb["loads"]),
                                                N.ptr(mb["dloads"]), N.ptr(mb["param"]), N.ptr(mb["op"]), N.ptr(prow),
                                                N.ptr(pvd), host[3].ctypes.data, int(Vd.shape[0]), N.ptr(Vd), N.ptr(psd),
                                                N.ptr(std), N.ptr(avg), s), "rh_turbine_channels")
            b.record()
            b.synchronize()
            if r >= 5:
                ev.append(a.elapsed_time(b))
        say(f"(d) the rh_turbine_channels launch, HIP events: {stats(ev, 'us', 1e3)}; "
            f"{nbytes / 1e6:.1f} MB read and stored, {nbytes / (np.median(ev) * 1e-3) / 1e12:.3f} TB/s")

        # (a) the yardstick: the host per case
        bems = fowt.rotorLoadsBatch([dict(c) for c in cases], m.device)
        sample = range(n) if m.nw <= 200 else sorted(rng.choice(n, size=min(n, 48), replace=False).tolist())
        fowt.Xi0 = np.zeros(6)
        ta = []
        for rep in range(2):                  # the first pass warms up
            ta = []
            for i in sample:
                t0 = time.perf_counter()
                fowt.calcTurbineConstants(dict(cases[i]), ptfm_pitch=0, bem=bems[i])
                fowt.Xi = np.concatenate([Xh[i], np.zeros([1, 6, m.nw])])
                res = {f"{k}_{st}": np.zeros(nrot) for k in ("Mbase", "omega", "torque", "bPitch")
                       for st in ("avg", "std", "max", "min")}
                res.update({f"{k}_PSD": np.zeros([m.nw, nrot]) for k in ("Mbase", "omega", "torque", "bPitch")})
                res["power_avg"] = np.zeros(nrot)
                fowt._aero_outputs(res, cases[i])
                ta.append(time.perf_counter() - t0)
        say(f"(a) the host per case (yardstick), {len(ta)} cases:     {stats(ta, 'ms', 1e3)}; "
            f"for {n} cases {np.median(ta) * n * 1e3:.0f} ms, {np.median(ta) * n / np.median(tb):.0f}x (b)")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512, sys.argv[2] if len(sys.argv) > 2 else None,
         tuple([None] + [int(x) for x in sys.argv[3:]]) if len(sys.argv) > 3 else (None, 1000))
