"""3D complex transform timed on the device: ONE 3D plan (fft_gpu_plan_3d_hip) against its own composition, against what a caller had to do
before it existed, and against a copy of the same bytes; fp32, forward, about 1 GiB per execute (64 volumes of 128^3 where the plane kernel
takes 128 x 128 planes, otherwise 512 volumes of 64^3):
  (a) fused     the plan's own path: plane_fft_kernel on the planes, the depth pass in place
  (b) no_fusion the same plan with FFT_GPU_OPT_NO_FUSION: the 2D plan on the planes, the same depth pass
  (c) caller    the 2D plan (fft_gpu_plan_2d_ex_hip) on the planes, a torch permute copy that brings depth last, a batched 1D plan, and the
                permute copy back -- all inside the timed region
  (d) copy      a device copy of the same bytes (torch copy_)

All legs run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps` executes between two
device synchronisations, timed with the host clock; every leg is warmed up first, and before anything is timed the outputs of (b) and (c)
are compared with (a)'s.  Raw per-round times, their medians and ranges go to profiles/fft3d_vs_composition.txt (or --out).  No ratio is
asserted: the file records what was measured.

--sizes adds further cubes at the same 1 GiB per execute (e.g. --sizes 128,64,32): the numbers behind the plan's rule for which planes take
the fused path.

    python tools/fft3d_time.py [--rounds 8] [--reps 5] [--sizes N,N,...] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fft-implementation-in-c_amd"))
import fftlib  # noqa: E402


def measure(nv, n, rounds, reps, lines):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn((nv, n, n, n, 2), generator=g, device=dev, dtype=torch.float32))
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY
    legs, plans, notes = {}, [], []

    def plan_leg(name, no_fusion):
        p = fftlib.ExtPlan.plan3d(n, n, n, nv, fftlib.FFT_FORWARD, np.complex64)
        if no_fusion:
            p.set_option(fftlib.OPT_NO_FUSION, 1)
        p.set_stream(stream)
        plans.append(p)
        y = torch.empty_like(x)
        notes.append("%s: fused %d, n_passes %d" % (name, p.info().fused, p.info().n_passes))
        legs[name] = (lambda: (p.execute_ptr(x.data_ptr(), y.data_ptr()), y)[1])

    plan_leg("(a) 3D plan", False)
    plan_leg("(b) 3D plan, NO_FUSION", True)
    p2 = fftlib.ExtPlan.fft2d(n, n, nv * n, fftlib.FFT_FORWARD, np.complex64)
    p1 = fftlib.Plan(n, nv * n * n, fftlib.FFT_FORWARD, np.complex64)
    for p in (p2, p1):
        p.set_stream(stream)
        plans.append(p)
    w = torch.empty_like(x)
    t = torch.empty((nv, n, n, n), device=dev, dtype=torch.complex64)  # [v][r][c][d]
    yc = torch.empty_like(x)

    def caller():
        p2.execute_ptr(x.data_ptr(), w.data_ptr())
        t.copy_(w.permute(0, 2, 3, 1))          # depth last, contiguous
        p1.execute_ptr(t.data_ptr(), t.data_ptr())
        yc.copy_(t.permute(0, 3, 1, 2))         # and back
        return yc
    legs["(c) caller: fft2d + permute + 1D + permute"] = caller
    cp = torch.empty_like(x)
    legs["(d) device copy of the same bytes"] = lambda: cp.copy_(x)

    ref = legs["(a) 3D plan"]().clone()
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    for name, f in legs.items():  # every transform's output checked before it is timed; this is the warm-up too
        out = f()
        torch.cuda.synchronize()
        if not name.startswith("(d)"):
            rel = float((out - ref).abs().max()) / scale
            notes.append("%s: max |out - (a)| / max = %.3g" % (name, rel))
            if not rel < 1e-4:
                raise SystemExit("fft3d_time: %s disagrees with (a) (%g)" % (name, rel))
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / reps)
    lines.append("## %d volumes of %d^3, forward, fp32: %.3f GiB per execute" % (nv, n, nv * n ** 3 * 8 / 2.0 ** 30))
    lines += ["# " + s for s in notes]
    for name, v in ms.items():
        lines.append("%-46s ms per execute: min %.3f median %.3f max %.3f | %s" % (name, min(v), float(np.median(v)), max(v), " ".join("%.3f" % q for q in v)))
    for p in plans:
        p.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="", help="cube edges, comma separated; default: 128 where the plane kernel takes 128 x 128, else 64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fft3d_vs_composition.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fft3d_time: no GPU; nothing is measured without one")
    fftlib.init()
    probe = fftlib.ExtPlan.plan3d(2, 128, 128, 1, fftlib.FFT_FORWARD, np.complex64)
    big = probe.info().fused == 1
    probe.destroy()
    lines = ["# tools/fft3d_time.py: the 3D plan against its own composition, the caller's fft2d / permute / 1D / permute, and a copy",
             "# device: %s; %d rounds x %d executes per leg, legs interleaved; host clock around a device synchronise" % (torch.cuda.get_device_name(0), a.rounds, a.reps)]
    sizes = [int(v) for v in a.sizes.split(",") if v] or [128 if big else 64]
    for n in sizes:
        measure((1 << 27) // n ** 3, n, a.rounds, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
