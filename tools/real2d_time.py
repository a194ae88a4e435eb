"""Real 2D transform timed on the device: ONE rfft2 plan (fft_gpu_plan_r2c_2d_hip) against what a caller had to do before it existed,
fp32, forward, 128 real images of 1024 x 1024:
  (plan)      the plan's own path (two launches on half-size data where info().fused says so)
  (no_fusion) the same plan with FFT_GPU_OPT_NO_FUSION: the 1D real plan on the rows, transpose, batched 1D plan, transpose
  (caller)    a torch widening copy of the real images to complex, a complex 2D plan (fft_gpu_plan_2d_ex_hip), and a contiguous slice to
              cols/2 + 1 columns -- all three inside the timed region.

All legs run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps` executes between two
device synchronisations, timed with the host clock; every leg is warmed up first, and before anything is timed every leg's output is compared
with the plan's.  Raw per-round times, their medians and ranges go to profiles/real2d_vs_plan2d.txt (or --out).  No ratio is asserted: the
file records what was measured.

    python tools/real2d_time.py [--rounds 8] [--reps 5] [--images 128] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fft-implementation-in-c_amd"))
import fftlib  # noqa: E402


def measure(M, rows, cols, rounds, reps, lines):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((M, rows, cols), generator=g, device=dev, dtype=torch.float32)
    hb = cols // 2 + 1
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY
    legs, plans, notes = {}, [], []

    def real_leg(name, no_fusion):
        p = fftlib.ExtPlan.real2d(rows, cols, M, False, np.float32)
        if no_fusion:
            p.set_option(fftlib.OPT_NO_FUSION, 1)
        p.set_stream(stream)
        plans.append(p)
        y = torch.empty((M, rows, hb), device=dev, dtype=torch.complex64)
        notes.append("%s: fused %d, n_passes %d" % (name, p.info().fused, p.info().n_passes))
        legs[name] = (lambda: (p.execute_real2d(x.data_ptr(), y.data_ptr(), 0, 0), y)[1])

    real_leg("(plan) rfft2 plan", False)
    real_leg("(no_fusion) rfft2 plan, NO_FUSION", True)
    full = fftlib.ExtPlan.fft2d(rows, cols, M, fftlib.FFT_FORWARD, np.complex64)
    full.set_stream(stream)
    plans.append(full)
    wide = torch.empty((M, rows, cols), device=dev, dtype=torch.complex64)
    yc = torch.empty((M, rows, hb), device=dev, dtype=torch.complex64)

    def caller():
        wide.copy_(x)                                              # the widening copy, twice the bytes
        full.execute_ptr(wide.data_ptr(), wide.data_ptr())
        yc.copy_(wide[:, :, :hb])                                  # the one-sided half, contiguous
        return yc
    legs["(caller) widen + complex 2D plan + slice"] = caller

    first = next(iter(legs))
    ref = legs[first]().clone()
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    for name, f in legs.items():  # every output checked before it is timed; this is the warm-up too
        out = f()
        torch.cuda.synchronize()
        rel = float((out - ref).abs().max()) / scale
        notes.append("%s: max |out - (plan)| / max = %.3g" % (name, rel))
        if not rel < 1e-4:
            raise SystemExit("real2d_time: %s disagrees with %s (%g)" % (name, first, rel))
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, f in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t) * 1e3 / reps)
    lines.append("## %d real images of %d x %d, forward, fp32: %.3f GiB of real input per execute" % (M, rows, cols, M * rows * cols * 4 / 2.0 ** 30))
    lines += ["# " + s for s in notes]
    for name, v in ms.items():
        lines.append("%-44s ms per execute: min %.3f median %.3f max %.3f | %s" % (name, min(v), float(np.median(v)), max(v), " ".join("%.3f" % t for t in v)))
    for p in plans:
        p.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "real2d_vs_plan2d.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("real2d_time: no GPU; nothing is measured without one")
    fftlib.init()
    lines = ["# tools/real2d_time.py: the rfft2 plan against its own fallback and against widen + complex 2D plan + slice",
             "# device: %s; %d rounds x %d executes per leg, legs interleaved; host clock around a device synchronise" % (torch.cuda.get_device_name(0), a.rounds, a.reps)]
    measure(a.images, 1024, 1024, a.rounds, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
