"""DCT-II timed on the device: ONE DCT plan (fft_gpu_plan_dct_hip), N = 1024, fp32, about 1 GiB of reals per execute, against what a
caller had to do before it existed:
  (plan)      the plan's own path (one launch where info().fused says so)
  (no_fusion) the same plan with FFT_GPU_OPT_NO_FUSION: permute kernel, length-N complex plan, twiddle kernel
  (caller)    a torch permute copy (even samples, then the odd ones backwards), fftlib's r2c plan, and a torch twiddle multiply taking
              the real part -- all three inside the timed region
  (copy)      a device copy of the same bytes: the yardstick
and one line for dctn on 128 images of 1024 x 1024.

All legs run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps` executes between two
device synchronisations, timed with the host clock; every leg is warmed up first, and before anything is timed every leg's output is compared
with the plan's.  Raw per-round times, their medians and ranges go to profiles/dct_vs_rfft.txt (or --out).  No ratio is asserted: the file
records what was measured.

    python tools/dct_time.py [--rounds 8] [--reps 5] [--rows 262144] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fft-implementation-in-c_amd"))
import fftlib  # noqa: E402


def timed(legs, rounds, reps):
    import torch
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, f in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t) * 1e3 / reps)
    return ms


def report(ms, lines):
    for name, v in ms.items():
        lines.append("%-46s ms per execute: min %.3f median %.3f max %.3f | %s" % (name, min(v), float(np.median(v)), max(v), " ".join("%.3f" % t for t in v)))


def measure_rows(B, N, rounds, reps, lines):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((B, N), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY
    legs, plans, notes = {}, [], []

    def dct_leg(name, no_fusion):
        p = fftlib.ExtPlan.dct(N, B, fftlib.DCT2, fftlib.DCT_NORM_NONE, np.float32)
        if no_fusion:
            p.set_option(fftlib.OPT_NO_FUSION, 1)
        p.set_stream(stream)
        plans.append(p)
        y = torch.empty((B, N), device=dev, dtype=torch.float32)
        notes.append("%s: fused %d, n_passes %d" % (name, p.info().fused, p.info().n_passes))
        legs[name] = (lambda: (p.execute_dct(x.data_ptr(), y.data_ptr(), 0, 0), y)[1])

    dct_leg("(plan) DCT-II plan", False)
    dct_leg("(no_fusion) DCT-II plan, NO_FUSION", True)
    r2c = fftlib.ExtPlan.r2c(N, B, np.float32)
    r2c.set_stream(stream)
    plans.append(r2c)
    hb = N // 2 + 1
    v = torch.empty((B, N), device=dev, dtype=torch.float32)
    V = torch.empty((B, hb), device=dev, dtype=torch.complex64)
    yc = torch.empty((B, N), device=dev, dtype=torch.float32)
    k = torch.arange(hb, device=dev, dtype=torch.float64)
    q = (2.0 * torch.exp(-1j * np.pi * k / (2.0 * N))).to(torch.complex64)

    def caller():
        v[:, :N // 2] = x[:, 0::2]                                  # the permute copy
        v[:, N // 2:] = torch.flip(x[:, 1::2], dims=(1,))
        r2c.execute_ptr(v.data_ptr(), V.data_ptr())
        c = V * q                                                   # the quarter-sample twiddle
        yc[:, :hb] = c.real
        yc[:, hb:] = -torch.flip(c.imag[:, 1:N // 2], dims=(1,))
        return yc
    legs["(caller) permute copy + rfft plan + twiddle"] = caller
    z = torch.empty_like(x)
    legs["(copy) device copy of the same bytes"] = lambda: z.copy_(x)

    first = next(iter(legs))
    ref = legs[first]().clone()
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    for name, f in legs.items():  # every output checked before it is timed; this is the warm-up too
        out = f()
        torch.cuda.synchronize()
        if not name.startswith("(copy)"):
            rel = float((out - ref).abs().max()) / scale
            notes.append("%s: max |out - (plan)| / max = %.3g" % (name, rel))
            if not rel < 1e-4:
                raise SystemExit("dct_time: %s disagrees with %s (%g)" % (name, first, rel))
        f()
    torch.cuda.synchronize()
    ms = timed(legs, rounds, reps)
    lines.append("## DCT-II, %d rows of N = %d, fp32: %.3f GiB of reals per execute" % (B, N, B * N * 4 / 2.0 ** 30))
    lines += ["# " + s for s in notes]
    report(ms, lines)
    for p in plans:
        p.destroy()


def measure_images(M, rows, cols, rounds, reps, lines):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn((M, rows, cols), generator=g, device=dev, dtype=torch.float32)
    y = torch.empty_like(x)
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY
    p = fftlib.ExtPlan.dct2d(rows, cols, M, fftlib.DCT2, fftlib.DCT_NORM_NONE, np.float32)
    p.set_stream(stream)
    legs = {"(dctn) 2D DCT-II plan": lambda: p.execute_dct(x.data_ptr(), y.data_ptr(), 0, 0)}
    legs["(dctn) 2D DCT-II plan"]()  # the warm-up
    torch.cuda.synchronize()
    ms = timed(legs, rounds, reps)
    lines.append("## dctn, %d images of %d x %d, fp32 (fused %d): %.3f GiB of reals per execute" % (M, rows, cols, p.info().fused, M * rows * cols * 4 / 2.0 ** 30))
    report(ms, lines)
    p.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dct_vs_rfft.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dct_time: no GPU; nothing is measured without one")
    fftlib.init()
    lines = ["# tools/dct_time.py: the DCT-II plan against its own fallback, against permute + rfft plan + twiddle in torch, and against a copy",
             "# device: %s; %d rounds x %d executes per leg, legs interleaved; host clock around a device synchronise" % (torch.cuda.get_device_name(0), a.rounds, a.reps)]
    measure_rows(a.rows, 1024, a.rounds, a.reps, lines)
    measure_images(128, 1024, 1024, a.rounds, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
