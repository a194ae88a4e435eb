"""2D convolution timed on the device: ONE conv2d plan (fft_gpu_plan_conv2d_hip, SAME) against what a caller had to do before it existed,
fp32, 512 x 512 images convolved with a 31 x 31 kernel (P = Q = 1024; 128 images = 1 GiB of padded work image per execute):
  (plan)      the plan's own path (the column round where info().fused says so)
  (no_fusion) the same plan with FFT_GPU_OPT_NO_FUSION: pad kernel, 2D plan, product kernel, 2D plan, crop kernel
  (caller)    a zero-padded copy made with torch, a forward 2D plan (fft_gpu_plan_2d), a torch multiply by the same H, an inverse 2D
              plan, and a torch crop-and-copy into the output -- all five inside the timed region.

All legs run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps` executes between two
device synchronisations, timed with the host clock; every leg is warmed up first, and before anything is timed every leg's output is compared
with the plan's.  Raw per-round times, their medians and ranges go to profiles/conv2d_vs_plan2d.txt (or --out).  No ratio is asserted: the
file records what was measured.

    python tools/conv2d_time.py [--rounds 8] [--reps 5] [--images 128] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fft-implementation-in-c_amd"))
import fftlib  # noqa: E402


def measure(M, rows, cols, kr, kc, rounds, reps, lines):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn((M, rows, cols, 2), generator=g, device=dev, dtype=torch.float32))
    rng = np.random.default_rng(2)
    k = (rng.standard_normal((kr, kc)) + 1j * rng.standard_normal((kr, kc))).astype(np.complex64)
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY
    legs, plans, notes = {}, [], []

    def conv_leg(name, no_fusion):
        p = fftlib.ExtPlan.conv2d(k, rows, cols, M, "same", np.complex64)
        if no_fusion:
            p.set_option(fftlib.OPT_NO_FUSION, 1)
        p.set_stream(stream)
        plans.append(p)
        y = torch.empty((M, rows, cols), device=dev, dtype=torch.complex64)
        notes.append("%s: fused %d, %d round trips, P x Q = %d x %d" % (name, p.info().fused, p.info().n_passes, p.padded[0], p.padded[1]))
        legs[name] = (lambda: (p.execute_conv2d(x.data_ptr(), y.data_ptr(), 0, 0), y)[1])
        return p

    p0 = conv_leg("(plan) conv2d plan", False)
    conv_leg("(no_fusion) conv2d plan, NO_FUSION", True)
    P, Q = p0.padded
    # the caller's own H: the kernel placed in [P][Q], shifted by SAME's offset, transformed once by the forward plan (not timed)
    fwd = fftlib.ExtPlan.fft2d(P, Q, M, fftlib.FFT_FORWARD, np.complex64)
    inv = fftlib.ExtPlan.fft2d(P, Q, M, fftlib.FFT_INVERSE, np.complex64)
    one = fftlib.ExtPlan.fft2d(P, Q, 1, fftlib.FFT_FORWARD, np.complex64)
    for p in (fwd, inv, one):
        p.set_stream(stream)
        plans.append(p)
    hp = np.zeros((P, Q), dtype=np.complex64)
    for i in range(kr):
        for j in range(kc):
            hp[(i - (kr - 1) // 2) % P, (j - (kc - 1) // 2) % Q] = k[i, j]
    H = torch.from_numpy(hp).to(dev)
    one.execute_ptr(H.data_ptr(), H.data_ptr())
    torch.cuda.synchronize()
    yc = torch.empty((M, rows, cols), device=dev, dtype=torch.complex64)
    spec = torch.empty((M, P, Q), device=dev, dtype=torch.complex64)

    def caller():
        w = torch.zeros((M, P, Q), device=dev, dtype=torch.complex64)   # the padded copy
        w[:, :rows, :cols] = x
        fwd.execute_ptr(w.data_ptr(), spec.data_ptr())
        spec.mul_(H)                                                     # the product, a round trip of its own
        inv.execute_ptr(spec.data_ptr(), spec.data_ptr())
        yc.copy_(spec[:, :rows, :cols])                                  # the crop
        return yc
    legs["(caller) pad + 2D plan + torch mul + 2D plan + crop"] = caller

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
            raise SystemExit("conv2d_time: %s disagrees with %s (%g)" % (name, first, rel))
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
    lines.append("## %d images of %d x %d, kernel %d x %d, SAME, fp32: %.3f GiB of padded work image per execute" % (M, rows, cols, kr, kc, M * P * Q * 8 / 2.0 ** 30))
    lines += ["# " + s for s in notes]
    for name, v in ms.items():
        lines.append("%-52s ms per execute: min %.3f median %.3f max %.3f | %s" % (name, min(v), float(np.median(v)), max(v), " ".join("%.3f" % t for t in v)))
    for p in plans:
        p.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2d_vs_plan2d.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conv2d_time: no GPU; nothing is measured without one")
    fftlib.init()
    lines = ["# tools/conv2d_time.py: the conv2d plan against its own fallback and against pad + 2D plan + torch multiply + 2D plan + crop",
             "# device: %s; %d rounds x %d executes per leg, legs interleaved; host clock around a device synchronise" % (torch.cuda.get_device_name(0), a.rounds, a.reps)]
    measure(a.images, 512, 512, 31, 31, a.rounds, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
