"""Overlap-save FIR filtering timed on the device: ONE filter plan (fft_gpu_plan_filter_hip) against what a caller had to do before it
existed, fp32, 255 taps, two shapes (256 signals x 2^20 samples = 2 GiB of signal per execute, one signal x 2^27 samples = 1 GiB), block
lengths n in {512, 1024, 2048, 4096}:
  (a) FFT_GPU_FUSED_CONV_LINEAR on the whole signals, where such a plan can be built;
  (b) a torch `unfold` copy of the signals to [blocks][n], a FFT_GPU_FUSED_CONV_CIRCULAR plan over those rows, a torch
      slice-and-copy of the valid parts into the output.  The zeros in front of and behind every signal that the blocks need are put
      there ONCE, outside the timed region (a caller is taken to keep its signals padded): the leg times unfold, plan and slice only.

All legs of a shape run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps`
executes between two device synchronisations, timed with the host clock; every leg is warmed up first, and before anything is timed
every leg's output is compared with the filter plan's.  Raw per-round times, their medians and ranges go to
profiles/filter_vs_fused_conv.txt (or --out).  No ratio is asserted: the file records what was measured.

    python tools/filter_time.py [--rounds 8] [--reps 3] [--taps 255] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fft-implementation-in-c_amd"))
import fftlib  # noqa: E402

BLOCKS = (512, 1024, 2048, 4096)


def measure(S, slen, M, rounds, reps, lines):
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn((S, slen, 2), generator=g, device=dev, dtype=torch.float32))
    rng = np.random.default_rng(2)
    h = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY
    ol = slen + M - 1
    lead = M - 1
    y = torch.empty((S, ol), device=dev, dtype=torch.complex64)
    legs, plans, notes = {}, [], []

    for n in BLOCKS:
        p = fftlib.ExtPlan.filter(h, slen, S, "full", n, np.complex64)
        p.set_stream(stream)
        plans.append(p)
        notes.append("filter n = %d: fused %d, %d blocks" % (n, p.info().fused, p.info().batch))
        legs["filter plan n=%d" % n] = (lambda p=p: (p.execute_filter(x.data_ptr(), y.data_ptr(), 0, 0), y)[1])
    try:
        lin = fftlib.ExtPlan.fused("conv", slen, S, h, np.complex64)
        lin.set_stream(stream)
        plans.append(lin)
        ya = torch.empty((S, ol), device=dev, dtype=torch.complex64)
        legs["(a) FUSED_CONV_LINEAR"] = (lambda: (lin.execute_fused(x.data_ptr(), None, ya.data_ptr()), ya)[1])
        notes.append("(a): passes %d, fused %d" % (lin.info().n_passes, lin.info().fused))
    except RuntimeError:
        notes.append("(a): no FFT_GPU_FUSED_CONV_LINEAR plan for this shape")
    for n in BLOCKS:
        B = n - lead
        nb = (ol + B - 1) // B
        hp = np.zeros(n, dtype=np.complex64)
        hp[:M] = h
        circ = fftlib.ExtPlan.fused("circ", n, S * nb, hp, np.complex64)
        circ.set_stream(stream)
        plans.append(circ)
        rows = torch.empty((S, nb, n), device=dev, dtype=torch.complex64)
        yb = torch.empty((S, ol), device=dev, dtype=torch.complex64)

        xp = F.pad(x, (lead, (nb - 1) * B + n - lead - slen))               # zeros in front of and behind every signal: not timed

        def leg_b(n=n, B=B, nb=nb, circ=circ, rows=rows, yb=yb, xp=xp):
            fr = xp.unfold(1, n, B).contiguous()                             # [S][nb][n]: the copy the filter plan does not make
            circ.execute_fused(fr.data_ptr(), None, rows.data_ptr())
            yb.copy_(rows[:, :, lead:].reshape(S, nb * B)[:, :ol])           # the slicing copy it does not make either
            return yb
        legs["(b) unfold + CIRCULAR + slice n=%d" % n] = leg_b

    first = next(iter(legs))
    ref = legs[first]().clone()
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    for k, f in legs.items():  # every output checked before it is timed; this is the warm-up too
        out = f()
        torch.cuda.synchronize()
        rel = float((out - ref).abs().max()) / scale
        notes.append("%s: max |out - %s| / max = %.3g" % (k, first, rel))
        if not rel < 1e-4:
            raise SystemExit("filter_time: %s disagrees with %s (%g)" % (k, first, rel))
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t) * 1e3 / reps)
    lines.append("## %d signal(s) x %d samples = %.3f GiB of signal per execute, %d taps, fp32" % (S, slen, S * slen * 8 / 2.0 ** 30, M))
    lines += ["# " + s for s in notes]
    for k, v in ms.items():
        lines.append("%-38s ms per execute: min %.3f median %.3f max %.3f | %s" % (k, min(v), float(np.median(v)), max(v), " ".join("%.3f" % t for t in v)))
    for p in plans:
        p.destroy()
    del x, y
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taps", type=int, default=255)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="256x1048576,1x134217728")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_vs_fused_conv.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filter_time: no GPU; nothing is measured without one")
    fftlib.init()
    lines = ["# tools/filter_time.py: overlap-save filter plan against (a) FFT_GPU_FUSED_CONV_LINEAR on whole signals and (b) unfold + FFT_GPU_FUSED_CONV_CIRCULAR + slice",
             "# device: %s; %d rounds x %d executes per leg, legs interleaved; host clock around a device synchronise" % (torch.cuda.get_device_name(0), a.rounds, a.reps)]
    for shape in a.shapes.split(","):
        S, slen = (int(v) for v in shape.split("x"))
        measure(S, slen, a.taps, a.rounds, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
