"""Welch PSD of REAL signals, timed on the device: ONE real frames plan (fft_gpu_plan_frames_real_hip, FFT_GPU_FRAMES_WELCH), which
reads the reals where they lie, against what a caller had to do before it existed -- widen the signal to complex on the device (a
copy into a complex buffer of twice the bytes), then the complex frames plan (fft_gpu_plan_frames_hip).  n = 1024, hop = 512, fp32,
about 1 GiB of real signal per execute (--signals x --len).

Both legs run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps` executes
between two device synchronisations, timed with the host clock; every shape is warmed up first.  Before anything is timed the
two results are compared.  Raw per-round times and their ranges go to profiles/rframes_vs_complex.txt (or --out).  No ratio is
asserted: the file records what was measured.

    python tools/rframes_time.py [--signals 256] [--len 1048576] [--rounds 12] [--reps 4] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fft-implementation-in-c_amd"))
import fftlib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--signals", type=int, default=256)
    ap.add_argument("--len", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rframes_vs_complex.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rframes_time: no GPU; nothing is measured without one")
    fftlib.init()
    n, hop, S, slen, fs = a.n, a.hop, a.signals, a.len, 48000.0
    nw = (slen - (n - hop)) // hop
    hb = n // 2 + 1
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((S, slen), generator=g, device=dev, dtype=torch.float32)
    xc = torch.zeros((S, slen), device=dev, dtype=torch.complex64)  # the widened copy a caller of the complex plan needs
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY

    welch = fftlib.ExtPlan.frames(n, hop, slen, S, "hann", "welch", np.float32)
    welch.set_stream(stream)
    cwelch = fftlib.ExtPlan.frames(n, hop, slen, S, "hann", "welch", np.complex64)
    cwelch.set_stream(stream)
    out_a = torch.empty((S, hb), device=dev, dtype=torch.float32)
    out_b = torch.empty((S, hb), device=dev, dtype=torch.float32)

    def leg_frames():
        welch.execute_frames(x.data_ptr(), out_a.data_ptr(), 0, fs)
        return out_a

    def leg_widen():
        xc.copy_(x)  # real -> complex: reads the signal, writes twice its bytes
        cwelch.execute_frames(xc.data_ptr(), out_b.data_ptr(), 0, fs)
        return out_b

    ra, rb = leg_frames().clone(), leg_widen().clone()
    torch.cuda.synchronize()
    rel = float((ra - rb).abs().max() / rb.abs().max())
    legs = {"real frames plan": leg_frames, "widen + complex frames plan": leg_widen}
    for f in legs.values():  # warm-up of every shape
        f(); f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.reps):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t) * 1e3 / a.reps)
    info = welch.info()
    cinfo = cwelch.info()
    lines = ["# tools/rframes_time.py: Welch PSD, n = %d, hop = %d, fp32, %d real signals x %d samples = %.3f GiB of signal per execute, %d frames"
             % (n, hop, S, slen, S * slen * 4 / 2.0 ** 30, S * nw),
             "# device: %s; real plan: passes %d, fused %d; complex plan: passes %d, fused %d; %d rounds x %d executes per leg, interleaved; host clock "
             "around a device synchronise" % (torch.cuda.get_device_name(0), info.n_passes, info.fused, cinfo.n_passes, cinfo.fused, a.rounds, a.reps),
             "# max |real plan - widened path| / max |widened path| = %.3g" % rel]
    for k, v in ms.items():
        lines.append("%-28s ms per execute: min %.3f median %.3f max %.3f | %s" % (k, min(v), float(np.median(v)), max(v), " ".join("%.3f" % t for t in v)))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lines.append("# real signal bytes / median time: real plan %.0f GB/s, widened path %.0f GB/s; median time widened / real = %.2f"
                 % (S * slen * 4 / (med["real frames plan"] * 1e6), S * slen * 4 / (med["widen + complex frames plan"] * 1e6),
                    med["widen + complex frames plan"] / med["real frames plan"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    welch.destroy()
    cwelch.destroy()


if __name__ == "__main__":
    main()
