"""Magnitude-squared coherence of REAL signal pairs, timed on the device: ONE cross frames plan (fft_gpu_plan_cross_frames_real_hip,
FFT_GPU_CROSS_COHERENCE) against what a caller had to do before it existed -- two real frames plans in STFT mode, then the conjugate
product, the means over the frames and the division in torch (in the rows' precision).  n = 1024, hop = 512, fp32, about 1 GiB of
real signal per execute (x and y together), at two shapes: many pairs (--signals x --len) and ONE long pair of the same size.

Both legs run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps` executes
between two device synchronisations, timed with the host clock; every shape is warmed up first.  Before anything is timed the
two results are compared.  Raw per-round times and their ranges go to profiles/cross_vs_torch.txt (or --out).  No ratio is
asserted: the file records what was measured.

    python tools/cross_time.py [--signals 128] [--len 1048576] [--rounds 12] [--reps 2] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fft-implementation-in-c_amd"))
import fftlib  # noqa: E402


def shape_lines(torch, n, hop, S, slen, rounds, reps):
    nw = (slen - (n - hop)) // hop
    hb = n // 2 + 1
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((S, slen), generator=g, device=dev, dtype=torch.float32)
    y = 0.8 * x + 0.5 * torch.randn((S, slen), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY
    cross = fftlib.ExtPlan.cross_frames(n, hop, slen, S, "hann", "coherence", np.float32)
    cross.set_stream(stream)
    stft = [fftlib.ExtPlan.frames(n, hop, slen, S, "hann", "stft", np.float32) for _ in range(2)]
    for p in stft:
        p.set_stream(stream)
    out_a = torch.empty((S, hb), device=dev, dtype=torch.float32)
    X = torch.empty((S, nw, hb), device=dev, dtype=torch.complex64)
    Y = torch.empty((S, nw, hb), device=dev, dtype=torch.complex64)

    def leg_plan():
        cross.execute_cross(x.data_ptr(), y.data_ptr(), out_a.data_ptr(), 0, 0, 1.0)
        return out_a

    def leg_torch():
        stft[0].execute_frames(x.data_ptr(), X.data_ptr(), 0, 1.0)
        stft[1].execute_frames(y.data_ptr(), Y.data_ptr(), 0, 1.0)
        pxy = (X.conj() * Y).mean(dim=1)
        pxx = (X.real * X.real + X.imag * X.imag).mean(dim=1)
        pyy = (Y.real * Y.real + Y.imag * Y.imag).mean(dim=1)
        return (pxy.real * pxy.real + pxy.imag * pxy.imag) / (pxx * pyy)

    ra, rb = leg_plan().clone(), leg_torch().clone()
    torch.cuda.synchronize()
    diff = float((ra - rb).abs().max())
    legs = {"cross frames plan": leg_plan, "2 stft plans + torch": leg_torch}
    for f in legs.values():  # warm-up of every shape
        f(); f()
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
    info = cross.info()
    lines = ["# coherence, n = %d, hop = %d, fp32, %d pairs x %d samples = %.3f GiB of real signal per execute (x and y), %d frames per side; "
             "chunk length C = %d frames, %d chunks per pair; inner plan: passes %d, fused %d"
             % (n, hop, S, slen, 2 * S * slen * 4 / 2.0 ** 30, S * nw, cross.chunk, -(-nw // cross.chunk), info.n_passes, info.fused),
             "# max |plan - torch path| = %.3g (coherence, fp32)" % diff]
    for k, v in ms.items():
        lines.append("%-22s ms per execute: min %.3f median %.3f max %.3f | %s" % (k, min(v), float(np.median(v)), max(v), " ".join("%.3f" % t for t in v)))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lines.append("# median time torch path / plan = %.2f" % (med["2 stft plans + torch"] / med["cross frames plan"]))
    cross.destroy()
    for p in stft:
        p.destroy()
    del x, y, X, Y
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--signals", type=int, default=128)
    ap.add_argument("--len", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_vs_torch.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cross_time: no GPU; nothing is measured without one")
    fftlib.init()
    lines = ["# tools/cross_time.py on %s; %d rounds x %d executes per leg, interleaved; host clock around a device synchronise"
             % (torch.cuda.get_device_name(0), a.rounds, a.reps)]
    for S, slen in ((a.signals, a.len), (1, a.signals * a.len)):  # many pairs; ONE long pair of the same size
        lines += shape_lines(torch, a.n, a.hop, S, slen, a.rounds, a.reps)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
