"""Welch PSD on overlapping frames, timed on the device: ONE frames plan (fft_gpu_plan_frames_hip, FFT_GPU_FRAMES_WELCH) against
what a caller had to do before it existed -- a torch `unfold` copy of the signal to [frames][n], a FFT_GPU_FUSED_PSD plan over
those rows, a torch mean over the frames.  n = 1024, hop = 512, fp32, about 1 GiB of signal per execute (--signals x --len).

Both legs run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps` executes
between two device synchronisations, timed with the host clock; every shape is warmed up first.  Before anything is timed the
two results are compared.  Raw per-round times and their ranges go to profiles/frames_vs_unfold.txt (or --out).  No ratio is
asserted: the file records what was measured.

    python tools/frames_time.py [--signals 128] [--len 1048576] [--rounds 12] [--reps 4] [--out FILE]
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
    ap.add_argument("--signals", type=int, default=128)
    ap.add_argument("--len", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_vs_unfold.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("frames_time: no GPU; nothing is measured without one")
    fftlib.init()
    n, hop, S, slen, fs = a.n, a.hop, a.signals, a.len, 48000.0
    nw = (slen - (n - hop)) // hop
    hb = n // 2 + 1
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn((S, slen, 2), generator=g, device=dev, dtype=torch.float32))
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY

    welch = fftlib.ExtPlan.frames(n, hop, slen, S, "hann", "welch", np.complex64)
    welch.set_stream(stream)
    psd = fftlib.ExtPlan.fused("psd", n, S * nw, None, np.complex64)
    psd.set_stream(stream)
    out_a = torch.empty((S, hb), device=dev, dtype=torch.float32)
    rows = torch.empty((S * nw, hb), device=dev, dtype=torch.float32)

    def leg_frames():
        welch.execute_frames(x.data_ptr(), out_a.data_ptr(), 0, fs)
        return out_a

    def leg_unfold():
        fr = x.unfold(1, n, hop).contiguous()  # [S][nw][n]: the copy the frames plan does not make
        psd.execute_fused(fr.data_ptr(), None, rows.data_ptr(), fs)
        return rows.view(S, nw, hb).mean(dim=1)

    ra, rb = leg_frames().clone(), leg_unfold().clone()
    torch.cuda.synchronize()
    rel = float((ra - rb).abs().max() / rb.abs().max())
    legs = {"frames plan": leg_frames, "unfold + FUSED_PSD + mean": leg_unfold}
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
    lines = ["# tools/frames_time.py: Welch PSD, n = %d, hop = %d, fp32, %d signals x %d samples = %.3f GiB of signal per execute, %d frames"
             % (n, hop, S, slen, S * slen * 8 / 2.0 ** 30, S * nw),
             "# device: %s; frames plan: passes %d, fused %d; %d rounds x %d executes per leg, interleaved; host clock around a device synchronise"
             % (torch.cuda.get_device_name(0), info.n_passes, info.fused, a.rounds, a.reps),
             "# max |frames plan - three-step path| / max |three-step path| = %.3g" % rel]
    for k, v in ms.items():
        lines.append("%-28s ms per execute: min %.3f median %.3f max %.3f | %s" % (k, min(v), float(np.median(v)), max(v), " ".join("%.3f" % t for t in v)))
    lines.append("# signal bytes / median time: frames plan %.0f GB/s, three-step path %.0f GB/s (the signal is read once; the three-step path also "
                 "writes and reads the [frames][n] copy and the spectrum)" % tuple(S * slen * 8 / (np.median(ms[k]) * 1e6) for k in ms))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    welch.destroy()
    psd.destroy()


if __name__ == "__main__":
    main()
