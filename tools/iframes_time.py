"""Inverse STFT of real signals, timed on the device: ONE inverse frames plan (fft_gpu_plan_iframes_real_hip), the same plan under
FFT_GPU_OPT_NO_FUSION (merge kernel + plain half-length inverse instead of the Hermitian rows load), and what a caller had to do
before the plan existed -- a c2r plan over all frames, a torch multiply by the window, a torch overlap-add (fold, on the transposed
frames) and a division by the envelope.  n = 1024, hop = 512, fp32, about 1 GiB of output signal per execute (--signals x --frames).

The three legs run in one process on one device, interleaved round by round, on torch's current stream; a round is `--reps` executes
between two device synchronisations, timed with the host clock; every shape is warmed up first.  Before anything is timed the
results are compared.  Raw per-round times and their ranges go to profiles/iframes_vs_c2r_fold.txt (or --out).  No ratio is asserted:
the file records what was measured.

    python tools/iframes_time.py [--signals 256] [--frames 2047] [--rounds 12] [--reps 3] [--out FILE]
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
    ap.add_argument("--frames", type=int, default=2047)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iframes_vs_c2r_fold.txt"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("iframes_time: no GPU; nothing is measured without one")
    fftlib.init()
    n, hop, S, nw = a.n, a.hop, a.signals, a.frames
    hb = n // 2 + 1
    out_len = (nw - 1) * hop + n
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.view_as_complex(torch.randn((S, nw, hb, 2), generator=g, device=dev, dtype=torch.float32))
    stream = torch.cuda.current_stream(dev).cuda_stream or fftlib.HIP_STREAM_LEGACY

    plan = fftlib.ExtPlan.iframes(n, hop, nw, S, "hamming", np.float32)
    plan.set_stream(stream)
    unfused = fftlib.ExtPlan.iframes(n, hop, nw, S, "hamming", np.float32)
    unfused.set_stream(stream)
    unfused.set_option(fftlib.OPT_NO_FUSION, 1)
    c2r = fftlib.ExtPlan.c2r(n, S * nw, np.float32)
    c2r.set_stream(stream)
    i = torch.arange(n, device=dev, dtype=torch.float64)
    win = (0.54 - 0.46 * torch.cos(2.0 * np.pi * i / (n - 1))).to(torch.float32)
    env = F.fold((win * win).reshape(1, n, 1).expand(1, n, nw).contiguous(), (1, out_len), (1, n), stride=(1, hop)).reshape(out_len)
    ya = torch.empty((S, out_len), device=dev, dtype=torch.float32)
    yb = torch.empty((S, out_len), device=dev, dtype=torch.float32)
    v = torch.empty((S, nw, n), device=dev, dtype=torch.float32)

    def leg_plan():
        plan.execute_iframes(X.data_ptr(), ya.data_ptr(), 0)
        return ya

    def leg_unfused():
        unfused.execute_iframes(X.data_ptr(), yb.data_ptr(), 0)
        return yb

    def leg_caller():
        c2r.execute_ptr(X.data_ptr(), v.data_ptr())
        v.mul_(win)
        y = F.fold(v.transpose(1, 2), (1, out_len), (1, n), stride=(1, hop)).reshape(S, out_len)
        return y.div_(env)

    ra, rb = leg_plan().clone(), leg_unfused().clone()
    torch.cuda.synchronize()
    rel_b = float((ra - rb).abs().max() / ra.abs().max())
    legs = {"inverse frames plan": leg_plan, "the plan, no fusion": leg_unfused, "c2r + window + fold + divide": leg_caller}
    try:
        rc = leg_caller().clone()
        torch.cuda.synchronize()
        rel_c = float((ra - rc).abs().max() / ra.abs().max())
        del rc
    except RuntimeError as e:  # torch cannot run the caller's path at this shape: the other two legs are still timed
        if "HIP error" in str(e) or "illegal" in str(e):  # a device fault is no such thing: nothing more runs
            raise
        print("iframes_time: the caller's path failed (%s); it is left out" % str(e).splitlines()[0])
        rel_c = float("nan")
        del legs["c2r + window + fold + divide"]
    del ra, rb
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
    info, uinfo = plan.info(), unfused.info()
    lines = ["# tools/iframes_time.py: inverse STFT, n = %d, hop = %d, Hamming, fp32, %d signals x %d frames -> %d samples each = %.3f GiB of signal "
             "per execute (%.3f GiB of one-sided rows in)" % (n, hop, S, nw, out_len, S * out_len * 4 / 2.0 ** 30, S * nw * hb * 8 / 2.0 ** 30),
             "# device: %s; plan: passes %d, fused %d; no fusion: passes %d, fused %d; %d rounds x %d executes per leg, interleaved; host clock "
             "around a device synchronise" % (torch.cuda.get_device_name(0), info.n_passes, info.fused, uinfo.n_passes, uinfo.fused, a.rounds, a.reps),
             "# max |plan - other| / max |plan|: no fusion %.3g, caller's path %.3g" % (rel_b, rel_c)]
    for k, t in ms.items():
        lines.append("%-30s ms per execute: min %.3f median %.3f max %.3f | %s" % (k, min(t), float(np.median(t)), max(t), " ".join("%.3f" % q for q in t)))
    med = {k: float(np.median(t)) for k, t in ms.items()}
    lines.append("# median time: no fusion / plan = %.2f, caller's path / plan = %.2f" %
                 (med["the plan, no fusion"] / med["inverse frames plan"],
                  med.get("c2r + window + fold + divide", float("nan")) / med["inverse frames plan"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    for p in (plan, unfused, c2r):
        p.destroy()


if __name__ == "__main__":
    main()
