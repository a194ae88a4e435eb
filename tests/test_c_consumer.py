"""A compiled-C consumer of the drop-in boundary: tests/c_consumer/gpu_demo_consumer.c restates the call sequence of
the reference's GPU harness (examples/demo_v2_features.c:50-229) and is built with plain `gcc -std=c99` against
include/*.h and libfft_mi355x.so -- no ctypes in between.  Compile + link run on the CPU box; the binary itself
(which checks every spectrum it computes) runs under -m gpu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fft-implementation-in-c_amd")
SRC = os.path.join(ROOT, "tests", "c_consumer", "gpu_demo_consumer.c")
BUILD = os.path.join(ROOT, "tests", "c_consumer", "build")
EXE = os.path.join(BUILD, "gpu_demo_consumer")


def _build():
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE,
           "-L" + PKG, "-lfft_mi355x", "-lm", "-Wl,-rpath," + PKG, "-Wl,-rpath-link,/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return EXE


def test_c_consumer_compiles_and_links_against_the_public_headers():
    exe = _build()
    syms = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    for name in ("fft_plan_dft_1d", "fft_execute", "fft_execute_dft", "fft_destroy_plan", "fft_auto", "fft_alloc_complex",
                 "fft_free", "fft_gpu_available", "fft_gpu_init", "fft_gpu_get_device_name", "fft_gpu_get_memory_info",
                 "fft_gpu_alloc", "fft_gpu_plan_1d", "fft_gpu_execute", "fft_gpu_copy_h2d", "fft_gpu_copy_d2h",
                 "fft_gpu_cleanup", "fft_get_hardware_capabilities", "fft_version"):
        assert (" U " + name) in syms, name + " is not taken from the library"


def test_c_consumer_fails_loudly_without_a_device():
    """No GPU in the build container: the program must report failures (NULL plans, -1), not crash or pretend."""
    # asked of the library the program links (torch imported after it has initialised HIP sees no device)
    import fftlib
    if fftlib.load().fft_gpu_available():
        pytest.skip("a GPU is present")
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "FAILED" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_c_consumer_runs_on_the_gpu():
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "c-consumer: OK" in out.stdout, out.stdout + out.stderr
