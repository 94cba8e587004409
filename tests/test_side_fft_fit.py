"""The batch rule of csrc/tomo_side_fft.h (fit_batch: the first batch, the one lowering, the tail plan, the remembered decision) and its
plan cache's stopwatch, driven by a fake plan source: tests/side_fft_fit.cpp is compiled for the host alone with the address and
undefined-behaviour sanitizers and run.  No device, no hipFFT call, nothing loaded into this process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"        # as csrc/side.mk


def test_the_batch_rule_with_a_fake_plan_source(tmp_path):
    exe = str(tmp_path / "side_fft_fit")
    include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    build = subprocess.run([HIPCC, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-std=c++17", "-Wall", "-g",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "side_fft_fit.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(build.stdout)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
