"""The z-group decomposition of csrc/tomo_side_zgroups.h (which groups a grid visits, what the group loads and stores touch, the region
test), walked on the host: tests/side_zgroups.cpp is compiled for the host alone with the address and undefined-behaviour sanitizers
and run.  No device, nothing loaded into this process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"        # as csrc/side.mk


def test_a_grid_walk_on_the_host(tmp_path):
    exe = str(tmp_path / "side_zgroups")
    include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    build = subprocess.run([HIPCC, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-std=c++17", "-Wall", "-g",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "side_zgroups.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(build.stdout)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
