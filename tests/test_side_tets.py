"""The brick and cell routines of csrc/tomo_side_tets.h (the tables, the vertex rule, the staging of a brick under both borders, both
element types and both access widths, the lane walk, count, scan and emit), run on the host: tests/side_tets.cpp is compiled for the
host alone with the address and undefined-behaviour sanitizers and run against a brute force.  No device, nothing loaded into this
process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"        # as csrc/side.mk


def test_the_tetrahedra_on_the_host(tmp_path):
    exe = str(tmp_path / "side_tets")
    include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    build = subprocess.run([HIPCC, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-std=c++17", "-Wall", "-g",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "side_tets.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(build.stdout)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
