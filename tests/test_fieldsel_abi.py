"""The field-selection layer, CPU side: the host part of csrc/bflbm_fieldsel.h (the refusals of the variable and pair
arguments, the selection a batch and a context observe by, the pair table) through a stand-alone host program built with
the address and undefined-behaviour sanitizers and run as a program.  What it checks is listed at the top of
tests/fieldsel_main.cpp; the expected values there are written out by hand."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")


def test_selections_and_refusals_of_the_host_layer(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "fieldsel_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "fieldsel_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 93  # the checks fieldsel_main.cpp makes: a check that silently stops running fails here
