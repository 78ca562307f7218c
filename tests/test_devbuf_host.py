"""csrc/devbuf.h and csrc/scratch_layout.h on the host: tests/host/devbuf_check.cpp, a stand-alone program, built with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own (nothing is loaded into this interpreter, no GPU
is touched).  It drives the buffer type with malloc / free in place of the HIP calls -- the growth rules against the formulas the
call sites spelled out by hand, `grew`, an allocation that fails, moves -- and walks every carved scratch block at its smallest
sizes and at the documented limits: no two members overlap, each starts at its alignment, the total covers the parts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "devbuf_check.cpp")
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compilers():
    for name in ("clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "c++", "g++"):
        path = shutil.which(name)
        if path:
            yield path


def sanitizing_compiler(tmp):
    """The first compiler that builds AND runs a sanitised program (a compiler without its sanitizer runtimes does not count)."""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for cxx in compilers():
        exe = os.path.join(tmp, "probe")
        if subprocess.run([cxx, *FLAGS, probe, "-o", exe], capture_output=True).returncode == 0 and \
                subprocess.run([exe], capture_output=True).returncode == 0:
            return cxx
    return None


def test_devbuf_and_layouts_under_sanitizers(tmp_path):
    cxx = sanitizing_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no C++ compiler with the address and undefined-behaviour sanitizers")
    exe = str(tmp_path / "devbuf_check")
    subprocess.run([cxx, *FLAGS, SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "devbuf_check ok" in run.stdout, run.stdout + run.stderr
