"""The stand-alone check programs of libx3dstep's host code (tests/*_check.cpp): one way to build and run them, shared by
the host suites of the step library."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compiler():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    return cxx


def run(tmp_path, name, cases):
    """tests/<name>.cpp and csrc_step/step_host.cpp compiled with -fsanitize=address,undefined into a program of their own
    and run as a child process on the case file `cases`; nothing sanitised is loaded into this interpreter.  Gives the words
    of the program's last line and its whole output."""
    exe = str(tmp_path / name)
    cmd = [compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", name + ".cpp"),
           os.path.join(ROOT, "x3d-multigrid_amd", "csrc_step", "step_host.cpp"), "-o", exe]
    # the sanitisers' runtimes linked into the program itself where the compiler ships them so (gcc needs to be told)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip().splitlines()[-1].split(), r.stdout
