"""Building and running the C++ host programs of tests/native: one g++ line for the product library, one for a library given by its
path (the emulator build of conftest.build_emu(), or the product library from a temporary directory), and one way to run a program and
check its exit status and its "OK ..." line."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
INCLUDE = os.path.join(ROOT, "include")
ROCM_LINK = ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"]
# a host of include/vmd_md_script_shim.h with the CPU mock of mdlib behind it: its flags, and the headers it is rebuilt for
SHIM_FLAGS = ["-std=c++17", "-Wall", "-I" + NATIVE]
SHIM_HEADERS = [os.path.join(INCLUDE, "vmd_md_script_shim.h")] + [os.path.join(NATIVE, h) for h in ("md_mock.h", "md_mock_eval.h", "shim_default_script_host.h")]


def source(name):
    return os.path.join(NATIVE, name + ".cpp")


def build_product(name, flags=("-std=c++17",), deps=()):
    """tests/native/<name>.cpp -> tests/native/<name>, -O2, linked against the product library (built first); left alone while it is
    newer than its source, the library and `deps`"""
    from viamd_amd import build
    lib = build.build()
    src, exe = source(name), os.path.join(NATIVE, name)
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in [src, lib, *deps]):
        return exe
    subprocess.check_call(["g++", *flags, "-O2", src, "-I" + INCLUDE, "-L" + os.path.join(ROOT, "viamd_amd"), "-lviamd_amd",
                           "-Wl,-rpath,$ORIGIN/../../viamd_amd", *ROCM_LINK, "-lpthread", "-o", exe])
    return exe


def build_against(lib_path, name, exe, flags=("-std=c++17",), opt="-O1", rocm=False):
    """tests/native/<name>.cpp -> `exe`, linked against the library at `lib_path` with an rpath to its directory"""
    subprocess.check_call(["g++", *flags, opt, source(name), "-I" + INCLUDE, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path),
                           *(ROCM_LINK if rocm else []), "-lpthread", "-o", str(exe)])
    return str(exe)


def build_shim(name, lib_path=None, exe=None, extra=()):
    """a shim host program (SHIM_FLAGS): against the product library, or against `lib_path` (the emulator build) into `exe`"""
    if lib_path is None:
        return build_product(name, SHIM_FLAGS, SHIM_HEADERS)
    return build_against(lib_path, name, exe, [*SHIM_FLAGS, *extra])


def run_ok(cmd, ok, timeout=600, env=None):
    """run a program: exit status 0 and a standard output that starts with `ok`; returns the CompletedProcess"""
    out = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith(ok), out.stdout
    return out
