"""Build tests/device_units/units.hip twice (TEST INFRASTRUCTURE ONLY): as host C++ against the CPU emulator, which compiles the
plain C++ twins of the building blocks, and with hipcc for gfx950 under the product's flags, which compiles the bodies that ship.
Outputs: tests/device_units/_build/libdevice_units_emu.so and libdevice_units_gfx950.so, rebuilt when the source or a header it
includes is newer."""
import fcntl
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "ddsp_svc_amd", "csrc")
SRC = os.path.join(HERE, "units.hip")
OUT = os.path.join(HERE, "_build")
LIB_EMU = os.path.join(OUT, "libdevice_units_emu.so")
LIB_GPU = os.path.join(OUT, "libdevice_units_gfx950.so")
HEADERS = [os.path.join(CSRC, h) for h in ("fft_1024p.h", "fft_r.h", "fft2048.h", "ddsp_common.h")]   # what units.hip includes


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _locked(target, deps, force, make):
    """one builder at a time (pytest-xdist workers arrive together after a source change): the others wait, then find it fresh"""
    if not force and not _stale(target, deps):
        return target
    os.makedirs(OUT, exist_ok=True)
    with open(target + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if force or _stale(target, deps):
            make()
    return target


def build_emu(force=False):
    from tests.hipemu import build as emu
    emu.build()                                              # the emulator runtime (hipemu.o) lives in the product's emulator build
    runtime = os.path.join(emu.OUT, "hipemu.o")
    deps = [SRC, *HEADERS, os.path.join(emu.HERE, "hip", "hip_runtime.h"), os.path.join(emu.HERE, "hipemu.cpp")]

    def make():
        obj = os.path.join(OUT, "units_emu.o")
        subprocess.run([emu._clang(), "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-I", emu.HERE, "-I", CSRC,
                        "-Wno-unknown-attributes", "-Wno-unused-function", "-c", SRC, "-o", obj], check=True)
        subprocess.run([emu._clang(), "-shared", "-fPIC", obj, runtime, "-o", LIB_EMU], check=True)
    return _locked(LIB_EMU, deps, force, make)


def gpu_stale():
    return _stale(LIB_GPU, [SRC, *HEADERS])


def build_gpu(force=False):
    from ddsp_svc_amd import build as product

    def make():
        subprocess.run([product._hipcc(), *product.FLAGS, "-I", CSRC, "-shared", SRC, "-o", LIB_GPU], check=True)
    return _locked(LIB_GPU, [SRC, *HEADERS], force, make)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    print(build_emu(force=True))
    print(build_gpu(force=True))
