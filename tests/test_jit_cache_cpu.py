"""The check a cached code object passes before the module loader sees it (csrc/elf_extent.hpp, used by csrc/jit_cache.hip):
hipModuleLoadData takes a pointer and no length, so a truncated file under the cache's final name must be told from a whole one by
the image's own headers.  A host program (tests/c/elf_extent_check.cpp, plain g++) runs the checker on a code object that hiprtc
returned for gfx950 (tests/golden/hiprtc_trivial_kernel_gfx950.elf: `extern "C" __global__ void k(float* x) { x[0] = 1.f; }`, -O3)
and on its own executable: whole images are accepted -- a false refusal would recompile on every process start --, every shorter
length, offsets and sizes past the end and a foreign magic are refused.  The GPU side is
tests/test_user_model_gpu.py::test_corrupt_jit_cache_file_is_rebuilt."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesianfiltering_amd", "csrc")


def test_whole_images_pass_and_damaged_ones_do_not(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path / "elf_extent_check"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "c", "elf_extent_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    obj = os.path.join(ROOT, "tests", "golden", "hiprtc_trivial_kernel_gfx950.elf")
    assert open(obj, "rb").read(4) == b"\x7fELF"
    r = subprocess.run([str(exe), obj], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "total unexpected: 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count("unexpected answers 0") == 2


def test_the_cache_checks_before_it_loads():
    src = open(os.path.join(CSRC, "jit_cache.hip")).read()
    assert "elf_image_is_whole(code.data(), code.size()) ? load() : hipErrorInvalidImage" in src
    hdr = open(os.path.join(CSRC, "elf_extent.hpp")).read()
    assert "hip" not in hdr.split("#pragma once")[1].lower()          # builds without the HIP runtime
