"""Builds tests/cpp/raster_test.cpp against include/infur_processor.hpp + libinfur_hip.so (g++, no HIP headers needed: the
boundary is plain C) and runs it -- the C++ mirror of the Python Raster processor."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def raster_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_raster") / "raster_test")
    lib = os.path.join(ROOT, "infur_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "raster_test.cpp"), "-o", out,
                           "-L", lib, "-linfur_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_cpp_raster_cpu(raster_bin):
    r = subprocess.run([raster_bin, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cpu ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_raster_gpu(raster_bin):
    r = subprocess.run([raster_bin, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gpu ok" in r.stdout, r.stdout + r.stderr
