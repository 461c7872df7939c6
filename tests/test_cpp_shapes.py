"""Builds tests/cpp/shapes_test.cpp against include/infur_processor.hpp + libinfur_hip.so (g++, no HIP headers needed: the
boundary is plain C) and runs it -- the C++ mirror of the Python Shapes processor."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shapes_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp_shapes") / "shapes_test")
    lib = os.path.join(ROOT, "infur_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shapes_test.cpp"), "-o", out,
                           "-L", lib, "-linfur_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_cpp_shapes_cpu(shapes_bin):
    r = subprocess.run([shapes_bin, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cpu ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_shapes_gpu(shapes_bin):
    r = subprocess.run([shapes_bin, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gpu ok" in r.stdout, r.stdout + r.stderr
