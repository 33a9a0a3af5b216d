"""Runs tests/cpp/test_gradients (the gradient members of the C++ drop-in class bdd_hip_parallel_mma<REAL>) on the GPU."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_cpp_gradient_members():
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_gradients")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-1000:])
    assert r.returncode == 0 and "0 failure(s)" in r.stdout, r.stdout[-3000:]
