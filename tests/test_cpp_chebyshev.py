"""The adapter knows the word Chebyshev and reads chebyshevDegree, chebyshevEigRatio and chebyshevLambdaMax from the
preconditioner sub-dictionary (tests/cpp/test_chebyshev_keyword.cpp over ogl_amd/host/OGLAdapter.H and the MiniFoam
stand-in): built here with g++ against libogl_amd.so, run on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_adapter_hands_the_keywords_on(tmp_path):
    exe = tmp_path / "test_chebyshev_keyword"
    lib = os.path.join(ROOT, "ogl_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
           "-I", os.path.join(ROOT, "ogl_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_chebyshev_keyword.cpp"),
           "-L", lib, "-logl_amd", f"-Wl,-rpath,{lib}", "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 failure(s)" in r.stdout
