"""cmusphinx_amd/csrc/s3a_hostmem.h without a GPU: tests/hostmem_check.cc -- the owner of an engine's allocations and its growing
buffers over counting stand-ins for the four HIP allocation functions, one scripted life with no failure and with a failure at every
allocation in turn -- built with the address and undefined-behaviour sanitizers and run as a program of its own.  It exits 0 only when
every life ends with nothing live and nothing freed twice, a failed reserve leaves its buffer empty (S3A_ENOMEM), a reserve that
fits keeps its pointers, an owner that goes out of scope frees what it still holds, a buffer taken out of its owner (forget) stays
live for the caller, and hipHostMalloc's flags arrive."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hostmem_header_under_sanitizers(tmp_path):
    exe = tmp_path / "hostmem_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cmusphinx_amd", "csrc"),
                    "-o", str(exe), os.path.join(ROOT, "tests", "hostmem_check.cc")], check=True)
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "hostmem_check: ok" in p.stdout
