"""CPU suite: the arithmetic the two sides of a reconciliation session share (qcrypto-ldpc_amd/csrc/qldpc_recon_core.h: CRC-32 serial and chunked,
the puncture map in both directions, the staging layouts), as the kernels and the host code of qldpc_recon.hip compile it.  No GPU compute."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_under_asan_ubsan(tmp_path):
    """the chunked CRC against the serial one and a known answer, position(rank(j)) == j over every (M, p) of the listed ranges, and the staging views
    tiling their blocks, as a stand-alone program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "recon_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "recon_sanitize.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
