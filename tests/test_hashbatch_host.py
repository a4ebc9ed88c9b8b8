"""CPU suite: what the batch contexts of the two privacy-amplification hashes share on the host (qcrypto-ldpc_amd/csrc/qldpc_hashbatch_core.h: the
limits of a context, the argument checks of a call, the row layout packed and a stride apart, the tail mask), as qldpc_privamp_batch.hip and
qldpc_toeplitz.hip compile it.  No GPU compute."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_under_asan_ubsan(tmp_path):
    """the layout of n in {0, 1, 2, 5} blocks against a restatement that works one block at a time, the limit checks at their edges (the 2^31
    staged words among them), the per-block, row-pointer and stride checks with the block they name, as a stand-alone program (nothing loaded
    into Python is sanitised)"""
    exe = str(tmp_path / "hashbatch_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "hashbatch_sanitize.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
