"""CPU suite: the allocation ledger of every context (qcrypto-ldpc_amd/csrc/qldpc_devmem.h) on the host, with malloc / free behind its two raw
hooks.  No GPU compute."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ledger_under_asan_ubsan(tmp_path):
    """the byte count after an alloc, a zero-count alloc, a pinned alloc, a release from the middle and a release of a pointer the ledger does not
    hold; a grow that fits, one that does not and one whose allocation fails; the k-th allocation of a sequence failing, for every k; dm_free_all
    twice; dm_scope left by an early return -- as a stand-alone program (nothing loaded into Python is sanitised).  LeakSanitizer proves the free
    paths complete"""
    exe = str(tmp_path / "devmem_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "devmem_sanitize.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
