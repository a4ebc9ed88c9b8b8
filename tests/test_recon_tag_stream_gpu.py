"""GPU suite: host/qldpc_stream.c -Y, the config-3 stream with verification inside the decode call (qldpc_recon_decode_blocks_tagged on Bob's side,
qldpc_recon_tag_blocks on Alice's), on a short stream."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_with_tags_inside_the_decode_call():
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    assert os.path.exists(exe), "qldpc_stream is not built"
    p = subprocess.run([exe, "-e", "16", "-k", "8192", "-b", "16", "-r", "2", "-V", "-Y"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    assert "tags equal: 16 / 16" in p.stderr
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["reconciled"] == d["yt_equal"] == d["vt_agree"] == 16 and d["yt_failed"] == 0 and d["yt_equals_vt"] == 1 and d["vt_equals_host"] == 1
    assert d["yt_leak_bits"] == 61 and d["ms_best"] > 0 and "decode_blocks_tagged" in d["workload"]
