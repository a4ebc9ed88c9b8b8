"""Every *_device_bytes getter against the numbers of the library before the contexts moved to one allocation ledger (csrc/qldpc_devmem.h):
tests/device_bytes_walk.py builds each kind of context, makes the calls that allocate lazily, and this test holds each step to
tests/golden/device_bytes.json, recorded by the same walk on that earlier library."""
import json
import os

import pytest

import device_bytes_walk

pytestmark = pytest.mark.gpu


def test_device_bytes_at_every_step(q, gold):
    """key for key: the same steps, and at each the same count"""
    want = json.load(open(os.path.join(gold, "device_bytes.json")))
    got = device_bytes_walk.walk(q)
    for k in sorted(set(want) | set(got)):
        print(k, want.get(k), got.get(k))
    assert list(got) == list(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    differ = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not differ, differ
