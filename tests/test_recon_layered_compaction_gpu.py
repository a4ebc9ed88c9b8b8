"""GPU suite: reconciliation sessions whose layered decoders compact their active frames (QLDPC_COMPACT=1 in the environment when the
session is created).  A batch of blocks with a QBER each is exactly the case compaction is for; nothing a session reports may change:
status, corrected-bit counts, iteration counts and the corrected keys are those of the uncompacted session, block for block, and the
device-side verification (CRC, flip count) reads the decisions through the generations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_sessions_with_compacting_layered_decoders_report_the_same(q, monkeypatch):
    rng = np.random.default_rng(321)
    n, key_bits, max_blocks = 384, 20011, 192      # decoders of three 64-frame groups, layered (max_blocks > 8)
    qb = rng.uniform(0.006, 0.058, n).astype(np.float32)      # spread over the rate table
    alice = rng.integers(0, 2, (n, key_bits)).astype(np.uint8)
    bob = alice ^ (rng.random((n, key_bits)) < qb[:, None])
    aw, bw = q.pack_bits(alice), q.pack_bits(bob)
    results, remap_launches = {}, {}
    for mode in ("unset", "1"):
        if mode == "unset":
            monkeypatch.delenv("QLDPC_COMPACT", raising=False)
        else:
            monkeypatch.setenv("QLDPC_COMPACT", mode)
        ra, rb = q.Recon(max_blocks=max_blocks), q.Recon(max_blocks=max_blocks)      # fresh sessions: the variable is read when the decoders are made
        rb.profile(True)
        msgs, pars = ra.encode_blocks([aw[i] for i in range(n)], [key_bits] * n, qb)
        st, fixed, co, it = rb.decode_blocks([bw[i] for i in range(n)], [key_bits] * n, qb, msgs, pars)
        prof = {s["name"]: s["launches"] for s in rb.profile_read()}
        remap_launches[mode] = prof.get("layer_update_remap", 0)
        print("QLDPC_COMPACT %s: %d of %d blocks ok, %d sweeps in all, profile %s" % (mode, int((np.asarray(st) == 0).sum()), n, int(np.asarray(it).sum()), prof))
        results[mode] = ([(m.rate_index, m.n_punct) for m in msgs], np.asarray(st).tolist(), [f.tobytes() for f in fixed], np.asarray(co).tolist(), np.asarray(it).tolist())
    groups = {}
    for r, _ in results["unset"][0]:
        groups[r] = groups.get(r, 0) + 1
    assert len(groups) >= 3 and max(groups.values()) > 64, groups      # several rate groups, at least one of more than one 64-frame group
    assert "layer_update" in prof                                     # the decoders are layered
    assert results["1"] == results["unset"]
    st = np.array(results["1"][1])
    assert (st == 0).mean() > 0.95 and all(results["1"][2][i] == aw[i].tobytes() for i in np.nonzero(st == 0)[0])      # every OK block's key is Alice's
    assert remap_launches["unset"] == 0 and remap_launches["1"] >= 1, remap_launches      # and the sessions of the second round did compact
