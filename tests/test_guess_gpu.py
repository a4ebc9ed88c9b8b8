"""The two kernels of a guessing round on the device (qldpc_guess_expand_dev, qldpc_guess_pick_dev) against their host mirrors
(qldpc_guess_trial_host, qldpc_guess_pick_host, which the CPU suite holds against the numpy restatement).  Exact equality everywhere."""
import numpy as np
import pytest

import blind_ref

pytestmark = pytest.mark.gpu


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def sources(rng, N, g, n_src):
    """guess rows of g VNs and random hard rows; source 0 has its VNs at the end of the row (the last, partial word), the last source, where
    there are three, fewer than g"""
    weak, hard = [], []
    for s in range(n_src):
        bits = np.zeros(N, np.uint8)
        if s == 0:
            bits[N - g:] = 1
        else:
            bits[rng.choice(N, g if s < 2 or s < n_src - 1 else g // 2, replace=False)] = 1
        weak.append(blind_ref.pack_row(bits))
        hard.append(blind_ref.pack_row(rng.integers(0, 2, N)))
    return np.stack(weak), np.stack(hard)


def expect(q, N, g, weak, hard):
    rows = [q.guess_trial_host(N, g, t, weak[s], hard[s]) for s in range(weak.shape[0]) for t in range(1 << g)]
    return np.stack([k for k, _ in rows]), np.stack([v for _, v in rows])


@pytest.mark.parametrize("N,g,n_src", [(20, 1, 3), (1008, 3, 5), (1008, 10, 2), (8300, 6, 3)])
def test_expand_equals_the_mirror(q, N, g, n_src):
    """(1008, 3, 5): 40 trial slots, not a multiple of 64; N = 20 and 8300: the last word half valid; N = 8300: 260 words, five trips of the row
    loop with a carry, and in source 1 VNs on both sides of the trip boundary at word 64"""
    import torch
    rng = np.random.default_rng(N + g)
    weak, hard = sources(rng, N, g, n_src)
    if N == 8300:
        bits = np.zeros(N, np.uint8)
        bits[[100, 63 * 32 + 31, 64 * 32, 64 * 32 + 1, 128 * 32, 8299]] = 1
        weak[1] = blind_ref.pack_row(bits)
    known, value = q.guess_expand(N, g, dev(torch, weak), dev(torch, hard))
    torch.cuda.synchronize()
    want_known, want_value = expect(q, N, g, weak, hard)
    assert known.shape == (n_src << g, (N + 31) // 32)
    assert (host(known) == want_known).all() and (host(value) == want_value).all()
    assert len({tuple(r) for r in host(value)[(1 << g):2 * (1 << g)]}) == 1 << g      # the trials of a full set are all different


def test_expand_of_small_and_empty_sets(q):
    """rows with popcount < g and an empty row: the bits of t above the ranks that exist are ignored; an empty row pins nothing in any trial"""
    import torch
    N, g = 1008, 3
    rng = np.random.default_rng(5)
    weak = np.zeros((4, 32), np.uint32)
    hard = np.stack([blind_ref.pack_row(rng.integers(0, 2, N)) for _ in range(4)])
    for s, vns in enumerate([[], [1007], [31, 32], [0, 500, 1000]]):
        bits = np.zeros(N, np.uint8)
        bits[vns] = 1
        weak[s] = blind_ref.pack_row(bits)
    known, value = q.guess_expand(N, g, dev(torch, weak), dev(torch, hard))
    torch.cuda.synchronize()
    want_known, want_value = expect(q, N, g, weak, hard)
    assert (host(known) == want_known).all() and (host(value) == want_value).all()
    v = host(value).reshape(4, 8, 32)
    assert not v[0].any() and not host(known)[:8].any()
    assert (v[1, 0] == v[1, 2]).all() and (v[1, 1] == v[1, 7]).all() and (v[1, 0] != v[1, 1]).any()
    assert (v[2, 1] == v[2, 5]).all() and len({tuple(r) for r in v[2, :4]}) == 4
    k0, v0 = q.guess_expand(N, 0, dev(torch, weak), dev(torch, hard))              # g = 0: one trial per source
    torch.cuda.synchronize()
    assert (host(k0) == weak).all() and (host(v0) == (hard & weak)).all()


@pytest.mark.parametrize("N,g", [(20, 1), (1008, 3), (1008, 10), (8300, 6)])
def test_pick_equals_the_mirror(q, N, g):
    """synthetic flags and rows, one source per case: none ok; only the last trial ok; all ok and equal; two ok trials that differ in the last valid
    position (ambiguous); two that differ only in the padding of the last word (not ambiguous); random flags over rows of which a third differ.
    The output row of a source without a winner keeps its sentinel."""
    import torch
    rng = np.random.default_rng(N * 11 + g)
    T, W = 1 << g, (N + 31) // 32
    last_valid, pad = np.uint32(1) << np.uint32((-N) % 32), np.uint32((1 << ((-N) % 32)) - 1)
    assert pad != 0
    base = np.stack([blind_ref.pack_row(rng.integers(0, 2, N)) for _ in range(7)])
    rows = np.repeat(base[:, None, :], T, 1)                                       # [7, T, W]
    ok = np.zeros((7, T), np.int32)
    ok[1, T - 1] = 1
    ok[2] = 1
    ok[3, [0, T - 1]] = 1
    rows[3, T - 1, W - 1] ^= last_valid
    ok[4, [0, T - 1]] = 1
    rows[4, T - 1, W - 1] ^= pad
    rows[4, 0, W - 1] ^= np.uint32(1)
    ok[5] = rng.random(T) < 0.3
    ok[5, T - 1] = 1
    for t in rng.choice(T, max(1, T // 3), replace=False):
        rows[5, t, rng.integers(0, W)] ^= np.uint32(1) << np.uint32(rng.integers(0, 32))
    ok[6, T // 2] = 1                                                              # one ok trial: its own row, never ambiguous
    rows[6] = rng.integers(0, 2 ** 32, (T, W), dtype=np.uint64).astype(np.uint32)
    want = [q.guess_pick_host(N, g, ok[s], rows[s]) for s in range(7)]
    assert want[0] == (-1, 0, 0) and want[1] == (T - 1, 1, 0) and want[2] == (0, T, 0) and want[3] == (0, 2, 1) and want[4] == (0, 2, 0) and want[6] == (T // 2, 1, 0)
    sentinel = np.uint32(0xA5A5A5A5)
    out = dev(torch, np.full((7, W), sentinel, np.uint32))
    win, nok, amb = q.guess_pick(N, g, dev(torch, ok.reshape(-1)), dev(torch, rows.reshape(7 * T, W)), out)
    torch.cuda.synchronize()
    got = list(zip(win.cpu().tolist(), nok.cpu().tolist(), amb.cpu().tolist()))
    assert got == want, (got, want)
    out = host(out)
    assert (out[0] == sentinel).all()
    for s in range(1, 7):
        assert (out[s] == rows[s, want[s][0]]).all(), s


def test_refused_calls_queue_nothing(q):
    import torch
    weak = dev(torch, np.zeros((2, 32), np.uint32))
    for N, g in [(1008, 11), (1008, -1)]:
        with pytest.raises(q.QldpcError) as e:
            q.guess_expand(N, g, weak, weak)
        assert e.value.status == -6, (N, g)
    out = dev(torch, np.full((2, 32), 9, np.uint32))
    with pytest.raises(q.QldpcError) as e:
        q.guess_pick(1008, 11, torch.zeros(2, dtype=torch.int32, device="cuda"), weak, out)
    assert e.value.status == -6
    torch.cuda.synchronize()
    assert (host(out) == 9).all()
    known, value = q.guess_expand(1008, 3, weak[:0], weak[:0])                     # n_src = 0
    assert known.shape == (0, 32) and value.shape == (0, 32)
