"""The staging of a hash context is one call's at a time (qcrypto-ldpc_amd/csrc/qldpc_hashbatch.h): host-form and device-form calls follow each other
on one context with no synchronisation of the caller's between them, and every one of them gives the words of the host mirrors."""
import numpy as np
import pytest

KEY_BITS, OUT_BITS = (1, 33, 1000), (0, 1, 33)        # a zero-bit block, a tail word, a row of several words
KEY_STRIDE, SEED_STRIDE, OUT_STRIDE = 32 + 1, 33 + 2, 2 + 1
FILL = 0xA5A5A5A5


def _device_rows(torch, rows, stride):
    a = np.full((len(rows), stride), FILL, np.uint32)
    for i, r in enumerate(rows):
        a[i, :r.size] = r
    return torch.from_numpy(a.view(np.int32)).cuda()


class _Lfsr:
    def __init__(self, q):
        self.q, self.ctx = q, q.PrivAmp(max_blocks=3, max_key_bits=1000, max_final_bits=33)

    def seeds(self, rng, shared):
        return [int(x) for x in rng.integers(1, 1 << 32, 3)]

    def seeds_dev(self, torch, seeds):
        return seeds

    def ref(self, keys, seeds):
        q = self.q
        return [q.privamp_expand_host(q.privamp_key_functional(k, n, 1), n, s, m) for k, n, s, m in zip(keys, KEY_BITS, seeds, OUT_BITS)]

    def host(self, keys, seeds):
        return self.ctx.blocks(keys, KEY_BITS, seeds, OUT_BITS)

    def dev(self, keys_t, seeds, out_t, stream):
        return self.ctx.blocks_dev(keys_t, KEY_BITS, seeds, OUT_BITS, out_t=out_t, stream=stream)


class _Toeplitz:
    def __init__(self, q, **how):
        self.q, self.ctx = q, q.Toeplitz(max_blocks=3, max_key_bits=1000, max_out_bits=33, **how)

    def seeds(self, rng, shared):
        """a seed per block, or one array for all of them"""
        words = [max(self.q.toeplitz_seed_words(n, m), 1) for n, m in zip(KEY_BITS, OUT_BITS)]
        if shared:
            return rng.integers(0, 1 << 32, max(words), dtype=np.uint32)
        return [rng.integers(0, 1 << 32, w, dtype=np.uint32) for w in words]

    def seeds_dev(self, torch, seeds):
        return torch.from_numpy(seeds.view(np.int32)).cuda() if isinstance(seeds, np.ndarray) else _device_rows(torch, seeds, SEED_STRIDE)

    def ref(self, keys, seeds):
        per_block = [seeds] * 3 if isinstance(seeds, np.ndarray) else seeds
        return [self.q.toeplitz_host(k, n, s, m) for k, n, s, m in zip(keys, KEY_BITS, per_block, OUT_BITS)]

    def host(self, keys, seeds):
        return self.ctx.blocks(keys, KEY_BITS, seeds, OUT_BITS)

    def dev(self, keys_t, seeds_t, out_t, stream):
        return self.ctx.blocks_dev(keys_t, KEY_BITS, seeds_t, OUT_BITS, seed_shared=seeds_t.dim() == 1, out_t=out_t, stream=stream)


@pytest.mark.gpu
def test_calls_of_both_forms_follow_each_other_on_one_context(q):
    """host form, device form on a side stream, host form with other keys, device form again: the second and the fourth return while their kernels may
    still read the descriptor rows, and the call after each must not overwrite them.  The LFSR hash, Toeplitz direct and Toeplitz NTT (small passes); the
    Toeplitz calls 3 and 4 share one seed where 1 and 2 have one per block"""
    import torch
    side = torch.cuda.Stream()
    for kind, h in (("lfsr", _Lfsr(q)), ("direct", _Toeplitz(q)), ("ntt", _Toeplitz(q, method="ntt", pass_log2=q.TOEPLITZ_PASS_LOG2_SMALL))):
        rng = np.random.default_rng(11)
        calls = []
        for c in range(4):
            keys = [q.pack_bits(rng.integers(0, 2, n)) for n in KEY_BITS]
            for k, n in zip(keys, KEY_BITS):
                k[-1] |= np.uint32((1 << ((-n) % 32)) - 1)          # garbage past the key bits must be ignored
            seeds = h.seeds(rng, shared=c >= 2)
            calls.append((keys, seeds, h.ref(keys, seeds)))
        dev_in = {c: (_device_rows(torch, calls[c][0], KEY_STRIDE), h.seeds_dev(torch, calls[c][1]),
                      torch.from_numpy(np.full((3, OUT_STRIDE), FILL, np.uint32).view(np.int32)).cuda()) for c in (1, 3)}
        torch.cuda.synchronize()                                  # the inputs are there; from here on nothing of the caller's waits
        bytes0 = h.ctx.device_bytes
        assert bytes0 > 0
        got = {}
        got[0] = h.host(*calls[0][:2])
        with torch.cuda.stream(side):
            h.dev(*dev_in[1], side)
        got[2] = h.host(*calls[2][:2])
        with torch.cuda.stream(side):
            h.dev(*dev_in[3], side)
        side.synchronize()
        for c in (0, 2):
            ref = calls[c][2]
            assert len(got[c]) == 3 and all(g.shape == r.shape and (g == r).all() for g, r in zip(got[c], ref)), (kind, c)
        for c in (1, 3):
            out, ref = dev_in[c][2].cpu().numpy().view(np.uint32), calls[c][2]
            for i, m in enumerate(OUT_BITS):
                ow = (m + 31) // 32
                assert ref[i].size == ow and (out[i, :ow] == ref[i]).all(), (kind, c, i)
                assert (out[i, ow:] == FILL).all(), (kind, c, i)   # exactly ceil(out_bits/32) words change; none for out_bits == 0
        assert h.ctx.device_bytes == bytes0, kind
