"""An independent restatement of the error-verification hash in Python integers (no call into the library): the Horner loop of the definition
with `%`, and the closed forms that the long-block tests compare against."""
import numpy as np

P = (1 << 61) - 1

# the lengths at which the decomposition changes: the first words, and around every count of coefficients c = W + 1 at which a lane row, a
# small tile or the production tile fills up (256 lanes x 4 words = 1024 per row)
EDGE_COEFS = [255, 256, 257, 1023, 1024, 1025, 2047, 2049, 3072]
EDGE_BITS = [1, 31, 32, 33, 63, 64, 65, 70] + [32 * c - 32 + d for c in EDGE_COEFS for d in (-1, 0, 1)] + [100000]


def key_of(hi, lo):
    k = (((int(hi) & 0xFFFFFFFF) << 32) | (int(lo) & 0xFFFFFFFF)) & P
    return 0 if k == P else k


def key_words(k64):
    """a 64-bit pattern as the two words (hi, lo) a caller hands over"""
    return np.array([(int(k64) >> 32) & 0xFFFFFFFF, int(k64) & 0xFFFFFFFF], np.uint32)


def edge_keys(rng):
    """64-bit patterns: 0, 1, 2, p - 1, p (-> 0), 2^61 (-> 0), 2^64 - 1 (-> 0) and a random one"""
    return [0, 1, 2, P - 1, P, 1 << 61, (1 << 64) - 1, int(rng.integers(0, 1 << 63)) * 2 + 1]


def coefficients(words, key_bits):
    n = int(key_bits)
    W = (n + 31) // 32
    c = [int(w) for w in np.asarray(words, dtype=np.uint32)[:W]]
    if n % 32:
        c[-1] &= (0xFFFFFFFF << (32 - n % 32)) & 0xFFFFFFFF
    return c + [n]


def tag_int(words, key_bits, k):
    h = 0
    for c in coefficients(words, key_bits):
        h = (h + c) * k % P
    return h


def tag(words, key_bits, hash_key):
    """hash_key: the two words (hi, lo) -> the tag's two words"""
    t = tag_int(words, key_bits, key_of(hash_key[0], hash_key[1]))
    return np.array([t >> 32, t & 0xFFFFFFFF], np.uint32)


def tags(words, key_bits, hash_keys):
    """hash_keys: 2 r words -> 2 r tag words"""
    hk = np.asarray(hash_keys, dtype=np.uint32)
    return np.concatenate([tag(words, key_bits, hk[2 * q:2 * q + 2]) for q in range(hk.size // 2)])


def as_words(t):
    return np.array([t >> 32, t & 0xFFFFFFFF], np.uint32)


def geometric(k, lo, hi):
    """SUM_{e = lo .. hi} k^e mod p, in closed form where k != 1"""
    k %= P
    if hi < lo:
        return 0
    if k == 1:
        return (hi - lo + 1) % P
    return (pow(k, hi + 1, P) - pow(k, lo, P)) * pow(k - 1, P - 2, P) % P


def closed_all_zero(n, k):
    return n * k % P


def closed_all_ones(n, k):
    """n a multiple of 32: W words of 2^32 - 1 at exponents 2 .. W + 1, then the length at exponent 1"""
    assert n % 32 == 0
    W = n // 32
    return (0xFFFFFFFF * geometric(k, 2, W + 1) + n * k) % P


def closed_single_bit(n, pos, k):
    """one bit set at index pos (MSB-first) of n bits"""
    W = (n + 31) // 32
    j = pos // 32
    return ((1 << (31 - pos % 32)) * pow(k, W + 1 - j, P) + n * k) % P
