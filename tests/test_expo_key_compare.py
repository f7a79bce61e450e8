"""kwk_expo_key_compare — the host build of the comparator expo_sort_kernel sorts a node's series
with (kwok_amd/csrc/keycmp.hpp: 8-byte big-endian words, zero padding, then the lengths) — against
Python's bytes ordering, which is std::string's: unsigned bytes, a proper prefix first.  No GPU."""
import numpy as np

from kwok_amd.host.expo import key_compare

# the names of tests/test_gpu_expo_incremental.py's comparator case, as the renderer's keys
# (namespace NUL pod NUL)
NAMES = ["a", "a-b", "a.b", "a0", "A", "b", "web", "web-0", "ab", "ba", "pod-name-x1", "pod-name-x2",
         "é1", "same", "same"]
KEYS = [ns.encode() + b"\0" + n.encode() + b"\0" for ns in ("ns", "ns-b") for n in NAMES]


def _sign(x):
    return (x > 0) - (x < 0)


def _want(a, b):
    return (a > b) - (a < b)


def _check(pairs):
    bad = [(a, b, key_compare(a, b)) for a, b in pairs if _sign(key_compare(a, b)) != _want(a, b)]
    assert not bad, bad[:10]


def test_names_of_the_device_case():
    _check([(a, b) for a in KEYS for b in KEYS])
    # the two names equal for 9 bytes differ in the second word; UTF-8 bytes sort above ASCII
    assert key_compare(b"pod-name-x1", b"pod-name-x2") < 0 and key_compare("é1".encode(), b"z") > 0
    assert key_compare(b"ab", b"ba") < 0 and key_compare(b"web", b"web-0") < 0 and key_compare(b"same", b"same") == 0


def test_prefixes_around_the_word_boundaries():
    base = bytes(range(0x61, 0x61 + 17))
    keys = [base[:n] for n in range(18)]
    assert keys[0] == b"" and len(keys[17]) == 17
    # a key, the key with a NUL / 0x01 / 0xFF appended, and with its last byte changed
    more = []
    for k in keys:
        more += [k + b"\0", k + b"\1", k + b"\xff", k + b"\0\0", k + b"\0a"]
        if k:
            more += [k[:-1] + b"\0", k[:-1] + b"\1", k[:-1] + bytes([k[-1] + 1])]
    keys += more
    _check([(a, b) for a in keys for b in keys])


def test_embedded_zero_and_one_bytes_and_the_empty_key():
    keys = [b"", b"\0", b"\1", b"\0\0", b"\0\1", b"\1\0", b"a\0b", b"a\0", b"a", b"a\1b", b"a\0\0\0\0\0\0\0",
            b"a\0\0\0\0\0\0\0\0", b"a\0\0\0\0\0\0\0\1", b"\0" * 8, b"\0" * 9, b"\0" * 16, b"\0" * 17,
            b"\0" * 7 + b"\1", b"\0" * 8 + b"\1", b"\xe9", b"\xe9\0", b"\0\xe9"]
    _check([(a, b) for a in keys for b in keys])


def test_random_pairs_from_a_four_byte_alphabet():
    rng = np.random.default_rng(0xE9)
    alphabet = np.array([0x00, 0x01, 0x61, 0xE9], dtype=np.uint8)
    pairs = []
    for _ in range(2000):
        a = alphabet[rng.integers(0, 4, size=rng.integers(0, 20))].tobytes()
        if rng.integers(0, 3) == 0:  # a shared prefix, so that the later words and the lengths decide
            b = a[:rng.integers(0, len(a) + 1)] + alphabet[rng.integers(0, 4, size=rng.integers(0, 12))].tobytes()
        else:
            b = alphabet[rng.integers(0, 4, size=rng.integers(0, 20))].tobytes()
        pairs.append((a, b))
    assert sum(a == b for a, b in pairs) < 400 and any(len(a) > 16 for a, _ in pairs)
    _check(pairs)
